// scale_rule.h -- the learned GGD scale (mlggd_set_scale_mode), stated once for host and device (the _learn loss kernels,
// the engine's argument checks, tests/scale_rule_main.cc).  Plain C++ with no device call, so that it also builds into a
// stand-alone host program.  All values are fp32, every statement is one IEEE operation, nothing is contracted
// (-ffp-contract=off).
//
// The alternating engine re-solves alpha_d = (beta S_d)^(1/beta), S_d = colsum_d / n, from every minibatch and forgets
// it.  Here alpha_d is a parameter: per output bin d < D a state (alpha, v) lives across minibatches and ln alpha moves
// by gradient descent with momentum, with the per-frame loss E = ln alpha + S / alpha^beta (the terms of the negative
// log-likelihood that hold alpha), dE/d ln alpha = 1 - beta S / alpha^beta.  Per step, with s the column sum of p the
// loss path already forms, beta the shape in effect and (eta, mu, vmax) the mode's parameters:
//   v1 = s / nf                      (existing)
//   v2 = v1 * beta                   (existing; = beta S, the closed form's alpha^beta)
//   if alpha == 0:                   seed: the bin has no scale yet
//       alpha' = pow_or_self(v2, 1/beta)    (the existing closed form, same bits)
//       v'     = 0
//       q      = pow_or_self(alpha', beta)
//   else:
//       q  = pow_or_self(alpha, beta)       the denominator of the W gradient: alpha BEFORE the update
//       r  = v2 / q
//       gl = 1.0f - r
//       v' = mu * v - eta * gl              two products, one subtraction
//       v' = clamp to [-vmax, vmax] by selects that let a NaN through
//       alpha' = alpha * exp_det(v')
// pow_or_self and exp_det are those of kernels.hip.h; the caller evaluates them and hands the values in, so that this
// header stays plain C++.
//
// Two identities hold exactly in fp32 and carry the tests:
//   seed     the first step of a fresh engine (alpha all zero) has the alternating engine's bits;
//   frozen   eta = 0 and mu = 0 give v' = +-0, exp_det(+-0) == 1.0f and alpha' = alpha.
#pragma once
#include <stddef.h>

#include <cmath>

#if defined(__HIPCC__)
#define SCALE_HD __host__ __device__
#else
#define SCALE_HD
#endif

namespace scale_rule {

constexpr int kAlternating = 0, kLearned = 1;                       // MLGGD_SCALE_ALTERNATING / MLGGD_SCALE_LEARNED
constexpr float kLrate = 0.05f, kMomentum = 0.5f, kVmax = 1.0f;     // the defaults: a choice, not a measured optimum

// the state of every bin is [2 copies][alpha, v][Dp]: where a value of copy c lives
SCALE_HD inline size_t alpha_at(int c, size_t Dp, size_t d) { return ((size_t)c * 2 + 0) * Dp + d; }
SCALE_HD inline size_t velocity_at(int c, size_t Dp, size_t d) { return ((size_t)c * 2 + 1) * Dp + d; }

// v2 = beta S from the column sum
SCALE_HD inline float beta_s(float s, float nf, float beta) {
    const float v1 = s / nf;
    return v1 * beta;
}

// alpha == 0: the bin takes the closed form this step
SCALE_HD inline bool seeds(float alpha) { return alpha == 0.0f; }

// v' from q = pow_or_self(alpha, beta); NaN > vmax and NaN < -vmax are false, so a NaN passes through the clamp
SCALE_HD inline float velocity(float v2, float q, float v, float eta, float mu, float vmax) {
    const float r = v2 / q;
    const float gl = 1.0f - r;
    const float keep = mu * v;
    const float push = eta * gl;
    float vn = keep - push;
    const float lo = -vmax;
    vn = vn > vmax ? vmax : vn;
    vn = vn < lo ? lo : vn;
    return vn;
}

// alpha' from ex = exp_det(v')
SCALE_HD inline float advance(float alpha, float ex) { return alpha * ex; }

// what mlggd_set_scale_mode accepts
inline bool valid(int mode, float lrate, float momentum, float vmax) {
    return (mode == kAlternating || mode == kLearned) && std::isfinite(lrate) && std::isfinite(momentum) && std::isfinite(vmax) &&
           lrate >= 0.0f && momentum >= 0.0f && momentum < 1.0f && vmax > 0.0f;
}

// a state's alpha: zero means "seed"
inline bool valid_alpha(float alpha) { return std::isfinite(alpha) && alpha >= 0.0f; }

}  // namespace scale_rule
