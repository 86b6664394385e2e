// adam_rule.h -- the Adam weight rule (mlggd_set_optimizer), stated once for host and device (k_adam_apply, the engine's
// argument checks, mlggd_adam_apply, tests/adam_rule_main.cc).  Plain C++ with no device call, so that it also builds
// into a stand-alone host program.  All values are fp32, every statement is one IEEE operation, nothing is contracted
// (-ffp-contract=off).
//
// Kingma and Ba's Adam beside the engine's SGD with momentum.  Per weight, with the engine's lrate, weightcost wc and the
// minibatch size nf, G the summed gradient the unfused dW launches write, (m, v) the weight's two moments:
//   t1 = G / nf
//   t2 = wc * w
//   g  = t1 + t2                 the SGD rule's own gradient expression; wc = 0 for a bias
//   m' = b1 * m + c1 * g         two products, one sum; c1 = (float)(1 - (double)b1), formed on the host
//   v' = b2 * v + (c2 * g) * g   three products, one sum; c2 likewise
//   s  = sqrt(v')                correctly rounded
//   q  = m' / (s + eps)          one sum, one IEEE division
//   w' = w - a_t * q             one product, one difference
// The step size a_t = (float)((double)lr * sqrt(1 - p2_t) / (1 - p1_t)) is the bias correction folded into the rate:
// p1_t = p1_{t-1} * (double)b1 and p2_t = p2_{t-1} * (double)b2 are running products kept in double from p_0 = 1 --
// repeated multiplications, not pow, so that no two math libraries can disagree in the last place.  The host forms a_t
// once per update and hands it to the launch; stepsize() re-forms the products by the loop when a state is restored.
// In real numbers this is the textbook rule with eps scaled: w -= lr * mhat / (sqrt(vhat) + eps / sqrt(1 - b2^t)).
//
// eps > 0 is required: a pad entry with G = w = m = v = 0 then stays exactly 0 (g = 0, m' = 0, v' = 0, q = 0 / eps = 0).
// Weight decay is the engine's L2 term inside g, so weightcost keeps its meaning.  Out of scope: decoupled decay (AdamW),
// AMSGrad, a rate per layer.
#pragma once
#include <stdint.h>

#include <cmath>

#if defined(__HIPCC__)
#define ADAM_HD __host__ __device__
#else
#define ADAM_HD
#endif

namespace adam_rule {

constexpr int kSgd = 0, kAdam = 1;                           // MLGGD_OPT_SGD / MLGGD_OPT_ADAM
constexpr float kBeta1 = 0.9f, kBeta2 = 0.999f, kEps = 1e-8f;  // Kingma and Ba's defaults: not evaluated on speech here

// what one update shares: formed on the host, a kernel argument
struct Consts {
    float nf, b1, c1, b2, c2, eps, a_t;
};

struct Moments {
    float w, m, v;
};

// the gradient expression of the SGD rule (kernels.hip.h k_apply_update)
ADAM_HD inline float gradient(float G, float w, float nf, float wc) {
    const float t1 = G / nf;
    const float t2 = wc * w;
    return t1 + t2;
}

// one weight, one step
ADAM_HD inline Moments step(float w, float m, float v, float G, float wc, const Consts &c) {
    const float g = gradient(G, w, c.nf, wc);
    const float keep_m = c.b1 * m;
    const float push_m = c.c1 * g;
    const float mn = keep_m + push_m;
    const float keep_v = c.b2 * v;
    const float cg = c.c2 * g;
    const float push_v = cg * g;
    const float vn = keep_v + push_v;
    const float s = sqrtf(vn);
    const float den = s + c.eps;
    const float q = mn / den;
    const float move = c.a_t * q;
    Moments out;
    out.w = w - move;
    out.m = mn;
    out.v = vn;
    return out;
}

// c = (float)(1 - (double)b)
inline float complement(float b) { return (float)(1.0 - (double)b); }

// the running products of an engine: p1 = b1^steps, p2 = b2^steps by repeated multiplication in double
struct Products {
    double p1 = 1.0, p2 = 1.0;
};
inline void advance(Products *p, float b1, float b2) {
    p->p1 = p->p1 * (double)b1;
    p->p2 = p->p2 * (double)b2;
}
// ... re-formed by the loop for a restored state.  The products only shrink, and below 2^-54 a product p gives
// 1 - p == 1 in double: it no longer reaches a_t.  So the loop ends once both are below kSpent = 2^-60 -- after
// 60 / -log2(b) multiplications, 41,600 for b = 0.999 -- whatever `steps` is; every a_t formed from what it returns,
// advanced further or not, is the one the uninterrupted products give.
constexpr double kSpent = 1.0 / 1152921504606846976.0;  // 2^-60
inline Products products(float b1, float b2, int64_t steps) {
    Products p;
    for (int64_t t = 0; t < steps && (p.p1 >= kSpent || p.p2 >= kSpent); t++) advance(&p, b1, b2);
    return p;
}
// a_t of the update that takes the products to (p1, p2)
inline float stepsize_of(float lr, const Products &p) {
    const double num = std::sqrt(1.0 - p.p2);
    const double den = 1.0 - p.p1;
    return (float)((double)lr * num / den);
}
// a_t of update number `steps` (>= 1): the step size of the update that follows steps - 1 earlier ones
inline float stepsize(float lr, float b1, float b2, int64_t steps) { return stepsize_of(lr, products(b1, b2, steps)); }

inline Consts consts(float nf, float lr, float b1, float b2, float eps, const Products &after) {
    Consts c;
    c.nf = nf, c.b1 = b1, c.c1 = complement(b1), c.b2 = b2, c.c2 = complement(b2), c.eps = eps;
    c.a_t = stepsize_of(lr, after);
    return c;
}

// what mlggd_set_optimizer accepts
inline bool valid_kind(int kind) { return kind == kSgd || kind == kAdam; }
inline bool valid(float b1, float b2, float eps) {
    return b1 >= 0.0f && b1 < 1.0f && b2 >= 0.0f && b2 < 1.0f && std::isfinite(eps) && eps > 0.0f;
}

}  // namespace adam_rule
