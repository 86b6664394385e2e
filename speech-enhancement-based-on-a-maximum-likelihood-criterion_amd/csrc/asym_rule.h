// asym_rule.h -- the asymmetric GGD error model (mlggd_set_asymmetry), stated once for host and device (the _asym loss
// kernels, k_cv_reduce_asym, the host-order CV loop, mlggd_asym_fit).  Plain C++ with no device call, so that it also
// builds into a stand-alone host program.
//
// Per output bin d, with shape beta > 0, scale alpha > 0 and skew kappa > 0, the error e = out - targ has the density
//   f(e) = beta / (alpha (kappa + 1/kappa) Gamma(1/beta)) exp(-(s(e) / alpha)^beta),
//   s(e) = kappa e      for e > 0     one fp32 multiplication
//        = (-e) / kappa for e < 0     one fp32 division by kappa; no reciprocal of kappa is ever formed
//        = 0            for e == 0
// kappa > 1 charges over-estimates more than under-estimates, kappa < 1 the opposite; kappa = 1 is the GGD, and there
// x * 1.0f and x / 1.0f are x: s is fabsf(e), ds/de leaves the gradient's bits alone and logf((1 + 1) / 2) is 0.
// Everything of the loss chain carries over with |e| replaced by s(e); the gradient gains the factor ds/de.
//
// Two identities hold exactly in fp32 and carry the tests:
//   kappa == 1   every intermediate is the symmetric kernel's value;
//   mirror       for kappa a power of two, kappa e and e / (1 / kappa) are the same float, so the model with 1/kappa
//                of the negated error is the model with kappa of the error: s is the same and the gradient is negated.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define ASYM_HD __host__ __device__
#else
#define ASYM_HD
#endif

namespace asym_rule {

// s(e): both forms are evaluated and one is selected on the element's own data, there is no branch
ASYM_HD inline float skewed(float e, float kappa) {
    const float up = kappa * e, down = (-e) / kappa;
    return e > 0 ? up : e == 0 ? 0.0f : down;
}

// v = |dE/ds| of the symmetric chain at s (the existing pow_or_self(s, beta - 1) * beta / denom), e the error:
// v kappa for e > 0, (-v) / kappa for e < 0 (the existing sign handling, then ds/de), 0 at e == 0
ASYM_HD inline float grad(float e, float v, float kappa) {
    const float up = v * kappa, down = (-v) / kappa;
    return e > 0 ? up : e == 0 ? 0.0f : down;
}

// what density1 of the CV log-likelihood loses per frame and bin: logf((kappa + 1/kappa) / 2), exactly 0 at kappa = 1
inline float log_norm(float kappa) { return logf((kappa + 1.0f / kappa) / 2.0f); }

// Closed-form fit for one shape (host, double).  With P+ = sum_{e>0} e^beta, P- = sum_{e<0} (-e)^beta over n errors
// the log-likelihood is
//   l = n [ln beta - ln(kappa + 1/kappa) - lgamma(1/beta) - ln alpha] - (kappa^beta P+ + kappa^-beta P-) / alpha^beta.
// dl/dalpha = 0 gives alpha^beta = (beta / n) (kappa^beta P+ + kappa^-beta P-) =: (beta / n) Q(kappa), and with it
// the profile l(kappa) = n [ln beta - ln(kappa + 1/kappa) - lgamma(1/beta) - (1/beta) ln((beta/n) Q) - 1/beta].
// dl/dkappa = 0:  (1 - kappa^-2) / (kappa + 1/kappa) = -(kappa^(beta-1) P+ - kappa^(-beta-1) P-) / Q.  Multiplied
// by kappa:  (kappa - 1/kappa) (kappa^beta P+ + kappa^-beta P-) = -(kappa + 1/kappa) (kappa^beta P+ - kappa^-beta P-);
// the kappa^(1-beta) P- and kappa^(beta-1) P+ terms are the same on both sides, which leaves
// 2 kappa^(beta+1) P+ = 2 kappa^(-beta-1) P-,  that is
//   kappa^(2 (beta + 1)) = P- / P+,   kappa = (P- / P+)^(1 / (2 (beta + 1))):
// the profile has this one stationary point in kappa > 0 and falls to -inf at both ends, so it is the maximum.
// P+ == 0 or P- == 0 (all errors on one side, or none) pushes kappa to an end: no fit.
struct Fit {
    double kappa, alpha, loglik;
    bool fitted;
};
inline Fit fit(double p_plus, double p_minus, double beta, double n) {
    Fit f;
    f.fitted = p_plus > 0.0 && p_minus > 0.0;
    if (!f.fitted) {
        f.kappa = f.loglik = nan("");
        f.alpha = 0.0;
        return f;
    }
    const double lnk = (log(p_minus) - log(p_plus)) / (2.0 * (beta + 1.0));
    f.kappa = exp(lnk);
    const double q = exp(beta * lnk) * p_plus + exp(-beta * lnk) * p_minus;
    const double lna = log(beta * q / n) / beta;  // alpha^beta = (beta / n) Q
    f.alpha = exp(lna);
    f.loglik = n * ((((log(beta) - log(f.kappa + 1.0 / f.kappa)) - lgamma(1.0 / beta)) - lna) - 1.0 / beta);
    return f;
}

}  // namespace asym_rule
