// gv_rule.h -- global variance equalisation (Xu, Du, Dai and Lee 2015, "A regression approach to speech enhancement
// based on deep neural networks", section III.A), stated once for host and device (k_out_stats, mlggd_gv_fit,
// k_lps_synthesis_gv).  Plain C++ with no device call, so that it also builds into a stand-alone host program.
//
// Everything lives in the NORMALISED domain, the one the net is trained in: y_n[d] is the fp32 network output (slab
// sum + bias, the bits mlggd_forward returns), t_n[d] the fp32 target.
//
// Statistics.  sums[4][D] in double: row 0 = sum y, row 1 = sum y y, row 2 = sum t, row 3 = sum t t over the samples,
// every term formed in double from the fp32 value (term()).  Additive over chunks.
//
// Fit (host, double, + - x / sqrt only).  With n samples per bin:
//   mu = S1 / n,  r2 = S2 / n,  gv = r2 - mu mu     for outputs (gv_est) and targets (gv_ref),
//   eta[d] = (float)sqrt(gv_ref[d] / gv_est[d]).
// A bin with gv_est <= 0 or gv_ref <= 0 (a constant output, a constant target, n = 1) has no fit: eta = 1, fitted = 0.
// The shared (dimension-independent) factor is the same expressions on the sums of the FITTED bins, added in bin
// order, with n times the number of fitted bins as its sample count (n D when every bin has a fit): the variance about
// the one global mean, as the paper defines it.  No fitted bin, or a pooled variance that is not positive: shared eta
// 1, fitted_shared 0.
//
// Apply.  Where a decoder de-normalises:  v = ((y * eta[k]) / inv[k]) + mean[k],  three IEEE fp32 operations from left
// to right, nothing contracted (-ffp-contract=off); y * 1.0f is y, so a vector of ones leaves every bit as it was.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GV_HD __host__ __device__
#else
#define GV_HD
#endif

namespace gv_rule {

constexpr int kRows = 4;  // sum y, sum y y, sum t, sum t t

GV_HD inline float apply(float y, float eta, float inv, float mean) {
    const float s = y * eta;
    const float q = s / inv;
    return q + mean;
}

// mu = s1 / n, r2 = s2 / n, gv = r2 - mu mu
inline double variance(double s1, double s2, double n) {
    const double mu = s1 / n, r2 = s2 / n;
    const double mm = mu * mu;  // its own statement: the product is rounded before the subtraction
    return r2 - mm;
}

struct Fit {
    double gv_est, gv_ref;
    float eta;
    bool fitted;
};

inline Fit fit(double sy, double syy, double st, double stt, double n) {
    Fit f;
    f.gv_est = variance(sy, syy, n);
    f.gv_ref = variance(st, stt, n);
    f.fitted = f.gv_est > 0.0 && f.gv_ref > 0.0;
    f.eta = f.fitted ? (float)sqrt(f.gv_ref / f.gv_est) : 1.0f;
    return f;
}

// per bin (every output optional) and shared; sums [4][D], n >= 1 samples per bin
inline Fit fit_all(int D, int64_t n, const double *sums, double *gv_est, double *gv_ref, float *eta, uint8_t *fitted) {
    double p[kRows] = {0.0, 0.0, 0.0, 0.0};
    int64_t bins = 0;
    for (int d = 0; d < D; d++) {
        const Fit f = fit(sums[d], sums[(size_t)D + d], sums[(size_t)2 * D + d], sums[(size_t)3 * D + d], (double)n);
        if (gv_est) gv_est[d] = f.gv_est;
        if (gv_ref) gv_ref[d] = f.gv_ref;
        if (eta) eta[d] = f.eta;
        if (fitted) fitted[d] = f.fitted ? 1 : 0;
        if (!f.fitted) continue;
        for (int r = 0; r < kRows; r++) p[r] += sums[(size_t)r * D + d];
        bins++;
    }
    if (bins == 0) return Fit{0.0, 0.0, 1.0f, false};
    return fit(p[0], p[1], p[2], p[3], (double)n * (double)bins);
}

}  // namespace gv_rule
