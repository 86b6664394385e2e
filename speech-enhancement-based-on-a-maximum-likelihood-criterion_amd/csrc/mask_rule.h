// mask_rule.h -- multi-objective learning with mask-based post-processing (Xu, Du, Dai and Lee: the net predicts a ratio
// mask beside the clean LPS and the decoder lets the mask choose, per time-frequency bin, between the noisy input, the
// estimate and their mean), stated once for host and device (k_lps_norm_pair_mask, k_mask_targets,
// k_lps_synthesis_mask / _mask_gv, mlggd_mask_select).  Plain C++ with no device call, so that it also builds into a
// stand-alone host program.  All values are fp32, every statement is one IEEE operation, nothing is contracted
// (-ffp-contract=off).  D is the rate's bin count; a mask engine's last layer has 2 D units, LPS first, mask last.
//
// Target for frame f, bin k.  c and y are the UN-normalised clean and noisy LPS rows of the analysis, s > 0 the scale:
//   a = c - y
//   h = 0.5f * a                      exact
//   m = min(1, exp_det(h))            the clean-to-noisy magnitude ratio sqrt(Pc / Py), capped at 1; a NaN stays a NaN
//   t = s * m
// exp_det is the exponential of kernels.hip.h; the caller evaluates it on half_diff() and hands the value to target(),
// so that this header stays plain C++.  The mask half of a target row is not z-normalised.  s exists because under
// MMSE the squared error of the mask half weighs s^2 against the LPS half; under ML-GGD it changes nothing but alpha.
//
// Post-filter for decoded frame t, bin k.  o_k is network output k (0 <= k < 2 D), x the de-normalised LPS estimate as
// an engine without a mask forms it (o_k / inv + mean, or gv_rule::apply), n the noisy LPS of that frame and bin,
// lo <= hi the thresholds:
//   m = o_{D+k} / s
//   v = m > hi ? n : (m >= lo ? 0.5f * (n + x) : x)          a NaN mask takes x
// v replaces x everywhere downstream.  Mode off: v = x, the mask half is ignored.
#pragma once
#include <stddef.h>

#include <cmath>

#if defined(__HIPCC__)
#define MASK_HD __host__ __device__
#else
#define MASK_HD
#endif

namespace mask_rule {

constexpr int kOff = 0, kSelect = 1;                        // MLGGD_MASK_OFF / MLGGD_MASK_SELECT
constexpr float kLo = 0.25f, kHi = 0.75f, kScale = 1.0f;    // the defaults: a choice, not a measured optimum

// h, the argument of the exponential
MASK_HD inline float half_diff(float c, float y) {
    const float a = c - y;
    return 0.5f * a;
}

// t from ex = exp_det(half_diff(c, y)); NaN > 1 is false, so a NaN passes through the cap
MASK_HD inline float target(float ex, float s) {
    const float m = ex > 1.0f ? 1.0f : ex;
    return s * m;
}

// v; both candidates are formed and one is selected on the element's own data
MASK_HD inline float select(float n, float x, float o_mask, float s, float lo, float hi) {
    const float m = o_mask / s;
    const float sum = n + x;
    const float mid = 0.5f * sum;
    return m > hi ? n : (m >= lo ? mid : x);
}

// what mlggd_set_mask accepts
inline bool valid(int mode, float lo, float hi, float s) {
    return (mode == kOff || mode == kSelect) && std::isfinite(lo) && std::isfinite(hi) && std::isfinite(s) && lo <= hi && s > 0.0f;
}

// rows [n][D] on the host: the float32 statement of the post-filter
inline void select_rows(int D, size_t n, const float *noisy, const float *lps, const float *mask, float lo, float hi,
                        float *out) {
    for (size_t i = 0; i < n * (size_t)D; i++) out[i] = select(noisy[i], lps[i], mask[i], 1.0f, lo, hi);
}

}  // namespace mask_rule
