// mask.hip.h -- the kernels of a multi-objective (mask) engine (mask_rule.h): the target-forming pass beside
// k_lps_norm_pair and the two post-filtering instances of the synthesis kernel.  They are DECLARED where their siblings
// live (mix.hip.h, spectral.hip.h) and DEFINED here, in one file that engine.hip includes last: everything a mask engine
// adds to the device code is read in one place, and the other headers hold what they held.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.hip.h"  // exp_det
#include "mask_rule.h"
#include "mix.hip.h"
#include "spectral.hip.h"

// k_lps_norm_pair for a mask engine: targ is [F][2 D], row f = [(lpsC - mean) * inv | s * min(1, exp_det(0.5 (lpsC -
// lpsN)))], the mask half from the UN-normalised rows and not normalised itself.  D is odd at every rate, so the mask
// half of row f starts at float f 2 D + D, 16-byte aligned for one row in four at best: scalar stores, a lane per bin,
// consecutive lanes on consecutive floats.  One pass over rows the analysis launches just wrote.
__global__ void k_lps_norm_pair_mask(const float *__restrict__ lpsN, const float *__restrict__ lpsC, int D,
                                     const float *__restrict__ mean, const float *__restrict__ inv, float scale,
                                     float *__restrict__ feat, float *__restrict__ targ) {
    const size_t row = (size_t)blockIdx.x * D, trow = 2 * row;
    for (int k = threadIdx.x; k < D; k += blockDim.x) {
        const float m = mean[k], s = inv[k];
        const float y = lpsN[row + k], c = lpsC[row + k];
        const float a = y - m;
        const float b = c - m;
        feat[row + k] = a * s;
        targ[trow + k] = b * s;
        targ[trow + D + k] = mask_rule::target(exp_det(mask_rule::half_diff(c, y)), scale);
    }
}

// out[i] = s * min(1, exp_det(0.5 (clean[i] - noisy[i]))), i < n: the arithmetic of the mask half above on given rows
__global__ void k_mask_targets(const float *__restrict__ noisy, const float *__restrict__ clean, size_t n, float scale,
                               float *__restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = mask_rule::target(exp_det(mask_rule::half_diff(clean[i], noisy[i])), scale);
}

// a mask engine's decode: src rows of 2 D outputs, the post-filter of mask_rule.h (MaskArgs, spectral.hip.h)
__global__ void __launch_bounds__(64 * SPEC_FRAMES) k_lps_synthesis_mask(
    const float *__restrict__ src, const float *__restrict__ mean, const float *__restrict__ inv,
    const float2 *__restrict__ X, int t0, int nf, SpecDims d, const float *__restrict__ win,
    const float2 *__restrict__ tw, const float2 *__restrict__ tws, float floor_exp, float *__restrict__ blk,
    float *__restrict__ lps_den, MaskArgs mk) {
    lps_synthesis_frames<false, true>(src, mean, inv, nullptr, X, t0, nf, d, win, tw, tws, floor_exp, blk, lps_den, mk);
}

// ... with the equalisation factors eta, of which the first D are read
__global__ void __launch_bounds__(64 * SPEC_FRAMES) k_lps_synthesis_mask_gv(
    const float *__restrict__ src, const float *__restrict__ mean, const float *__restrict__ inv,
    const float *__restrict__ eta, const float2 *__restrict__ X, int t0, int nf, SpecDims d,
    const float *__restrict__ win, const float2 *__restrict__ tw, const float2 *__restrict__ tws, float floor_exp,
    float *__restrict__ blk, float *__restrict__ lps_den, MaskArgs mk) {
    lps_synthesis_frames<true, true>(src, mean, inv, eta, X, t0, nf, d, win, tw, tws, floor_exp, blk, lps_den, mk);
}
