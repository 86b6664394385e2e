// colstats.hip.h -- the column statistics of a CV chunk: per output bin d, sums over the chunk's samples of a few
// double terms of the network output x and the target t, formed beside the CV forward pass so that nothing of size
// n x D leaves the device.  Three sets of terms, one kernel each, what the per-bin models of the host are fitted from:
//   k_err_stats         e, e^2, e^3, e^4 and |e|^beta_k over a grid of K shapes   (mlggd_error_stats, mlggd_ggd_fit)
//   k_err_stats_signed  |e|^beta_k split by the sign of e, no moment sums   (mlggd_error_stats_signed, mlggd_asym_fit)
//   k_out_stats         y, y^2, t, t^2 with y = x, both normalised (gv_rule.h)        (mlggd_output_stats, mlggd_gv_fit)
// Included by engine.hip after kernels.hip.h (slab_sum, pow_or_self); col_stats_resident there launches all three.
//
// Per element:  x = slab_sum + bias[d] in fp32 by the expression of k_cv_reduce / k_out_rowmajor (the bits
// mlggd_forward returns);  t the fp32 target;  e = x - t, one fp32 subtraction (the loss chain's kernerror);  every
// term in DOUBLE from those fp32 values.
//
// The cut is that of the loss kernels: one workgroup = COLSTATS_DT = 8 bins x 32 frames, lanes along the frames (slab
// rows read in 128-byte segments, targets in 32-byte pieces).  A half-wave owns ONE bin for the whole bunch: lane j adds
// the rows j, j + 32, j + 64, ... of the bunch in that order into its double accumulators, the 32 lanes are combined
// by an xor butterfly (16, 8, 4, 2, 1: both partners form the same commutative sum), and lane 0 folds the bunch's sum
// into acc[rows][D] -- written when the bunch is the call's first, added otherwise.  Bunches follow each other on the
// engine's stream, so the order of every addition is a function of the row's position in its bunch, of the bunch index
// and of bunchsize alone: no atomics, one launch per bunch, and device memory that does not depend on the number of
// samples.  The accumulators are indexed by unrolled constants only (K <= 32 is tested against the unrolled index, a
// wave-uniform branch): at most 64 doubles in registers, no scratch.
//
// The three kernels share the work split, the row loop, the element, the butterfly and the fold, and are still three
// texts: as instantiations of one body over a terms policy (the accumulators in one array, or in a struct the policy
// owns; the argument struct by reference or by value) the compiler gave every one of them other code than it gives
// these -- more SGPR spills, more instructions (profiles/col_stats_isa.txt).  What is shared is the argument prefix the
// host fills (slab .. acc, the same names in both structs) and this description.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mlggd.h"

constexpr int COLSTATS_DT = 8;  // bins per workgroup, one per half-wave

struct ErrStatsArgs {
    const float *slab;
    int S;
    const float *bias, *targ;
    int B, D, Dp, Bp;
    const int *first;
    int toff;
    int K;       // 1..MLGGD_MAX_BETAS
    int fresh;   // 1: this bunch is the call's first -- acc is written, not added to
    double *acc; // k_err_stats [4 + K][D], k_err_stats_signed [2 K][D]
    float betas[MLGGD_MAX_BETAS];
};

// acc [4 + K][D]: the four moment sums e, e*e, (e*e)*e, (e*e)*(e*e), then the K power sums pow_or_self(fabsf(e),
// beta_k), the fp32 value of the trainer's own pow_det -- evaluated once per beta ON PURPOSE: one logarithm shared by
// the grid would be cheaper and would leave the bits the trainer and oracle/pyoracle.pow_det agree on -- widened to
// double.
__global__ __launch_bounds__(256) void k_err_stats(ErrStatsArgs A) {
    const int tx = threadIdx.x & 31;
    const int d = (int)blockIdx.x * COLSTATS_DT + (int)(threadIdx.x >> 5);  // < Dp: the grid is Dp / COLSTATS_DT
    double m1 = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0;
    double pw[MLGGD_MAX_BETAS];
#pragma unroll
    for (int k = 0; k < MLGGD_MAX_BETAS; k++) pw[k] = 0.0;
    if (d < A.D) {
        const float bias = A.bias[d];
        for (int b = tx; b < A.B; b += 32) {
            float x = slab_sum(A.slab, (size_t)d * A.Bp + b, (size_t)A.Dp * A.Bp, A.S);
            x = x + bias;
            const float t = A.targ[(size_t)(A.first ? A.first[b] + A.toff : b) * A.D + d];
            const float e = x - t;
            const double e1 = (double)e, e2 = e1 * e1;
            m1 += e1;
            m2 += e2;
            m3 += e2 * e1;
            m4 += e2 * e2;
            const float a = fabsf(e);
#pragma unroll
            for (int k = 0; k < MLGGD_MAX_BETAS; k++)
                if (k < A.K) pw[k] += (double)pow_or_self(a, A.betas[k]);
        }
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
        m1 += __shfl_xor(m1, off, 64);
        m2 += __shfl_xor(m2, off, 64);
        m3 += __shfl_xor(m3, off, 64);
        m4 += __shfl_xor(m4, off, 64);
    }
#pragma unroll
    for (int k = 0; k < MLGGD_MAX_BETAS; k++)
        if (k < A.K) {
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) pw[k] += __shfl_xor(pw[k], off, 64);
        }
    if (tx == 0 && d < A.D) {
        double *p = A.acc + d;
        const size_t D = (size_t)A.D;
        p[0 * D] = A.fresh ? m1 : p[0 * D] + m1;
        p[1 * D] = A.fresh ? m2 : p[1 * D] + m2;
        p[2 * D] = A.fresh ? m3 : p[2 * D] + m3;
        p[3 * D] = A.fresh ? m4 : p[3 * D] + m4;
#pragma unroll
        for (int k = 0; k < MLGGD_MAX_BETAS; k++)
            if (k < A.K) p[(4 + k) * D] = A.fresh ? pw[k] : p[(4 + k) * D] + pw[k];
    }
}

// acc [2 K][D] (asym_rule.h): the K rows of  P+_k[d] = sum_{e > 0} pow_or_self(e, beta_k),  then the K rows of
// P-_k[d] = sum_{e < 0} pow_or_self(-e, beta_k).  The power is evaluated once per element at fabsf(e), which is e or -e,
// and a select on the lane's own e sends it to one side and +0.0 to the other (adding +0.0 to a sum of non-negative
// terms leaves its bits), so the exponent stays wave-uniform.
__global__ __launch_bounds__(256) void k_err_stats_signed(ErrStatsArgs A) {
    const int tx = threadIdx.x & 31;
    const int d = (int)blockIdx.x * COLSTATS_DT + (int)(threadIdx.x >> 5);  // < Dp: the grid is Dp / COLSTATS_DT
    double pp[MLGGD_MAX_BETAS], pm[MLGGD_MAX_BETAS];
#pragma unroll
    for (int k = 0; k < MLGGD_MAX_BETAS; k++) pp[k] = pm[k] = 0.0;
    if (d < A.D) {
        const float bias = A.bias[d];
        for (int b = tx; b < A.B; b += 32) {
            float x = slab_sum(A.slab, (size_t)d * A.Bp + b, (size_t)A.Dp * A.Bp, A.S);
            x = x + bias;
            const float t = A.targ[(size_t)(A.first ? A.first[b] + A.toff : b) * A.D + d];
            const float e = x - t;
            const float a = fabsf(e);
#pragma unroll
            for (int k = 0; k < MLGGD_MAX_BETAS; k++)
                if (k < A.K) {
                    const double v = (double)pow_or_self(a, A.betas[k]);
                    pp[k] += e > 0 ? v : 0.0;
                    pm[k] += e < 0 ? v : 0.0;
                }
        }
    }
#pragma unroll
    for (int k = 0; k < MLGGD_MAX_BETAS; k++)
        if (k < A.K) {
#pragma unroll
            for (int off = 16; off > 0; off >>= 1) {
                pp[k] += __shfl_xor(pp[k], off, 64);
                pm[k] += __shfl_xor(pm[k], off, 64);
            }
        }
    if (tx == 0 && d < A.D) {
        double *p = A.acc + d;
        const size_t D = (size_t)A.D;
#pragma unroll
        for (int k = 0; k < MLGGD_MAX_BETAS; k++)
            if (k < A.K) {
                p[k * D] = A.fresh ? pp[k] : p[k * D] + pp[k];
                p[(A.K + k) * D] = A.fresh ? pm[k] : p[(A.K + k) * D] + pm[k];
            }
    }
}

struct OutStatsArgs {
    const float *slab;
    int S;
    const float *bias, *targ;
    int B, D, Dp, Bp;
    const int *first;
    int toff;
    int fresh;    // as in ErrStatsArgs
    double *acc;  // [4][D]
};

// acc [4][D] (gv_rule::kRows): y, y*y, t, t*t.
__global__ __launch_bounds__(256) void k_out_stats(OutStatsArgs A) {
    const int tx = threadIdx.x & 31;
    const int d = (int)blockIdx.x * COLSTATS_DT + (int)(threadIdx.x >> 5);  // < Dp: the grid is Dp / COLSTATS_DT
    double y1 = 0.0, y2 = 0.0, t1 = 0.0, t2 = 0.0;
    if (d < A.D) {
        const float bias = A.bias[d];
        for (int b = tx; b < A.B; b += 32) {
            float x = slab_sum(A.slab, (size_t)d * A.Bp + b, (size_t)A.Dp * A.Bp, A.S);
            x = x + bias;
            const float t = A.targ[(size_t)(A.first ? A.first[b] + A.toff : b) * A.D + d];
            const double yd = (double)x, td = (double)t;
            y1 += yd;
            y2 += yd * yd;
            t1 += td;
            t2 += td * td;
        }
    }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
        y1 += __shfl_xor(y1, off, 64);
        y2 += __shfl_xor(y2, off, 64);
        t1 += __shfl_xor(t1, off, 64);
        t2 += __shfl_xor(t2, off, 64);
    }
    if (tx == 0 && d < A.D) {
        double *p = A.acc + d;
        const size_t D = (size_t)A.D;
        p[0 * D] = A.fresh ? y1 : p[0 * D] + y1;
        p[1 * D] = A.fresh ? y2 : p[1 * D] + y2;
        p[2 * D] = A.fresh ? t1 : p[2 * D] + t1;
        p[3 * D] = A.fresh ? t2 : p[3 * D] + t2;
    }
}
