// outstats.hip.h -- the output statistics of a CV chunk (mlggd_output_stats): per output bin d the sums over the
// chunk's samples of  y, y*y, t, t*t  with y the network output and t the target, both normalised (gv_rule.h).  They
// are what the global variance equalisation factors are fitted from (mlggd_gv_fit), formed beside the CV forward pass
// so that nothing of size n x D leaves the device.  Included by engine.hip after kernels.hip.h (slab_sum).
//
// Per element:  y = slab_sum + bias[d] in fp32 by the expression of k_err_stats / k_out_rowmajor (the bits
// mlggd_forward returns);  t the fp32 target;  the four terms in DOUBLE from those fp32 values.
//
// The cut is k_err_stats': one workgroup = OS_DT = 8 bins x 32 frames, a half-wave owns ONE bin for the whole bunch,
// lane j adds the rows j, j + 32, j + 64, ... of the bunch in that order into its four double accumulators, the 32
// lanes are combined by an xor butterfly (16, 8, 4, 2, 1: both partners form the same commutative sum), and lane 0
// folds the bunch's sum into acc[4][D] -- written when the bunch is the call's first, added otherwise.  Bunches follow
// each other on the engine's stream: no atomics, no scratch, one launch per bunch, and device memory that does not
// depend on the number of samples.
#pragma once
#include <hip/hip_runtime.h>

constexpr int OS_DT = 8;  // bins per workgroup, one per half-wave

struct OutStatsArgs {
    const float *slab;
    int S;
    const float *bias, *targ;
    int B, D, Dp, Bp;
    const int *first;
    int toff;
    int fresh;    // 1: this bunch is the call's first -- acc is written, not added to
    double *acc;  // [4][D]
};

__global__ __launch_bounds__(256) void k_out_stats(OutStatsArgs A) {
    const int tx = threadIdx.x & 31;
    const int d = (int)blockIdx.x * OS_DT + (int)(threadIdx.x >> 5);  // < Dp: the grid is Dp / OS_DT
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
