// mix.hip.h -- training data from waves (mlggd_mix_waves, mlggd_lps_stats, mlggd_load_waves, mlggd_train_waves): the
// mixer of clean speech and noise at an SNR (the rule is mix_rule.h), the normalised feature / target streams of a
// wave pair and the per-bin statistics the norm vectors come from.  Included by engine.hip after spectral.hip.h.
//
//   k_mix_energy     Ec = sum clean^2, En = sum noise^2 per utterance, exact 64-bit integers
//   k_mix_apply      gain from (Ec, En, r), noisy = sat16(rint(clean + gain * noise)), gain[u], clipped[u]
//   k_lps_norm_pair  (lpsN - mean) * inv_std and (lpsC - mean) * inv_std into the raw set's feat / targ
//   k_lps_norm_pair_mask  the same for a mask engine: targ rows are [normalised clean LPS | ratio mask], mask_rule.h
//   k_mask_targets   the mask half alone from given rows (mlggd_mask_targets)
//   k_lps_colstats   per bin sum x and sum x^2 in double over a fixed number of rows; k_lps_colfold adds the partials
//
// The cut of the two mixing kernels: the host cuts every utterance into blocks of mix_rule::kBlock consecutive samples
// (the table is mix_rule::Block); one workgroup takes one block.  A block is walked in slots of 8 samples aligned to
// 16 bytes of the PACKED wave (clean and noisy are packed alike and their buffers are 16-byte aligned): a slot that
// lies inside the block is one 16-byte load / store per lane, consecutive lanes taking consecutive slots; the slots a
// block's first and last samples share with its neighbours take the 2-byte path, element by element with a bounds
// check.  The noise index of a lane's first sample is phase + j with ONE compare-and-subtract where the segment is at
// least a block long (phase < len and j < kBlock <= len), and a 64-bit modulo only where it is shorter; from there on
// it advances by increment and compare.  The noise is read 2 bytes at a time: its alignment against the clean wave is
// arbitrary and it may wrap inside a slot; a lane's 8 reads fall into one or two 16-byte pieces of a cache line.
//
// Determinism: the energies are integer sums (wave butterfly, LDS, one 64-bit atomicAdd per workgroup: any order gives
// the same integer); every sample of noisy is a fixed sequence of IEEE double operations on (clean, noise, Ec, En, r);
// clipped is an integer count.  The column statistics add a fixed set of rows per workgroup in a fixed order and the
// partials are folded in index order: no floating-point atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mask_rule.h"
#include "mix_rule.h"

constexpr int MIX_THREADS = 256;
constexpr int MIX_WAVES = MIX_THREADS / 64;

// the noise index (inside the segment) of sample j of the block
__device__ __forceinline__ long long mix_phase(const mix_rule::Block &b, int j) {
    if (b.len >= mix_rule::kBlock) {
        const long long i = b.phase + j;
        return i >= b.len ? i - b.len : i;
    }
    return (long long)((unsigned long long)(b.phase + j) % (unsigned long long)b.len);
}

__device__ __forceinline__ int mix_half(const int4 &q, int e) {  // element e of 8 int16 (e is an unrolled constant)
    const int w = (e >> 1) == 0 ? q.x : (e >> 1) == 1 ? q.y : (e >> 1) == 2 ? q.z : q.w;
    return (int)(int16_t)((unsigned)w >> (16 * (e & 1)));
}

// E [2 n_utts] (zeroed by the caller): Ec, En of utterance u at E[2 u], E[2 u + 1]
__global__ __launch_bounds__(MIX_THREADS) void k_mix_energy(const mix_rule::Block *__restrict__ blocks,
                                                            const int16_t *__restrict__ clean,
                                                            const int16_t *__restrict__ noise,
                                                            unsigned long long *__restrict__ E) {
    __shared__ unsigned long long s_e[MIX_WAVES][2];
    const mix_rule::Block b = blocks[blockIdx.x];
    const long long s0 = b.at & ~7LL;
    const int nslots = (int)(((b.at + b.n + 7) >> 3) - (b.at >> 3));
    unsigned long long ec = 0, en = 0;
    for (int slot = threadIdx.x; slot < nslots; slot += MIX_THREADS) {
        const long long g0 = s0 + (long long)slot * 8;
        const int j0 = (int)(g0 - b.at);
        const bool full = j0 >= 0 && j0 + 8 <= b.n;
        long long idx = mix_phase(b, j0 < 0 ? 0 : j0);
        int4 q = make_int4(0, 0, 0, 0);
        if (full) q = *reinterpret_cast<const int4 *>(clean + g0);
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int j = j0 + e;
            if (j < 0 || j >= b.n) continue;
            const int c = full ? mix_half(q, e) : (int)clean[g0 + e];
            const int z = (int)noise[b.lo + idx];
            idx = idx + 1 == b.len ? 0 : idx + 1;
            ec += (unsigned long long)(unsigned)(c * c);
            en += (unsigned long long)(unsigned)(z * z);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ec += __shfl_xor(ec, off, 64);
        en += __shfl_xor(en, off, 64);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_e[wv][0] = ec;
        s_e[wv][1] = en;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long a = 0, c = 0;
#pragma unroll
        for (int w = 0; w < MIX_WAVES; w++) {
            a += s_e[w][0];
            c += s_e[w][1];
        }
        atomicAdd(&E[2 * (size_t)b.u], a);
        atomicAdd(&E[2 * (size_t)b.u + 1], c);
    }
}

// noisy (packed like clean), gain [n_utts] and clipped [n_utts] (both zeroed by the caller: an utterance without
// samples has no block and keeps gain 0)
__global__ __launch_bounds__(MIX_THREADS) void k_mix_apply(const mix_rule::Block *__restrict__ blocks,
                                                           const int16_t *__restrict__ clean,
                                                           const int16_t *__restrict__ noise,
                                                           const unsigned long long *__restrict__ E,
                                                           const double *__restrict__ r, int16_t *__restrict__ noisy,
                                                           double *__restrict__ gain, int *__restrict__ clipped) {
    __shared__ int s_c[MIX_WAVES];
    const mix_rule::Block b = blocks[blockIdx.x];
    const double g = mix_rule::gain(E[2 * (size_t)b.u], E[2 * (size_t)b.u + 1], r[b.u]);
    if (b.first && threadIdx.x == 0) gain[b.u] = g;
    const long long s0 = b.at & ~7LL;
    const int nslots = (int)(((b.at + b.n + 7) >> 3) - (b.at >> 3));
    int clip = 0;
    for (int slot = threadIdx.x; slot < nslots; slot += MIX_THREADS) {
        const long long g0 = s0 + (long long)slot * 8;
        const int j0 = (int)(g0 - b.at);
        const bool full = j0 >= 0 && j0 + 8 <= b.n;
        long long idx = mix_phase(b, j0 < 0 ? 0 : j0);
        int4 q = make_int4(0, 0, 0, 0);
        if (full) q = *reinterpret_cast<const int4 *>(clean + g0);
        unsigned o[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const int j = j0 + e;
            if (j < 0 || j >= b.n) continue;
            const int c = full ? mix_half(q, e) : (int)clean[g0 + e];
            const int z = (int)noise[b.lo + idx];
            idx = idx + 1 == b.len ? 0 : idx + 1;
            const int16_t v = mix_rule::mix(c, z, g, &clip);
            if (full) o[e >> 1] |= (unsigned)(uint16_t)v << (16 * (e & 1));
            else noisy[g0 + e] = v;
        }
        if (full) *reinterpret_cast<int4 *>(noisy + g0) = make_int4((int)o[0], (int)o[1], (int)o[2], (int)o[3]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) clip += __shfl_xor(clip, off, 64);
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = clip;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
#pragma unroll
        for (int w = 0; w < MIX_WAVES; w++) t += s_c[w];
        if (t) atomicAdd(&clipped[b.u], t);
    }
}

// One workgroup per packed frame: feat[f][d] = (lpsN[f][d] - mean[d]) * inv[d], targ[f][d] = (lpsC[f][d] - mean[d]) *
// inv[d], subtraction and product as two fp32 operations; the targets take the NOISY statistics, as the trainer's
// loader does.  No edge replication: a training sample is a window of consecutive frames inside one utterance.
__global__ void k_lps_norm_pair(const float *__restrict__ lpsN, const float *__restrict__ lpsC, int D,
                                const float *__restrict__ mean, const float *__restrict__ inv,
                                float *__restrict__ feat, float *__restrict__ targ) {
    const size_t row = (size_t)blockIdx.x * D;
    for (int k = threadIdx.x; k < D; k += blockDim.x) {
        const float m = mean[k], s = inv[k];
        const float a = lpsN[row + k] - m;
        const float c = lpsC[row + k] - m;
        feat[row + k] = a * s;
        targ[row + k] = c * s;
    }
}

// The same for a mask engine (mask_rule.h): targ is [F][2 D], row f = [(lpsC - mean) * inv | s * min(1, exp_det(0.5
// (lpsC - lpsN)))]; and the mask half alone on n given values.  Defined in mask.hip.h.
__global__ void k_lps_norm_pair_mask(const float *__restrict__ lpsN, const float *__restrict__ lpsC, int D,
                                     const float *__restrict__ mean, const float *__restrict__ inv, float scale,
                                     float *__restrict__ feat, float *__restrict__ targ);
__global__ void k_mask_targets(const float *__restrict__ noisy, const float *__restrict__ clean, size_t n, float scale,
                               float *__restrict__ out);

// Per bin the sums of x and x^2 in double over rows [chunk CS_ROWS, (chunk + 1) CS_ROWS) of the packed LPS rows
// [F][D]: the cut of k_err_stats, a half-wave per bin, lane j adding rows j, j + 32, ... in that order, an xor
// butterfly over the 32 lanes.  x * x of an fp32 value is exact in double.  part is [chunks][2][D]; grid (ceil(D /
// CS_BINS), chunks).
constexpr int CS_BINS = 8, CS_ROWS = 1024;
__global__ __launch_bounds__(256) void k_lps_colstats(const float *__restrict__ lps, int F, int D,
                                                      double *__restrict__ part) {
    const int tx = threadIdx.x & 31;
    const int d = (int)blockIdx.x * CS_BINS + (int)(threadIdx.x >> 5);
    const int r0 = (int)blockIdx.y * CS_ROWS;
    const int r1 = F - r0 < CS_ROWS ? F : r0 + CS_ROWS;
    double s1 = 0.0, s2 = 0.0;
    if (d < D)
        for (int r = r0 + tx; r < r1; r += 32) {
            const double x = (double)lps[(size_t)r * D + d];
            s1 += x;
            s2 += x * x;
        }
#pragma unroll
    for (int off = 16; off > 0; off >>= 1) {
        s1 += __shfl_xor(s1, off, 64);
        s2 += __shfl_xor(s2, off, 64);
    }
    if (tx == 0 && d < D) {
        part[((size_t)blockIdx.y * 2 + 0) * D + d] = s1;
        part[((size_t)blockIdx.y * 2 + 1) * D + d] = s2;
    }
}

// sums[i] = part[0][i] + part[1][i] + ... in chunk order, i < n = 2 D
__global__ void k_lps_colfold(const double *__restrict__ part, int chunks, int n, double *__restrict__ sums) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int c = 0; c < chunks; c++) s += part[(size_t)c * n + i];
    sums[i] = s;
}
