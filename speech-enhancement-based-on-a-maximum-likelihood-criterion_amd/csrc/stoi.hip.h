// stoi.hip.h -- STOI (Taal, Hendriks, Heusdens, Jensen 2011; the rules and tables in stoi_rule.h) of processed int16
// waves against clean int16 waves on the device, per utterance of a packed batch.  Included by engine.hip after
// score.hip.h, whose wave reductions and whose FFT butterflies (spectral.hip.h, here with M = 256: the 512-point real
// spectrum of a zero-padded frame of 256) it calls; no kernel of those files changes.
//
//   k_stoi_resample  one thread per 10 kHz sample: y[n] = sum_k h[n q - k p + Lh] x[k] over the taps in range, in
//                    increasing k from 0.0f, for the clean and the processed wave
//   k_stoi_energy    one wavefront per frame of the clean 10 kHz signal: e = 20 log10(||x w|| / 16)
//   k_stoi_select    one workgroup per utterance: the maximum of e, the keep mask (e - max + 40 > 0) and its exclusive
//                    scan in frame order -> the map from kept index to frame index, and the kept count
//   k_stoi_bands     one wavefront per frame m of the compacted signals (the kept windowed frames overlap-added at hop
//                    K, rebuilt on the fly: a sample is the sum of at most 2 kept frames, the earlier one first), windowed
//                    again -> 512-point spectrum -> the 15 band roots of the clean (X) and the processed (Y) signal
//   k_stoi_utt       one workgroup per utterance: the correlation of every (segment, band), and their mean
//
// The host knows only upper bounds (every frame kept): the grids of k_stoi_bands run over them and a wavefront beyond
// the device-side count takes part in the barriers and writes nothing; nothing is read back between the launches.
//
// Everything is fp32 with log10 evaluated in double and rounded.  Every reduction is a fixed sequence: a lane's strided
// partial sum in index order and the 64-lane xor butterfly (k_stoi_energy); a band's bins in increasing k; a segment's
// 30 frames in frame order; the 15 band values of a segment in lanes 0..14 of a butterfly whose other lanes hold 0.0f;
// per-wave partials over the segments s = wave, wave + SCORE_UTT_WAVES, ... and the halving tree of k_score_utt.  The
// order depends on local indices and the utterance's own counts alone, so an utterance's value is a function of that
// utterance: bit-identical whatever its neighbours, its position, the batch and the run.  No atomics.
#pragma once
#include <math.h>

#include "score.hip.h"

#define STOI_N 256
#define STOI_K 128
#define STOI_BANDS 15
#define STOI_SEG 30
#define STOI_SELECT_WAVES 4

// one utterance of the batch: where its clean / processed samples start, how many are scored, and where its 10 kHz
// samples and its frames start in the packed work buffers
struct StoiUtt {
    long long coff, poff, off10;
    int len, len10, foff, frames;
};

struct StoiBandTable {
    int lo[STOI_BANDS], hi[STOI_BANDS];
};

// the largest u with utt[u].off10 <= gi (an utterance without samples shares its offset with its successor)
__device__ __forceinline__ int stoi_utt_of_sample(const StoiUtt *__restrict__ utt, int n_utts, long long gi) {
    int lo = 0, hi = n_utts - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (utt[mid].off10 <= gi) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int stoi_utt_of_frame(const StoiUtt *__restrict__ utt, int n_utts, int g) {
    int lo = 0, hi = n_utts - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (utt[mid].foff <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// grid: ceil(total10 / 256) workgroups of 256 threads.  h [2 Lh + 1].
__global__ void __launch_bounds__(256) k_stoi_resample(const int16_t *__restrict__ clean, const int16_t *__restrict__ proc,
                                                       const StoiUtt *__restrict__ utt, int n_utts,
                                                       const float *__restrict__ h, int p, int q, int Lh,
                                                       long long total10, float *__restrict__ xc,
                                                       float *__restrict__ xp) {
    const long long gi = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gi >= total10) return;
    const StoiUtt U = utt[stoi_utt_of_sample(utt, n_utts, gi)];
    const long long nq = (gi - U.off10) * q;
    long long k0 = nq - Lh;  // ceil((nq - Lh) / p), at least 0
    k0 = k0 <= 0 ? 0 : (k0 + p - 1) / p;
    long long k1 = (nq + Lh) / p;
    if (k1 > U.len - 1) k1 = U.len - 1;
    const int16_t *c = clean + U.coff, *d = proc + U.poff;
    float ac = 0.0f, ad = 0.0f;
    for (long long k = k0; k <= k1; k++) {
        const float t = h[nq - k * p + Lh];
        ac += t * (float)c[k];
        ad += t * (float)d[k];
    }
    xc[gi] = ac;
    xp[gi] = ad;
}

// grid: ceil(FT / 4) workgroups of 256 threads, one wavefront per packed frame of the clean signal
__global__ void __launch_bounds__(256) k_stoi_energy(const float *__restrict__ xc, const StoiUtt *__restrict__ utt,
                                                     int n_utts, int FT, const float *__restrict__ win,
                                                     float *__restrict__ e) {
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= FT) return;
    const int u = stoi_utt_of_frame(utt, n_utts, g);
    const float *x = xc + utt[u].off10 + (size_t)(g - utt[u].foff) * STOI_K;  // frame t: inside the utterance's len10
    float s = 0.0f;
    for (int i = lane; i < STOI_N; i += 64) {
        const float v = x[i] * win[i];
        s += v * v;
    }
    s = score_wave_sum(s);
    if (lane == 0) e[g] = 20.0f * (float)log10((double)(sqrtf(s) / 16.0f));
}

// grid: n_utts workgroups of 64 * STOI_SELECT_WAVES threads.  map [foff[u] + i] = the frame of kept index i.
__global__ void __launch_bounds__(64 * STOI_SELECT_WAVES) k_stoi_select(const StoiUtt *__restrict__ utt,
                                                                        const float *__restrict__ e,
                                                                        int *__restrict__ map, int *__restrict__ kept) {
    __shared__ float s_mx[STOI_SELECT_WAVES];
    __shared__ int s_cnt[STOI_SELECT_WAVES];
    const int u = blockIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int fo = utt[u].foff, F = utt[u].frames;
    float mx = -INFINITY;
    for (int i = threadIdx.x; i < F; i += 64 * STOI_SELECT_WAVES) mx = fmaxf(mx, e[fo + i]);
    mx = score_wave_max(mx);
    if (lane == 0) s_mx[wv] = mx;
    __syncthreads();
    mx = s_mx[0];
    for (int i = 1; i < STOI_SELECT_WAVES; i++) mx = fmaxf(mx, s_mx[i]);
    int base = 0;
    for (int a = 0; a < F; a += 64 * STOI_SELECT_WAVES) {  // the same trips in every thread
        const int t = a + threadIdx.x;
        // a silent utterance: max = -inf and e - max is NaN: nothing is kept
        const bool keep = t < F && (e[fo + (t < F ? t : 0)] - mx) + 40.0f > 0.0f;
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) s_cnt[wv] = __popcll(mask);
        __syncthreads();
        int off = base, tot = 0;
        for (int i = 0; i < STOI_SELECT_WAVES; i++) {
            if (i < wv) off += s_cnt[i];
            tot += s_cnt[i];
        }
        if (keep) map[fo + off + __popcll(mask & ((1ull << lane) - 1ull))] = t;
        base += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) kept[u] = base;
}

// sample i of compacted frame m of the signal x (the utterance's 10 kHz samples), not yet windowed again; mp = the
// utterance's part of the map; m + 1 < kept
__device__ __forceinline__ float stoi_compacted(const float *__restrict__ x, const int *__restrict__ mp, int m, int i,
                                                const float *__restrict__ win) {
    const float mid = x[(size_t)mp[m] * STOI_K + i] * win[i];
    if (i < STOI_K) {
        if (m == 0) return mid;
        return x[(size_t)mp[m - 1] * STOI_K + i + STOI_K] * win[i + STOI_K] + mid;
    }
    return mid + x[(size_t)mp[m + 1] * STOI_K + i - STOI_K] * win[i - STOI_K];
}

// grid: ceil(FT / SPEC_FRAMES) workgroups of 64 * SPEC_FRAMES threads; compacted frame m of utterance u is packed row
// foff[u] + m of Xb / Yb [FT][STOI_BANDS]; it exists while m < kept[u] - 1.  tw [128] = exp(-2 pi i j / 256), tws [257]
// = exp(-2 pi i k / 512): the 16 kHz tables of the spectral front end.
__global__ void __launch_bounds__(64 * SPEC_FRAMES) k_stoi_bands(
    const float *__restrict__ xc, const float *__restrict__ xp, const StoiUtt *__restrict__ utt, int n_utts, int FT,
    const float *__restrict__ win, const float2 *__restrict__ tw, const float2 *__restrict__ tws,
    const int *__restrict__ map, const int *__restrict__ kept, StoiBandTable bands, float *__restrict__ Xb,
    float *__restrict__ Yb) {
    __shared__ float s_re[SPEC_FRAMES][SPEC_ROW], s_im[SPEC_FRAMES][SPEC_ROW], s_pw[SPEC_FRAMES][SPEC_MAXM + 1];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * SPEC_FRAMES + wv;
    const int gg = g < FT ? g : 0;
    const int u = stoi_utt_of_frame(utt, n_utts, gg);
    const int fo = utt[u].foff, m = gg - fo;
    const bool live = g < FT && m < kept[u] - 1;
    const int *mp = map + fo;
    float *re = s_re[wv], *im = s_im[wv], *pw = s_pw[wv];
    const int M = SPEC_MAXM, logM = 8;
    for (int sig = 0; sig < 2; sig++) {
        const float *x = (sig ? xp : xc) + utt[u].off10;
        // z_j = v_2j + i v_2j+1 of the frame zero-padded to 512, in bit-reversed order
        for (int j = lane; j < M; j += 64) {
            const int n0 = 2 * j, n1 = 2 * j + 1;
            float v0 = 0.0f, v1 = 0.0f;
            if (live && n1 < STOI_N) {
                v0 = stoi_compacted(x, mp, m, n0, win) * win[n0];
                v1 = stoi_compacted(x, mp, m, n1, win) * win[n1];
            }
            const int r = spec_pad(spec_bitrev(j, logM));
            re[r] = v0;
            im[r] = v1;
        }
        __syncthreads();
        spec_fft_rows(re, im, tw, M, logM, lane);
        // the real split step of spec_analysis_frame, and the power of bins 0..256
        for (int k = lane; k <= M; k += 64) {
            const int ka = (k == M) ? 0 : k, kb = (k == 0) ? 0 : M - k;
            const float zr = re[spec_pad(ka)], zi = im[spec_pad(ka)];
            const float cr = re[spec_pad(kb)], ci = -im[spec_pad(kb)];
            const float er = (zr + cr) * 0.5f, ei = (zi + ci) * 0.5f;
            const float orr = (zr - cr) * 0.5f, oi = (zi - ci) * 0.5f;
            const float2 w = tws[k];
            const float pr = w.x * orr - w.y * oi, pi = w.x * oi + w.y * orr;
            const float xr = er + pi, xi = ei - pr;
            pw[k] = xr * xr + xi * xi;
        }
        __syncthreads();
        if (live && lane < STOI_BANDS) {
            float s = 0.0f;
            for (int k = bands.lo[lane]; k < bands.hi[lane]; k++) s += pw[k];
            (sig ? Yb : Xb)[(size_t)gg * STOI_BANDS + lane] = sqrtf(s);
        }
        __syncthreads();  // the rows are loaded again
    }
}

// min(a, b) for b >= 0 that keeps a NaN in a, as the definition's minimum does (fminf would drop it and return b): a
// band of exact zeros over a segment has alpha = inf and alpha Y = NaN, and the utterance then has no value
__device__ __forceinline__ float stoi_min_keep_nan(float a, float b) { return b < a ? b : a; }

// grid: n_utts workgroups of 64 * SCORE_UTT_WAVES threads.  clip = (float) 10^(15/20).  Fewer than STOI_SEG compacted
// frames: stoi = NaN, segments = 0.  A band of a segment whose processed signal is exactly zero: stoi = NaN with the
// segments counted.
__global__ void __launch_bounds__(64 * SCORE_UTT_WAVES) k_stoi_utt(const StoiUtt *__restrict__ utt,
                                                                   const int *__restrict__ kept,
                                                                   const float *__restrict__ Xb,
                                                                   const float *__restrict__ Yb, float clip,
                                                                   float *__restrict__ stoi, int *__restrict__ segments) {
    __shared__ float s_acc[SCORE_UTT_WAVES];
    const int u = blockIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int Mc = kept[u] > 0 ? kept[u] - 1 : 0;
    const int S = Mc >= STOI_SEG ? Mc - (STOI_SEG - 1) : 0;
    if (S == 0) {  // the same in every thread
        if (threadIdx.x == 0) {
            stoi[u] = NAN;
            segments[u] = 0;
        }
        return;
    }
    float acc = 0.0f;
    for (int s = wv; s < S; s += SCORE_UTT_WAVES) {  // segment s: compacted frames s .. s + 29
        float d = 0.0f;
        if (lane < STOI_BANDS) {
            const float *X = Xb + (size_t)(utt[u].foff + s) * STOI_BANDS + lane;
            const float *Y = Yb + (size_t)(utt[u].foff + s) * STOI_BANDS + lane;
            float ex = 0.0f, ey = 0.0f, sx = 0.0f;
            for (int f = 0; f < STOI_SEG; f++) {
                const float a = X[f * STOI_BANDS], b = Y[f * STOI_BANDS];
                ex += a * a;
                ey += b * b;
                sx += a;
            }
            const float alpha = sqrtf(ex / ey);
            float sy = 0.0f;
            for (int f = 0; f < STOI_SEG; f++) {
                const float a = X[f * STOI_BANDS];
                sy += stoi_min_keep_nan(alpha * Y[f * STOI_BANDS], a + a * clip);
            }
            const float mx = sx / (float)STOI_SEG, my = sy / (float)STOI_SEG;
            float sxx = 0.0f, syy = 0.0f, sxy = 0.0f;
            for (int f = 0; f < STOI_SEG; f++) {
                const float a = X[f * STOI_BANDS];
                const float xn = a - mx, yn = stoi_min_keep_nan(alpha * Y[f * STOI_BANDS], a + a * clip) - my;
                sxx += xn * xn;
                syy += yn * yn;
                sxy += xn * yn;
            }
            d = sxy / (sqrtf(sxx) * sqrtf(syy));
        }
        acc += score_wave_sum(d);
    }
    if (lane == 0) s_acc[wv] = acc;
    __syncthreads();
    if (threadIdx.x) return;
    for (int h = SCORE_UTT_WAVES / 2; h > 0; h >>= 1)
        for (int i = 0; i < h; i++) s_acc[i] += s_acc[i + h];
    stoi[u] = s_acc[0] / (float)(STOI_BANDS * S);
    segments[u] = S;
}
