// spectral.hip.h -- the spectral front end and back end of the original project's Wav2LPS_be / LPS2Wav_be
// (Wav2LogSpec_be.c, LogSpec2Wav.c with OLA_KIND 1, FEfunc.c) on the device.  Included by engine.hip.
//
//   k_lps_analysis   int16 frames -> window -> real N-point FFT in LDS -> log power rows (and the complex spectrum X)
//   k_lps_stream     LPS rows -> (lps - mean) * inv_std, edge-replicated context stream for the forward pass
//   k_lps_synthesis  LPS rows, or the forward pass's outputs de-normalised, + X -> noisy phase, inverse FFT, window
//                    (k_lps_synthesis_gv: de-normalised with the equalisation factors of gv_rule.h;
//                    k_lps_synthesis_mask / _mask_gv: a mask engine's rows, post-filtered by mask_rule.h)
//   k_ola            overlap-add of the windowed time blocks, / sum w^2, float and saturated int16 output
//
// The *_seg kernels are the same steps over a packed batch of utterances (mlggd_enhance_waves): global frame g of
// the batch is local frame g - frame_off[u] of utterance u, and every edge (frame positions, context replication,
// overlap-add coverage) is the utterance's own.  Per element they run the operation sequences of the kernels above.
//
// FFT form: the real N-point spectrum is an M = N/2-point complex FFT of z_m = x_2m + i x_2m+1
// (radix-2 decimation in time: bit-reversed load, log2(M) butterfly stages in LDS) followed by the real split step
// X_k = (Z_k + conj Z_{M-k}) / 2 - i W_N^k (Z_k - conj Z_{M-k}) / 2.  The inverse runs the same steps backwards
// (the conjugate trick: IDFT(Z) = conj(DFT(conj Z)) / M).  One wavefront per frame, SPEC_FRAMES frames per
// workgroup.  Twiddles and the window come from tables computed on the host in double and rounded to float; the log
// and exp are evaluated in double as the original does.  Every output element is a fixed sequence of IEEE fp32
// operations (-ffp-contract=off), so results are deterministic and independent of launch geometry and chunking.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gv_rule.h"    // gv_rule::apply
#include "mask_rule.h"  // mask_rule::select
#include "spec_rule.h"  // SpecDims

#define SPEC_FRAMES 4     // frames (= wavefronts) per workgroup
#define SPEC_MAXM 256     // largest complex FFT (N = 512)
#define SPEC_FLOOR (-50.0f)

// LDS index with one float of padding every 32: the power-of-two strides of the butterflies do not all land on
// one bank (cdna_hip_programming.md Guideline 4)
__device__ __forceinline__ int spec_pad(int i) { return i + (i >> 5); }
#define SPEC_ROW (SPEC_MAXM + SPEC_MAXM / 32)

// forward complex FFT of the M points in (re, im) of one wavefront's LDS row, data already in bit-reversed order
__device__ __forceinline__ void spec_fft_rows(float *re, float *im, const float2 *__restrict__ tw, int M, int logM,
                                              int lane) {
    for (int s = 0; s < logM; s++) {
        const int h = 1 << s, tstep = M >> (s + 1);
        for (int b = lane; b < M / 2; b += 64) {
            const int j = b & (h - 1);
            const int i0 = ((b >> s) << (s + 1)) + j, i1 = i0 + h;
            const float2 w = tw[j * tstep];
            const float ar = re[spec_pad(i0)], ai = im[spec_pad(i0)];
            const float br = re[spec_pad(i1)], bi = im[spec_pad(i1)];
            const float cr = br * w.x - bi * w.y, ci = br * w.y + bi * w.x;
            re[spec_pad(i0)] = ar + cr;
            im[spec_pad(i0)] = ai + ci;
            re[spec_pad(i1)] = ar - cr;
            im[spec_pad(i1)] = ai - ci;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ int spec_bitrev(int m, int logM) { return (int)(__brev((unsigned)m) >> (32 - logM)); }

// one wavefront: the frame of L samples at x -> row t of lps / X (each optional, nullptr).  win [L] (full, mirrored),
// tw [M/2] = exp(-2 pi i j / M), tws [D] = exp(-2 pi i k / N).  A dead wave (!live) still takes part in the barriers.
__device__ __forceinline__ void spec_analysis_frame(const int16_t *__restrict__ x, bool live, size_t t, const SpecDims &d,
                                                    const float *__restrict__ win, const float2 *__restrict__ tw,
                                                    const float2 *__restrict__ tws, float floor_p,
                                                    float *__restrict__ lps, float2 *__restrict__ X, float *re,
                                                    float *im, int lane) {
    for (int m = lane; m < d.M; m += 64) {
        const int n0 = 2 * m, n1 = 2 * m + 1;
        const float v0 = (live && n0 < d.L) ? (float)x[n0] * win[n0] : 0.0f;  // zero padding to N
        const float v1 = (live && n1 < d.L) ? (float)x[n1] * win[n1] : 0.0f;
        const int r = spec_pad(spec_bitrev(m, d.logM));
        re[r] = v0;
        im[r] = v1;
    }
    __syncthreads();
    spec_fft_rows(re, im, tw, d.M, d.logM, lane);
    if (!live) return;
    for (int k = lane; k < d.D; k += 64) {
        const int ka = (k == d.M) ? 0 : k, kb = (k == 0) ? 0 : d.M - k;  // Z_{k mod M}, Z_{(M-k) mod M}
        const float zr = re[spec_pad(ka)], zi = im[spec_pad(ka)];
        const float cr = re[spec_pad(kb)], ci = -im[spec_pad(kb)];   // conj Z_{M-k}
        const float er = (zr + cr) * 0.5f, ei = (zi + ci) * 0.5f;
        const float orr = (zr - cr) * 0.5f, oi = (zi - ci) * 0.5f;
        const float2 w = tws[k];
        const float pr = w.x * orr - w.y * oi, pi = w.x * oi + w.y * orr;  // W^k O
        const float xr = er + pi, xi = ei - pr;                             // E - i W^k O
        if (X) X[t * d.D + k] = make_float2(xr, xi);
        if (lps) {
            const float P = xr * xr + xi * xi;
            lps[t * d.D + k] = (P < floor_p) ? SPEC_FLOOR : (float)log((double)P);
        }
    }
}

// grid: ceil(F / SPEC_FRAMES) workgroups of 64 * SPEC_FRAMES threads, one wavefront per frame
__global__ void __launch_bounds__(64 * SPEC_FRAMES) k_lps_analysis(const int16_t *__restrict__ wave, int F, SpecDims d,
                                                                   const float *__restrict__ win,
                                                                   const float2 *__restrict__ tw,
                                                                   const float2 *__restrict__ tws, float floor_p,
                                                                   float *__restrict__ lps, float2 *__restrict__ X) {
    __shared__ float s_re[SPEC_FRAMES][SPEC_ROW], s_im[SPEC_FRAMES][SPEC_ROW];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int t = blockIdx.x * SPEC_FRAMES + wv;
    const bool live = t < F;
    const int16_t *x = wave + (size_t)(live ? t : 0) * d.S;  // frame t: samples [t S, t S + L), inside the wave
    spec_analysis_frame(x, live, (size_t)(live ? t : 0), d, win, tw, tws, floor_p, lps, X, s_re[wv], s_im[wv], lane);
}

// The utterance of global frame g: the largest u with frame_off[u] <= g (every utterance has at least one frame, so
// frame_off is strictly increasing).  utt_of, when given, is the per-frame table of the same answer.
__device__ __forceinline__ int seg_of_frame(const int *__restrict__ frame_off, int n_utts,
                                            const int *__restrict__ utt_of, int g) {
    if (utt_of) return utt_of[g];
    int lo = 0, hi = n_utts - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (frame_off[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// k_lps_analysis over a packed batch: global frame g = local frame g - frame_off[u] of utterance u, whose samples
// start at wave + wave_off[u].  lps / X rows are indexed by g.
__global__ void __launch_bounds__(64 * SPEC_FRAMES) k_lps_analysis_seg(
    const int16_t *__restrict__ wave, const long long *__restrict__ wave_off, const int *__restrict__ frame_off,
    const int *__restrict__ utt_of, int n_utts, int F, SpecDims d, const float *__restrict__ win,
    const float2 *__restrict__ tw, const float2 *__restrict__ tws, float floor_p, float *__restrict__ lps,
    float2 *__restrict__ X) {
    __shared__ float s_re[SPEC_FRAMES][SPEC_ROW], s_im[SPEC_FRAMES][SPEC_ROW];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * SPEC_FRAMES + wv;
    const bool live = g < F;
    const int gg = live ? g : 0;
    const int u = seg_of_frame(frame_off, n_utts, utt_of, gg);
    const int16_t *x = wave + wave_off[u] + (size_t)(gg - frame_off[u]) * d.S;
    spec_analysis_frame(x, live, (size_t)gg, d, win, tw, tws, floor_p, lps, X, s_re[wv], s_im[wv], lane);
}

// The forward pass's input for output frames [a, a + n) of an F-frame utterance: n + 2 half rows, row j = frame
// clamp(a - half + j, 0, F - 1) normalised as (lps - mean) * inv_std (two IEEE operations); and first[i] = i.
__global__ void k_lps_stream(const float *__restrict__ lps, int F, int D, int a, int rows, int half,
                             const float *__restrict__ mean, const float *__restrict__ inv, float *__restrict__ stream,
                             int *__restrict__ first, int n_first) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)n_first) first[i] = (int)i;
    if (i >= (size_t)rows * D) return;
    const int j = (int)(i / D), k = (int)(i % D);
    int src = a - half + j;
    src = src < 0 ? 0 : (src >= F ? F - 1 : src);
    const float c = lps[(size_t)src * D + k] - mean[k];
    stream[i] = c * inv[k];
}

// The forward pass's input for the packed frames [a, a + n), which touch utterances u0..u1: utterance u contributes
// the rows of its frames in the chunk plus ctx - 1 context rows, edge-replicated inside the utterance, so its section
// starts at row rs(u) = max(frame_off[u], a) - a + (u - u0) (ctx - 1) and sample i (frame a + i of utterance u)
// starts at first[i] = i + (u - u0) (ctx - 1).  One workgroup per stream row; the row's utterance is found by a
// search every lane runs alike.
__global__ void k_lps_stream_seg(const float *__restrict__ lps, const int *__restrict__ frame_off,
                                 const int *__restrict__ utt_of, int n_utts, int D, int a, int n, int u0, int u1, int ctx,
                                 const float *__restrict__ mean, const float *__restrict__ inv,
                                 float *__restrict__ stream, int *__restrict__ first) {
    const int r = blockIdx.x, half = (ctx - 1) / 2;
    if (r < n && threadIdx.x == 0) first[r] = r + (seg_of_frame(frame_off, n_utts, utt_of, a + r) - u0) * (ctx - 1);
    int lo = u0, hi = u1;  // the largest u with rs(u) <= r
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int fo = frame_off[mid];
        if ((fo > a ? fo : a) - a + (mid - u0) * (ctx - 1) <= r) lo = mid;
        else hi = mid - 1;
    }
    const int u = lo, fo = frame_off[u], Fu = frame_off[u + 1] - fo;
    const int ga = fo > a ? fo : a;
    int t = (ga - fo) - half + (r - (ga - a + (u - u0) * (ctx - 1)));
    t = t < 0 ? 0 : (t >= Fu ? Fu - 1 : t);
    const float *src = lps + (size_t)(fo + t) * D;
    float *dst = stream + (size_t)r * D;
    for (int k = threadIdx.x; k < D; k += blockDim.x) {
        const float c = src[k] - mean[k];
        dst[k] = c * inv[k];
    }
}

// Frames [t0, t0 + nf): target LPS row r = src[(t - t0) * D + k] (de-normalised first when mean != nullptr: y / inv +
// mean, two IEEE operations; GV: (y * eta) / inv + mean, gv_rule::apply), noisy spectrum X [t][k] -> windowed time block
// blk [t][L].  lps_den (optional, with mean): receives the de-normalised rows, [t][D].  The body of k_lps_synthesis
// (GV = false: eta is never read) and of k_lps_synthesis_gv.
// MASK (k_lps_synthesis_mask, _mask_gv; mean and inv are given): src holds the 2 D outputs of a mask engine per frame,
// LPS half first.  Two frame indices: the output rows of a chunk are chunk-local, row r of src; X, lps_den AND the
// noisy LPS rows `noisy` [t][D] of the analysis are indexed by the packed frame t = t0 + r.  The de-normalised
// estimate x is formed as without a mask and v = mask_rule::select(noisy, x, src[r][D + k], ...) takes its place
// (mode off: v = x and neither the mask half nor the noisy rows are read).  MaskArgs is empty for the other kernels.
struct MaskArgs {
    const float *noisy;  // [t][D] un-normalised noisy LPS
    float lo, hi, scale;
    int mode;  // mask_rule::kOff / kSelect
};
template <bool GV, bool MASK = false>
__device__ __forceinline__ void lps_synthesis_frames(const float *__restrict__ src, const float *__restrict__ mean,
                                                     const float *__restrict__ inv, const float *__restrict__ eta,
                                                     const float2 *__restrict__ X, int t0, int nf, SpecDims d,
                                                     const float *__restrict__ win, const float2 *__restrict__ tw,
                                                     const float2 *__restrict__ tws, float floor_exp,
                                                     float *__restrict__ blk, float *__restrict__ lps_den,
                                                     const MaskArgs mk = MaskArgs{nullptr, 0.0f, 0.0f, 0.0f, 0}) {
    __shared__ float s_yr[SPEC_FRAMES][SPEC_MAXM + 1], s_yi[SPEC_FRAMES][SPEC_MAXM + 1];
    __shared__ float s_re[SPEC_FRAMES][SPEC_ROW], s_im[SPEC_FRAMES][SPEC_ROW];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = blockIdx.x * SPEC_FRAMES + wv;
    const bool live = r < nf;
    const size_t t = (size_t)t0 + (live ? r : 0);
    float *yr = s_yr[wv], *yi = s_yi[wv], *re = s_re[wv], *im = s_im[wv];
    // magnitude substitution, LogSpec2Wav.c:481-494, 683-696
    for (int k = lane; k < d.D; k += 64) {
        float v = live ? src[(size_t)(live ? r : 0) * (MASK ? 2 * d.D : d.D) + k] : 0.0f;
        if (MASK) {
            if (GV) {
                v = gv_rule::apply(v, eta[k], inv[k], mean[k]);
            } else {
                const float q = v / inv[k];
                v = q + mean[k];
            }
            if (live && mk.mode == mask_rule::kSelect)
                v = mask_rule::select(mk.noisy[t * d.D + k], v, src[(size_t)r * (2 * d.D) + d.D + k], mk.scale, mk.lo,
                                      mk.hi);
            if (lps_den && live) lps_den[t * d.D + k] = v;
        } else if (GV) {  // always de-normalising: the factors belong to the net's outputs
            v = gv_rule::apply(v, eta[k], inv[k], mean[k]);
            if (lps_den && live) lps_den[t * d.D + k] = v;
        } else if (mean) {
            const float q = v / inv[k];
            v = q + mean[k];
            if (lps_den && live) lps_den[t * d.D + k] = v;
        }
        const float ph = (v < SPEC_FLOOR) ? floor_exp : (float)exp((double)v);
        const float mag = sqrtf(ph);
        const float2 x = live ? X[t * d.D + k] : make_float2(0.0f, 0.0f);
        const float A = sqrtf(x.x * x.x + x.y * x.y);
        float or_ = mag, oi = 0.0f;  // |X| = 0 (digital silence): phase 0
        if (A > 0.0f) {
            const float g = mag / A;
            or_ = x.x * g;
            oi = x.y * g;
        }
        yr[k] = or_;
        yi[k] = oi;
    }
    __syncthreads();
    // inverse split: Z_k = A_k + i B_k, A_k = (Y_k + conj Y_{M-k}) / 2, B_k = conj(W_N^k) (Y_k - conj Y_{M-k}) / 2,
    // loaded conjugated and bit-reversed for the forward butterflies
    for (int k = lane; k < d.M; k += 64) {
        const float ar = yr[k], ai = yi[k], cr = yr[d.M - k], ci = -yi[d.M - k];
        const float er = (ar + cr) * 0.5f, ei = (ai + ci) * 0.5f;
        const float dr = (ar - cr) * 0.5f, di = (ai - ci) * 0.5f;
        const float2 w = tws[k];
        const float br = w.x * dr + w.y * di, bi = w.x * di - w.y * dr;  // conj(W) (dr + i di)
        const float zr = er - bi, zi = ei + br;                            // A + i B
        const int p = spec_pad(spec_bitrev(k, d.logM));
        re[p] = zr;
        im[p] = -zi;
    }
    __syncthreads();
    spec_fft_rows(re, im, tw, d.M, d.logM, lane);
    if (!live) return;
    const float scale = 1.0f / (float)d.M;  // a power of two: exact
    for (int n = lane; n < d.L; n += 64) {
        const int m = n >> 1;
        const float v = (n & 1) ? -im[spec_pad(m)] * scale : re[spec_pad(m)] * scale;  // rifft divides by N
        blk[t * d.L + n] = v * win[n];                                                  // OLA_KIND 1: window again
    }
}

__global__ void __launch_bounds__(64 * SPEC_FRAMES) k_lps_synthesis(const float *__restrict__ src, const float *__restrict__ mean,
                                                                    const float *__restrict__ inv, const float2 *__restrict__ X,
                                                                    int t0, int nf, SpecDims d, const float *__restrict__ win,
                                                                    const float2 *__restrict__ tw,
                                                                    const float2 *__restrict__ tws, float floor_exp,
                                                                    float *__restrict__ blk, float *__restrict__ lps_den) {
    lps_synthesis_frames<false>(src, mean, inv, nullptr, X, t0, nf, d, win, tw, tws, floor_exp, blk, lps_den);
}

// the same with the global variance equalisation factors eta [D] of the engine (mlggd_set_gv); mean and inv are given
__global__ void __launch_bounds__(64 * SPEC_FRAMES) k_lps_synthesis_gv(
    const float *__restrict__ src, const float *__restrict__ mean, const float *__restrict__ inv,
    const float *__restrict__ eta, const float2 *__restrict__ X, int t0, int nf, SpecDims d,
    const float *__restrict__ win, const float2 *__restrict__ tw, const float2 *__restrict__ tws, float floor_exp,
    float *__restrict__ blk, float *__restrict__ lps_den) {
    lps_synthesis_frames<true>(src, mean, inv, eta, X, t0, nf, d, win, tw, tws, floor_exp, blk, lps_den);
}

// a mask engine's decode: src rows of 2 D outputs, the post-filter of mask_rule.h (MaskArgs above), without and with
// the equalisation factors eta, of which the first D are read.  Defined in mask.hip.h.
__global__ void __launch_bounds__(64 * SPEC_FRAMES) k_lps_synthesis_mask(
    const float *__restrict__ src, const float *__restrict__ mean, const float *__restrict__ inv,
    const float2 *__restrict__ X, int t0, int nf, SpecDims d, const float *__restrict__ win,
    const float2 *__restrict__ tw, const float2 *__restrict__ tws, float floor_exp, float *__restrict__ blk,
    float *__restrict__ lps_den, MaskArgs mk);
__global__ void __launch_bounds__(64 * SPEC_FRAMES) k_lps_synthesis_mask_gv(
    const float *__restrict__ src, const float *__restrict__ mean, const float *__restrict__ inv,
    const float *__restrict__ eta, const float2 *__restrict__ X, int t0, int nf, SpecDims d,
    const float *__restrict__ win, const float2 *__restrict__ tw, const float2 *__restrict__ tws, float floor_exp,
    float *__restrict__ blk, float *__restrict__ lps_den, MaskArgs mk);

// One thread per output sample i of F S + L - S: the frames that cover it, in frame order, then / sum w^2 (formed in
// the same order, LogSpec2Wav.c:799-826).  int16 out = trunc toward zero, saturated.
__global__ void k_ola(const float *__restrict__ blk, int F, SpecDims d, const float *__restrict__ win,
                      float *__restrict__ out_f, int16_t *__restrict__ out_i, int n_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    int lo = i - d.L + 1;
    lo = lo <= 0 ? 0 : (lo + d.S - 1) / d.S;
    int hi = i / d.S;
    if (hi > F - 1) hi = F - 1;
    float acc = 0.0f, cnt = 0.0f;
    for (int t = lo; t <= hi; t++) {
        const int j = i - t * d.S;
        acc += blk[(size_t)t * d.L + j];
        cnt += win[j] * win[j];
    }
    const float v = acc / cnt;
    if (out_f) out_f[i] = v;
    const float c = truncf(v);
    out_i[i] = (int16_t)(c >= 32767.0f ? 32767 : (c <= -32768.0f ? -32768 : (int)c));
}

// k_ola over a packed batch: output sample i belongs to the utterance u with out_off[u] <= i < out_off[u + 1]; the
// frames that cover it are clamped to that utterance's F_u frames (time blocks frame_off[u] ..), summed in frame order
// and divided by sum w^2 formed in the same order, as k_ola does.
__global__ void k_ola_seg(const float *__restrict__ blk, const int *__restrict__ frame_off,
                          const long long *__restrict__ out_off, int n_utts, SpecDims d, const float *__restrict__ win,
                          float *__restrict__ out_f, int16_t *__restrict__ out_i, long long n_out) {
    const long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= n_out) return;
    int ul = 0, uh = n_utts - 1;
    while (ul < uh) {
        const int mid = (ul + uh + 1) >> 1;
        if (out_off[mid] <= gi) ul = mid;
        else uh = mid - 1;
    }
    const int fo = frame_off[ul], F = frame_off[ul + 1] - fo;
    const int i = (int)(gi - out_off[ul]);
    int lo = i - d.L + 1;
    lo = lo <= 0 ? 0 : (lo + d.S - 1) / d.S;
    int hi = i / d.S;
    if (hi > F - 1) hi = F - 1;
    float acc = 0.0f, cnt = 0.0f;
    for (int t = lo; t <= hi; t++) {
        const int j = i - t * d.S;
        acc += blk[(size_t)(fo + t) * d.L + j];
        cnt += win[j] * win[j];
    }
    const float v = acc / cnt;
    if (out_f) out_f[gi] = v;
    const float c = truncf(v);
    out_i[gi] = (int16_t)(c >= 32767.0f ? 32767 : (c <= -32768.0f ? -32768 : (int)c));
}
