// live.hip.h -- the kernels of a live group (mlggd_live_push): sessions decoded block by block with their state
// resident on the device.  Included by engine.hip after spectral.hip.h, whose analysis (k_lps_analysis_seg) and
// synthesis (k_lps_synthesis) kernels a push runs unchanged on compact per-push buffers.
//
// Resident state per session slot, shift-down buffers in two copies (a push reads one copy and writes the other, so no
// kernel reads a row that another workgroup of the same launch overwrites; the host flips the copy after the push):
//   tail [L]            int16  the unconsumed samples, from the next frame's first sample on (fewer than L)
//   lps  [ctx - 1][D]   float  LPS rows of frames max(0, T - half) .. A - 1: left context of frame T + analysed frames
//                              not yet decoded (A analysed, T decoded; A - T <= half while the session runs)
//   X    [half][D]      float2 noisy spectra of frames T .. A - 1
//   blk  [K][L]         float  time blocks of frames max(0, T - K) .. T - 1, K = ceil(L / S) - 1: the decoded frames
//                              that still cover samples not yet emitted
// Row 0 of each buffer is the oldest frame it holds.  Every count, offset and clamp comes from the host's own
// counters (LiveSess and the offset tables of one push); no kernel keeps a counter.
//
// Per element the kernels run the operation sequences of k_lps_stream and k_ola: the same bits as the single call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spectral.hip.h"

// one session's push; frame indices are those of its recording
struct LiveSess {
    long long in_off;  // its new samples in the uploaded block
    int p, a;          // resident tail samples, new samples: its window is tail[0 .. p) then the a new ones
    int cut;           // window samples the new frames consume (new frames x S): the new tail starts there
    int T0, A0;        // decoded / analysed frames before the push
    int T1, A1;        // ... after it
    int keep;          // 0: the push ends the session and nothing is carried
    int nf_off;        // first row of its new frames in the push's lps / X
    int dec_off;       // first row of its decoded frames in the push's X / time blocks
};

// the largest u in [0, n) with off[u] <= g; off is non-decreasing and g < off[n], so that entry is not empty
template <typename T>
__device__ __forceinline__ int live_find(const T *__restrict__ off, int n, T g) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Each session's sample window = its resident tail, then its part of the uploaded block, packed at win_off[u]; and the
// tail it leaves behind: the window from `cut` on.  One thread per window sample.
__global__ void k_live_window(const int16_t *__restrict__ in, const int16_t *__restrict__ tail_old,
                              int16_t *__restrict__ tail_new, const LiveSess *__restrict__ sess,
                              const long long *__restrict__ win_off, int n_sessions, int L, int16_t *__restrict__ win,
                              long long total) {
    const long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= total) return;
    const int u = live_find(win_off, n_sessions, gi);
    const LiveSess s = sess[u];
    const int q = (int)(gi - win_off[u]);
    const int16_t v = q < s.p ? tail_old[(size_t)u * L + q] : in[s.in_off + (q - s.p)];
    win[gi] = v;
    if (s.keep && q >= s.cut) tail_new[(size_t)u * L + (q - s.cut)] = v;
}

// The forward pass's input for the packed decoded frames [a, a + n) of a push, which belong to the decoding sessions
// dk0..dk1 (dk_off: their first packed frame, strictly increasing; dk_slot: their slots).  As in k_lps_stream_seg a
// session contributes the rows of its frames in the chunk plus ctx - 1 context rows: its section starts at row
// rs(k) = max(dk_off[k], a) - a + (k - dk0) (ctx - 1), and sample i starts at first[i] = i + (k - dk0) (ctx - 1).
// Row frame t is clamped to [0, A1 - 1]: the left clamp acts only at the recording's frame 0; the right one only in the
// push that ends the session (a running session decodes no frame beyond A1 - 1 - half).  Rows of frames below A0 are
// resident, the others were analysed in this push.  (lps - mean) * inv: the two operations of k_lps_stream.
__global__ void k_live_stream(const float *__restrict__ lps_res, const float *__restrict__ lps_new,
                              const LiveSess *__restrict__ sess, const int *__restrict__ dk_off,
                              const int *__restrict__ dk_slot, int n_dk, int D, int a, int n, int dk0, int dk1, int ctx,
                              const float *__restrict__ mean, const float *__restrict__ inv,
                              float *__restrict__ stream, int *__restrict__ first) {
    const int r = blockIdx.x, half = (ctx - 1) / 2;
    if (r < n && threadIdx.x == 0) first[r] = r + (live_find(dk_off, n_dk, a + r) - dk0) * (ctx - 1);
    int lo = dk0, hi = dk1;  // the largest k with rs(k) <= r
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const int fo = dk_off[mid];
        if ((fo > a ? fo : a) - a + (mid - dk0) * (ctx - 1) <= r) lo = mid;
        else hi = mid - 1;
    }
    const int k = lo, fo = dk_off[k], slot = dk_slot[k];
    const LiveSess s = sess[slot];
    const int ga = fo > a ? fo : a;
    int t = s.T0 + (ga - fo) - half + (r - (ga - a + (k - dk0) * (ctx - 1)));
    t = t < 0 ? 0 : (t >= s.A1 ? s.A1 - 1 : t);
    const int base = s.T0 > half ? s.T0 - half : 0;  // the frame of resident row 0
    const float *src = t < s.A0 ? lps_res + ((size_t)slot * (ctx - 1) + (t - base)) * D
                                : lps_new + (size_t)(s.nf_off + (t - s.A0)) * D;
    float *dst = stream + (size_t)r * D;
    for (int j = threadIdx.x; j < D; j += blockDim.x) {
        const float c = src[j] - mean[j];
        dst[j] = c * inv[j];
    }
}

// The noisy spectra of the packed decoded frames, in decoding order, for k_lps_synthesis: resident rows (frames below
// A0) and rows analysed in this push.  One workgroup per decoded frame.
__global__ void k_live_gather_x(const float2 *__restrict__ X_res, const float2 *__restrict__ X_new,
                                const LiveSess *__restrict__ sess, const int *__restrict__ dk_off,
                                const int *__restrict__ dk_slot, int n_dk, int D, int half, float2 *__restrict__ X_dec) {
    const int g = blockIdx.x;
    const int k = live_find(dk_off, n_dk, g), slot = dk_slot[k];
    const LiveSess s = sess[slot];
    const int f = s.T0 + (g - dk_off[k]);
    const float2 *src = f < s.A0 ? X_res + ((size_t)slot * half + (f - s.T0)) * D
                                 : X_new + (size_t)(s.nf_off + (f - s.A0)) * D;
    float2 *dst = X_dec + (size_t)g * D;
    for (int j = threadIdx.x; j < D; j += blockDim.x) dst[j] = src[j];
}

// One thread per emitted sample: sample i = T0 S + (its position in the session's part of the output) of the
// recording, the frames that cover it summed in frame order from the carried time blocks (frames below T0) and the
// push's own, then / sum w^2 formed in the same order, as k_ola does.  hi never exceeds T1 - 1: the last decoded frame,
// which for an ended session is its last frame (k_ola's clamp) and for a running one covers every emitted sample.
__global__ void k_live_ola(const float *__restrict__ blk_res, const float *__restrict__ blk_new,
                           const LiveSess *__restrict__ sess, const long long *__restrict__ out_off, int n_sessions,
                           int K, SpecDims d, const float *__restrict__ win, float *__restrict__ out_f,
                           int16_t *__restrict__ out_i, long long n_out) {
    const long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gi >= n_out) return;
    const int u = live_find(out_off, n_sessions, gi);
    const LiveSess s = sess[u];
    const int i = s.T0 * d.S + (int)(gi - out_off[u]);
    int lo = i - d.L + 1;
    lo = lo <= 0 ? 0 : (lo + d.S - 1) / d.S;
    int hi = i / d.S;
    if (hi > s.T1 - 1) hi = s.T1 - 1;
    const int base = s.T0 > K ? s.T0 - K : 0;  // the frame of carried block 0
    float acc = 0.0f, cnt = 0.0f;
    for (int t = lo; t <= hi; t++) {
        const int j = i - t * d.S;
        acc += t < s.T0 ? blk_res[((size_t)u * K + (t - base)) * d.L + j]
                        : blk_new[(size_t)(s.dec_off + (t - s.T0)) * d.L + j];
        cnt += win[j] * win[j];
    }
    const float v = acc / cnt;
    if (out_f) out_f[gi] = v;
    const float c = truncf(v);
    out_i[gi] = (int16_t)(c >= 32767.0f ? 32767 : (c <= -32768.0f ? -32768 : (int)c));
}

// The state the push leaves behind, written to the other copy: one workgroup per (slot, row) of the ctx - 1 LPS rows,
// the half X rows and the K time blocks.  A row of the new state is a frame; it comes from the old copy or from the
// push's buffers, whichever holds that frame.  Sessions the push did not touch are copied as they are.
__global__ void k_live_carry(const LiveSess *__restrict__ sess, int ctx, int K, int D, int L,
                             const float *__restrict__ lps_old, const float *__restrict__ lps_new,
                             float *__restrict__ lps_next, const float2 *__restrict__ X_old,
                             const float2 *__restrict__ X_new, float2 *__restrict__ X_next,
                             const float *__restrict__ blk_old, const float *__restrict__ blk_new,
                             float *__restrict__ blk_next) {
    const int half = (ctx - 1) / 2, RL = ctx - 1, per = RL + half + K;
    const int u = blockIdx.x / per;
    int j = blockIdx.x % per;
    const LiveSess s = sess[u];
    if (!s.keep) return;
    if (j < RL) {
        const int lo0 = s.T0 > half ? s.T0 - half : 0, lo1 = s.T1 > half ? s.T1 - half : 0;
        const int f = lo1 + j;
        if (f >= s.A1) return;
        const float *src = f < s.A0 ? lps_old + ((size_t)u * RL + (f - lo0)) * D
                                    : lps_new + (size_t)(s.nf_off + (f - s.A0)) * D;
        float *dst = lps_next + ((size_t)u * RL + j) * D;
        for (int i = threadIdx.x; i < D; i += blockDim.x) dst[i] = src[i];
        return;
    }
    j -= RL;
    if (j < half) {
        const int f = s.T1 + j;
        if (f >= s.A1) return;
        const float2 *src = f < s.A0 ? X_old + ((size_t)u * half + (f - s.T0)) * D
                                     : X_new + (size_t)(s.nf_off + (f - s.A0)) * D;
        float2 *dst = X_next + ((size_t)u * half + j) * D;
        for (int i = threadIdx.x; i < D; i += blockDim.x) dst[i] = src[i];
        return;
    }
    j -= half;
    const int lo0 = s.T0 > K ? s.T0 - K : 0, lo1 = s.T1 > K ? s.T1 - K : 0;
    const int f = lo1 + j;
    if (f >= s.T1) return;
    const float *src = f < s.T0 ? blk_old + ((size_t)u * K + (f - lo0)) * L
                                : blk_new + (size_t)(s.dec_off + (f - s.T0)) * L;
    float *dst = blk_next + ((size_t)u * K + j) * L;
    for (int i = threadIdx.x; i < L; i += blockDim.x) dst[i] = src[i];
}
