// spec_rule.h -- the layout rule of the spectral front end, host only: plain C++ with no device call, so that it also
// builds into a stand-alone program under the host sanitizers (tests/spec_rule_main.cc).  Every wave entry goes through
// it: the rate table, the frames of n samples, the tables of a packed batch and the utterances a decode chunk touches.
//
// A wave of n samples has F(n) = 0 frames if n < L, else (n - (L - S)) / S frames of L samples at a hop of S; F frames
// cover, and resynthesise to, F S + L - S samples.  A packed batch is offsets[n_utts + 1] into one int16 array.
// A check returns 0, or -1 with msg filled.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>

// at global scope: the kernels of spectral.hip.h take it by value
struct SpecDims {
    int L, S, N, M, logM, D;  // frame length, hop, FFT length, N/2, log2(M), N/2 + 1
};

namespace spec_rule {

// how a check of a *_rule.h header fails: the message goes to msg [cap], the check returns this -1
__attribute__((format(printf, 3, 4))) inline int refuse(char *msg, size_t cap, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, cap, fmt, ap);
    va_end(ap);
    return -1;
}

// the three rates (Wav2LogSpec_be.c / LogSpec2Wav.c #defines); slot (optional) numbers them 0, 1, 2
inline bool rate(int fs_khz, SpecDims *d, int *slot = nullptr) {
    int L, S, N, at;
    switch (fs_khz) {
        case 8: L = 256, S = 128, N = 256, at = 0; break;
        case 11: L = 256, S = 110, N = 256, at = 1; break;
        case 16: L = 512, S = 256, N = 512, at = 2; break;
        default: return false;
    }
    d->L = L, d->S = S, d->N = N, d->M = N / 2, d->D = N / 2 + 1;
    d->logM = 0;
    while ((1 << d->logM) < d->M) d->logM++;
    if (slot) *slot = at;
    return true;
}
inline bool rate(int fs_khz, int *L, int *S) {  // for a caller that wants the frame length and the hop alone
    SpecDims d;
    if (!rate(fs_khz, &d)) return false;
    *L = d.L, *S = d.S;
    return true;
}

inline int64_t frames(int L, int S, int64_t n) { return n < L ? 0 : (n - (L - S)) / S; }
inline int64_t frames(const SpecDims &d, int64_t n) { return frames(d.L, d.S, n); }
inline int64_t out_samples(int L, int S, int64_t F) { return F * S + L - S; }
inline int64_t out_samples(const SpecDims &d, int64_t F) { return out_samples(d.L, d.S, F); }

// what layout() makes of an utterance shorter than one frame
enum Short {
    kShortFails,  // an error: the decode and score entries
    kShortEmpty,  // an utterance without frames: the loaders, mlggd_lps_stats, mlggd_wave_samples
    kUnframed,    // nothing is cut into frames (STOI): only the offsets are checked, only wave_off is filled
};

// The tables of a packed batch, each [n_utts + 1] and each optional: frame_off (frames before utterance u), out_off
// (resynthesised samples before it) and wave_off (offsets re-based to offsets[0], what the kernels index the uploaded
// waves with).  n_utts = 0 gives the one 0 of each table and reads no offsets.
inline int layout(const SpecDims &d, int n_utts, const int64_t *offsets, Short policy, int32_t *frame_off,
                  long long *out_off, long long *wave_off, char *msg, size_t cap) {
    if (n_utts < 0) return refuse(msg, cap, "n_utts %d < 0", n_utts);
    if (frame_off) frame_off[0] = 0;
    if (out_off) out_off[0] = 0;
    if (wave_off) wave_off[0] = 0;
    if (n_utts == 0) return 0;
    if (!offsets) return refuse(msg, cap, "offsets is NULL");
    long long fsum = 0, osum = 0;
    for (int u = 0; u < n_utts; u++) {
        if (offsets[u + 1] < offsets[u])
            return refuse(msg, cap, "offsets decrease at utterance %d (%lld after %lld)", u, (long long)offsets[u + 1],
                          (long long)offsets[u]);
        if (wave_off) wave_off[u + 1] = (long long)offsets[u + 1] - (long long)offsets[0];
        if (policy == kUnframed) continue;
        const long long len = (long long)offsets[u + 1] - (long long)offsets[u];
        if (len < d.L && policy == kShortFails)
            return refuse(msg, cap, "utterance %d: %lld samples is shorter than one frame (%d)", u, len, d.L);
        const long long F = frames(d, len);
        fsum += F;
        if (F > 0) osum += out_samples(d, F);
        if (fsum > INT32_MAX)
            return refuse(msg, cap, "the batch has more than %d frames (reached at utterance %d)", INT32_MAX, u);
        if (frame_off) frame_off[u + 1] = (int32_t)fsum;
        if (out_off) out_off[u + 1] = osum;
    }
    return 0;
}

// every window of ctx frames from first_frame[s] on must lie inside one utterance of frame_off [n_utts + 1]; the
// message names the sample
inline int check_windows(int n_utts, const int32_t *frame_off, int ctx, int n_samples, const int32_t *first_frame,
                         char *msg, size_t cap) {
    const int FT = frame_off[n_utts];
    for (int s = 0; s < n_samples; s++) {
        const long long f = first_frame[s];
        if (f < 0 || f + ctx > FT)
            return refuse(msg, cap, "sample %d: window [%lld,%lld) outside the %d packed frames", s, f, f + ctx, FT);
        // the last u with frame_off[u] <= f: utterances without frames are stepped over
        const int u = (int)(std::upper_bound(frame_off, frame_off + n_utts + 1, (int32_t)f) - frame_off) - 1;
        if (f + ctx > frame_off[u + 1])
            return refuse(msg, cap, "sample %d: window [%lld,%lld) crosses the end of utterance %d at frame %d", s, f,
                          f + ctx, u, (int)frame_off[u + 1]);
    }
    return 0;
}

// the tables k_lps_analysis_seg reads, over the utterances that have frames (its search needs frame_off to increase):
// cf / cw hold up to n_utts + 1 entries; returns how many utterances they describe
inline int compact_tables(int n_utts, const int32_t *frame_off, const long long *wave_off, int32_t *cf, long long *cw) {
    int nc = 0;
    for (int u = 0; u < n_utts; u++)
        if (frame_off[u + 1] > frame_off[u]) {
            cf[nc] = frame_off[u];
            cw[nc++] = wave_off[u];
        }
    cf[nc] = frame_off[n_utts];
    cw[nc] = wave_off[n_utts];
    return nc;
}

// score_frames[u] (NULL: every frame) against the frames of the layout
inline int check_score_frames(int n_utts, const int32_t *frame_off, const int32_t *score_frames, char *msg,
                              size_t cap) {
    if (!score_frames) return 0;
    for (int u = 0; u < n_utts; u++) {
        const int Fu = frame_off[u + 1] - frame_off[u];
        if (score_frames[u] < 0 || score_frames[u] > Fu)
            return refuse(msg, cap, "utterance %d: score_frames %d is outside 0..%d, its frames", u,
                          (int)score_frames[u], Fu);
    }
    return 0;
}

// A decode chunk of the packed frames [a, a + n) over the segments of `off` (an increasing table: every segment has a
// frame, and a + n <= its last entry): the first and last segment it touches, and the rows of its stream -- its
// frames plus the ctx - 1 context rows of every segment touched.  *hint is the first segment of the chunk before
// (0 at the start); chunks are asked for in order and it moves along.
struct Span {
    int u0, u1, rows;
};
inline Span chunk_span(const int32_t *off, int *hint, int a, int n, int ctx) {
    while (off[*hint + 1] <= a) ++*hint;
    int u1 = *hint;
    while (off[u1 + 1] < a + n) u1++;
    return Span{*hint, u1, n + (u1 - *hint + 1) * (ctx - 1)};
}

}  // namespace spec_rule
