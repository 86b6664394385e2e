// nat_rule.h -- noise-aware training (Xu, Du, Dai and Lee 2014 / 2015): the noise row of an utterance and the layout of
// an input row, stated once for host and device (mlggd_nat_estimate, mlggd_nat_rows, k_nat_estimate,
// k_transpose_in_nat).  Plain C++ with no device call, so that it also builds into a stand-alone host program.
//
// A NAT engine has nat_frames = T >= 1.  An utterance u of F_u >= 1 frames uses its first T_u = min(T, F_u) frames.
// With x_t[k] = (lps_t[k] - mean[k]) * inv_std[k] -- two IEEE fp32 operations, the stream's own -- its noise row is
//   z_u[k] = (((x_0[k] + x_1[k]) + x_2[k]) + ... + x_{T_u - 1}[k]) / (float)T_u:
// the additions from left to right in fp32, then one fp32 division, nothing contracted (-ffp-contract=off).  An
// utterance without frames has a zero row.  The input row of a sample is its window of fea_context frames followed by
// the D values of its utterance's noise row: layersizes[0] = (fea_context + 1) * D.  Targets are unchanged.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NAT_HD __host__ __device__
#else
#define NAT_HD
#endif

namespace nat_rule {

NAT_HD inline int frames_used(int T, int F) { return F < T ? F : T; }

// width of a stream row of an engine whose layer 0 has K0 units: K0 / fea_context, or K0 / (fea_context + 1) with the
// noise row appended; 0 when it does not divide
NAT_HD inline int stream_width(int K0, int fea_context, bool nat) {
    const int parts = fea_context + (nat ? 1 : 0);
    return (fea_context < 1 || K0 % parts != 0) ? 0 : K0 / parts;
}

// z[k] of one (utterance, bin): x = bin k of the utterance's first normalised row, ld floats from row to row
NAT_HD inline float chain(const float *x, size_t ld, int Tu) {
    if (Tu < 1) return 0.0f;
    float s = x[0];
    for (int t = 1; t < Tu; t++) s = s + x[(size_t)t * ld];
    return s / (float)Tu;
}

// the same from raw LPS rows: every term is normalised by the stream's two operations first
NAT_HD inline float chain_lps(const float *lps, size_t ld, int Tu, float mean, float inv_std) {
    if (Tu < 1) return 0.0f;
    float s = (lps[0] - mean) * inv_std;
    for (int t = 1; t < Tu; t++) {
        const float x = (lps[(size_t)t * ld] - mean) * inv_std;
        s = s + x;
    }
    return s / (float)Tu;
}

// the utterance that holds packed frame f: the last u with frame_off[u] <= f (utterances without frames are stepped
// over); frame_off [n_utts + 1] is non-decreasing, 0 <= f < frame_off[n_utts]
inline int utt_of_frame(int n_utts, const int32_t *frame_off, int32_t f) {
    int lo = 0, hi = n_utts - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (frame_off[mid] <= f) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

}  // namespace nat_rule
