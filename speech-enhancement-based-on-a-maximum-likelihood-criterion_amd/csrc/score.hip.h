// score.hip.h -- the quality report of the original project's LPS2Wav_be (LogSpec2Wav.c:597-613, 700-712, 747-797,
// 828-842; host/tool_io.h quality()) on the device: segmental SNR and log-spectral distortion of enhanced LPS rows
// against the clean wave, per utterance of a packed batch.  Included by engine.hip after spectral.hip.h, whose
// helpers (tables, FFT butterflies, the analysis of one frame, the packed frame lookup) it calls; no kernel of that
// file changes.
//
//   k_score_frames  one wavefront per packed frame g = local frame t of utterance u (SPEC_FRAMES frames per workgroup,
//                   as the spectral kernels): the clean frame's spectrum Xc (spec_analysis_frame, the operations of
//                   k_lps_analysis), pd = exp(lps) floored at exp(-50), the enhanced spectrum with the noisy phase and
//                   its inverse FFT exactly as k_lps_synthesis forms them, the de-windowed frame against the clean
//                   samples -> snr[g]; and the frame's maxima of pc = |Xc|^2 and of pd.
//   k_score_utt     one workgroup per utterance: the 1e-5 floors from the maxima of its scored frames, the
//                   log-spectral distance of every scored frame, and the two means.
//
// Everything is fp32 with the log10 and the exp evaluated in double and rounded, as the spectral kernels do.  Every
// reduction is a fixed tree: a lane's strided partial sum in index order, a 64-lane xor butterfly (both operands of
// each addition are the same pair in every lane, so all lanes hold the same bits), per-wave partials over the frames
// t = wave, wave + SCORE_UTT_WAVES, ... in frame order, and a halving tree over the waves.  The order depends on the
// local indices t, k, n and on the number of scored frames alone, so an utterance's two numbers are a function of that
// utterance: bit-identical whatever its neighbours, its position, the batch, the chunking and the run.  No atomics.
#pragma once
#include "spectral.hip.h"

#define SCORE_UTT_WAVES 16  // wavefronts of a k_score_utt workgroup

__device__ __forceinline__ float score_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ float score_wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// pd of one bin, the expression of k_lps_synthesis
__device__ __forceinline__ float score_pd(float v, float floor_exp) {
    return (v < SPEC_FLOOR) ? floor_exp : (float)exp((double)v);
}

// grid: ceil(F / SPEC_FRAMES) workgroups of 64 * SPEC_FRAMES threads.  clean is packed like the noisy wave (utterance
// u from wave_off[u]); lps / X / Xc rows and snr / maxc / maxd entries are indexed by the packed frame g.  A frame
// t >= score_frames[u] (score_frames NULL: none) is not scored: its wave takes part in the barriers and writes nothing.
__global__ void __launch_bounds__(64 * SPEC_FRAMES) k_score_frames(
    const int16_t *__restrict__ clean, const long long *__restrict__ wave_off, const int *__restrict__ frame_off,
    const int *__restrict__ utt_of, const int *__restrict__ score_frames, int n_utts, int F, SpecDims d,
    const float *__restrict__ win, const float2 *__restrict__ tw, const float2 *__restrict__ tws, float floor_p,
    float floor_exp, const float *__restrict__ lps, const float2 *__restrict__ X, float2 *Xc, float *__restrict__ snr,
    float *__restrict__ maxc, float *__restrict__ maxd) {
    __shared__ float s_yr[SPEC_FRAMES][SPEC_MAXM + 1], s_yi[SPEC_FRAMES][SPEC_MAXM + 1];
    __shared__ float s_re[SPEC_FRAMES][SPEC_ROW], s_im[SPEC_FRAMES][SPEC_ROW];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = blockIdx.x * SPEC_FRAMES + wv;
    const int gg = g < F ? g : 0;
    const int u = seg_of_frame(frame_off, n_utts, utt_of, gg);
    const int tl = gg - frame_off[u];
    const bool live = g < F && (!score_frames || tl < score_frames[u]);
    const size_t t = (size_t)gg;
    const int16_t *x = clean + wave_off[u] + (size_t)tl * d.S;  // clean frame tl: inside the utterance
    float *yr = s_yr[wv], *yi = s_yi[wv], *re = s_re[wv], *im = s_im[wv];
    // clean spectrum: row t of Xc, read back below by other lanes of this wave (after the barrier)
    spec_analysis_frame(x, live, t, d, win, tw, tws, floor_p, nullptr, Xc, re, im, lane);
    __syncthreads();
    // enhanced power, its noisy-phase spectrum (k_lps_synthesis' magnitude substitution), and the frame maxima
    float mc = 0.0f, md = 0.0f;
    for (int k = lane; k < d.D; k += 64) {
        float or_ = 0.0f, oi = 0.0f;
        if (live) {
            const float2 c = Xc[t * d.D + k];
            mc = fmaxf(mc, c.x * c.x + c.y * c.y);
            const float ph = score_pd(lps[t * d.D + k], floor_exp);
            md = fmaxf(md, ph);
            const float mag = sqrtf(ph);
            const float2 xn = X[t * d.D + k];
            const float A = sqrtf(xn.x * xn.x + xn.y * xn.y);
            or_ = mag;  // |X| = 0 (digital silence): phase 0
            if (A > 0.0f) {
                const float q = mag / A;
                or_ = xn.x * q;
                oi = xn.y * q;
            }
        }
        yr[k] = or_;
        yi[k] = oi;
    }
    __syncthreads();
    // inverse split, loaded conjugated and bit-reversed for the forward butterflies (as k_lps_synthesis)
    for (int k = lane; k < d.M; k += 64) {
        const float ar = yr[k], ai = yi[k], cr = yr[d.M - k], ci = -yi[d.M - k];
        const float er = (ar + cr) * 0.5f, ei = (ai + ci) * 0.5f;
        const float dr = (ar - cr) * 0.5f, di = (ai - ci) * 0.5f;
        const float2 w = tws[k];
        const float br = w.x * dr + w.y * di, bi = w.x * di - w.y * dr;
        const float zr = er - bi, zi = ei + br;
        const int p = spec_pad(spec_bitrev(k, d.logM));
        re[p] = zr;
        im[p] = -zi;
    }
    __syncthreads();
    spec_fft_rows(re, im, tw, d.M, d.logM, lane);
    if (!live) return;
    // the de-windowed frame (DeWindow: the first L samples / w) against the clean samples
    const float scale = 1.0f / (float)d.M;
    float s1 = 0.0f, s2 = 0.0f;
    for (int n = lane; n < d.L; n += 64) {
        const int m = n >> 1;
        const float v = (n & 1) ? -im[spec_pad(m)] * scale : re[spec_pad(m)] * scale;
        const float c = (float)x[n], e = v / win[n] - c;
        s1 += c * c;
        s2 += e * e;
    }
    s1 = score_wave_sum(s1);
    s2 = score_wave_sum(s2);
    mc = score_wave_max(mc);
    md = score_wave_max(md);
    if (lane) return;
    // a silent clean frame: log10(0) = -inf -> -20; no error at all: +inf -> 30.  0 / 0 would stay NaN through both
    // compares, as on the host; it cannot occur: pd >= exp(-50) > 0 on every bin, so a silent clean frame has s2 > 0
    float v = 10.0f * (float)log10((double)(s1 / s2));
    if (v > 30.0f) v = 30.0f;
    if (v < -20.0f) v = -20.0f;
    snr[t] = v;
    maxc[t] = mc;
    maxd[t] = md;
}

// grid: n_utts workgroups of 64 * SCORE_UTT_WAVES threads.  Utterance u scores its first score_frames[u] frames (NULL:
// all of them); none: segsnr = lsd = 0.
__global__ void __launch_bounds__(64 * SCORE_UTT_WAVES) k_score_utt(
    const int *__restrict__ frame_off, const int *__restrict__ score_frames, int D, float floor_exp,
    const float *__restrict__ lps, const float2 *__restrict__ Xc, const float *__restrict__ snr,
    const float *__restrict__ maxc, const float *__restrict__ maxd, float *__restrict__ segsnr,
    float *__restrict__ lsd) {
    __shared__ float s_mc[SCORE_UTT_WAVES], s_md[SCORE_UTT_WAVES], s_snr[SCORE_UTT_WAVES], s_lsd[SCORE_UTT_WAVES];
    const int u = blockIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int fo = frame_off[u];
    const int Fs = score_frames ? score_frames[u] : frame_off[u + 1] - fo;
    if (Fs == 0) {  // the same in every thread
        if (threadIdx.x == 0) segsnr[u] = lsd[u] = 0.0f;
        return;
    }
    // the 50 dB floors: 1e-5 of the maxima over this utterance's scored frames
    float mc = 0.0f, md = 0.0f;
    for (int i = threadIdx.x; i < Fs; i += 64 * SCORE_UTT_WAVES) {
        mc = fmaxf(mc, maxc[fo + i]);
        md = fmaxf(md, maxd[fo + i]);
    }
    mc = score_wave_max(mc);
    md = score_wave_max(md);
    if (lane == 0) s_mc[wv] = mc, s_md[wv] = md;
    __syncthreads();
    mc = md = 0.0f;
    for (int i = 0; i < SCORE_UTT_WAVES; i++) {
        mc = fmaxf(mc, s_mc[i]);
        md = fmaxf(md, s_md[i]);
    }
    mc *= 1e-5f;
    md *= 1e-5f;
    // frames wv, wv + SCORE_UTT_WAVES, ...: one frame per wavefront at a time
    float acc_snr = 0.0f, acc_lsd = 0.0f;
    for (int t = wv; t < Fs; t += SCORE_UTT_WAVES) {
        const size_t row = (size_t)(fo + t) * D;
        float s = 0.0f;
        for (int k = lane; k < D; k += 64) {
            const float2 c = Xc[row + k];
            const float pc = c.x * c.x + c.y * c.y;
            const float pd = score_pd(lps[row + k], floor_exp);
            const float r = fmaxf(pd, md) / fmaxf(pc, mc);
            const float v = 10.0f * (float)log10((double)r);
            s += v * v;
        }
        s = score_wave_sum(s);
        acc_lsd += sqrtf(s / (float)D);
        acc_snr += snr[fo + t];
    }
    if (lane == 0) s_snr[wv] = acc_snr, s_lsd[wv] = acc_lsd;
    __syncthreads();
    if (threadIdx.x) return;
    for (int h = SCORE_UTT_WAVES / 2; h > 0; h >>= 1)
        for (int i = 0; i < h; i++) {
            s_snr[i] += s_snr[i + h];
            s_lsd[i] += s_lsd[i + h];
        }
    segsnr[u] = s_snr[0] / (float)Fs;
    lsd[u] = s_lsd[0] / (float)Fs;
}
