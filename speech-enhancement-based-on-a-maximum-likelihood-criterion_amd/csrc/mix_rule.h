// mix_rule.h -- the rule by which clean speech and noise are mixed at an SNR (mlggd_mix_waves, mlggd_train_waves),
// stated once for host and device code: plain C++ with no device call, so that it also builds into a host program.
//
// Utterance u of `len` int16 samples names a segment [noise_lo, noise_lo + noise_len) of the packed noise and a start
// inside it; sample i is paired with noise[noise_lo + (noise_start + i) mod noise_len], so a segment shorter than the
// utterance wraps (a segment of one sample is legal).  Ec = sum clean^2 and En = sum noise^2 over exactly those pairs
// are 64-bit unsigned integers: a term is at most 2^30 and an utterance has fewer than 2^31 samples, so both sums are
// exact and their order is free.  gain = sqrt((double)Ec / (double)En) * r with r = 10^(-snr_db / 20) formed on the
// host (libm pow, in double); Ec == 0, En == 0 or r == 0 (snr_db = +inf) give gain 0, the noisy wave is the clean wave.
// noisy[i] = sat16(rint(clean[i] + gain * noise[.])): product and sum are two double operations (never fused), rint
// rounds to nearest even, sat16 clamps to [-32768, 32767]; `clipped` counts the samples the clamp changed.
#pragma once
#include <cmath>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#if defined(__HIPCC__)
#define MIX_HD __host__ __device__
#else
#define MIX_HD
#endif

namespace mix_rule {

// consecutive samples of one utterance that one workgroup of k_mix_energy / k_mix_apply handles
constexpr int kBlock = 4096;
// an utterance is indexed in int on the device and its energies must fit 64 bits
constexpr int64_t kMaxSamples = INT32_MAX;

// one workgroup's work: n <= kBlock samples of utterance u from packed index `at` on (clean and noisy are packed
// alike), first noise sample noise[lo + phase], phase = (noise_start + offset of the block in the utterance) mod len
struct Block {
    long long at, lo, len, phase;
    int n, u;
    int first, pad;  // first != 0: the utterance's first block (its lane 0 writes gain[u])
};

MIX_HD inline double gain(unsigned long long Ec, unsigned long long En, double r) {
    if (Ec == 0 || En == 0 || r == 0.0) return 0.0;
    const double q = (double)Ec / (double)En;  // the integers convert round-to-nearest
    return sqrt(q) * r;
}

// one sample; *clipped is incremented where the clamp changed the value
MIX_HD inline int16_t mix(int clean, int noise, double g, int *clipped) {
    const double p = g * (double)noise;
    const double s = (double)clean + p;
    double v = rint(s);
    if (v > 32767.0) {
        v = 32767.0;
        ++*clipped;
    } else if (v < -32768.0) {
        v = -32768.0;
        ++*clipped;
    }
    return (int16_t)(int)v;
}

// r = 10^(-snr_db / 20); false for NaN and -inf (no finite gain); +inf gives r = 0
inline bool ratio(double snr_db, double *r) {
    if (snr_db != snr_db || (snr_db < 0 && std::isinf(snr_db))) return false;
    *r = pow(10.0, -snr_db / 20.0);
    return std::isfinite(*r);
}

// the argument checks of a batch, before any device call; 0, or -1 with msg filled (it names the utterance)
inline int check(int n_utts, const int64_t *offsets, int64_t n_noise, const int64_t *noise_lo, const int64_t *noise_len,
                 const int64_t *noise_start, const double *snr_db, char *msg, size_t cap) {
    for (int u = 0; u < n_utts; u++) {
        if (offsets[u + 1] < offsets[u]) {
            snprintf(msg, cap, "offsets decrease at utterance %d (%lld after %lld)", u, (long long)offsets[u + 1],
                     (long long)offsets[u]);
            return -1;
        }
        if (offsets[u + 1] - offsets[u] > kMaxSamples) {
            snprintf(msg, cap, "utterance %d: %lld samples exceed the %lld one utterance may have", u,
                     (long long)(offsets[u + 1] - offsets[u]), (long long)kMaxSamples);
            return -1;
        }
        if (noise_len[u] < 1) {
            snprintf(msg, cap, "utterance %d: noise_len %lld < 1", u, (long long)noise_len[u]);
            return -1;
        }
        if (noise_lo[u] < 0 || noise_lo[u] > n_noise || noise_len[u] > n_noise - noise_lo[u]) {
            snprintf(msg, cap, "utterance %d: noise segment [%lld, %lld) is outside the %lld noise samples", u,
                     (long long)noise_lo[u], (long long)((unsigned long long)noise_lo[u] + (unsigned long long)noise_len[u]),
                     (long long)n_noise);
            return -1;
        }
        if (noise_start[u] < 0 || noise_start[u] >= noise_len[u]) {
            snprintf(msg, cap, "utterance %d: noise_start %lld is outside its segment of %lld samples", u,
                     (long long)noise_start[u], (long long)noise_len[u]);
            return -1;
        }
        double r;
        if (!ratio(snr_db[u], &r)) {
            snprintf(msg, cap, "utterance %d: snr_db %g has no finite gain", u, snr_db[u]);
            return -1;
        }
    }
    return 0;
}

}  // namespace mix_rule
