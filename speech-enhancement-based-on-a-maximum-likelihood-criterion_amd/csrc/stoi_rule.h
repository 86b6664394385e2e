// stoi_rule.h -- the host-side rules of STOI on the device (mlggd_stoi_layout, mlggd_stoi_waves; stoi.hip.h): the
// resampling ratio of a rate, the lengths and frame counts of an utterance, the resampling filter, the analysis window
// and the third-octave band table.  Host only: plain C++ with no device call.
//
// Taal, Hendriks, Heusdens, Jensen, "An Algorithm for Intelligibility Prediction of Time-Frequency Weighted Noisy
// Speech", IEEE TASL 2011: 10 kHz, frames of 256 at hop 128, 512-point spectra, 15 third-octave bands from 150 Hz,
// segments of 30 frames, clipping at -15 dB, 40 dB of dynamic range for the silent-frame removal.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

namespace stoi_rule {

constexpr int kN = 256, kK = 128, kFft = 512, kBands = 15, kSeg = 30;
// a wave is indexed in int on the device: its samples stay below this (live_rule::kMaxSamples)
constexpr int64_t kMaxSamples = INT32_MAX - 1024;

// band j sums the power of the bins lo <= k < hi: the original script's thirdoct() at 10 kHz / 512
// (tests/test_stoi_model.py derives the table from that rule)
constexpr int kBandLo[kBands] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174};
constexpr int kBandHi[kBands] = {9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

// fs -> 10 kHz is resampling by p / q ("11" is 11 000 Hz); slot = the rate's index in per-rate tables
inline bool rate(int fs_khz, int *p, int *q, int *slot) {
    switch (fs_khz) {
        case 8: *p = 5, *q = 4, *slot = 0; return true;
        case 11: *p = 10, *q = 11, *slot = 1; return true;
        case 16: *p = 5, *q = 8, *slot = 2; return true;
    }
    return false;
}

inline int half_taps(int p, int q) { return 10 * (p > q ? p : q); }

inline int64_t len10(int64_t n, int p, int q) { return (n * p + q - 1) / q; }

// frame starts 0, K, 2K, ... <= length - N - 1 (the original's 1:K:(len-N))
inline int64_t frames(int64_t length) { return length <= kN ? 0 : (length - kN - 1) / kK + 1; }

// frames of the kept frames overlap-added at hop K: (kept - 1) K + N samples framed by the same rule
inline int64_t compacted(int64_t kept) { return kept > 0 ? frames((kept - 1) * kK + kN) : 0; }

inline int64_t segments(int64_t compacted_frames) { return compacted_frames >= kSeg ? compacted_frames - (kSeg - 1) : 0; }

inline double bessel_i0(double x) {  // sum ((x/2)^k / k!)^2
    double term = 1.0, s = 1.0;
    for (int k = 1; k < 60; k++) {
        term = term * (x / 2.0) / k;
        s = s + term * term;
    }
    return s;
}

// h[t + Lh], t = -Lh..Lh: 2 fc sinc(2 fc t) kaiser(2 Lh + 1, 5)[t + Lh], fc = 1 / (2 max(p, q)), scaled to sum p; in
// double, rounded to float
inline std::vector<float> filter(int p, int q) {
    const int Lh = half_taps(p, q);
    const double fc = 1.0 / (2.0 * (p > q ? p : q));
    std::vector<double> h(2 * Lh + 1);
    double sum = 0.0;
    for (int t = -Lh; t <= Lh; t++) {
        const double a = M_PI * 2.0 * fc * t, r = (double)t / Lh;
        const double sinc = t == 0 ? 1.0 : sin(a) / a;
        const double root = 1.0 - r * r;
        h[t + Lh] = 2.0 * fc * sinc * bessel_i0(5.0 * sqrt(root > 0.0 ? root : 0.0)) / bessel_i0(5.0);
        sum += h[t + Lh];
    }
    std::vector<float> out(h.size());
    for (size_t i = 0; i < h.size(); i++) out[i] = (float)(h[i] * ((double)p / sum));
    return out;
}

// w[n] = 0.5 (1 - cos(2 pi (n + 1) / (N + 1))): the open Hann window of the original script
inline std::vector<float> window() {
    std::vector<float> w(kN);
    for (int n = 0; n < kN; n++) w[n] = (float)(0.5 * (1.0 - cos(2.0 * M_PI * (n + 1) / (kN + 1))));
    return w;
}

}  // namespace stoi_rule
