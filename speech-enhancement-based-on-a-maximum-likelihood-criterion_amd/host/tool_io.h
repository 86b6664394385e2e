// tool_io.h -- file formats shared by the command-line tools (enhance_lps, enhance_wav, wav2lps, lps2wav): the
// trainer's .wts container, the norm file, big-endian HTK feature files, RIFF PCM16 / headerless 16-bit waves, and
// the quality report of LogSpec2Wav.c.  Header-only; each tool defines die().
#pragma once
#include <algorithm>
#include <cmath>
#include <complex>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../include/mlggd.h"

[[noreturn]] void die(const std::string &m);

namespace tool_io {

inline uint32_t bswap32(uint32_t v) { return __builtin_bswap32(v); }
inline uint16_t bswap16(uint16_t v) { return (uint16_t)((v >> 8) | (v << 8)); }

struct Htk {
    int nframes = 0, samp_period = 0, samp_size = 0, parm_kind = 0;
    std::vector<float> data;  // [nframes][samp_size/4]
};

inline Htk read_htk(const std::string &path) {  // readHTK_new.m, 'be'
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) die("cannot open " + path);
    uint32_t h[2];
    uint16_t s[2];
    if (fread(h, 4, 2, fp) != 2 || fread(s, 2, 2, fp) != 2) die("short HTK header in " + path);
    Htk f;
    f.nframes = (int)bswap32(h[0]);
    f.samp_period = (int)bswap32(h[1]);
    f.samp_size = bswap16(s[0]);
    f.parm_kind = bswap16(s[1]);
    const size_t n = (size_t)f.nframes * (f.samp_size / 4);
    std::vector<uint32_t> raw(n);
    if (f.nframes <= 0 || f.samp_size % 4 || fread(raw.data(), 4, n, fp) != n) die("bad HTK body in " + path);
    fclose(fp);
    f.data.resize(n);
    for (size_t i = 0; i < n; i++) {
        const uint32_t v = bswap32(raw[i]);
        memcpy(&f.data[i], &v, 4);
    }
    return f;
}

// sampPeriod 160000, sampSize 4 * dim, parmKind 9 (writeHTK_new.m; the header Wav2LPS_be writes); header = false:
// the body alone (Wav2LPS_be -noh)
inline void write_htk(const std::string &path, const float *data, int nframes, int dim, bool header = true) {
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp) die("cannot open " + path + " for writing");
    if (header) {
        const uint32_t h[2] = {bswap32((uint32_t)nframes), bswap32(160000u)};
        const uint16_t s[2] = {bswap16((uint16_t)(dim * 4)), bswap16(9)};
        fwrite(h, 4, 2, fp);
        fwrite(s, 2, 2, fp);
    }
    std::vector<uint32_t> raw((size_t)nframes * dim);
    for (size_t i = 0; i < raw.size(); i++) {
        uint32_t v;
        memcpy(&v, &data[i], 4);
        raw[i] = bswap32(v);
    }
    fwrite(raw.data(), 4, raw.size(), fp);
    fclose(fp);
}

// the trainer's .wts container (Interface.cc:484-516): layer sizes, W[l] / B[l] for l = 1..L-1 (slot 0 empty)
struct Model {
    std::vector<int> ls;
    std::vector<std::vector<float>> W{1}, B{1};
};

inline Model read_wts(const std::string &wts) {
    Model m;
    FILE *fp = fopen(wts.c_str(), "rb");
    if (!fp) die("cannot open " + wts);
    int32_t stat[5];
    char name[256];
    while (fread(stat, 4, 5, fp) == 5) {
        if (stat[4] < 1 || stat[4] > 255 || fread(name, 1, stat[4], fp) != (size_t)stat[4]) die("bad matrix header in " + wts);
        std::vector<float> a((size_t)stat[1] * stat[2]);
        if (fread(a.data(), 4, a.size(), fp) != a.size()) die("truncated matrix in " + wts);
        if (stat[1] != 1) {  // weights: mrows = out, ncols = in
            if (m.ls.empty()) m.ls.push_back(stat[2]);
            if (m.ls.back() != stat[2]) die("layer sizes in " + wts + " do not chain");
            m.ls.push_back(stat[1]);
            m.W.push_back(a);
        } else {
            m.B.push_back(a);
        }
    }
    fclose(fp);
    if (m.W.size() < 2 || m.W.size() != m.B.size() || (int)m.W.size() > MLGGD_MAXLAYER) die("unexpected matrix list in " + wts);
    return m;
}

// norm file (Interface.cc:373-399 layout: "vec N", N means, "vec N", N inverse std-devs)
inline void read_norm(const std::string &norm_file, int dim, std::vector<float> &mean, std::vector<float> &inv) {
    mean.assign(dim, 0.0f);
    inv.assign(dim, 0.0f);
    std::ifstream f(norm_file);
    if (!f) die("cannot open " + norm_file);
    std::string line;
    std::getline(f, line);
    for (int j = 0; j < dim; j++) { std::getline(f, line); mean[j] = (float)atof(line.c_str()); }
    std::getline(f, line);
    for (int j = 0; j < dim; j++) { std::getline(f, line); inv[j] = (float)atof(line.c_str()); }
}

// an engine for inference with the model (bunchsize frames per forward bunch)
// activation=sigmoid|relu of the decoders: the .wts container carries no such flag, so the decoder is told what the
// trainer was told.  Anything else ends the run here, before a device is opened.
inline int parse_activation(const std::string &v) {
    if (v == "sigmoid") return MLGGD_ACT_SIGMOID;
    if (v == "relu") return MLGGD_ACT_RELU;
    die("activation=" + v + ": must be sigmoid or relu");
}

// nat=T of the decoding tools: the net was trained noise-aware over the first T frames (mlggd_config.nat_frames)
inline int parse_nat(const std::string &v) {
    char *end = nullptr;
    const long t = strtol(v.c_str(), &end, 10);
    if (v.empty() || *end || t < 0 || t > 1000000) die("nat=" + v + ": must be a number of frames, 0 = off");
    return (int)t;
}

// gv=FILE [gv_mode=bin|shared] of the decoding tools: the global variance equalisation factors of the D output bins
// (mlggd_read_gv: a plain list or the file MLGGD_GVFILE wrote); without gv= no factors (an empty vector)
inline std::vector<float> read_gv_arg(const std::string &path, const std::string &mode, int D) {
    if (mode != "bin" && mode != "shared") die("gv_mode=" + mode + ": must be bin or shared");
    std::vector<float> eta;
    if (path.empty()) return eta;
    eta.resize(D);
    if (mlggd_read_gv(path.c_str(), D, mode == "shared", eta.data()) != MLGGD_OK) die(std::string("gv=") + mlggd_last_error());
    return eta;
}

// mask=select|off [mask_lo=] [mask_hi=] [mask_scale=] of enhance_wav: the net is a multi-objective one (csrc/mask_rule.h)
struct MaskArg {
    bool given = false;  // mask= was on the command line: the last layer holds the LPS and the mask
    int mode = MLGGD_MASK_SELECT;
    float lo = 0.25f, hi = 0.75f, scale = 1.0f;
};
inline int parse_mask_mode(const std::string &v) {
    if (v == "select") return MLGGD_MASK_SELECT;
    if (v == "off") return MLGGD_MASK_OFF;
    die("mask=" + v + ": must be select or off");
}
inline float parse_mask_value(const std::string &k, const std::string &v) {
    char *end = nullptr;
    const float x = strtof(v.c_str(), &end);
    if (v.empty() || *end) die(k + "=" + v + ": must be a number");
    return x;
}

inline mlggd_handle create_engine(const Model &m, int gpu, int bunch, int max_cache_frames = 0,
                                  int activation = MLGGD_ACT_SIGMOID, int nat_frames = 0, int mask_bins = 0) {
    const int L = (int)m.ls.size();
    mlggd_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.struct_size = sizeof(cfg);
    cfg.device = gpu;
    cfg.numlayers = L;
    for (int i = 0; i < L; i++) cfg.layersizes[i] = m.ls[i];
    cfg.bunchsize = bunch;
    cfg.shapefactor = 2.0f;
    cfg.max_cache_frames = max_cache_frames;
    cfg.activation = activation;
    cfg.nat_frames = nat_frames;
    cfg.mask_bins = mask_bins;
    std::vector<const float *> wp(L, nullptr), bp(L, nullptr);
    for (int l = 1; l < L; l++) { wp[l] = m.W[l].data(); bp[l] = m.B[l].data(); }
    mlggd_handle h = nullptr;
    if (mlggd_create(&cfg, wp.data(), bp.data(), &h) != MLGGD_OK) die(std::string("mlggd_create: ") + mlggd_last_error());
    return h;
}

// ---- waves
inline std::vector<uint8_t> read_file(const std::string &path) {
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) die("cannot open " + path);
    std::vector<uint8_t> d;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), fp)) > 0) d.insert(d.end(), buf, buf + n);
    fclose(fp);
    return d;
}

// headerless 16-bit samples in the machine's byte order, byte-swapped when swap (fileio.c ReadWave)
inline std::vector<int16_t> read_raw16(const std::string &path, bool swap) {
    const std::vector<uint8_t> d = read_file(path);
    std::vector<int16_t> w(d.size() / 2);
    memcpy(w.data(), d.data(), w.size() * 2);
    if (swap)
        for (auto &s : w) s = (int16_t)bswap16((uint16_t)s);
    return w;
}

inline uint32_t le32(const uint8_t *p) { return p[0] | (p[1] << 8) | (p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint16_t le16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }

// RIFF WAVE, PCM 16-bit mono; *rate receives the sample rate
inline std::vector<int16_t> read_wav(const std::string &path, int *rate) {
    const std::vector<uint8_t> d = read_file(path);
    if (d.size() < 12 || memcmp(d.data(), "RIFF", 4) || memcmp(d.data() + 8, "WAVE", 4)) die(path + ": not a RIFF WAVE file");
    size_t pos = 12;
    bool fmt = false;
    while (pos + 8 <= d.size()) {
        const uint32_t size = le32(&d[pos + 4]);
        const size_t body = pos + 8, end = std::min(d.size(), body + (size_t)size);
        if (!memcmp(&d[pos], "fmt ", 4)) {
            if (size < 16 || body + 16 > d.size()) die(path + ": short fmt chunk");
            if (le16(&d[body]) != 1 || le16(&d[body + 2]) != 1 || le16(&d[body + 14]) != 16)
                die(path + ": only PCM 16-bit mono RIFF WAVE is supported");
            *rate = (int)le32(&d[body + 4]);
            fmt = true;
        } else if (!memcmp(&d[pos], "data", 4)) {
            if (!fmt) die(path + ": data chunk before fmt chunk");
            std::vector<int16_t> w((end - body) / 2);
            for (size_t i = 0; i < w.size(); i++) w[i] = (int16_t)le16(&d[body + 2 * i]);
            return w;
        }
        pos = body + size + (size & 1);
    }
    die(path + ": no data chunk");
}

inline void write_wav(const std::string &path, const int16_t *w, size_t n, int rate) {
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp) die("cannot open " + path + " for writing");
    std::vector<uint8_t> h(44);
    auto put32 = [&](int at, uint32_t v) { for (int i = 0; i < 4; i++) h[at + i] = (uint8_t)(v >> (8 * i)); };
    auto put16 = [&](int at, uint16_t v) { h[at] = (uint8_t)v; h[at + 1] = (uint8_t)(v >> 8); };
    memcpy(&h[0], "RIFF", 4);
    put32(4, (uint32_t)(36 + 2 * n));
    memcpy(&h[8], "WAVEfmt ", 8);
    put32(16, 16);
    put16(20, 1);
    put16(22, 1);
    put32(24, (uint32_t)rate);
    put32(28, (uint32_t)rate * 2);
    put16(32, 2);
    put16(34, 16);
    memcpy(&h[36], "data", 4);
    put32(40, (uint32_t)(2 * n));
    fwrite(h.data(), 1, h.size(), fp);
    std::vector<uint8_t> b(2 * n);
    for (size_t i = 0; i < n; i++) { b[2 * i] = (uint8_t)w[i]; b[2 * i + 1] = (uint8_t)((uint16_t)w[i] >> 8); }
    fwrite(b.data(), 1, b.size(), fp);
    fclose(fp);
}

inline void write_raw16(const std::string &path, const int16_t *w, size_t n) {
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp) die("cannot open " + path + " for writing");
    fwrite(w, 2, n, fp);
    fclose(fp);
}

// 16 / 11 / 8 kHz from a sample rate in Hz (0 if none of them)
inline int rate_khz(int hz) { return hz == 16000 ? 16 : hz == 11000 ? 11 : hz == 8000 ? 8 : 0; }

inline void spectral_params(int fs_khz, int *L, int *S, int *N) {
    *L = fs_khz == 16 ? 512 : 256;
    *S = fs_khz == 16 ? 256 : fs_khz == 11 ? 110 : 128;
    *N = *L;
}

// ---- quality report of LogSpec2Wav.c (597-613, 700-712, 747-797, 828-842), in double on the host.  Not on the hot
// path; its own radix-2 FFT in double.
inline void fft64(std::vector<std::complex<double>> &a, bool inverse) {
    const size_t n = a.size();
    for (size_t i = 1, j = 0; i < n; i++) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        for (size_t i = 0; i < n; i += len)
            for (size_t k = 0; k < len / 2; k++) {
                const double ang = (inverse ? 2.0 : -2.0) * M_PI * (double)k / (double)len;
                const std::complex<double> w(cos(ang), sin(ang));
                const std::complex<double> u = a[i + k], v = a[i + k + len / 2] * w;
                a[i + k] = u + v;
                a[i + k + len / 2] = u - v;
            }
    }
    if (inverse)
        for (auto &x : a) x /= (double)n;
}

// segmental SNR (per frame clamped to [-20, 30]) and log-spectral distortion (50 dB floor) of the enhanced LPS rows
// lps [F][N/2+1] (F = the frames of min(clean, noisy)) against the clean wave
inline void quality(int fs_khz, const std::vector<int16_t> &clean, const std::vector<int16_t> &noisy, const float *lps,
                    int F, double *segsnr, double *lsd) {
    int L, S, N;
    spectral_params(fs_khz, &L, &S, &N);
    const int D = N / 2 + 1;
    std::vector<double> w(L);
    for (int i = 0; i < L / 2; i++) w[i] = (double)(float)(0.54 - 0.46 * cos(2.0 * M_PI * i / (L - 1)));
    for (int i = L / 2; i < L; i++) w[i] = w[L - 1 - i];
    std::vector<double> pc((size_t)F * D), pd((size_t)F * D);
    double snr_sum = 0.0;
    std::vector<std::complex<double>> xc(N), xn(N);
    for (int t = 0; t < F; t++) {
        for (int n = 0; n < N; n++) {
            xc[n] = n < L ? (double)clean[(size_t)t * S + n] * w[n] : 0.0;
            xn[n] = n < L ? (double)noisy[(size_t)t * S + n] * w[n] : 0.0;
        }
        fft64(xc, false);
        fft64(xn, false);
        for (int k = 0; k < D; k++) {
            const double v = lps[(size_t)t * D + k];
            const double ph = v < -50.0 ? exp(-50.0) : exp(v);
            pc[(size_t)t * D + k] = std::norm(xc[k]);
            pd[(size_t)t * D + k] = ph;
            const double a = std::abs(xn[k]);
            const std::complex<double> y = a > 0 ? xn[k] * (sqrt(ph) / a) : std::complex<double>(sqrt(ph), 0.0);
            xn[k] = y;
            if (k > 0 && k < N / 2) xn[N - k] = std::conj(y);
        }
        fft64(xn, true);
        double s1 = 0.0, s2 = 0.0;
        for (int n = 0; n < L; n++) {
            const double c = clean[(size_t)t * S + n], e = xn[n].real() / w[n] - c;  // de-windowed (DeWindow) vs clean
            s1 += c * c;
            s2 += e * e;
        }
        double v = 10.0 * log10(s1 / s2);
        if (v > 30.0) v = 30.0;
        if (v < -20.0) v = -20.0;
        snr_sum += v;
    }
    double mc = 0.0, md = 0.0;
    for (size_t i = 0; i < pc.size(); i++) { mc = std::max(mc, pc[i]); md = std::max(md, pd[i]); }
    mc *= 1e-5;
    md *= 1e-5;
    double lsd_sum = 0.0;
    for (int t = 0; t < F; t++) {
        double s = 0.0;
        for (int k = 0; k < D; k++) {
            const double v = 10.0 * log10(std::max(pd[(size_t)t * D + k], md) / std::max(pc[(size_t)t * D + k], mc));
            s += v * v;
        }
        lsd_sum += sqrt(s / D);
    }
    *segsnr = snr_sum / F;
    *lsd = lsd_sum / F;
}

inline void write_info(const std::string &path, double segsnr, double lsd) {
    FILE *fp = fopen(path.c_str(), "wt");
    if (!fp) die("cannot open " + path + " for writing");
    fprintf(fp, "Segmental SNR:\n%f\nLog-Spectral Distortion:\n%f\n", segsnr, lsd);
    fclose(fp);
}

}  // namespace tool_io
