// optfile.h -- the state of the Adam optimizer (mlggd_set_optimizer, csrc/adam_rule.h) as a binary file, so that the
// trainer can carry it from one epoch's process to the next (MLGGD_OPT_FILE=PATH, read in train_options.cc): a .wts file holds
// weights only.  Also behind mlggd_read_optimizer_header / mlggd_read_optimizer_state / mlggd_write_optimizer_state.
// Not in the reference: the 28-key command line, the log file and the weights' format (binfile.h) do not change.  No
// dependency on mlggd.h.
//
// Little-endian throughout, no padding:
//   u32  magic     'M' 'L' 'O' 'P' (0x504F4C4D)
//   u32  version   1
//   i32  numlayers L (>= 0; the net's layer count, input layer included)
//   i32  layersizes[L]
//   f32  beta1, beta2, eps
//   i64  steps     updates taken so far
//   then for l = 1 .. L - 1:  f32 m_w[K N], v_w[K N] (row-major [K][N], K = layersizes[l - 1], N = layersizes[l]),
//                             f32 m_b[N], v_b[N]
// The moments are the engine's unpadded, in the shapes mlggd_get_weights uses.  A reader is told the layer sizes it
// expects; a file for another net is refused with both lists in the message, and so are a file that ends early (the
// field it ends in is named), bytes behind the last array, another magic or version, a negative step count, a beta
// outside [0, 1), an eps that is not finite or not positive.  Every refusal is *err = "PATH: what is wrong".
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace mlggd_host {

constexpr uint32_t kOptMagic = 0x504F4C4Du, kOptVersion = 1u;
constexpr int kOptMaxLayers = 64;  // of a file: nothing larger is ever written, and a reader allocates by this count

struct OptState {
    std::vector<int> layersizes;  // [L]
    float beta1 = 0.9f, beta2 = 0.999f, eps = 1e-8f;
    long long steps = 0;
    std::vector<std::vector<float>> m_w, v_w, m_b, v_b;  // [L - 1] each: layer l at index l - 1
};

inline bool optfile_bad(const std::string &path, const std::string &what, std::string *err) {
    *err = path + ": " + what;
    return false;
}
inline std::string optfile_sizes(const int *ls, int L) {
    std::string s;
    for (int l = 0; l < L; l++) s += (l ? "," : "") + std::to_string(ls[l]);
    return L > 0 ? s : std::string("(no layers)");
}
inline bool optfile_host_le() {
    const uint32_t one = 1;
    unsigned char b[4];
    memcpy(b, &one, 4);
    return b[0] == 1;
}
inline void optfile_put32(unsigned char *b, uint32_t v) {
    for (int i = 0; i < 4; i++) b[i] = (unsigned char)(v >> (8 * i));
}
inline uint32_t optfile_get32(const unsigned char *b) {
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}
inline uint32_t optfile_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
inline float optfile_float(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}
// floats of the arrays behind the header
inline unsigned long long optfile_body_floats(const int *ls, int L) {
    unsigned long long n = 0;
    for (int l = 1; l < L; l++) n += 2ull * (unsigned long long)ls[l - 1] * (unsigned long long)ls[l] + 2ull * (unsigned long long)ls[l];
    return n;
}

// m_w .. v_b: [L] pointers with slot 0 unused, like mlggd_get_weights
inline bool write_opt_state(const std::string &path, int L, const int *ls, float beta1, float beta2, float eps, long long steps,
                            const float *const *m_w, const float *const *v_w, const float *const *m_b, const float *const *v_b,
                            std::string *err) {
    if (!optfile_host_le()) return optfile_bad(path, "the arrays are written as the host holds them: a little-endian host is required", err);
    if (L < 0 || L > kOptMaxLayers) return optfile_bad(path, std::to_string(L) + " layers: 0 .. " + std::to_string(kOptMaxLayers) + " can be written", err);
    if (steps < 0) return optfile_bad(path, "steps " + std::to_string(steps) + " < 0", err);
    for (int l = 0; l < L; l++)
        if (ls[l] < 1) return optfile_bad(path, "layersizes[" + std::to_string(l) + "] = " + std::to_string(ls[l]) + " < 1", err);
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp) return optfile_bad(path, "cannot write the file", err);
    std::vector<unsigned char> h((size_t)(3 + L + 3 + 2) * 4);
    size_t o = 0;
    auto put = [&](uint32_t v) { optfile_put32(&h[o], v), o += 4; };
    put(kOptMagic), put(kOptVersion), put((uint32_t)L);
    for (int l = 0; l < L; l++) put((uint32_t)ls[l]);
    put(optfile_bits(beta1)), put(optfile_bits(beta2)), put(optfile_bits(eps));
    put((uint32_t)((unsigned long long)steps & 0xFFFFFFFFull)), put((uint32_t)((unsigned long long)steps >> 32));
    bool ok = fwrite(h.data(), 1, h.size(), fp) == h.size();
    for (int l = 1; l < L && ok; l++) {
        const size_t kn = (size_t)ls[l - 1] * ls[l], n = (size_t)ls[l];
        ok = fwrite(m_w[l], 4, kn, fp) == kn && fwrite(v_w[l], 4, kn, fp) == kn && fwrite(m_b[l], 4, n, fp) == n &&
             fwrite(v_b[l], 4, n, fp) == n;
    }
    if (fclose(fp) != 0 || !ok) return optfile_bad(path, "cannot write the file", err);
    return true;
}
inline bool write_opt_state(const std::string &path, const OptState &s, std::string *err) {
    const int L = (int)s.layersizes.size();
    const size_t nl = L > 0 ? (size_t)L - 1 : 0;
    if (s.m_w.size() != nl || s.v_w.size() != nl || s.m_b.size() != nl || s.v_b.size() != nl)
        return optfile_bad(path, "a state of " + std::to_string(L) + " layers holds " + std::to_string(nl) + " arrays of each kind", err);
    std::vector<const float *> p[4];
    for (auto &q : p) q.assign((size_t)L + 1, nullptr);
    for (int l = 1; l < L; l++) {
        const size_t kn = (size_t)s.layersizes[l - 1] * s.layersizes[l], n = (size_t)s.layersizes[l];
        if (s.m_w[l - 1].size() != kn || s.v_w[l - 1].size() != kn || s.m_b[l - 1].size() != n || s.v_b[l - 1].size() != n)
            return optfile_bad(path, "the arrays of layer " + std::to_string(l) + " do not have the layer's sizes", err);
        p[0][l] = s.m_w[l - 1].data(), p[1][l] = s.v_w[l - 1].data(), p[2][l] = s.m_b[l - 1].data(), p[3][l] = s.v_b[l - 1].data();
    }
    return write_opt_state(path, L, s.layersizes.data(), s.beta1, s.beta2, s.eps, s.steps, p[0].data(), p[1].data(), p[2].data(),
                           p[3].data(), err);
}

// The header of `fp` into s (layersizes, betas, eps, steps), every field checked; *body: the floats that must follow.
inline bool read_opt_header(FILE *fp, const std::string &path, OptState *s, unsigned long long *body, std::string *err) {
    unsigned char b[4];
    auto get = [&](const char *field, uint32_t *v) {
        if (fread(b, 1, 4, fp) != 4) return optfile_bad(path, std::string("the file ends inside ") + field, err);
        *v = optfile_get32(b);
        return true;
    };
    uint32_t v = 0, lo = 0, hi = 0;
    if (!get("the magic word", &v)) return false;
    if (v != kOptMagic) return optfile_bad(path, "not an optimizer state file (the magic word differs)", err);
    if (!get("the version", &v)) return false;
    if (v != kOptVersion) return optfile_bad(path, "version " + std::to_string(v) + ", this reader knows version " + std::to_string(kOptVersion), err);
    if (!get("the layer count", &v)) return false;
    if (v > (uint32_t)kOptMaxLayers) return optfile_bad(path, "layer count " + std::to_string((int32_t)v) + " not in 0 .. " + std::to_string(kOptMaxLayers), err);
    s->layersizes.assign(v, 0);
    for (size_t l = 0; l < s->layersizes.size(); l++) {
        if (!get("the layer sizes", &v)) return false;
        if ((int32_t)v < 1) return optfile_bad(path, "layersizes[" + std::to_string(l) + "] = " + std::to_string((int32_t)v) + " < 1", err);
        s->layersizes[l] = (int32_t)v;
    }
    if (!get("beta1", &v)) return false;
    s->beta1 = optfile_float(v);
    if (!get("beta2", &v)) return false;
    s->beta2 = optfile_float(v);
    if (!get("eps", &v)) return false;
    s->eps = optfile_float(v);
    if (!get("steps", &lo) || !get("steps", &hi)) return false;
    s->steps = (long long)(((unsigned long long)hi << 32) | lo);
    if (!(s->beta1 >= 0.0f && s->beta1 < 1.0f) || !(s->beta2 >= 0.0f && s->beta2 < 1.0f))
        return optfile_bad(path, "beta1 " + std::to_string(s->beta1) + ", beta2 " + std::to_string(s->beta2) + ": both must lie in [0, 1)", err);
    if (!std::isfinite(s->eps) || !(s->eps > 0.0f)) return optfile_bad(path, "eps " + std::to_string(s->eps) + " is not finite or not positive", err);
    if (s->steps < 0) return optfile_bad(path, "steps " + std::to_string(s->steps) + " < 0", err);
    *body = optfile_body_floats(s->layersizes.data(), (int)s->layersizes.size());
    return true;
}
inline bool read_opt_header(const std::string &path, OptState *s, std::string *err) {
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) return optfile_bad(path, "cannot read the file", err);
    unsigned long long body = 0;
    const bool ok = read_opt_header(fp, path, s, &body, err);
    fclose(fp);
    return ok;
}

// The whole state.  expect_ls != nullptr: the layer sizes of the run; a file for another net is refused naming both.
// The file's length is checked against the header BEFORE anything is allocated for the arrays.
inline bool read_opt_state(const std::string &path, const int *expect_ls, int expect_L, OptState *s, std::string *err) {
    if (!optfile_host_le()) return optfile_bad(path, "the arrays are read as the host holds them: a little-endian host is required", err);
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) return optfile_bad(path, "cannot read the file", err);
    struct Close {
        FILE *f;
        ~Close() { fclose(f); }
    } closer{fp};
    unsigned long long body = 0;
    if (!read_opt_header(fp, path, s, &body, err)) return false;
    const int L = (int)s->layersizes.size();
    if (expect_ls) {
        bool same = L == expect_L;
        for (int l = 0; same && l < L; l++) same = s->layersizes[l] == expect_ls[l];
        if (!same)
            return optfile_bad(path, "the state is of a net with layer sizes " + optfile_sizes(s->layersizes.data(), L) +
                                         ", this run's net has " + optfile_sizes(expect_ls, expect_L), err);
    }
    const long at = ftell(fp);
    if (at < 0 || fseek(fp, 0, SEEK_END) != 0) return optfile_bad(path, "cannot read the file", err);
    const long end = ftell(fp);
    if (end < 0 || fseek(fp, at, SEEK_SET) != 0) return optfile_bad(path, "cannot read the file", err);
    const unsigned long long have = (unsigned long long)(end - at);
    if (have < body * 4ull)
        return optfile_bad(path, "the file ends inside the moments: " + std::to_string(have) + " bytes behind the header, " +
                                     std::to_string(body * 4ull) + " belong there", err);
    if (have > body * 4ull)
        return optfile_bad(path, std::to_string(have - body * 4ull) + " bytes behind the last array", err);
    const size_t nl = L > 0 ? (size_t)L - 1 : 0;
    s->m_w.assign(nl, {}), s->v_w.assign(nl, {}), s->m_b.assign(nl, {}), s->v_b.assign(nl, {});
    for (int l = 1; l < L; l++) {
        const size_t kn = (size_t)s->layersizes[l - 1] * s->layersizes[l], n = (size_t)s->layersizes[l];
        s->m_w[l - 1].resize(kn), s->v_w[l - 1].resize(kn), s->m_b[l - 1].resize(n), s->v_b[l - 1].resize(n);
        if (fread(s->m_w[l - 1].data(), 4, kn, fp) != kn || fread(s->v_w[l - 1].data(), 4, kn, fp) != kn ||
            fread(s->m_b[l - 1].data(), 4, n, fp) != n || fread(s->v_b[l - 1].data(), 4, n, fp) != n)
            return optfile_bad(path, "the file ends inside the moments of layer " + std::to_string(l), err);
    }
    return true;
}

}  // namespace mlggd_host
