// adam_rule_main.cc -- csrc/adam_rule.h and host/optfile.h as a stand-alone host program (tests/test_adam_model.py builds it
// with -fsanitize=address,undefined and runs it; it is never loaded into Python).
//
//   adam_rule_main DIR < lines
//
// stdin, every float as the 8 hex digits of its bits:
//   S w m v G wc nf lr b1 b2 eps STEPS_BEFORE   ->  "S w' m' v'"     one weight, one update (adam_rule::step)
//   T lr b1 b2 STEPS                            ->  "T a_t"          adam_rule::stepsize
//   V b1 b2 eps                                 ->  "V 0|1"          adam_rule::valid
// Then, in DIR, the state file: a state of zero layers and one of a single layer (no arrays) go round; a two-layer state
// goes round with steps = INT64_MAX; the file cut after every byte count up to its header's end -- so inside every
// header field -- and inside the arrays is refused with a message that names the place; a file with bytes behind the
// last array, another magic, another version and a file for another net (both size lists named) are refused.  The last
// line is "adam_rule_main OK".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "adam_rule.h"
#include "optfile.h"

static float f_of(const char *hex) {
    const uint32_t u = (uint32_t)strtoul(hex, nullptr, 16);
    float f;
    memcpy(&f, &u, 4);
    return f;
}
static unsigned bits_of(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}
#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) {                                                         \
            fprintf(stderr, "line %d: %s does not hold\n", __LINE__, #c);   \
            return 1;                                                       \
        }                                                                   \
    } while (0)

static std::vector<unsigned char> slurp(const std::string &p) {
    std::vector<unsigned char> b;
    FILE *fp = fopen(p.c_str(), "rb");
    if (!fp) return b;
    int c;
    while ((c = fgetc(fp)) != EOF) b.push_back((unsigned char)c);
    fclose(fp);
    return b;
}
static bool spit(const std::string &p, const std::vector<unsigned char> &b, size_t n) {
    FILE *fp = fopen(p.c_str(), "wb");
    if (!fp) return false;
    const bool ok = n == 0 || fwrite(b.data(), 1, n, fp) == n;
    return fclose(fp) == 0 && ok;
}

static int file_checks(const std::string &dir) {
    using namespace mlggd_host;
    std::string err;
    // zero layers, and one layer: a header and nothing else
    for (int L = 0; L <= 1; L++) {
        OptState s, r;
        if (L) s.layersizes = {7};
        s.steps = 3;
        const std::string p = dir + "/empty" + std::to_string(L) + ".opt";
        REQUIRE(write_opt_state(p, s, &err));
        REQUIRE(read_opt_state(p, s.layersizes.data(), L, &r, &err));
        REQUIRE(r.layersizes == s.layersizes && r.steps == 3 && r.m_w.empty() && r.v_b.empty());
        REQUIRE(slurp(p).size() == (size_t)(3 + L + 3 + 2) * 4);
    }
    // two weight layers, steps at the far end
    OptState s;
    s.layersizes = {3, 5, 2};
    s.beta1 = 0.5f, s.beta2 = 0.75f, s.eps = 1e-6f, s.steps = INT64_MAX;
    for (int l = 1; l < 3; l++) {
        const size_t kn = (size_t)s.layersizes[l - 1] * s.layersizes[l], n = (size_t)s.layersizes[l];
        std::vector<float> a(kn), b(kn), c(n), d(n);
        for (size_t i = 0; i < kn; i++) a[i] = (float)i - 3.5f * l, b[i] = 0.25f * (float)i * l;
        for (size_t i = 0; i < n; i++) c[i] = -(float)i, d[i] = (float)(i + l);
        s.m_w.push_back(a), s.v_w.push_back(b), s.m_b.push_back(c), s.v_b.push_back(d);
    }
    const std::string p = dir + "/two.opt";
    REQUIRE(write_opt_state(p, s, &err));
    OptState r;
    REQUIRE(read_opt_state(p, s.layersizes.data(), 3, &r, &err));
    REQUIRE(r.layersizes == s.layersizes && r.steps == INT64_MAX && r.beta1 == 0.5f && r.beta2 == 0.75f && r.eps == 1e-6f);
    REQUIRE(r.m_w == s.m_w && r.v_w == s.v_w && r.m_b == s.m_b && r.v_b == s.v_b);
    OptState h;
    REQUIRE(read_opt_header(p, &h, &err) && h.layersizes == s.layersizes && h.steps == INT64_MAX && h.m_w.empty());
    REQUIRE(read_opt_state(p, nullptr, 0, &r, &err));  // no expectation: any net
    // cut: every length short of the whole file
    const std::vector<unsigned char> whole = slurp(p);
    const size_t header = (size_t)(3 + 3 + 3 + 2) * 4;
    REQUIRE(whole.size() == header + 4 * (2 * (15 + 10) + 2 * (5 + 2)));
    const std::string q = dir + "/cut.opt";
    for (size_t n = 0; n < whole.size(); n++) {
        REQUIRE(spit(q, whole, n));
        err.clear();
        REQUIRE(!read_opt_state(q, s.layersizes.data(), 3, &r, &err));
        REQUIRE(err.find(q + ": ") == 0 && err.find("the file ends inside") != std::string::npos);
        const char *field = n < 4 ? "the magic word" : n < 8 ? "the version" : n < 12 ? "the layer count" : n < 24 ? "the layer sizes"
                            : n < 28 ? "beta1" : n < 32 ? "beta2" : n < 36 ? "eps" : n < 44 ? "steps" : "the moments";
        REQUIRE(err.find(field) != std::string::npos);
        if (n < header) REQUIRE(!read_opt_header(q, &h, &err));
    }
    // bytes behind the last array, another magic, another version
    std::vector<unsigned char> more = whole;
    more.push_back(0);
    REQUIRE(spit(q, more, more.size()) && !read_opt_state(q, s.layersizes.data(), 3, &r, &err));
    REQUIRE(err.find("1 bytes behind the last array") != std::string::npos);
    more = whole, more[0] ^= 1;
    REQUIRE(spit(q, more, more.size()) && !read_opt_state(q, s.layersizes.data(), 3, &r, &err));
    REQUIRE(err.find("magic") != std::string::npos);
    more = whole, more[4] = 2;
    REQUIRE(spit(q, more, more.size()) && !read_opt_state(q, s.layersizes.data(), 3, &r, &err));
    REQUIRE(err.find("version 2") != std::string::npos);
    more = whole, more[8] = 0xFF, more[9] = 0xFF, more[10] = 0xFF, more[11] = 0x7F;  // a layer count no reader allocates for
    REQUIRE(spit(q, more, more.size()) && !read_opt_state(q, s.layersizes.data(), 3, &r, &err));
    REQUIRE(err.find("layer count") != std::string::npos);
    more = whole, more[43] = 0x80;  // steps < 0
    REQUIRE(spit(q, more, more.size()) && !read_opt_state(q, s.layersizes.data(), 3, &r, &err));
    REQUIRE(err.find("steps") != std::string::npos);
    // another net: both lists are named
    const int other[3] = {3, 6, 2};
    REQUIRE(!read_opt_state(p, other, 3, &r, &err));
    REQUIRE(err.find("3,5,2") != std::string::npos && err.find("3,6,2") != std::string::npos);
    REQUIRE(!read_opt_state(p, other, 2, &r, &err) && err.find("3,6") != std::string::npos);
    REQUIRE(!read_opt_state(dir + "/none.opt", other, 3, &r, &err) && err.find("cannot read") != std::string::npos);
    // the step size at the far end: the loop ends when the products are spent
    const float a = adam_rule::stepsize(0.001f, 0.9f, 0.999f, INT64_MAX);
    REQUIRE(a == 0.001f);
    REQUIRE(adam_rule::stepsize(0.001f, 0.0f, 0.0f, INT64_MAX) == 0.001f);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: adam_rule_main DIR < lines\n");
        return 2;
    }
    char line[512];
    while (fgets(line, sizeof(line), stdin)) {
        char w[16][32];
        const int n = sscanf(line, "%31s %31s %31s %31s %31s %31s %31s %31s %31s %31s %31s %31s", w[0], w[1], w[2], w[3], w[4], w[5],
                             w[6], w[7], w[8], w[9], w[10], w[11]);
        if (n < 1) continue;
        if (w[0][0] == 'S' && n == 12) {
            const float b1 = f_of(w[8]), b2 = f_of(w[9]);
            const long long before = atoll(w[11]);
            const adam_rule::Consts c = adam_rule::consts(f_of(w[6]), f_of(w[7]), b1, b2, f_of(w[10]),
                                                          adam_rule::products(b1, b2, before == INT64_MAX ? before : before + 1));
            const adam_rule::Moments r = adam_rule::step(f_of(w[1]), f_of(w[2]), f_of(w[3]), f_of(w[4]), f_of(w[5]), c);
            printf("S %08x %08x %08x\n", bits_of(r.w), bits_of(r.m), bits_of(r.v));
        } else if (w[0][0] == 'T' && n == 5) {
            printf("T %08x\n", bits_of(adam_rule::stepsize(f_of(w[1]), f_of(w[2]), f_of(w[3]), atoll(w[4]))));
        } else if (w[0][0] == 'V' && n == 4) {
            printf("V %d\n", adam_rule::valid(f_of(w[1]), f_of(w[2]), f_of(w[3])) ? 1 : 0);
        } else {
            fprintf(stderr, "bad line: %s", line);
            return 2;
        }
    }
    if (file_checks(argv[1]) != 0) return 1;
    printf("adam_rule_main OK\n");
    return 0;
}
