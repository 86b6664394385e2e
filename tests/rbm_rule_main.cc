// rbm_rule_main.cc -- the draws and the visible-bias arithmetic of CD-1 pre-training (csrc/rbm_rule.h) on tables, as a
// stand-alone host program: tests/test_rbm_rule.py builds it with AddressSanitizer + UBSan and compares every bit with
// the NumPy restatement of tests/rbm64.py.
//
// stdin, one row per line (fp32 values as the 8 hex digits of their bits, integers decimal):
//   "D seed step B N"               the draws of one step -> stdout "D r ..." (B N words)
//   "S r p"                         one sample            -> stdout "S s"
//   "U sum nf mom lr dc c"          one bias update       -> stdout "U dc' c'"
//   "T v0 v1"                       one frame's terms     -> stdout "T (v1 - v0) sqerr" (the second as a float64, 16 digits)
//   "V layer L visible"             mlggd_rbm_open's argument check -> stdout "V 0|1 0|1"
// rbm_rule::draws must give what rbm_rule::draw gives element by element; "rbm_rule_main OK" ends the output.
#include <inttypes.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "rbm_rule.h"

static float f(uint32_t u) {
    float v;
    memcpy(&v, &u, 4);
    return v;
}
static uint32_t u(float v) {
    uint32_t w;
    memcpy(&w, &v, 4);
    return w;
}

int main() {
    char kind;
    while (scanf(" %c", &kind) == 1) {
        uint32_t a[6];
        if (kind == 'D') {
            int B, N;
            if (scanf("%" SCNu32 " %" SCNu32 " %d %d", &a[0], &a[1], &B, &N) != 4 || B < 0 || N < 0 || B * N > (1 << 20)) return 2;
            std::vector<float> r((size_t)B * N);
            rbm_rule::draws(a[0], a[1], B, N, r.data());
            printf("D");
            for (int i = 0; i < B * N; i++) {
                if (u(r[i]) != u(rbm_rule::draw(a[0], a[1], (uint32_t)i)) || !(r[i] >= 0.0f && r[i] < 1.0f)) {
                    printf("\ndraws differs from draw at %d\n", i);
                    return 1;
                }
                printf(" %08x", u(r[i]));
            }
            printf("\n");
        } else if (kind == 'S') {
            if (scanf("%x %x", &a[0], &a[1]) != 2) return 2;
            printf("S %08x\n", u(rbm_rule::sample(f(a[0]), f(a[1]))));
        } else if (kind == 'U') {
            if (scanf("%x %x %x %x %x %x", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) != 6) return 2;
            float dc = f(a[4]), c = f(a[5]);
            rbm_rule::update_bias(f(a[0]), f(a[1]), f(a[2]), f(a[3]), &dc, &c);
            printf("U %08x %08x\n", u(dc), u(c));
        } else if (kind == 'T') {
            if (scanf("%x %x", &a[0], &a[1]) != 2) return 2;
            const double q = rbm_rule::sqerr_term(f(a[0]), f(a[1]));
            uint64_t w;
            memcpy(&w, &q, 8);
            printf("T %08x %016" PRIx64 "\n", u(rbm_rule::bias_term(f(a[0]), f(a[1]))), w);
        } else if (kind == 'V') {
            int layer, L, vis;
            if (scanf("%d %d %d", &layer, &L, &vis) != 3) return 2;
            printf("V %d %d\n", rbm_rule::valid_layer(layer, L) ? 1 : 0, rbm_rule::valid_visible(vis) ? 1 : 0);
        } else {
            return 2;
        }
    }
    printf("rbm_rule_main OK\n");
    return 0;
}
