// mask_rule_main.cc -- the ratio-mask target and the mask post-filter (csrc/mask_rule.h) on tables, as a stand-alone host
// program: tests/test_mask_rule.py builds it with AddressSanitizer + UBSan, feeds it the tables of tests/mask64.py and
// compares every bit with the NumPy float32 restatement.
//
// stdin, the bits of every fp32 value as 8 hex digits, one row per line:
//   "T c y ex s"          a target row: ex is the exponential's value at half_diff(c, y), handed in because the header
//                         takes it as an argument                       -> stdout "T h t"
//   "S n x o s lo hi"     a post-filter row                              -> stdout "S v"
//   "V mode lo hi s"      mlggd_set_mask's argument check (mode decimal) -> stdout "V 0|1"
// After the last row select_rows runs over all S rows that share the first row's lo and hi with their mask formed as
// o / s, and must give the values already printed; "mask_rule_main OK" ends the output.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "mask_rule.h"

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
    std::vector<float> rn, rx, rm, rv;
    float lo0 = 0.0f, hi0 = 0.0f;
    while (scanf(" %c", &kind) == 1) {
        uint32_t a[6];
        if (kind == 'T') {
            if (scanf("%x %x %x %x", &a[0], &a[1], &a[2], &a[3]) != 4) return 2;
            const float h = mask_rule::half_diff(f(a[0]), f(a[1]));
            const float t = mask_rule::target(f(a[2]), f(a[3]));
            printf("T %08x %08x\n", u(h), u(t));
        } else if (kind == 'S') {
            if (scanf("%x %x %x %x %x %x", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) != 6) return 2;
            const float v = mask_rule::select(f(a[0]), f(a[1]), f(a[2]), f(a[3]), f(a[4]), f(a[5]));
            printf("S %08x\n", u(v));
            if (rn.empty()) lo0 = f(a[4]), hi0 = f(a[5]);
            if (u(lo0) == a[4] && u(hi0) == a[5]) {
                rn.push_back(f(a[0])), rx.push_back(f(a[1])), rm.push_back(f(a[2]) / f(a[3])), rv.push_back(v);
            }
        } else if (kind == 'V') {
            int mode;
            if (scanf("%d %x %x %x", &mode, &a[0], &a[1], &a[2]) != 4) return 2;
            printf("V %d\n", mask_rule::valid(mode, f(a[0]), f(a[1]), f(a[2])) ? 1 : 0);
        } else {
            return 2;
        }
    }
    std::vector<float> out(rn.size());
    const int D = 3;  // rows of 3: the remainder of the table is left out
    mask_rule::select_rows(D, rn.size() / D, rn.data(), rx.data(), rm.data(), lo0, hi0, out.data());
    for (size_t i = 0; i < rn.size() / D * D; i++)
        if (u(out[i]) != u(rv[i])) {
            printf("select_rows differs from select at row %zu\n", i);
            return 1;
        }
    printf("mask_rule_main OK\n");
    return 0;
}
