// scale_rule_main.cc -- the learned GGD scale (csrc/scale_rule.h) on tables, as a stand-alone host program:
// tests/test_scale_rule.py builds it with AddressSanitizer + UBSan, feeds it tables and compares every bit with the NumPy
// float32 restatement of tests/scale_model.py.
//
// stdin, the bits of every fp32 value as 8 hex digits, one row per line:
//   "B s nf beta"               beta_s                                          -> stdout "B v2"
//   "R v2 q v eta mu vmax"      velocity, q = pow_or_self(alpha, beta) handed in -> stdout "R v'"
//   "A alpha ex"                advance, ex = exp_det(v') handed in              -> stdout "A alpha'"
//   "Z alpha"                   seeds                                           -> stdout "Z 0|1"
//   "V mode lrate momentum vmax" mlggd_set_scale_mode's argument check (mode decimal) -> stdout "V 0|1"
//   "P alpha"                   a state's alpha                                 -> stdout "P 0|1"
// After the last row the index functions are walked over a state of Dp = 40 padded bins: the four quarters of
// [2 copies][alpha, v][Dp] must tile 0 .. 4 Dp - 1 exactly once; "scale_rule_main OK" ends the output.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "scale_rule.h"

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
        if (kind == 'B') {
            if (scanf("%x %x %x", &a[0], &a[1], &a[2]) != 3) return 2;
            printf("B %08x\n", u(scale_rule::beta_s(f(a[0]), f(a[1]), f(a[2]))));
        } else if (kind == 'R') {
            if (scanf("%x %x %x %x %x %x", &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) != 6) return 2;
            printf("R %08x\n", u(scale_rule::velocity(f(a[0]), f(a[1]), f(a[2]), f(a[3]), f(a[4]), f(a[5]))));
        } else if (kind == 'A') {
            if (scanf("%x %x", &a[0], &a[1]) != 2) return 2;
            printf("A %08x\n", u(scale_rule::advance(f(a[0]), f(a[1]))));
        } else if (kind == 'Z') {
            if (scanf("%x", &a[0]) != 1) return 2;
            printf("Z %d\n", scale_rule::seeds(f(a[0])) ? 1 : 0);
        } else if (kind == 'V') {
            int mode;
            if (scanf("%d %x %x %x", &mode, &a[0], &a[1], &a[2]) != 4) return 2;
            printf("V %d\n", scale_rule::valid(mode, f(a[0]), f(a[1]), f(a[2])) ? 1 : 0);
        } else if (kind == 'P') {
            if (scanf("%x", &a[0]) != 1) return 2;
            printf("P %d\n", scale_rule::valid_alpha(f(a[0])) ? 1 : 0);
        } else {
            return 2;
        }
    }
    const size_t Dp = 40;
    std::vector<int> seen(4 * Dp, 0);
    for (int c = 0; c < 2; c++)
        for (size_t d = 0; d < Dp; d++) {
            seen.at(scale_rule::alpha_at(c, Dp, d))++;
            seen.at(scale_rule::velocity_at(c, Dp, d))++;
        }
    for (size_t i = 0; i < seen.size(); i++)
        if (seen[i] != 1) {
            printf("the state's layout does not tile: slot %zu is named %d times\n", i, seen[i]);
            return 1;
        }
    if (scale_rule::alpha_at(1, Dp, 0) != 2 * Dp || scale_rule::velocity_at(0, Dp, 0) != Dp) {
        printf("the state's layout is not [2 copies][alpha, v][Dp]\n");
        return 1;
    }
    printf("scale_rule_main OK\n");
    return 0;
}
