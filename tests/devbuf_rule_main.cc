// devbuf_rule_main.cc -- the capacity rule of the engine's raw buffer sets (csrc/devbuf_rule.h, what raw_set_acquire in
// csrc/engine.hip applies through DevBuf::grow) followed through a sequence of acquisitions, as a stand-alone host
// program: tests/test_devbuf_rule.py feeds it the call sequences of tests/test_gpu_engine_reuse.py.
//
// argv[1]: 1 for a NAT engine (every acquisition also sizes the noise table), else 0.  stdin: one acquisition per line,
// "rows ctx fdim n_nat".  The two sets alternate.  stdout, one line per call:
//   i set grew_feat grew_targ grew_nat   feat targ nat (set 0)   feat targ nat (set 1)
// feat and nat in floats, targ in rows, all after the call.
#include <stdio.h>
#include <stdlib.h>

#include "devbuf_rule.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    const bool nat_engine = atoi(argv[1]) != 0;
    struct Set {
        devbuf_rule::Cap feat, targ, nat;
    } sets[2];
    unsigned long long rows, ctx, fdim, n_nat;
    for (int i = 0; scanf("%llu %llu %llu %llu", &rows, &ctx, &fdim, &n_nat) == 4; i++) {
        Set &s = sets[i % 2];
        const size_t n_feat = devbuf_rule::raw_feat_floats(rows, ctx, fdim), n_targ = devbuf_rule::raw_rows(rows, ctx);
        const size_t n_tab = devbuf_rule::nat_floats(n_nat, fdim);
        const bool gf = s.feat.grow(n_feat, n_feat), gt = s.targ.grow(n_targ, n_targ);
        const bool gn = nat_engine && s.nat.grow(n_tab, n_tab);
        printf("%d %d %d %d %d", i, i % 2, (int)gf, (int)gt, (int)gn);
        for (const Set &q : sets) printf("  %zu %zu %zu", q.feat.cap, q.targ.cap, q.nat.cap);
        printf("\n");
    }
    return 0;
}
