// live_sanitize.cc -- the host-only emission rule of a live group (csrc/live_rule.h, what mlggd_live_layout and
// mlggd_live_push compute their tables from) as a stand-alone program for AddressSanitizer + UBSan; driven by
// tests/test_live_sanitizers.py.  It walks every rate and context 1, 7, 11: lengths around every frame boundary cut
// into pushes every which way, groups of many sessions with NULL and given end flags, and the refused arguments, and
// checks the counts against the rule written out once more.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "live_rule.h"

static int fails = 0;
#define EXPECT(c)                                               \
    do {                                                        \
        if (!(c)) {                                             \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                            \
        }                                                       \
    } while (0)

static int64_t emitted(int L, int S, int half, int64_t n, bool ended) {
    const int64_t F = n < L ? 0 : (n - (L - S)) / S;
    if (ended) return F > 0 ? F * S + L - S : 0;
    return (F > half ? F - half : 0) * S;
}

int main() {
    char msg[256];
    unsigned seed = 12345;
    auto rnd = [&](unsigned m) {
        seed = seed * 1664525u + 1013904223u;
        return (seed >> 8) % m;
    };
    for (int fs : {8, 11, 16})
        for (int ctx : {1, 7, 11}) {
            int L = 0, S = 0;
            EXPECT(spec_rule::rate(fs, &L, &S));
            const int half = (ctx - 1) / 2;
            // one session, every length around the boundaries, random cuts; the counts telescope
            for (int k = 0; k <= half + 2; k++)
                for (int dlt = -1; dlt <= 1; dlt++) {
                    const int64_t n = L + (int64_t)k * S + dlt;
                    for (int rep = 0; rep < 8; rep++) {
                        int64_t had = 0, total = 0;
                        while (had < n) {
                            const int64_t add = rep == 0 ? n : (int64_t)rnd((unsigned)(2 * S + 1));
                            const int64_t a = add > n - had ? n - had : add;
                            const uint8_t end = had + a == n && rnd(2);
                            int64_t off[2];
                            EXPECT(live_rule::layout(fs, ctx, 1, &had, &a, &end, off, msg, sizeof msg) == 0);
                            EXPECT(off[0] == 0 && off[1] == emitted(L, S, half, had + a, end) - emitted(L, S, half, had, false));
                            total += off[1];
                            had += a;
                            if (end) had = -1;
                            if (had < 0) break;
                        }
                        if (had >= 0) {  // the end alone, in an empty push
                            const int64_t zero = 0;
                            const uint8_t end = 1;
                            int64_t off[2];
                            EXPECT(live_rule::layout(fs, ctx, 1, &had, &zero, &end, off, msg, sizeof msg) == 0);
                            total += off[1];
                        }
                        EXPECT(total == emitted(L, S, half, n, true));
                    }
                }
            // a group of many sessions in heap arrays of the exact size; end NULL and given
            for (int n_sessions : {1, 2, 63, 1024}) {
                std::vector<int64_t> had(n_sessions), add(n_sessions), off((size_t)n_sessions + 1);
                std::vector<uint8_t> end(n_sessions);
                for (int u = 0; u < n_sessions; u++) {
                    had[u] = rnd(40u * S), add[u] = rnd(3u * S), end[u] = rnd(4) == 0;
                }
                EXPECT(live_rule::layout(fs, ctx, n_sessions, had.data(), add.data(), end.data(), off.data(), msg, sizeof msg) == 0);
                int64_t sum = 0;
                for (int u = 0; u < n_sessions; u++) {
                    sum += emitted(L, S, half, had[u] + add[u], end[u]) - emitted(L, S, half, had[u], false);
                    EXPECT(off[u + 1] == sum);
                    const live_rule::Step st = live_rule::step(L, S, half, had[u], add[u], end[u]);
                    EXPECT(st.p0 >= 0 && st.p0 < L && st.p1 >= 0 && st.p1 < L && st.A1 >= st.A0 && st.T1 >= st.T0);
                    EXPECT(st.A0 - st.T0 <= half && (end[u] || st.A1 - st.T1 <= half));
                }
                EXPECT(live_rule::layout(fs, ctx, n_sessions, had.data(), add.data(), nullptr, off.data(), msg, sizeof msg) == 0);
                EXPECT(off[n_sessions] % S == 0);
            }
        }
    // refused arguments: each leaves a message, none reads or writes beyond its arrays
    int64_t had = 5, add = 3, off[2] = {0, 0};
    const int64_t neg = -1, big = live_rule::kMaxSamples;
    EXPECT(live_rule::layout(12, 7, 1, &had, &add, nullptr, off, msg, sizeof msg) == -1 && strstr(msg, "fs_khz 12"));
    EXPECT(live_rule::layout(16, 4, 1, &had, &add, nullptr, off, msg, sizeof msg) == -1 && strstr(msg, "odd"));
    EXPECT(live_rule::layout(16, -1, 1, &had, &add, nullptr, off, msg, sizeof msg) == -1);
    EXPECT(live_rule::layout(16, 7, 0, &had, &add, nullptr, off, msg, sizeof msg) == -1 && strstr(msg, "n_sessions"));
    EXPECT(live_rule::layout(16, 7, 1, nullptr, &add, nullptr, off, msg, sizeof msg) == -1 && strstr(msg, "NULL"));
    EXPECT(live_rule::layout(16, 7, 1, &had, nullptr, nullptr, off, msg, sizeof msg) == -1);
    EXPECT(live_rule::layout(16, 7, 1, &had, &add, nullptr, nullptr, msg, sizeof msg) == -1);
    EXPECT(live_rule::layout(16, 7, 1, &had, &neg, nullptr, off, msg, sizeof msg) == -1 && strstr(msg, "negative"));
    EXPECT(live_rule::layout(16, 7, 1, &neg, &add, nullptr, off, msg, sizeof msg) == -1);
    EXPECT(live_rule::layout(16, 7, 1, &big, &add, nullptr, off, msg, sizeof msg) == -1 && strstr(msg, "exceed"));
    EXPECT(live_rule::layout(16, 7, 1, &had, &big, nullptr, off, msg, sizeof msg) == -1);
    const int64_t most = big - had;
    EXPECT(live_rule::layout(16, 7, 1, &had, &most, nullptr, off, msg, sizeof msg) == 0 && off[1] > 0);
    char tiny[8];
    EXPECT(live_rule::layout(12, 7, 1, &had, &add, nullptr, off, tiny, sizeof tiny) == -1 && strlen(tiny) == 7);
    if (fails) return 1;
    printf("live_sanitize OK\n");
    return 0;
}
