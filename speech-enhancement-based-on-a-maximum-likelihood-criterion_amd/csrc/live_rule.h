// live_rule.h -- the emission rule of a live group (mlggd_live_layout, mlggd_live_push), host only: plain C++ with no
// device call, so that it also builds into a stand-alone program under the host sanitizers (tests/live_sanitize.cc).
//
// A session that has received n samples has analysed F(n) frames, the frame count of the offline calls.  While it
// runs it has decoded T = max(0, F(n) - half) of them (frame t needs the rows up to t + half) and emitted T S samples;
// the push that ends it decodes the rest against the right edge and emits up to F S + L - S (nothing if F = 0).
// The rate table, F(n) and F S + L - S are spec_rule.h's, as for every wave entry.
#pragma once
#include <stdint.h>
#include <stdio.h>

#include "spec_rule.h"

namespace live_rule {
using spec_rule::refuse;

// a recording is indexed in int on the device: its samples stay below this
constexpr int64_t kMaxSamples = INT32_MAX - 1024;

// what one push does to one session
struct Step {
    int64_t A0, A1;    // analysed frames before / after
    int64_t T0, T1;    // decoded frames before / after
    int64_t p0, p1;    // unconsumed samples before / after (p1 of an ended session: what it drops)
    int64_t emit;      // samples that become final
};

inline Step step(int L, int S, int half, int64_t had, int64_t add, bool end) {
    Step s;
    const int64_t n1 = had + add;
    s.A0 = spec_rule::frames(L, S, had);
    s.A1 = spec_rule::frames(L, S, n1);
    s.T0 = s.A0 > half ? s.A0 - half : 0;
    s.T1 = end ? s.A1 : (s.A1 > half ? s.A1 - half : 0);
    s.p0 = had - s.A0 * S;  // n < L: all of them; else the L - S .. L - 1 samples from the next frame's start on
    s.p1 = n1 - s.A1 * S;
    const int64_t upto = end ? (s.A1 > 0 ? spec_rule::out_samples(L, S, s.A1) : 0) : s.T1 * S;
    s.emit = upto - s.T0 * S;
    return s;
}

// the checks shared by mlggd_live_layout and mlggd_live_open; 0 or -1 with msg filled
inline int check_group(int fs_khz, int fea_context, int n_sessions, int *L, int *S, char *msg, size_t cap) {
    if (!spec_rule::rate(fs_khz, L, S)) return refuse(msg, cap, "fs_khz %d: must be 8, 11 or 16", fs_khz);
    if (fea_context < 1 || fea_context % 2 == 0) return refuse(msg, cap, "fea_context %d must be odd", fea_context);
    if (n_sessions < 1) return refuse(msg, cap, "n_sessions %d < 1", n_sessions);
    return 0;
}

// out_off [n_sessions + 1] of the push that adds add[u] samples to a session holding had[u]; 0, or -1 with msg filled
inline int layout(int fs_khz, int fea_context, int n_sessions, const int64_t *had, const int64_t *add,
                  const uint8_t *end, int64_t *out_off, char *msg, size_t cap) {
    int L, S;
    if (check_group(fs_khz, fea_context, n_sessions, &L, &S, msg, cap)) return -1;
    if (!had || !add || !out_off) return refuse(msg, cap, "had/add/out_off is NULL");
    const int half = (fea_context - 1) / 2;
    out_off[0] = 0;
    for (int u = 0; u < n_sessions; u++) {
        if (had[u] < 0 || add[u] < 0)
            return refuse(msg, cap, "session %d: had %lld / add %lld is negative", u, (long long)had[u],
                          (long long)add[u]);
        if (had[u] > kMaxSamples || add[u] > kMaxSamples - had[u])
            return refuse(msg, cap, "session %d: %lld + %lld samples exceed the %lld one recording may have: end it", u,
                          (long long)had[u], (long long)add[u], (long long)kMaxSamples);
        out_off[u + 1] = out_off[u] + step(L, S, half, had[u], add[u], end && end[u]).emit;
    }
    return 0;
}

}  // namespace live_rule
