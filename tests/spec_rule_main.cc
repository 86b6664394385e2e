// spec_rule_main.cc -- the host-only layout rule of the spectral front end (csrc/spec_rule.h, what every wave entry
// computes its tables from) as a stand-alone program for AddressSanitizer + UBSan; driven by tests/test_spec_rule.py.
// For 8, 11 and 16 kHz it checks the frame count around every boundary, the tables of a packed batch under both
// policies for a short utterance, the window, score-frame and compaction checks and the span of a decode chunk, each
// against the rule written out once more.  Every array is a heap array of exactly the size the rule may touch.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "spec_rule.h"

namespace sr = spec_rule;

static int fails = 0;
#define EXPECT(c)                                                 \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            fails++;                                              \
        }                                                         \
    } while (0)

// the rule once more: the frames are the windows [t S, t S + L) that fit into n samples
static int64_t frames_of(int L, int S, int64_t n) {
    int64_t F = 0;
    while (F * S + L <= n) F++;
    return F;
}
static int64_t samples_of(int L, int S, int64_t F) { return (F - 1) * S + L; }  // the end of the last window

static char msg[256];

static void check_rates() {
    SpecDims d;
    int slot = -1, L = 0, S = 0;
    EXPECT(!sr::rate(12, &d, &slot) && !sr::rate(0, &L, &S));
    const int want[3][4] = {{8, 256, 128, 256}, {11, 256, 110, 256}, {16, 512, 256, 512}};
    for (int r = 0; r < 3; r++) {
        EXPECT(sr::rate(want[r][0], &d, &slot) && slot == r);
        EXPECT(d.L == want[r][1] && d.S == want[r][2] && d.N == want[r][3]);
        EXPECT(d.M == d.N / 2 && d.D == d.N / 2 + 1 && (1 << d.logM) == d.M);
        EXPECT(sr::rate(want[r][0], &d) && sr::rate(want[r][0], &L, &S) && L == d.L && S == d.S);
        std::vector<int64_t> ns = {0, 1, d.L - 1, d.L};
        for (int k = 0; k <= 4; k++)
            for (int dlt = -1; dlt <= 1; dlt++) ns.push_back(d.L + (int64_t)k * d.S + dlt);
        for (int64_t n : ns) {
            const int64_t F = frames_of(d.L, d.S, n);
            EXPECT(sr::frames(d, n) == F && sr::frames(d.L, d.S, n) == F);
            if (F > 0) EXPECT(sr::out_samples(d, F) == samples_of(d.L, d.S, F) && sr::out_samples(d, F) <= n);
        }
    }
}

// the three tables of lens[] packed from `base` on, under `policy`, against the restatement; each table alone too
static void check_layout_of(const SpecDims &d, const std::vector<int64_t> &lens, int64_t base, sr::Short policy) {
    const int n = (int)lens.size();
    std::vector<int64_t> off((size_t)n + 1);
    std::vector<int32_t> wf((size_t)n + 1), gf((size_t)n + 1, -7), gf1((size_t)n + 1, -7);
    std::vector<long long> wo((size_t)n + 1), ww((size_t)n + 1), go((size_t)n + 1, -7), gw((size_t)n + 1, -7);
    std::vector<long long> go1((size_t)n + 1, -7), gw1((size_t)n + 1, -7);
    off[0] = base, wf[0] = 0, wo[0] = 0, ww[0] = 0;
    for (int u = 0; u < n; u++) {
        const int64_t F = frames_of(d.L, d.S, lens[u]);
        off[u + 1] = off[u] + lens[u];
        wf[u + 1] = wf[u] + (int32_t)F;
        wo[u + 1] = wo[u] + (F ? samples_of(d.L, d.S, F) : 0);
        ww[u + 1] = off[u + 1] - base;
    }
    EXPECT(sr::layout(d, n, off.data(), policy, gf.data(), go.data(), gw.data(), msg, sizeof msg) == 0);
    EXPECT(gf == wf && go == wo && gw == ww);
    EXPECT(sr::layout(d, n, off.data(), policy, gf1.data(), nullptr, nullptr, msg, sizeof msg) == 0 && gf1 == wf);
    EXPECT(sr::layout(d, n, off.data(), policy, nullptr, go1.data(), nullptr, msg, sizeof msg) == 0 && go1 == wo);
    EXPECT(sr::layout(d, n, off.data(), policy, nullptr, nullptr, gw1.data(), msg, sizeof msg) == 0 && gw1 == ww);
    EXPECT(sr::layout(d, n, off.data(), policy, nullptr, nullptr, nullptr, msg, sizeof msg) == 0);
    std::fill(gw.begin(), gw.end(), -7);  // not cut into frames: the re-based offsets alone
    EXPECT(sr::layout(d, n, off.data(), sr::kUnframed, nullptr, nullptr, gw.data(), msg, sizeof msg) == 0);
    EXPECT(gw == ww);
}

static void check_layouts(int fs) {
    SpecDims d;
    EXPECT(sr::rate(fs, &d));
    const int64_t L = d.L, S = d.S;
    const std::vector<int64_t> full = {L, L + S - 1, L + 40 * S + 7, L + S, 3 * L};
    const std::vector<int64_t> holes = {L - 1, L, 0, L + S - 1, 1, L + 40 * S + 7, L - 1};
    for (sr::Short policy : {sr::kShortFails, sr::kShortEmpty})
        for (int64_t base : {(int64_t)0, (int64_t)1000}) check_layout_of(d, full, base, policy);
    check_layout_of(d, holes, 1000, sr::kShortEmpty);
    {   // a short utterance is an error where every utterance must have a frame; the message names it and its length
        std::vector<int64_t> off = {1000, 1000 + L, 1000 + 2 * L + S, 1000 + 3 * L + S - 1, 1000 + 5 * L};
        std::vector<int32_t> gf(5);
        char want[128];
        snprintf(want, sizeof want, "utterance 2: %d samples is shorter than one frame (%d)", (int)L - 1, (int)L);
        EXPECT(sr::layout(d, 4, off.data(), sr::kShortFails, gf.data(), nullptr, nullptr, msg, sizeof msg) == -1);
        EXPECT(!strcmp(msg, want));
        EXPECT(sr::layout(d, 4, off.data(), sr::kShortEmpty, gf.data(), nullptr, nullptr, msg, sizeof msg) == 0);
        EXPECT(gf[3] == gf[2] && gf[2] == gf[1] + 2 && gf[4] > gf[3]);
    }
    {   // offsets that decrease, under every policy
        std::vector<int64_t> off = {0, 5000, 4000, 9000};
        std::vector<long long> gw(4);
        for (sr::Short policy : {sr::kShortFails, sr::kShortEmpty, sr::kUnframed}) {
            EXPECT(sr::layout(d, 3, off.data(), policy, nullptr, nullptr, gw.data(), msg, sizeof msg) == -1);
            EXPECT(!strcmp(msg, "offsets decrease at utterance 1 (4000 after 5000)"));
        }
    }
    {   // n_utts = 0 reads no offsets and gives the one 0 of each table; a negative count and NULL offsets are refused
        std::vector<int32_t> gf(1, -7);
        std::vector<long long> go(1, -7), gw(1, -7);
        EXPECT(sr::layout(d, 0, nullptr, sr::kShortFails, gf.data(), go.data(), gw.data(), msg, sizeof msg) == 0);
        EXPECT(gf[0] == 0 && go[0] == 0 && gw[0] == 0);
        EXPECT(sr::layout(d, 0, nullptr, sr::kShortEmpty, nullptr, nullptr, nullptr, msg, sizeof msg) == 0);
        EXPECT(sr::layout(d, -1, nullptr, sr::kShortEmpty, nullptr, nullptr, nullptr, msg, sizeof msg) == -1);
        EXPECT(!strcmp(msg, "n_utts -1 < 0"));
        EXPECT(sr::layout(d, 2, nullptr, sr::kShortFails, nullptr, nullptr, nullptr, msg, sizeof msg) == -1);
        EXPECT(!strcmp(msg, "offsets is NULL"));
        char tiny[8];
        EXPECT(sr::layout(d, 2, nullptr, sr::kShortFails, nullptr, nullptr, nullptr, tiny, sizeof tiny) == -1);
        EXPECT(strlen(tiny) == 7);
    }
}

static void check_frame_overflow() {  // 2^30 + 2^31 frames of 128 samples do not fit the int32 frame index
    SpecDims d;
    EXPECT(sr::rate(8, &d));
    std::vector<int64_t> off = {0, (int64_t)1 << 37, ((int64_t)1 << 38) + ((int64_t)1 << 37)};
    std::vector<int32_t> gf(3);
    std::vector<long long> gw(3);
    for (sr::Short policy : {sr::kShortFails, sr::kShortEmpty}) {
        EXPECT(sr::layout(d, 2, off.data(), policy, gf.data(), nullptr, nullptr, msg, sizeof msg) == -1);
        EXPECT(!strcmp(msg, "the batch has more than 2147483647 frames (reached at utterance 1)"));
    }
    EXPECT(sr::layout(d, 1, off.data(), sr::kShortFails, gf.data(), nullptr, nullptr, msg, sizeof msg) == 0);
    EXPECT(gf[1] == (1 << 30) - 1);
    EXPECT(sr::layout(d, 2, off.data(), sr::kUnframed, nullptr, nullptr, gw.data(), msg, sizeof msg) == 0);
    EXPECT(gw[2] == off[2]);
}

static void check_windows_and_tables() {
    // utterances of 3, 0, 5, 0, 0 and 2 frames
    const std::vector<int32_t> foff = {0, 3, 3, 8, 8, 8, 10};
    const int n = 6, ctx = 3;
    auto one = [&](int32_t f) {
        std::vector<int32_t> first = {0, f};  // sample 1 is the one looked at
        return sr::check_windows(n, foff.data(), ctx, 2, first.data(), msg, sizeof msg);
    };
    for (int32_t f : {0, 3, 4, 5}) EXPECT(one(f) == 0);  // 3 starts utterance 2: the empty one is stepped over
    EXPECT(one(1) == -1 && !strcmp(msg, "sample 1: window [1,4) crosses the end of utterance 0 at frame 3"));
    EXPECT(one(2) == -1 && strstr(msg, "utterance 0 at frame 3"));
    EXPECT(one(6) == -1 && !strcmp(msg, "sample 1: window [6,9) crosses the end of utterance 2 at frame 8"));
    EXPECT(one(7) == -1 && strstr(msg, "utterance 2 at frame 8"));
    EXPECT(one(8) == -1 && !strcmp(msg, "sample 1: window [8,11) outside the 10 packed frames"));
    EXPECT(one(-1) == -1 && !strcmp(msg, "sample 1: window [-1,2) outside the 10 packed frames"));
    EXPECT(one(INT32_MAX) == -1 && strstr(msg, "outside the 10 packed frames"));
    {
        std::vector<int32_t> first = {8};  // a window of 2 fits the last utterance, past the two empty ones
        EXPECT(sr::check_windows(n, foff.data(), 2, 1, first.data(), msg, sizeof msg) == 0);
        EXPECT(sr::check_windows(n, foff.data(), 2, 0, nullptr, msg, sizeof msg) == 0);
    }
    {   // compaction: empty utterances at the front, in the middle and at the end
        const std::vector<int32_t> f2 = {0, 0, 3, 3, 3, 8, 8};
        const std::vector<long long> w2 = {0, 10, 500, 501, 501, 1400, 1500};
        std::vector<int32_t> cf(3, -7);
        std::vector<long long> cw(3, -7);
        EXPECT(sr::compact_tables(6, f2.data(), w2.data(), cf.data(), cw.data()) == 2);
        EXPECT(cf == std::vector<int32_t>({0, 3, 8}) && cw == std::vector<long long>({10, 501, 1500}));
        const std::vector<int32_t> f0 = {0, 0, 0};  // no frames at all: the one closing entry
        const std::vector<long long> w0 = {0, 5, 9};
        std::vector<int32_t> c0(1, -7);
        std::vector<long long> d0(1, -7);
        EXPECT(sr::compact_tables(2, f0.data(), w0.data(), c0.data(), d0.data()) == 0 && c0[0] == 0 && d0[0] == 9);
        std::vector<int32_t> cf7(7);  // nothing empty: a copy
        std::vector<long long> cw7(7);
        const std::vector<int32_t> f7 = {0, 1, 3, 4, 8, 9, 10};
        EXPECT(sr::compact_tables(6, f7.data(), w2.data(), cf7.data(), cw7.data()) == 6 && cf7 == f7 && cw7 == w2);
    }
    {   // score_frames: NULL is every frame; 0..frames of the utterance is legal
        const std::vector<int32_t> f3 = {0, 3, 8, 10};
        const std::vector<int32_t> ok = {3, 0, 2}, over = {3, 6, 2}, neg = {0, 0, -1};
        EXPECT(sr::check_score_frames(3, f3.data(), nullptr, msg, sizeof msg) == 0);
        EXPECT(sr::check_score_frames(3, f3.data(), ok.data(), msg, sizeof msg) == 0);
        EXPECT(sr::check_score_frames(3, f3.data(), over.data(), msg, sizeof msg) == -1);
        EXPECT(!strcmp(msg, "utterance 1: score_frames 6 is outside 0..5, its frames"));
        EXPECT(sr::check_score_frames(3, f3.data(), neg.data(), msg, sizeof msg) == -1);
        EXPECT(!strcmp(msg, "utterance 2: score_frames -1 is outside 0..2, its frames"));
    }
}

// the span of every chunk against brute force: the segment of a chunk's first and of its last frame
static void check_spans() {
    const std::vector<std::vector<int>> tables = {{1, 40, 7, 16, 2}, {40, 1, 1, 1, 40}, {16, 16, 16, 16, 16},
                                                  {3, 5, 2, 1, 4},   {1, 1, 1, 1, 1},   {17, 2, 33, 1, 15}};
    for (const auto &lens : tables) {
        std::vector<int32_t> off(6);
        off[0] = 0;
        for (int k = 0; k < 5; k++) off[k + 1] = off[k] + lens[k];
        const int FT = off[5];
        auto seg_of = [&](int f) {
            int k = 0;
            while (!(off[k] <= f && f < off[k + 1])) k++;
            return k;
        };
        for (int ctx : {1, 7})
            for (int cap : {1, 2, 16}) {
                int hint = 0;  // the walk of a decode call: chunks in order, one running hint
                for (int a = 0; a < FT; a += cap) {
                    const int n = cap < FT - a ? cap : FT - a;
                    const sr::Span sp = sr::chunk_span(off.data(), &hint, a, n, ctx);
                    EXPECT(sp.u0 == seg_of(a) && sp.u1 == seg_of(a + n - 1) && hint == sp.u0);
                    EXPECT(sp.rows == n + (sp.u1 - sp.u0 + 1) * (ctx - 1));
                }
                for (int a = 0; a < FT; a++)  // every (a, n) from a fresh hint
                    for (int n = 1; n <= cap && a + n <= FT; n++) {
                        int h0 = 0;
                        const sr::Span sp = sr::chunk_span(off.data(), &h0, a, n, ctx);
                        int touched = 0;
                        for (int k = 0; k < 5; k++) touched += off[k] < a + n && off[k + 1] > a;
                        EXPECT(sp.u0 == seg_of(a) && sp.u1 == seg_of(a + n - 1) && sp.rows == n + touched * (ctx - 1));
                    }
            }
    }
}

int main() {
    check_rates();
    for (int fs : {8, 11, 16}) check_layouts(fs);
    check_frame_overflow();
    check_windows_and_tables();
    check_spans();
    if (fails) return 1;
    printf("spec_rule_main OK\n");
    return 0;
}
