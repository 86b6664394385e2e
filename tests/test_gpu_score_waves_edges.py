"""GPU: the quality report (score.hip.h) where its two kernels take another path -- more frames than the 16 wavefronts
of k_score_utt (its frame loop comes round again), more than 1024 (its maxima loop does), thousands of utterances under
both frame lookups, |X| = 0 in the noisy wave, full scale, the engine's grow-only workspace across scored calls, the
129-bin rates and a packed buffer that does not start at sample 0.

Accuracy cases go through test_gpu_score_waves.check_case unchanged (MARGIN 16, the largest distance over a batch of at
least four scored utterances).  The reduction order DESIGN.md section 8 documents is pinned bit for bit against
spec64.score_tree_mean32.  tests/test_score_model.py shows on the CPU, on the very inputs built here, that each
planted slip of that model (spec64.SCORE_TREE_SLIPS, score_floors64(first=1024)) moves a result by more than 100 x
what check_case allows, or, for the order of the 16 partials, changes its bits; the docstrings name the slip a case
catches."""
import ctypes as C
import functools

import numpy as np
import pytest

import spec64
import test_gpu_score_waves as base
from test_gpu_score_waves import F32, add_noise, check_case, engine, mixed_lps, n_samples, norm_stats, same, small_net

pytestmark = pytest.mark.gpu
TREE_FRAMES = [15, 16, 17, 31, 32, 33, 64, 65]    # either side of one, two and four trips of the 16 wavefronts
LONG_FRAMES = [1030, 1025, 40, 17]                # 1024 = the threads of a k_score_utt workgroup
LOUD_AT = 1027                                    # the loud frame of the 1030-frame utterance: in the second trip
PERIODIC_FRAMES = [1, 17, 40, 1030]
N_MANY = 3000


def frozen(*lists):
    for l in lists:
        for a in l:
            a.setflags(write=False)
    return lists


def eq(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- inputs: built once, never written to; tests/test_score_model.py reads the same objects
@functools.lru_cache(maxsize=None)
def tree_batch(fs):
    """utterances of TREE_FRAMES frames, noise at 5 dB, as test_gpu_score_waves.batch builds them"""
    rng = np.random.default_rng(2000 + fs)
    cleans = [spec64.synth_speech(n_samples(F, fs, extra=3 * i), fs, seed=100 + fs + 7 * i)
              for i, F in enumerate(TREE_FRAMES)]
    noisys = [add_noise(c, 5, rng) for c in cleans]
    lps = [mixed_lps(c, n, fs, rng) for c, n in zip(cleans, noisys)]
    return frozen(cleans, noisys, lps)


@functools.lru_cache(maxsize=None)
def order_batch(fs):
    """tree_batch's utterances above 16 frames and 16 more of 17 to 48 frames (seeded): enough sums that adding the 16
    partials in another order changes the bits of several of the means, whichever they are"""
    rng = np.random.default_rng(2050 + fs)
    cleans, noisys, lps = (list(l[u] for u, F in enumerate(TREE_FRAMES) if F > 16) for l in tree_batch(fs))
    for i, F in enumerate(int(f) for f in rng.integers(17, 49, 16)):
        cleans.append(spec64.synth_speech(n_samples(F, fs, extra=i % 3), fs, seed=150 + fs + 5 * i))
        noisys.append(add_noise(cleans[-1], 5, rng))
        lps.append(mixed_lps(cleans[-1], noisys[-1], fs, rng))
    return frozen(cleans, noisys, lps)


def one_frame_cuts(cleans, noisys, lps, fs, which):
    """every frame t of the utterances `which` as a one-frame utterance: wave[t S : t S + L], lps[t : t + 1]"""
    L, S, _ = spec64.params(fs)
    cl, no, lp = [], [], []
    for u in which:
        for t in range(lps[u].shape[0]):
            cl.append(cleans[u][t * S:t * S + L])
            no.append(noisys[u][t * S:t * S + L])
            lp.append(lps[u][t:t + 1])
    return cl, no, lp


@functools.lru_cache(maxsize=None)
def periodic_batch():
    """8 kHz (L = 2 S): clean and noisy waves of period S and equal LPS rows, PERIODIC_FRAMES frames: every frame, and
    its maxima, are those of the one-frame utterance"""
    fs = 8
    S = spec64.params(fs)[1]
    rng = np.random.default_rng(2100)
    pc = spec64.synth_speech(S, fs, seed=211)
    pn = add_noise(pc, 5, rng)
    row = mixed_lps(np.tile(pc, 2), np.tile(pn, 2), fs, rng)
    return frozen([np.tile(pc, F + 1) for F in PERIODIC_FRAMES], [np.tile(pn, F + 1) for F in PERIODIC_FRAMES],
                  [np.repeat(row, F, axis=0) for F in PERIODIC_FRAMES])


@functools.lru_cache(maxsize=None)
def long_batch():
    """8 kHz, LONG_FRAMES frames; frame LOUD_AT of the first utterance is 50 times as loud as the rest (the gain of
    test_the_floor_is_the_utterance_s_own), so its 1e-5 floors come from a frame past the first 1024"""
    fs = 8
    L, S, _ = spec64.params(fs)
    rng = np.random.default_rng(2200)
    quiet = spec64.synth_speech(n_samples(LONG_FRAMES[0], fs), fs, seed=221).astype(np.float64) * 0.08
    gain = np.ones(quiet.size)
    gain[LOUD_AT * S:LOUD_AT * S + L] = 50.0
    cleans = [np.clip(np.round(quiet * gain), -32768, 32767).astype(np.int16)]
    cleans += [spec64.synth_speech(n_samples(F, fs, extra=5 * i), fs, seed=222 + i)
               for i, F in enumerate(LONG_FRAMES[1:])]
    noisys = [add_noise(cleans[0], 10, rng)] + [add_noise(c, 5, rng) for c in cleans[1:]]
    lps = [mixed_lps(c, n, fs, rng) for c, n in zip(cleans, noisys)]
    return frozen(cleans, noisys, lps)


@functools.lru_cache(maxsize=None)
def many_batch():
    """8 kHz: N_MANY utterances of 1 to 3 frames (seeded), cut one after the other from one long clean / noisy pair, so
    one analysis of the long waves gives every utterance's LPS rows"""
    fs = 8
    L, S, _ = spec64.params(fs)
    rng = np.random.default_rng(2300)
    frames = rng.integers(1, 4, N_MANY)
    at = np.concatenate([[0], np.cumsum(frames)])
    clean = spec64.synth_speech(n_samples(int(at[-1]), fs), fs, seed=231)
    noisy = add_noise(clean, 5, rng)
    rows = mixed_lps(clean, noisy, fs, rng)
    cut = lambda w: [w[at[u] * S:at[u] * S + n_samples(int(frames[u]), fs)] for u in range(N_MANY)]
    return frozen(cut(clean), cut(noisy), [rows[at[u]:at[u + 1]] for u in range(N_MANY)])


SILENT_ONE_FRAME = 5        # the utterance of silence_batch that check_case cannot take: its LSD is +inf on both sides


@functools.lru_cache(maxsize=None)
def silence_batch(fs):
    """0: noisy zero over frames 3 and 4 whole; 1: noisy zero throughout; 2: clean and noisy both zero in frame 2;
    3: clean and noisy at +-32767 on every sample; 4: an ordinary utterance; 5: one frame, clean and noisy both zero.
    LPS rows from the waves before the zeroing: none at the floor"""
    L, S, _ = spec64.params(fs)
    rng = np.random.default_rng(2400 + fs)
    frames = [9, 5, 7, 6, 17, 1]
    cleans = [spec64.synth_speech(n_samples(F, fs, extra=2 * i), fs, seed=240 + fs + i) for i, F in enumerate(frames)]
    cleans[3] = np.where(cleans[3] >= 0, 32767, -32767).astype(np.int16)
    noisys = [add_noise(c, 5, rng) for c in cleans]
    noisys[3] = np.where(noisys[3] >= 0, 32767, -32767).astype(np.int16)
    lps = [mixed_lps(c, n, fs, rng) for c, n in zip(cleans, noisys)]
    noisys[0][3 * S:4 * S + L] = 0
    noisys[1][:] = 0
    cleans[2][2 * S:2 * S + L] = 0
    noisys[2][2 * S:2 * S + L] = 0
    cleans[5][:] = 0
    noisys[5][:] = 0
    assert all((l > -50.0).all() for l in lps)
    return frozen(cleans, noisys, lps)


@functools.lru_cache(maxsize=None)
def pool_batch():
    """8 kHz: 41 utterances of 1 to 12 frames for the engine's workspace sequence"""
    fs = 8
    rng = np.random.default_rng(2500)
    frames = [int(f) for f in rng.integers(1, 13, 41)]
    cleans = [spec64.synth_speech(n_samples(F, fs, extra=i % 4), fs, seed=250 + i) for i, F in enumerate(frames)]
    noisys = [add_noise(c, 5, rng) for c in cleans]
    return frozen(cleans, noisys) + (frames,)


# ---- frame counts around the wavefront count
@pytest.mark.parametrize("fs", [8, 11])
def test_frame_counts_around_the_wavefront_count(pkg, fs):
    """15 ... 65 frames against float64: catches first_trip_only (every utterance above 16 frames) and
    divide_by_padded_count (every count that is no multiple of 16)"""
    cleans, noisys, lps = tree_batch(fs)
    got = pkg.score_waves(cleans, noisys, lps, fs_khz=fs)
    check_case("%d kHz, 15 ... 65 frames" % fs, got, cleans, noisys, lps, fs)


@pytest.mark.parametrize("fs", [8, 11])
def test_segsnr_is_the_documented_tree_over_its_frames(pkg, fs):
    """a frame's SNR does not depend on the floors, so frame t scored as a one-frame utterance is the value that
    enters the utterance's mean: the mean must be score_tree_mean32 of those values, bit for bit.  Fails for a frame
    dropped, doubled or read from a neighbour and for every slip of SCORE_TREE_SLIPS (shown below on the device's own
    per-frame values, so the comparison cannot pass by coincidence)"""
    cleans, noisys, lps = order_batch(fs)
    counts = [l.shape[0] for l in lps]
    assert {17, 33, 65} <= set(counts) and min(counts) > 16
    full = pkg.score_waves(cleans, noisys, lps, fs_khz=fs)
    frames = pkg.score_waves(*one_frame_cuts(cleans, noisys, lps, fs, range(len(counts))), fs_khz=fs)[0]
    at, reordered = 0, 0
    for u, F in enumerate(counts):
        v = frames[at:at + F]
        at += F
        assert spec64.score_tree_mean32(v) == full[0][u], (F, spec64.score_tree_mean32(v), full[0][u])
        assert spec64.score_tree_mean32(v, "first_trip_only") != full[0][u]
        if F % 16:
            assert spec64.score_tree_mean32(v, "divide_by_padded_count") != full[0][u]
        reordered += spec64.score_tree_mean32(v, "left_to_right") != full[0][u]
    assert at == frames.size and reordered > 0


def test_both_means_are_the_documented_tree_over_equal_frames(pkg):
    """a frame's LSD depends on its utterance's floors, so here every frame is the same frame (periodic_batch): with v
    the two numbers of the one-frame utterance, F frames must give score_tree_mean32([v] * F) bit for bit, at 17, 40
    and 1030 frames.  Catches first_trip_only and divide_by_padded_count in the LSD mean"""
    cleans, noisys, lps = periodic_batch()
    got = pkg.score_waves(cleans, noisys, lps, fs_khz=8)
    assert PERIODIC_FRAMES[0] == 1 and np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    for q in (0, 1):
        v = got[q][0]
        for u, F in enumerate(PERIODIC_FRAMES):
            assert spec64.score_tree_mean32([v] * F) == got[q][u], (q, F, v, got[q][u])
            if F > 16:
                assert spec64.score_tree_mean32([v] * F, "first_trip_only") != got[q][u]
                assert spec64.score_tree_mean32([v] * F, "divide_by_padded_count") != got[q][u]


def test_score_frames_around_the_wavefront_count(pkg):
    """16, 17 and 32 of the 33 frames: the bits of the waves cut to that length"""
    fs = 8
    cleans, noisys, lps = tree_batch(fs)
    u = TREE_FRAMES.index(33)
    counts = [16, 17, 32, 33]
    got = pkg.score_waves([cleans[u]] * 4, [noisys[u]] * 4, [lps[u]] * 4, fs_khz=fs, score_frames=counts)
    cut = pkg.score_waves([cleans[u][:n_samples(k, fs)] for k in counts],
                          [noisys[u][:n_samples(k, fs)] for k in counts], [lps[u][:k] for k in counts], fs_khz=fs)
    assert eq(got, cut)
    assert len(set(got[0].tolist())) == 4 and len(set(got[1].tolist())) == 4


# ---- more than 1024 frames
def test_more_than_1024_frames(pkg):
    """1030, 1025, 40 and 17 frames; the floors of the first come from its frame 1027 (test_score_model shows that
    floors taken over the first 1024 frames move its LSD by more than 100 x the allowed distance).  Then score_frames
    1024 1025 40 0 = the cut waves, where the loud frame is not scored and the floor must drop; and the 1025-frame
    utterance alone = itself first and last in the batch"""
    fs = 8
    cleans, noisys, lps = long_batch()
    got = pkg.score_waves(cleans, noisys, lps, fs_khz=fs)
    check_case("8 kHz, 1030 1025 40 17 frames", got, cleans, noisys, lps, fs)
    counts = [1024, 1025, 40, 0]
    part = pkg.score_waves(cleans, noisys, lps, fs_khz=fs, score_frames=counts)
    keep = [0, 1, 2]
    cut = pkg.score_waves([cleans[u][:n_samples(counts[u], fs)] for u in keep],
                          [noisys[u][:n_samples(counts[u], fs)] for u in keep], [lps[u][:counts[u]] for u in keep],
                          fs_khz=fs)
    assert np.array_equal(part[0][keep], cut[0]) and np.array_equal(part[1][keep], cut[1])
    assert part[0][3] == 0.0 and part[1][3] == 0.0
    assert part[0][1] == got[0][1] and part[1][1] == got[1][1] and part[0][2] == got[0][2] and part[1][2] == got[1][2]
    assert abs(float(part[1][0]) - float(got[1][0])) > 0.1              # without the loud frame the floors are lower
    check_case("8 kHz, score_frames 1024 1025 40 0", part, cleans, noisys, lps, fs, counts=counts)
    alone = pkg.score_waves(cleans[1:2], noisys[1:2], lps[1:2], fs_khz=fs)
    last = pkg.score_waves([cleans[u] for u in (0, 2, 3, 1)], [noisys[u] for u in (0, 2, 3, 1)],
                           [lps[u] for u in (0, 2, 3, 1)], fs_khz=fs)
    first = pkg.score_waves([cleans[u] for u in (1, 0, 2, 3)], [noisys[u] for u in (1, 0, 2, 3)],
                            [lps[u] for u in (1, 0, 2, 3)], fs_khz=fs)
    for q in (0, 1):
        assert alone[q][0] == got[q][1] == first[q][0] == last[q][3], q


# ---- many utterances, both lookups
def test_three_thousand_utterances(pkg):
    """3000 utterances of 1 to 3 frames: the search of seg_of_frame runs 12 levels deep over a count that is no power
    of two; all of them against float64 in groups of 100, ten seeded picks against the utterance scored alone"""
    fs = 8
    cleans, noisys, lps = many_batch()
    got = pkg.score_waves(cleans, noisys, lps, fs_khz=fs)
    for a in range(0, N_MANY, 100):
        s = slice(a, a + 100)
        check_case("8 kHz, 3000 utterances, %d-%d" % (a, a + 99), (got[0][s], got[1][s]), cleans[s], noisys[s], lps[s],
                   fs)
    for u in np.random.default_rng(2301).choice(N_MANY, 10, replace=False):
        alone = pkg.score_waves(cleans[u:u + 1], noisys[u:u + 1], lps[u:u + 1], fs_khz=fs)
        assert alone[0][0] == got[0][u] and alone[1][0] == got[1][u], u


def test_three_thousand_utterances_on_the_engine_under_both_lookups(pkg, monkeypatch):
    """the same list decoded and scored by an engine (129 bins, context 3) with the binary search and with
    MLGGD_WAVES_LOOKUP=table (read when the engine is created): wave, LPS rows and both scores agree bit for bit, and
    the scores equal the stateless path on the returned rows"""
    fs, ctx = 8, 3
    cleans, noisys, _ = many_batch()
    rng = np.random.default_rng(2302)
    ls, ws, bs = small_net(rng, ctx=ctx, D=129)
    mean, inv = norm_stats(rng, 129)
    res = []
    for lookup in ("search", "table"):
        if lookup == "table":
            monkeypatch.setenv("MLGGD_WAVES_LOOKUP", "table")
        else:
            monkeypatch.delenv("MLGGD_WAVES_LOOKUP", raising=False)
        eng = engine(pkg, ls, ws, bs, 64)
        res.append(eng.enhance_waves(noisys, mean, inv, fs_khz=fs, fea_context=ctx, return_lps=True, cleans=cleans))
        eng.close()
    monkeypatch.delenv("MLGGD_WAVES_LOOKUP", raising=False)
    (out, rows, segsnr, lsd), (out_t, rows_t, segsnr_t, lsd_t) = res
    same(out_t, out)
    same(rows_t, rows)
    assert np.array_equal(segsnr_t, segsnr) and np.array_equal(lsd_t, lsd)
    assert eq(pkg.score_waves(cleans, noisys, rows, fs_khz=fs), (segsnr, lsd))
    assert np.isfinite(segsnr).all() and np.isfinite(lsd).all()


# ---- |X| = 0 and full scale
@pytest.mark.parametrize("fs", [8, 16])
def test_silence_in_the_noisy_wave_and_full_scale(pkg, fs):
    """silence_batch: the A > 0 else-branch of k_score_frames (phase 0 where the noisy spectrum is exactly zero; the
    host's quality(), quality64 and quality32 do the same), a frame silent in both waves (-20 exactly, as a one-frame
    utterance; its LSD is +inf on the device as in float64: 0 floors under a zero clean power), and a pair at +-32767
    on every sample"""
    cleans, noisys, lps = silence_batch(fs)
    got = pkg.score_waves(cleans, noisys, lps, fs_khz=fs)
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any()
    k = SILENT_ONE_FRAME
    assert got[0][k] == F32(-20.0) and got[1][k] == np.inf
    assert spec64.quality64(cleans[k], noisys[k], lps[k], fs) == (-20.0, np.inf)
    check_case("%d kHz, silent noisy frames, full scale" % fs, (got[0][:k], got[1][:k]), cleans[:k], noisys[:k],
               lps[:k], fs)
    # the both-silent frame inside utterance 2, on its own
    L, S, _ = spec64.params(fs)
    one = pkg.score_waves([cleans[2][2 * S:2 * S + L]], [noisys[2][2 * S:2 * S + L]], [lps[2][2:3]], fs_khz=fs)
    assert one[0][0] == F32(-20.0)


# ---- the engine: workspace across calls, the 129-bin rates
def test_engine_workspace_across_scored_calls_of_other_sizes(pkg):
    """one engine (129 bins, 8 kHz, context 3, chunks of 7 frames, which cut inside utterances): scored as its very
    first call and without the LPS rows, scored on 40 utterances, on 2 with score_frames, a plain call, 40 with other
    norm vectors, 41 (every buffer grows).  Each call = the same call on a fresh engine, and its scores = the stateless
    path on that call's own rows"""
    fs, ctx = 8, 3
    cleans, noisys, frames = pool_batch()
    rng = np.random.default_rng(2501)
    ls, ws, bs = small_net(rng, ctx=ctx, D=129)
    norm_a, norm_b = norm_stats(rng, 129), norm_stats(rng, 129)
    big = max(range(41), key=lambda u: frames[u])
    two = [big, 3]
    counts = [frames[big] - 1, frames[3]]
    assert frames[big] > 7
    calls = [                                                          # (utterances, norm, scored, score_frames, f32)
        (list(range(7)), norm_a, True, None, False),
        (list(range(40)), norm_a, True, None, True),
        (two, norm_a, True, counts, False),
        (list(range(1, 30)), norm_a, False, None, True),
        (list(range(1, 41)), norm_b, True, None, False),
        (list(range(41)), norm_b, True, None, True),
    ]
    eng = engine(pkg, ls, ws, bs, 16, cap=7)
    for i, (us, (mean, inv), scored, sf, f32) in enumerate(calls):
        no, cl = [noisys[u] for u in us], [cleans[u] for u in us]
        kw = dict(fs_khz=fs, fea_context=ctx, return_f32=f32)
        if scored:
            kw.update(cleans=cl, score_frames=sf)
        got = eng.enhance_waves(no, mean, inv, **kw)
        fresh = engine(pkg, ls, ws, bs, 16, cap=7)
        want = fresh.enhance_waves(no, mean, inv, return_lps=True, **kw)
        fresh.close()
        if not scored:
            for g, w in zip(got, want[:2]):
                same(g, w)
            continue
        rows = want[1 + f32]
        same(got[0], want[0])
        if f32:
            same(got[1], want[1])
        assert eq(got[-2:], want[-2:]), i
        assert eq(got[-2:], pkg.score_waves(cl, no, rows, fs_khz=fs, score_frames=sf)), i
    eng.close()


@pytest.mark.parametrize("fs", [8, 11])
def test_engine_path_equals_the_stateless_path_at_129_bins(pkg, fs):
    """test_engine_path_equals_the_stateless_path_at_any_chunking at the 129-bin rates: capacity 4 cuts inside the
    utterances of 5 and 9 frames, 1000 holds the batch"""
    ctx = 3
    cleans, noisys, _ = base.batch(fs, 5)
    rng = np.random.default_rng(2600 + fs)
    ls, ws, bs = small_net(rng, ctx=ctx, D=129)
    mean, inv = norm_stats(rng, 129)
    counts = [1, 2, 0, 7]
    res = []
    for cap in (1000, 4):
        eng = engine(pkg, ls, ws, bs, 16, cap=cap)
        plain = eng.enhance_waves(noisys, mean, inv, fs_khz=fs, fea_context=ctx, return_f32=True, return_lps=True)
        out, outf, lps, segsnr, lsd = eng.enhance_waves(noisys, mean, inv, fs_khz=fs, fea_context=ctx, return_f32=True,
                                                        return_lps=True, cleans=cleans)
        for g, w in zip((out, outf, lps), plain):
            same(g, w)
        assert eq((segsnr, lsd), pkg.score_waves(cleans, noisys, lps, fs_khz=fs))
        part = eng.enhance_waves(noisys, mean, inv, fs_khz=fs, cleans=cleans, score_frames=counts)
        assert eq(part[1:], pkg.score_waves(cleans, noisys, lps, fs_khz=fs, score_frames=counts)) and part[1][2] == 0.0
        same(eng.enhance_waves(noisys, mean, inv, fs_khz=fs), out)
        eng.close()
        res.append((segsnr, lsd, lps))
    assert eq(res[0], res[1])
    same(res[0][2], res[1][2])
    check_case("%d kHz, engine path, net output" % fs, res[0][:2], cleans, noisys, res[0][2], fs)


# ---- offsets[0] != 0
def raw_scored(pkg, eng, cleans, noisys, fs, base_at, lps=None, mean=None, inv=None, ctx=3):
    """mlggd_score_waves (eng None) or mlggd_enhance_waves_scored through ctypes with offsets[0] = base_at: the clean
    and the noisy buffer start with base_at samples of (different) non-zero junk and end with a gap of it.  Returns
    (status, segsnr, lsd) and, for the engine, out and the LPS rows as well"""
    fp, sp, lp = C.POINTER(C.c_float), C.POINTER(C.c_int16), C.POINTER(C.c_int64)
    n = len(noisys)
    off = base_at + np.concatenate([[0], np.cumsum([w.size for w in noisys])]).astype(np.int64)
    junk = np.tile(np.array([32767, -32767, 12345], np.int16), (base_at + 778) // 3 + 2)
    pn = np.concatenate([junk[:base_at], *noisys, junk[1:778]])
    pc = np.concatenate([-junk[2:2 + base_at], *cleans, junk[2:779]])
    segsnr, lsd = np.zeros(n, np.float32), np.zeros(n, np.float32)
    if eng is None:
        rows = np.ascontiguousarray(np.concatenate(lps), np.float32)
        rc = pkg.load().mlggd_score_waves(0, fs, n, pc.ctypes.data_as(sp), pn.ctypes.data_as(sp),
                                          off.ctypes.data_as(lp), rows.ctypes.data_as(fp), None,
                                          segsnr.ctypes.data_as(fp), lsd.ctypes.data_as(fp))
        return rc, segsnr, lsd
    _, frame_off, out_off = pkg.enhance_waves_layout([w.size for w in noisys], fs)
    out = np.zeros(int(out_off[-1]), np.int16)
    rows = np.zeros((int(frame_off[-1]), mean.size), np.float32)
    rc = pkg.load().mlggd_enhance_waves_scored(eng._h, fs, ctx, mean.ctypes.data_as(fp), inv.ctypes.data_as(fp), n,
                                               pn.ctypes.data_as(sp), pc.ctypes.data_as(sp), off.ctypes.data_as(lp),
                                               None, out.ctypes.data_as(sp), None, rows.ctypes.data_as(fp),
                                               segsnr.ctypes.data_as(fp), lsd.ctypes.data_as(fp))
    return rc, segsnr, lsd, out, rows


def test_a_wave_base_other_than_zero(pkg):
    """offsets[0] = 1 and 12345: clean + offsets[0] must move with noisy + offsets[0]; the numbers are those of base 0
    and of the wrapper, bit for bit, on both entry points"""
    fs, ctx = 8, 3
    cleans, noisys, lps = (l[:5] for l in tree_batch(fs))
    want = pkg.score_waves(cleans, noisys, lps, fs_khz=fs)
    for at in (0, 1, 12345):
        rc, segsnr, lsd = raw_scored(pkg, None, cleans, noisys, fs, at, lps=lps)
        assert rc == 0 and eq((segsnr, lsd), want), at
    rng = np.random.default_rng(2700)
    ls, ws, bs = small_net(rng, ctx=ctx, D=129)
    mean, inv = norm_stats(rng, 129)
    eng = engine(pkg, ls, ws, bs, 16, cap=20)
    out, rows, segsnr, lsd = eng.enhance_waves(noisys, mean, inv, fs_khz=fs, fea_context=ctx, return_lps=True,
                                               cleans=cleans)
    for at in (0, 1, 12345):
        rc, s, l, o, r = raw_scored(pkg, eng, cleans, noisys, fs, at, mean=mean, inv=inv, ctx=ctx)
        assert rc == 0 and eq((s, l), (segsnr, lsd)), at
        assert np.array_equal(o, np.concatenate(out)) and np.array_equal(r, np.concatenate(rows)), at
    eng.close()
