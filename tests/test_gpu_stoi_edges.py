"""GPU: STOI on the device where the short batch of tests/test_gpu_stoi.py does not reach: k_stoi_select beyond one trip
of 256 frames (the carry, a trip that keeps nothing, kept runs across frames 255 / 256 and 511 / 512), compaction of
frames that are no neighbours with 1 to 4 segments (nothing diluted), utterances without a frame anywhere in a batch,
digital silence in the processed wave, and inputs on which the clipping decides the value.  The inputs are those of
tests/stoi_cases.py; tests/test_stoi_model.py shows on the CPU that a wrong scan order would exceed the allowance.

Tolerance: the rule and the factor of tests/test_gpu_stoi.py (check_case): per batch, the GPU's largest distance to
stoi64 is at most 16 x stoi32's, and the segment counts are equal.  The value is rounded to fp32 once, so no fp32
evaluation can be promised closer than 2^-25 near 1: a batch whose model distance is smaller was lucky and is no bound,
and every batch asserts that its own is not.  Everything else here is bit equality.  Before the device is touched each
case asserts on the CPU its frames, kept frames, compacted frames and segments, a keep margin of 1e-3 dB and, for the
rows with a value, that no band of a segment is without variance."""
import numpy as np
import pytest

import stoi64
import stoi_cases as sc
from test_gpu_score_waves import engine, norm_stats, small_net
from test_gpu_stoi import MARGIN, MIN_KEEP_MARGIN_DB, bits, check_case

pytestmark = pytest.mark.gpu
LUCKY = 2.0 ** -25
COUNTS = {sc.case_a: (600, 34, 33, 4), sc.case_b: (700, 347, 346, 317), sc.case_d: (0, 0, 0, 0),
          sc.case_e: (155, 155, 154, 125)}
C_COUNTS = {32: (300, 32, 31, 2), 31: (300, 31, 30, 1), 30: (300, 30, 29, 0)}


def prepared(spec, muted=()):
    """cleans, procs, models of the batch, after the conditions on its inputs were asserted on the CPU"""
    cleans, procs, models = sc.rows(spec)
    for u, ((b, *a), (m64, m32)) in enumerate(zip(spec, models)):
        want = C_COUNTS[a[1]] if b is sc.case_c else COUNTS[b]
        assert (m64.frames, m64.kept, m64.M, m64.segments) == want, (u, m64)
        assert (m32.frames, m32.kept, m32.M, m32.segments) == want, (u, m32)
        assert m64.min_margin >= MIN_KEEP_MARGIN_DB and m32.min_margin >= MIN_KEEP_MARGIN_DB, (u, m64)
        if u in muted:
            assert np.isnan(m64.value) and np.isnan(m32.value), (u, m64)
        elif m64.segments:
            assert m64.min_var > 1e-3 and np.isfinite(m64.value) and np.isfinite(m32.value), (u, m64)
    assert sc.model_distance(models, muted) >= LUCKY, sc.model_distance(models, muted)
    return cleans, procs, models


def score(pkg, cleans, procs, fs):
    got, seg = pkg.stoi_waves(cleans, procs, fs_khz=fs, return_segments=True)
    assert got.dtype == np.float32 and got.shape == (len(cleans),) and seg.dtype == np.int32
    return got, seg


# ---- accuracy
@pytest.mark.parametrize("fs", [8, 16])
def test_kept_runs_across_the_trips_and_sparse_frames_against_float64(pkg, fs):
    """A at +5 and -5 dB, C with 32, 31 and 30 kept frames, utterances of 1, 100 and 0 samples first, between, last"""
    spec = sc.trips_batch(fs)
    cleans, procs, models = prepared(spec)
    assert [cleans[u].size for u in (0, 3, 7)] == [1, 100, 0] and models[3][0].len10 > 0
    got, seg = score(pkg, cleans, procs, fs)
    check_case("%d kHz, A +5 / -5 dB, C 32 / 31 / 30, D" % fs, got, seg, models)
    assert np.isnan(got[[0, 3, 6, 7]]).all() and not seg[[0, 3, 6, 7]].any()
    assert got[2] < got[1] < 1.0                                # -5 dB is worse than +5 dB


@pytest.mark.parametrize("fs", [8, 11, 16])
def test_a_long_mostly_kept_utterance_against_float64(pkg, fs):
    spec = sc.long_batch(fs)
    cleans, procs, models = prepared(spec)
    got, seg = score(pkg, cleans, procs, fs)
    check_case("%d kHz, B, A +5 dB, C 32, D" % fs, got, seg, models)
    assert np.isnan(got[[0, 2, 5]]).all() and not seg[[0, 2, 5]].any()


# ---- independence
def test_a_long_utterance_s_value_does_not_depend_on_the_batch(pkg):
    """A and B alone, first, last and between other neighbours: the same bits"""
    fs = 16
    spec = sc.long_batch(fs)
    cleans, procs, _ = prepared(spec)
    n = len(spec)

    def run(order):
        return bits(pkg.stoi_waves([cleans[v] for v in order], [procs[v] for v in order], fs_khz=fs))

    full = run(range(n))
    assert np.array_equal(full, run(range(n)))
    for u in (1, 3):
        others = [v for v in range(n) if v != u]
        mid = [4, u, 3 if u == 1 else 1]                        # C before it and the other long one after it
        assert run([u])[0] == run([u] + others)[0] == run(others + [u])[n - 1] == run(mid)[1] == full[u], u
        assert np.isfinite(full[u:u + 1].view(np.float32)).all()


# ---- silence in the processed wave
def test_a_muted_processed_wave_has_no_value(pkg):
    """all zeros (E1) and a zeroed stretch that covers whole segments (E2): a band's sum of Y^2 is 0, alpha is inf and
    alpha Y is NaN, which the definition's minimum keeps: NaN, with the segments counted.  A zeroed stretch of about 10
    frames (E3) leaves exact zeros in Y and every segment's sum positive: a value, inside the bound.

    Before k_stoi_utt's minimum kept the NaN (fminf drops it and takes the clipping bound, so the band correlates X
    with itself) the device gave E1 the value 1.0 and E2 0.53706217, each with 125 segments."""
    fs = 16
    spec = [(sc.case_e, fs, 1), (sc.case_e, fs, 3), (sc.case_a, fs, 5), (sc.case_e, fs, 2), (sc.case_e, fs, 0),
            (sc.case_c, fs, 32)]
    muted = (0, 3)
    cleans, procs, models = prepared(spec, muted)
    assert not procs[0].any() and not procs[3][9000:19000].any() and not procs[1][9000:11048].any()
    got, seg = score(pkg, cleans, procs, fs)
    print("stoi muted | all zeros: %r, segments %d | zeroed stretch: %r, segments %d" %
          (float(got[0]), seg[0], float(got[3]), seg[3]))
    check_case("16 kHz, muted: E1, E3, A, E2, E0, C 32", got, seg, models, muted=muted)
    assert got[1] < got[4]                                      # the dropout costs something


# ---- the clipping
def test_inputs_on_which_the_clipping_decides(pkg):
    """impulsive noise on the 2 s utterance (E4) and on A: without min(alpha Y, X + X 10^(15/20)) the float64 value is
    further from the true one than the GPU may be.  (On A at -5 dB nothing is clipped: its value is the same without.)"""
    fs = 16
    spec = [(sc.case_e, fs, 4), (sc.case_a, fs, "impulsive"), (sc.case_a, fs, -5), (sc.case_c, fs, 32),
            (sc.case_a, fs, 5)]
    cleans, procs, models = prepared(spec)
    allowance = MARGIN * sc.model_distance(models)
    for u in (0, 1):
        unclipped = stoi64.stoi64(cleans[u], procs[u], fs, clip=False).value
        print("stoi clip | row %d: %.9f, without the minimum %.9f, allowance %.3g" %
              (u, models[u][0].value, unclipped, allowance))
        assert abs(unclipped - models[u][0].value) > allowance, (u, unclipped, models[u][0].value, allowance)
    got, seg = score(pkg, cleans, procs, fs)
    check_case("16 kHz, impulsive: E4, A, A -5 dB, C 32, A +5 dB", got, seg, models)


# ---- the engine path
def test_engine_path_scores_long_utterances_at_any_chunking(pkg):
    """an A-shaped and a B-shaped clean wave through enhance_waves(stoi=True): capacity 2000 holds the batch, 64 cuts
    inside both utterances; the second call of an engine reuses its workspaces"""
    fs, ctx = 16, 7
    cleans, noisys, _ = prepared([(sc.case_a, fs, 5), (sc.case_b, fs)])
    rng = np.random.default_rng(83)
    ls, ws, bs = small_net(rng, ctx=ctx)
    mean, inv = norm_stats(rng)
    res = []
    for cap in (2000, 64):
        eng = engine(pkg, ls, ws, bs, 16, cap=cap)
        out = eng.enhance_waves(noisys, mean, inv, fs_khz=fs, fea_context=ctx, cleans=cleans, stoi=True)
        assert len(out) == 4 and out[3].dtype == np.float32 and out[3].shape == (2,)
        assert min(w.size for w in out[0]) > 64 * 256 + 512     # more frames than the small capacity: both are cut
        want, seg = pkg.stoi_waves(cleans, out[0], fs_khz=fs, return_segments=True)
        assert np.array_equal(bits(out[3]), bits(want)) and np.isfinite(want).all()
        # the enhanced wave ends with its last whole frame: the segments are those of the clean wave cut there
        assert list(seg) == [stoi64.stoi64(c, c, fs, samples=w.size).segments for c, w in zip(cleans, out[0])]
        assert seg[0] == 4 and seg[1] > 300
        again = eng.enhance_waves(noisys, mean, inv, fs_khz=fs, fea_context=ctx, cleans=cleans, stoi=True)
        assert np.array_equal(bits(again[3]), bits(out[3]))
        for a, b in zip(again[0], out[0]):
            assert np.array_equal(a, b)
        eng.close()
        res.append(out[3])
    assert np.array_equal(bits(res[0]), bits(res[1]))
