"""CPU: spec64.score_tree_mean32 / score_floors64, the model of the two means and the floors of k_score_utt, and the
proof that the inputs of tests/test_gpu_score_waves_edges.py see each planted slip: on those very inputs a slip moves
a result by more than 100 x the distance check_case allows on that batch (MARGIN x the float32 model's distance to
float64).  The one exception is stated where it is tested: adding the 16 partials left to right instead of by the
halving tree is another valid float32 order, a few ulps away by construction, so no accuracy bound can see it; the
inputs are shown to change its bits, which is what the bit-exact GPU case compares."""
import numpy as np
import pytest

import spec64
import test_gpu_score_waves as base
import test_gpu_score_waves_edges as edges

F32 = np.float32
U = spec64.U
SEEN = 100.0


def model(cleans, noisys, lps, fs):
    """per utterance the float32 model's per-frame (snr, lsd); and what check_case allows on the batch, per quantity"""
    frames = [base.quality32(c, n, l, fs, per_frame=True) for c, n, l in zip(cleans, noisys, lps)]
    want = [spec64.quality64(c, n, l, fs) for c, n, l in zip(cleans, noisys, lps)]
    got = [base.quality32(c, n, l, fs) for c, n, l in zip(cleans, noisys, lps)]
    allowed = [base.MARGIN * max(abs(g[q] - w[q]) for g, w in zip(got, want)) for q in (0, 1)]
    assert all(a > 0 for a in allowed)
    return frames, allowed


def moved(v, slip):
    return abs(float(spec64.score_tree_mean32(v, slip)) - float(spec64.score_tree_mean32(v)))


# ---- the model itself
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 31, 32, 33, 64, 65, 1024, 1030])
def test_tree_mean_is_a_float32_mean(n):
    """n - 1 additions and a division, each within u relative of a partial sum bounded by n max|v|"""
    rng = np.random.default_rng(n)
    for v in (rng.uniform(-20, 30, n).astype(F32), rng.uniform(0, 300, n).astype(F32), np.full(n, 7.3, F32)):
        got = spec64.score_tree_mean32(v)
        assert got.dtype == F32
        assert abs(float(got) - v.astype(np.float64).mean()) <= n * U * float(np.abs(v).max())
    assert spec64.score_tree_mean32(v[:1]) == v[0]


def test_tree_mean_order_by_hand():
    """18 values: partials 0 and 1 hold two, the tree pairs (0, 8), (4, 12), ... as written out here"""
    v = (np.arange(18) * F32(1.1) + F32(0.3)).astype(F32)
    s = [F32(0.0) + x for x in v[:16]]
    s[0], s[1] = s[0] + v[16], s[1] + v[17]
    q = [s[i] + s[i + 8] for i in range(8)]
    r = [q[i] + q[i + 4] for i in range(4)]
    t = (r[0] + r[2]) + (r[1] + r[3])
    assert spec64.score_tree_mean32(v) == F32(t / F32(18))
    first = [F32(0.0) + x for x in v[:16]]
    q = [first[i] + first[i + 8] for i in range(8)]
    r = [q[i] + q[i + 4] for i in range(4)]
    assert spec64.score_tree_mean32(v, "first_trip_only") == F32(((r[0] + r[2]) + (r[1] + r[3])) / F32(18))
    assert spec64.score_tree_mean32(v, "divide_by_padded_count") == F32(t / F32(32))
    lr = s[0]
    for i in range(1, 16):
        lr = lr + s[i]
    assert spec64.score_tree_mean32(v, "left_to_right") == F32(lr / F32(18))
    v16 = v[:16]
    assert spec64.score_tree_mean32(v16, "first_trip_only") == spec64.score_tree_mean32(v16) == \
        spec64.score_tree_mean32(v16, "divide_by_padded_count")


def test_floors64():
    pc = np.array([[1.0, 2.0], [8.0, 3.0], [4.0, 100.0]])
    pd = np.array([[5.0, 1.0], [2.0, 2.0], [50.0, 1.0]])
    assert spec64.score_floors64(pc, pd) == (100.0 * 1e-5, 50.0 * 1e-5)
    assert spec64.score_floors64(pc, pd, first=2) == (8.0 * 1e-5, 5.0 * 1e-5)
    assert spec64.score_floors64(pc, pd, first=3) == spec64.score_floors64(pc, pd)


# ---- the inputs of the GPU cases see the slips
@pytest.mark.parametrize("fs", [8, 11])
def test_the_tree_batch_sees_every_slip(fs):
    """test_frame_counts_around_the_wavefront_count / test_segsnr_is_the_documented_tree_over_its_frames"""
    cleans, noisys, lps = edges.tree_batch(fs)
    frames, allowed = model(cleans, noisys, lps, fs)
    for F, pf in zip(edges.TREE_FRAMES, frames):
        assert pf[0].size == pf[1].size == F
        for q in (0, 1):
            if F > 16:
                assert moved(pf[q], "first_trip_only") > SEEN * allowed[q], (F, q)
            else:
                assert moved(pf[q], "first_trip_only") == 0.0
            if F % 16:
                assert moved(pf[q], "divide_by_padded_count") > SEEN * allowed[q], (F, q)


@pytest.mark.parametrize("fs", [8, 11])
def test_the_order_batch_sees_the_order_of_the_partials(fs):
    """test_segsnr_is_the_documented_tree_over_its_frames.  Adding the 16 partials left to right is another valid
    float32 order: it stays within a few ulps of the tree, below any accuracy bound, and the division's rounding often
    hides it.  Over the 22 utterances of order_batch it changes the bits of several means, so a bit-exact comparison of
    all of them sees it"""
    cleans, noisys, lps = edges.order_batch(fs)
    frames = [base.quality32(c, n, l, fs, per_frame=True)[0] for c, n, l in zip(cleans, noisys, lps)]
    assert len(frames) == 22 and all(v.size > 16 for v in frames)
    assert all(moved(v, "left_to_right") <= v.size * U * 30.0 for v in frames)
    changed = sum(spec64.score_tree_mean32(v, "left_to_right") != spec64.score_tree_mean32(v) for v in frames)
    print("left_to_right changes the bits of %d of %d means" % (changed, len(frames)))
    assert changed >= 4


def test_the_periodic_batch_has_equal_frames_and_sees_the_slips():
    """test_both_means_are_the_documented_tree_over_equal_frames: the model's per-frame values are all equal within an
    utterance, so the F-frame result is the tree mean of F copies of one value.  (Across utterances the model's
    values differ in the last bits, because numpy's row sums take another order for another array shape; the kernels'
    order per frame is fixed.)"""
    cleans, noisys, lps = edges.periodic_batch()
    frames, allowed = model(cleans, noisys, lps, 8)
    for F, pf in zip(edges.PERIODIC_FRAMES, frames):
        for q in (0, 1):
            v = pf[q][0]
            assert pf[q].size == F and (pf[q] == v).all() and np.isfinite(v) and -20.0 < v and (q or v < 30.0)
            assert abs(float(v) - float(frames[0][q][0])) <= 8 * U * abs(float(v))
            if F > 16:
                assert moved(pf[q], "first_trip_only") > SEEN * allowed[q]
                assert moved(pf[q], "divide_by_padded_count") > SEEN * allowed[q]


def test_the_long_batch_needs_the_floors_of_a_frame_past_1024():
    """test_more_than_1024_frames: the floors engage inside the 1030-frame utterance, and floors taken over its first
    1024 frames only (the maxima loop of k_score_utt not coming round again) are seen"""
    fs = 8
    cleans, noisys, lps = edges.long_batch()
    frames, allowed = model(cleans, noisys, lps, fs)
    pd = np.exp(lps[0].astype(np.float64))
    pc = np.abs(spec64.spectrum64(cleans[0], fs)[0]) ** 2
    assert int(pd.max(axis=1).argmax()) in (edges.LOUD_AT - 1, edges.LOUD_AT, edges.LOUD_AT + 1)
    assert int(pc.max(axis=1).argmax()) == edges.LOUD_AT
    assert (pd < 1e-5 * pd.max()).mean() > 0.05 and (pc < 1e-5 * pc.max()).mean() > 0.05
    mc, md = spec64.score_floors64(pc, pd)
    mc1, md1 = spec64.score_floors64(pc, pd, first=1024)
    assert mc1 < 0.1 * mc and md1 < 0.1 * md
    full = spec64.quality64(cleans[0], noisys[0], lps[0], fs)
    early = spec64.quality64(cleans[0], noisys[0], lps[0], fs, floors_first=1024)
    print("LSD %.6f, with the floors of the first 1024 frames %.6f; allowed %.3g" % (full[1], early[1], allowed[1]))
    assert early[0] == full[0] and abs(early[1] - full[1]) > SEEN * allowed[1]
    for u in (1, 2, 3):                                              # no loud frame: the same floors either way
        assert spec64.quality64(cleans[u], noisys[u], lps[u], fs, floors_first=1024) == \
            spec64.quality64(cleans[u], noisys[u], lps[u], fs)
    for F, pf in zip(edges.LONG_FRAMES, frames):
        for q in (0, 1):
            assert moved(pf[q], "first_trip_only") > SEEN * allowed[q]
            assert moved(pf[q], "divide_by_padded_count") > SEEN * allowed[q]


def test_the_many_batch_is_what_its_case_says():
    cleans, noisys, lps = edges.many_batch()
    frames = [l.shape[0] for l in lps]
    assert len(frames) == edges.N_MANY == 3000 and set(frames) == {1, 2, 3}
    assert all(spec64.n_frames(c.size, 8) == f == spec64.n_frames(n.size, 8) for c, n, f in zip(cleans, noisys, frames))
    assert 2 ** 11 < edges.N_MANY < 2 ** 12


# ---- |X| = 0
@pytest.mark.parametrize("fs", [8, 16])
def test_phase_0_where_the_noisy_spectrum_is_zero(fs):
    """test_silence_in_the_noisy_wave_and_full_scale: where |X| = 0 the estimate is the inverse transform of the bare
    magnitude (host/tool_io.h quality()); quality64 and quality32 both take that branch and agree"""
    L, S, N = spec64.params(fs)
    cleans, noisys, lps = edges.silence_batch(fs)
    assert not noisys[1].any() and not noisys[0][3 * S:4 * S + L].any() and noisys[0][:3 * S].any()
    mag = np.sqrt(np.exp(lps[1].astype(np.float64)))
    est = np.fft.irfft(mag + 0j, n=N, axis=1)[:, :L] / spec64.window(L).astype(np.float64)     # de-windowed
    cf = spec64.frames(cleans[1], fs)
    snr = np.clip(10.0 * np.log10((cf * cf).sum(axis=1) / ((est - cf) ** 2).sum(axis=1)), -20.0, 30.0)
    assert abs(spec64.quality64(cleans[1], noisys[1], lps[1], fs)[0] - snr.mean()) < 1e-9
    for u, (c, n, l) in enumerate(zip(cleans, noisys, lps)):
        q64, q32 = spec64.quality64(c, n, l, fs), base.quality32(c, n, l, fs)
        if u == edges.SILENT_ONE_FRAME:
            assert q64 == (-20.0, np.inf) == q32
        else:
            assert np.isfinite(q64).all() and abs(q32[0] - q64[0]) < 1e-4 and abs(q32[1] - q64[1]) < 1e-4, (u, q64, q32)
    # the frame silent in both waves enters its utterance as -20
    pf = base.quality32(cleans[2], noisys[2], lps[2], fs, per_frame=True)
    assert pf[0][2] == F32(-20.0) and np.isfinite(pf[1]).all()
    assert np.abs(cleans[3]).min() == 32767 and np.abs(noisys[3]).min() == 32767
