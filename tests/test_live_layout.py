"""CPU: mlggd_live_layout, the emission rule of a live group (BPGpu.live), against a restatement of the rule: at every
rate and context, around every boundary of the frame count; the per-push counts of any cutting of a recording
telescope to the single call's length; argument checks.  No device is needed."""
import numpy as np
import pytest

import spec64

RATES = [8, 11, 16]
CONTEXTS = [1, 7, 11]


def emitted(n, ended, fs, ctx):
    """samples a session has emitted after n samples: the rule of include/mlggd.h restated"""
    L, S, _ = spec64.params(fs)
    half = (ctx - 1) // 2
    F = 0 if n < L else (n - (L - S)) // S
    if ended:
        return F * S + L - S if F > 0 else 0
    return max(0, F - half) * S


def rule(had, add, end, fs, ctx):
    counts = [emitted(h + a, e, fs, ctx) - emitted(h, False, fs, ctx) for h, a, e in zip(had, add, end)]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def boundaries(fs, ctx):
    L, S, _ = spec64.params(fs)
    half = (ctx - 1) // 2
    pts = {0, 1, L - 1, L, L + 1}
    for k in range(half + 3):
        pts |= {L + k * S - 1, L + k * S, L + k * S + 1}
    return sorted(pts)


@pytest.mark.parametrize("ctx", CONTEXTS)
@pytest.mark.parametrize("fs", RATES)
def test_layout_equals_the_rule_around_every_boundary(pkg, fs, ctx):
    """had + add on L - 1, L and L + k S - 1, L + k S, L + k S + 1 for k up to half + 2, from every had below it (add =
    0 included), running and ended: an end below L samples, an end with F <= half, an end with nothing added"""
    pts = boundaries(fs, ctx)
    had, add, end = [], [], []
    for total in pts:
        for h in [p for p in pts if p <= total]:
            for e in (0, 1):
                had.append(h), add.append(total - h), end.append(e)
    got = pkg.live_layout(had, add, end, fs_khz=fs, fea_context=ctx)
    want = rule(had, add, end, fs, ctx)
    assert got.dtype == np.int64 and np.array_equal(got, want)
    assert np.array_equal(pkg.live_layout(had, add, None, fs_khz=fs, fea_context=ctx), rule(had, add, [0] * len(had), fs, ctx))
    L, S, _ = spec64.params(fs)
    half = (ctx - 1) // 2
    assert pkg.live_layout([0], [L - 1], [1], fs, ctx).tolist() == [0, 0]            # ended below one frame: nothing
    assert pkg.live_layout([0], [L], [1], fs, ctx).tolist() == [0, L]                # one frame, both edges at once
    assert pkg.live_layout([0], [L + half * S - 1], [0], fs, ctx).tolist() == [0, 0]  # F = half: nothing decodable yet
    assert pkg.live_layout([0], [L + half * S], [0], fs, ctx).tolist() == [0, S]
    assert pkg.live_layout([L + half * S], [0], [1], fs, ctx).tolist() == [0, half * S + L - S]  # the end alone


@pytest.mark.parametrize("ctx", CONTEXTS)
@pytest.mark.parametrize("fs", RATES)
def test_counts_of_any_cutting_telescope(pkg, fs, ctx):
    L, S, _ = spec64.params(fs)
    half = (ctx - 1) // 2
    rng = np.random.default_rng(1000 * fs + ctx)
    for n in [0, 1, L - 1, L, L + S - 1, L + 3 * S + 5, L + (half + 4) * S + 17, int(rng.integers(L, 40 * S))]:
        for _ in range(4):
            cuts = np.sort(rng.integers(0, n + 1, int(rng.integers(0, 12))))
            sizes = np.diff(np.concatenate([[0], cuts, [n]]))
            had, total = 0, 0
            for i, a in enumerate(sizes):
                last = i == len(sizes) - 1
                total += int(pkg.live_layout([had], [a], [last], fs, ctx)[1])
                had += int(a)
                if not last:
                    F = 0 if had < L else (had - (L - S)) // S
                    assert total == max(0, F - half) * S                 # every running prefix
            F = 0 if n < L else (n - (L - S)) // S
            assert total == (F * S + L - S if n >= L else 0)


def test_argument_checks(pkg):
    with pytest.raises(pkg.MlggdError, match=r"error 1: session 1: .*negative"):
        pkg.live_layout([0, 5], [3, -1])
    with pytest.raises(pkg.MlggdError, match=r"error 1: session 0: .*negative"):
        pkg.live_layout([-2], [3])
    with pytest.raises(pkg.MlggdError, match=r"error 1: fs_khz 12"):
        pkg.live_layout([0], [3], fs_khz=12)
    with pytest.raises(pkg.MlggdError, match=r"error 1: fea_context 4 must be odd"):
        pkg.live_layout([0], [3], fea_context=4)
    with pytest.raises(pkg.MlggdError, match=r"error 1: n_sessions 0 < 1"):
        pkg.live_layout([], [])
    with pytest.raises(pkg.MlggdError, match=r"error 1: session 0: .*exceed"):
        pkg.live_layout([2 ** 31 - 2000], [2000])
    with pytest.raises(ValueError):
        pkg.live_layout([0, 1], [3])
    with pytest.raises(ValueError):
        pkg.live_layout([0, 1], [3, 4], end=[1])
    import ctypes as C
    lp = C.POINTER(C.c_int64)
    one = np.zeros(2, np.int64)
    assert pkg.load().mlggd_live_layout(16, 7, 1, None, one.ctypes.data_as(lp), None, one.ctypes.data_as(lp)) == 1
    assert "NULL" in pkg.load().mlggd_last_error().decode()
