"""GPU: mlggd_lps_stats -- per bin the sum and the sum of squares of the LPS rows of a list of waves -- against the
float64 sums over wave_to_lps's own rows, within the bound of any summation order; and norm_from_stats on top of it."""
import math

import numpy as np
import pytest

import spec64

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


def waves_for(fs):
    """a dozen short waves: one of a single frame, one shorter than a frame (no rows), one empty -- and at 8 kHz one
    long enough that the rows leave the first 1024-row workgroup"""
    L, S, _ = spec64.params(fs)
    frames = [1, 2, 3, 5, 9, 17, 33, 4, 1, 40, 12, 7]
    waves = [spec64.synth_speech(F * S + L - S + 3 * i, fs, seed=fs + i) for i, F in enumerate(frames)]
    waves.insert(3, spec64.synth_speech(L - 1, fs, seed=99))
    waves.insert(7, np.zeros(0, np.int16))
    if fs == 8:
        waves.insert(5, spec64.synth_speech(1100 * S + L - S, fs, seed=5))
    return waves


@pytest.fixture(scope="module", params=[8, 16])
def case(pkg, request):
    fs = request.param
    waves = waves_for(fs)
    rows = [pkg.wave_to_lps(w, fs_khz=fs) for w in waves]
    return fs, waves, rows, pkg.lps_stats(waves, fs_khz=fs)


def reference(rows):
    """(n, sums [2][D] correctly rounded, sum |term| [2][D]) over the float32 rows in float64; x * x is exact"""
    x = np.concatenate(rows).astype(np.float64)
    terms = (x, x * x)
    sums = np.array([[math.fsum(t[:, d]) for d in range(x.shape[1])] for t in terms])
    mags = np.array([[math.fsum(np.abs(t[:, d])) for d in range(x.shape[1])] for t in terms])
    return x.shape[0], sums, mags


def within(got, n, sums, mags):
    bound = n * U / (1 - n * U) * mags
    err = np.abs(got - sums)
    print("n %d: largest error / bound %.3g" % (n, float((err / bound).max())))
    return bool((err <= bound).all())


def test_the_frame_count_is_wave_to_lps_own(case):
    fs, waves, rows, (n, sums) = case
    assert n == sum(r.shape[0] for r in rows) and sums.shape == (2, rows[0].shape[1]) and sums.dtype == np.float64
    assert any(r.shape[0] == 1 for r in rows) and any(r.shape[0] == 0 for r in rows)
    assert fs != 8 or n > 1024


def test_every_sum_is_within_the_bound_of_any_summation_order(case):
    fs, waves, rows, (n, sums) = case
    assert within(sums, *reference(rows))


def test_two_calls_return_the_same_bits(pkg, case):
    fs, waves, rows, (n, sums) = case
    n2, sums2 = pkg.lps_stats(waves, fs_khz=fs)
    assert n2 == n and sums2.tobytes() == sums.tobytes()


def test_two_halves_add_up_to_the_whole(pkg, case):
    fs, waves, rows, (n, sums) = case
    h = len(waves) // 2
    na, a = pkg.lps_stats(waves[:h], fs_khz=fs)
    nb, b = pkg.lps_stats(waves[h:], fs_khz=fs)
    assert na + nb == n and na == sum(r.shape[0] for r in rows[:h])
    assert within(a + b, *reference(rows))


def test_the_norm_vectors_normalise_the_rows(pkg, case):
    fs, waves, rows, (n, sums) = case
    mean, inv = pkg.norm_from_stats(n, sums)
    x = np.concatenate(rows).astype(np.float64)
    # one float32 rounding (2^-24) of values whose double error is far below it
    assert np.allclose(mean, x.mean(0), rtol=2.0 ** -23, atol=0) and np.allclose(inv, 1.0 / x.std(0), rtol=2.0 ** -23, atol=0)
