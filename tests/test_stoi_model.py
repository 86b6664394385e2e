"""CPU: the float64 definition of STOI (tests/stoi64.py) and its float32 restatement: the band table against the
original script's rule, the resampling filter, and properties of the value on a synthetic utterance (1 s at 16 kHz, a
speech-like signal with two gaps 70 dB down: 77 frames, 65 kept, 35 segments); and, for the inputs of
tests/test_gpu_stoi_edges.py (tests/stoi_cases.py): that a wrong order of the kept frames would exceed the GPU's
allowance, the counts of the sparse utterances, and the rule for a processed band of exact zeros."""
import os
import re

import numpy as np
import pytest

import stoi64
import stoi_cases as sc

FS = 16


@pytest.fixture(scope="module")
def clean():
    c = stoi64.speech(16000, FS, 3, gaps=[(3000, 5000), (9000, 10000)])
    c.setflags(write=False)
    return c


def test_the_band_table_is_the_rule_s(pkg):
    assert stoi64.thirdoct_rule() == stoi64.BANDS and len(stoi64.BANDS) == stoi64.J
    src = open(os.path.join(os.path.dirname(pkg.LIB_PATH), "stoi_rule.h")).read()
    lo = [int(v) for v in re.search(r"kBandLo\[kBands\] = \{([^}]*)\}", src).group(1).split(",")]
    hi = [int(v) for v in re.search(r"kBandHi\[kBands\] = \{([^}]*)\}", src).group(1).split(",")]
    assert list(zip(lo, hi)) == stoi64.BANDS                       # the table the kernels sum over


@pytest.mark.parametrize("fs", [8, 11, 16])
def test_the_filter_sums_to_p_and_is_symmetric(fs):
    p, q = stoi64.RATES[fs]
    h = stoi64.resample_filter(p, q)
    assert h.size == 2 * 10 * max(p, q) + 1
    assert abs(h.sum() - p) < 1e-12 and np.array_equal(h, h[::-1])
    assert abs(float(h.astype(np.float32).sum(dtype=np.float64)) - p) < 1e-5
    t = np.arange(-(h.size // 2), h.size // 2 + 1)
    g = np.sinc(t / max(p, q)) * np.kaiser(h.size, 5.0)             # numpy's Kaiser window gives the same taps
    assert np.abs(g * (p / g.sum()) - h).max() < 1e-12


@pytest.mark.parametrize("fs", [8, 11, 16])
def test_resampling_keeps_a_tone(fs):
    """a 440 Hz tone comes out as a 440 Hz tone at 10 kHz with its amplitude, away from the edges"""
    rate = {8: 8000.0, 11: 11000.0, 16: 16000.0}[fs]
    x = np.round(8000.0 * np.sin(2 * np.pi * 440.0 * np.arange(4000) / rate)).astype(np.int16)
    y = stoi64.resample(x, fs)
    assert y.size == stoi64.len10(4000, fs)
    n = np.arange(y.size)
    want = 8000.0 * np.sin(2 * np.pi * 440.0 * n / 10000.0)
    assert np.abs(y - want)[300:-300].max() < 8000.0 * 2e-3


def test_counts_of_the_synthetic_utterance(clean):
    r = stoi64.stoi64(clean, clean, FS)
    assert (r.len10, r.frames, r.kept, r.M, r.segments) == (10000, 77, 65, 64, 35)
    assert r.min_margin > 1.0 and r.min_var > 0.01


def test_a_wave_against_itself_is_one(clean):
    assert abs(stoi64.stoi64(clean, clean, FS).value - 1.0) < 1e-12


def test_the_value_falls_with_the_noise(clean):
    v = [stoi64.stoi64(clean, stoi64.add_noise(clean, snr, 9), FS).value for snr in (20, 5, -5)]
    assert 1.0 > v[0] > v[1] > v[2] > 0.2
    assert v[0] > 0.85 and v[2] < 0.6


def test_scaling_the_processed_wave_changes_nothing(clean):
    """the normalisation alpha removes a gain: halving the processed signal before any int16 rounding moves the
    float64 value by less than 1e-9"""
    noisy = stoi64.add_noise(clean, 5, 9)
    assert abs(stoi64.stoi64(clean, noisy, FS, proc_gain=0.5).value - stoi64.stoi64(clean, noisy, FS).value) < 1e-9


def test_too_short_and_silent_have_no_value(clean):
    n = stoi64.shortest_with_frames(31, FS)                        # 31 frames kept: 30 compacted, one segment
    x = stoi64.speech(n, FS, 5)
    assert stoi64.stoi64(x, x, FS).segments == 1 and stoi64.stoi32(x, x, FS).segments == 1
    for f in (stoi64.stoi64, stoi64.stoi32):
        r = f(x[:n - 1], x[:n - 1], FS)
        assert np.isnan(r.value) and r.segments == 0 and r.frames == 30
        r = f(np.zeros(16000, np.int16), clean, FS)
        assert np.isnan(r.value) and r.segments == 0 and r.kept == 0
        r = f(clean, clean, FS, samples=0)
        assert np.isnan(r.value) and r.segments == 0 and r.len10 == 0


@pytest.mark.parametrize("fs", [8, 11, 16])
def test_float32_follows_float64(fs):
    n = stoi64.shortest_with_frames(45, fs)
    c = stoi64.speech(n, fs, 11, gaps=[(n // 3, n // 3 + n // 8)])
    for snr in (15, 0):
        p = stoi64.add_noise(c, snr, 4)
        a, b = stoi64.stoi64(c, p, fs), stoi64.stoi32(c, p, fs)
        assert (a.frames, a.kept, a.segments) == (b.frames, b.kept, b.segments) and a.kept < a.frames
        assert abs(a.value - b.value) < 2e-6
    assert abs(stoi64.stoi32(c, c, fs).value - 1.0) < 2e-6


# ---- the inputs of tests/test_gpu_stoi_edges.py (tests/stoi_cases.py)
def test_a_wrong_scan_order_exceeds_the_allowance():
    """case A keeps frames 247..263 and 503..519: three kept lists that a broken scan of k_stoi_select would write
    have the right count, so the segment count cannot see them; each moves the value by more than the GPU is allowed
    (16 x the model distance of the batch A is scored in)"""
    fs = 16
    _, _, models = sc.rows(sc.trips_batch(fs))
    allowance = 16.0 * sc.model_distance(models)
    assert 2.0 ** -25 <= allowance / 16.0 < 2e-7
    true = list(range(247, 264)) + list(range(503, 520))
    swapped = list(true)
    i = swapped.index(sc.TRIP)
    swapped[i - 1], swapped[i] = swapped[i], swapped[i - 1]                    # frames 255 and 256 change places
    neighbour = list(true)
    neighbour[i] = 264                                                         # trip 2's first kept frame: the nearest dropped one
    trip2 = [t for t in true if sc.TRIP <= t < 2 * sc.TRIP]
    carry = list(true)
    carry[i:i + len(trip2)] = [0] * len(trip2)                                 # trip 2 written from offset 0: its own
    carry[:len(trip2)] = trip2                                                 # places keep a cleared buffer's frame 0
    for snr in (5, -5):
        c, p = sc.case_a(fs, snr)
        m64, m32 = sc.models(sc.case_a, fs, snr)
        assert m64.kept == len(true) and stoi64.stoi64(c, p, fs, kept=true).value == m64.value
        assert stoi64.stoi32(c, p, fs, kept=true).value == m32.value
        for name, kept in (("swapped", swapped), ("neighbour", neighbour), ("carry", carry)):
            assert len(kept) == len(true) and kept != true
            for f in (stoi64.stoi64, stoi64.stoi32):
                r = f(c, p, fs, kept=kept)
                assert r.segments == m64.segments
                assert abs(r.value - m64.value) > allowance, (name, snr, f.__name__, r.value, m64.value, allowance)


@pytest.mark.parametrize("fs", [8, 16])
def test_counts_of_the_sparse_utterances(pkg, fs):
    """bursts of one frame keep 2 frames each, a burst of a frame and a half 3: 32, 31 and 30 kept of 300 frames; the
    compacted frames and segments of a kept count are those mlggd_stoi_layout gives an utterance of that many frames"""
    for variant, (ones, longs) in sc.C_VARIANTS.items():
        assert 2 * ones + 3 * longs == variant
        c, _ = sc.case_c(fs, variant)
        for m in sc.models(sc.case_c, fs, variant):
            assert (m.len10, m.frames) == pkg.stoi_layout(c.size, fs_khz=fs)[:2] and m.frames == 300
            assert (m.kept, m.M) == (variant, variant - 1)
            assert m.segments == pkg.stoi_layout(stoi64.shortest_with_frames(m.kept, fs), fs_khz=fs)[2] == variant - 30
            assert np.isnan(m.value) == (variant == 30)
        assert pkg.stoi_layout(c.size, fs_khz=fs)[2] == 300 - 30               # the bound: every frame kept


def test_a_zero_band_over_a_segment_has_no_value():
    """the definition: sum Y^2 = 0 in a band of a segment -> alpha = inf, alpha Y = NaN, the minimum keeps it"""
    fs = 16
    plain = sc.models(sc.case_e, fs, 0)[0]
    assert plain.segments == 125 and np.isfinite(plain.value)
    for kind in (1, 2):
        for m in sc.models(sc.case_e, fs, kind):
            assert np.isnan(m.value) and (m.frames, m.kept, m.M, m.segments) == (155, 155, 154, 125)
    for m in sc.models(sc.case_e, fs, 3):
        assert np.isfinite(m.value) and m.segments == 125 and 0.2 < m.value < plain.value


def test_samples_is_the_cut(clean):
    noisy = stoi64.add_noise(clean, 5, 9)
    for f in (stoi64.stoi64, stoi64.stoi32):
        assert f(clean, noisy, FS, samples=12345).value == f(clean[:12345], noisy[:12345], FS).value
