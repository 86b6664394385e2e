"""CPU: the float64 definition of STOI (tests/stoi64.py) and its float32 restatement: the band table against the
original script's rule, the resampling filter, and properties of the value on a synthetic utterance (1 s at 16 kHz, a
speech-like signal with two gaps 70 dB down: 77 frames, 65 kept, 35 segments)."""
import os
import re

import numpy as np
import pytest

import stoi64

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


def test_samples_is_the_cut(clean):
    noisy = stoi64.add_noise(clean, 5, 9)
    for f in (stoi64.stoi64, stoi64.stoi32):
        assert f(clean, noisy, FS, samples=12345).value == f(clean[:12345], noisy[:12345], FS).value
