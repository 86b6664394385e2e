"""The float64 spectral restatement (tests/spec64.py) against the original project's own recorded front-end output
(tests/golden/ref_lps_*.npz, made by tools/make_spec_golden.py), and its synthesis identities (CPU only)."""
import os
import struct

import numpy as np
import pytest

import spec64

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = {"sx289": 168, "sx379": 156}


@pytest.fixture(scope="module", params=sorted(FIXTURES))
def fixture(request):
    f = spec64.load_fixture(os.path.join(GOLD, "ref_lps_%s.npz" % request.param))
    f["tag"] = request.param
    return f


def test_restatement_reproduces_the_recorded_lps_within_the_fft_bound(fixture):
    lps, X, E = spec64.analysis64(fixture["samples"])
    rec = fixture["lps"]
    assert rec.shape == lps.shape == (56, 257)
    assert spec64.lps_ok(rec, X, E).all()
    assert spec64.lps_err_ratio(rec, X, E) < 1.0
    d = np.abs(rec.astype(np.float64) - lps)
    assert d.max() <= 3.1e-3                          # the original's own fp32 FFT rounding (SX379 frame 44: 3.0e-3)
    assert d[np.exp(lps) > 1e2].max() <= 3e-4
    assert np.median(d) < 1e-6


def test_frame_count_and_header_match_the_recorded_file(fixture):
    n, F = int(fixture["n_samples"]), int(fixture["n_frames"])
    assert F == FIXTURES[fixture["tag"]]
    assert spec64.n_frames(n, 16) == F
    assert bytes(fixture["header"]) == struct.pack(">iihh", F, 160000, 257 * 4, 9)


def test_frame_counts_at_every_rate():
    for fs, (L, S, _) in spec64.PARAMS.items():
        assert spec64.n_frames(L - 1, fs) == 0
        assert spec64.n_frames(L, fs) == 1
        assert spec64.n_frames(L + S - 1, fs) == 1
        assert spec64.n_frames(L + S, fs) == 2


def test_own_lps_returns_the_wave_within_one_sample(fixture):
    w = fixture["samples"]
    lps, _, _ = spec64.analysis64(w)
    y = spec64.synthesis64(w, lps)
    d = spec64.trunc_sat(y).astype(np.int64) - w.astype(np.int64)
    assert np.abs(d).max() <= 1
    assert np.all(d * np.sign(w) <= 0)                  # truncation: off only toward zero
    assert 0.3 < float((d != 0).mean()) < 0.6           # ~44 %: the round trip lands just below the integer


def test_lps_lowered_by_log2_returns_trunc_x_over_sqrt2(fixture):
    w = fixture["samples"]
    lps, _, _ = spec64.analysis64(w)
    got = spec64.trunc_sat(spec64.synthesis64(w, lps - np.log(2.0)))
    assert np.array_equal(got, np.trunc(w / np.sqrt(2.0)).astype(np.int16))


def test_quality_of_the_noisy_wave_against_itself(fixture):
    w = fixture["samples"]
    lps, _, _ = spec64.analysis64(w)
    snr, lsd = spec64.quality64(w, w, lps)
    assert snr == 30.0 and abs(lsd) < 1e-9
    noisy = np.clip(w + np.random.default_rng(3).normal(0, 200, w.size), -32768, 32767).astype(np.int16)
    lps_n, _, _ = spec64.analysis64(noisy)
    snr, lsd = spec64.quality64(w, noisy, lps_n)
    assert -20.0 < snr < 30.0 and lsd > 0.1


def test_bound_holds_for_a_float32_fft_at_every_rate():
    """The bound is not vacuous: a plain float32 FFT (numpy's, in single precision) stays inside it, and a
    perturbation of a few times the bound in one bin is caught."""
    for fs in (8, 11, 16):
        w = spec64.synth_speech(4000, fs, seed=fs)
        lps64, X, E = spec64.analysis64(w, fs)
        L, S, N = spec64.params(fs)
        xw = (spec64.frames(w, fs).astype(np.float32) * spec64.window(L)).astype(np.float32)
        X32 = np.fft.rfft(xw, n=N, axis=1).astype(np.complex64)
        P = (X32.real * X32.real + X32.imag * X32.imag).astype(np.float32)
        with np.errstate(divide="ignore"):
            lps32 = np.where(P >= np.float32(spec64.FLOOR_P), np.log(P.astype(np.float64)), -50.0).astype(np.float32)
        assert spec64.lps_ok(lps32, X, E).all()
        bad = lps32.copy()
        k = int(np.argmax(np.abs(X[3])))
        bad[3, k] += np.float32(20 * E[3] / np.abs(X[3, k]))
        assert not spec64.lps_ok(bad, X, E).all()
