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


# ---------------------------------------------------------------------------------------------------------------------
# the synthesis bound is sound (a correct fp32 twin of k_lps_synthesis + k_ola passes it) and sharp (one-line slips of
# that twin fail it by a wide margin)
RATES = (8, 11, 16)


def synthesis_inputs(fs):
    """(name, noisy wave, lps rows) at rate fs: speech-like, the two recorded utterances, a clipping wave, digital
    silence with a non-floor target, rows shifted by +-log 4"""
    L, S, _ = spec64.params(fs)
    out = []
    w = spec64.synth_speech(fs * 1000 + 321, fs, seed=fs)
    lps = spec64.analysis32(w, fs)[0]
    out.append(("speech", w, lps))
    for tag in sorted(FIXTURES):
        f = spec64.load_fixture(os.path.join(GOLD, "ref_lps_%s.npz" % tag))["samples"]
        out.append((tag, f, spec64.analysis32(f, fs)[0]))
    rng = np.random.default_rng(fs)
    t = np.arange(fs * 1000)
    clip = np.clip(np.round(30000 * np.sign(np.sin(2 * np.pi * 220 * t / (fs * 1000.0))) + rng.normal(0, 500, t.size)),
                   -32768, 32767).astype(np.int16)
    out.append(("clipping x2", clip, (spec64.analysis32(clip, fs)[0] + np.float32(np.log(4.0))).astype(np.float32)))
    sil = w.copy()
    sil[10 * S:10 * S + 8 * S + L] = 0
    lps_s = spec64.analysis32(sil, fs)[0]
    assert np.all(lps_s[11:18] == -50.0)
    lps_s[12:16] = 12.0                                           # a non-floor target on silent frames: phase 0
    out.append(("silence, target 12", sil, lps_s))
    for sgn in (1, -1):
        out.append(("lps %+d log 4" % sgn, w, (lps + np.float32(sgn * np.log(4.0))).astype(np.float32)))
    return out


def test_float32_synthesis_twin_is_within_the_synthesis_bound_at_every_rate():
    rows = []
    for fs in RATES:
        for name, w, lps in synthesis_inputs(fs):
            out, outf = spec64.synthesis32(w, lps, fs)
            r = spec64.synthesis_ratio(outf, w, lps, fs)
            rows.append((fs, name, r))
            assert r <= 1.0, (fs, name, r)
            assert np.array_equal(out, spec64.trunc_sat(outf))
            if name == "clipping x2":
                assert (out == 32767).sum() > 50 and (out == -32768).sum() > 50
    print("\nfp32 synthesis twin, worst |err| / synthesis_bound")
    for fs, name, r in rows:
        print("  %2d kHz  %-20s %.3e" % (fs, name, r))


def test_synthesis_mutation_is_killed():
    """Each slip of SYNTH_MUTATIONS on synth_speech input reaches a worst ratio of at least 10 against the bound at every
    rate, except one the bound cannot resolve at that margin:
    * twiddle_10bit (the inverse's twiddle table rounded to a 10-bit mantissa) reaches only ~3-4: the FFT term of the
      bound is the worst case C_FFT log2(N) u ||Y|| / sqrt(N), ~2^-18 of the frame's energy, while the 10-bit rounding
      errors (<= 2^-11 each, exact for 0, +-1 and the many twiddles that fit in 10 bits) enter the output with random
      signs, a factor ~100 below their worst case; it is still caught (ratio > 1), but not with a factor of 10 in hand.
    Slips the bound cannot see at all: the floor compare `<` against `<=` at exactly -50 (both give exp(-50)), and a
    one-ulp error in a single twiddle (a relative 2^-24 change, inside the per-operation u of the bound)."""
    below_10 = {"twiddle_10bit"}
    rows = []
    for fs in RATES:
        w = spec64.synth_speech(fs * 1000 + 321, fs, seed=fs)
        lps = spec64.analysis32(w, fs)[0]
        good = spec64.synthesis_ratio(spec64.synthesis32(w, lps, fs)[1], w, lps, fs)
        rows.append((fs, "(correct twin)", good))
        assert good <= 1.0
        for mut in spec64.SYNTH_MUTATIONS:
            r = spec64.synthesis_ratio(spec64.synthesis32(w, lps, fs, mut=mut)[1], w, lps, fs)
            rows.append((fs, mut, r))
            assert r >= (1.0 if mut in below_10 else 10.0), (fs, mut, r)
    print("\nsynthesis mutations, worst |err| / synthesis_bound (>= 10 required, >= 1 for %s)" % sorted(below_10))
    for fs, mut, r in rows:
        print("  %2d kHz  %-24s %.3e" % (fs, mut, r))


def test_float32_analysis_twin_is_within_the_analysis_bound_at_every_rate():
    for fs in RATES:
        for name, w, _ in synthesis_inputs(fs):
            lps32 = spec64.analysis32(w, fs)[0]
            _, X, E = spec64.analysis64(w, fs)
            assert spec64.lps_ok(lps32, X, E).all(), (fs, name)


# ---------------------------------------------------------------------------------------------------------------------
# the decode.m chain bound (decode64): an fp32 decode passes it, planted slips fail it
def chain_net(rng, ctx, D):
    ls = [ctx * D, 64, 48, D]
    Ws = [rng.normal(0, 0.05, (ls[i], ls[i + 1])).astype(np.float32) for i in range(3)]
    bs = [rng.normal(0, 0.1, ls[i + 1]).astype(np.float32) for i in range(3)]
    mean = rng.normal(10, 2, D).astype(np.float32)
    inv = (1.0 / rng.uniform(2, 4, D)).astype(np.float32)
    return Ws, bs, mean, inv


@pytest.mark.parametrize("fs,ctx", [(8, 11), (11, 3), (16, 7), (16, 1)])
def test_float32_decode_is_within_the_decode64_bound(fs, ctx):
    rng = np.random.default_rng(fs * 100 + ctx)
    D = spec64.params(fs)[2] // 2 + 1
    Ws, bs, mean, inv = chain_net(rng, ctx, D)
    w = spec64.synth_speech(fs * 1000 + 11, fs, seed=ctx)
    lps = spec64.analysis32(w, fs)[0]
    want, eps = spec64.decode64(lps, mean, inv, ctx, Ws, bs)
    got = spec64.decode32(lps, mean, inv, ctx, Ws, bs)
    assert np.all(np.abs(got - want) <= eps)
    # and the whole chain into the synthesis: the fp32 twin de-normalising on the fly, within the propagated bound
    y = spec64.decode32(lps, mean, inv, ctx, Ws, bs, mut="raw")   # network output before de-normalisation
    _, outf = spec64.synthesis32(w, y, fs, mean=mean, inv=inv)
    r = spec64.synthesis_ratio(outf, w, want, fs, lps_eps=eps)
    print("fs %d ctx %d: decode %.3e, chain into synthesis %.3e" % (fs, ctx, float((np.abs(got - want) / eps).max()), r))
    assert r <= 1.0


@pytest.mark.parametrize("mut", ["denorm_order", "shift", "wrap"])
def test_decode_chain_slip_is_killed(mut):
    """Each slip fails decode64's bound in the LPS domain.  This kill does NOT carry over to the wave domain: carried
    through synthesis_bound (which sums the per-bin error over all bins, while the real errors partly cancel) a context
    shifted by one frame or wrapped at the edges stays below a ratio of 1 on small nets (printed below).  So the GPU
    tests do not rely on the float64 wave check to see the context: tests/test_gpu_spectral.py::check_enhance also
    requires enhance_wave to equal, bit for bit, the chain built from the public pieces with the context formed in
    numpy (chain_from_pieces), at every rate, context and length."""
    for fs, ctx in ((8, 11), (16, 7), (11, 3)):
        rng = np.random.default_rng(fs * 100 + ctx)
        D = spec64.params(fs)[2] // 2 + 1
        Ws, bs, mean, inv = chain_net(rng, ctx, D)
        w = spec64.synth_speech(fs * 1000 + 11, fs, seed=ctx)
        lps = spec64.analysis32(w, fs)[0]
        want, eps = spec64.decode64(lps, mean, inv, ctx, Ws, bs)
        got = spec64.decode32(lps, mean, inv, ctx, Ws, bs, mut=mut)
        r = np.abs(got - want) / eps
        y = spec64.decode32(lps, mean, inv, ctx, Ws, bs, mut="raw")
        if mut == "denorm_order":
            wave_r = spec64.synthesis_ratio(spec64.synthesis32(w, got, fs)[1], w, want, fs, lps_eps=eps)
        else:
            sl = spec64.decode32(lps, mean, inv, ctx, Ws, bs, mut=mut)
            wave_r = spec64.synthesis_ratio(spec64.synthesis32(w, sl, fs)[1], w, want, fs, lps_eps=eps)
        print("%-12s fs %d ctx %d: LPS worst %.3e, %d elements over; wave-domain ratio %.3e" %
              (mut, fs, ctx, r.max(), (r > 1).sum(), wave_r))
        assert r.max() > 1.0 and (r > 1).sum() > 0
