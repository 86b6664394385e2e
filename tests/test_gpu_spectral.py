"""The spectral front end and back end on the device (wave_to_lps / lps_to_wave / BPGpu.enhance_wave, the tools
wav2lps / lps2wav / enhance_wav) against the float64 restatement of tests/spec64.py and the original project's own
recorded LPS (tests/golden/ref_lps_*.npz)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import hostlib
import spec64

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = spec64.U
TABLE = []


def record(case, ratio):
    TABLE.append((case, ratio))


@pytest.fixture(scope="module", autouse=True)
def print_table():
    yield
    if TABLE:
        print("\n%-64s %s" % ("enhance_wave / synthesis case", "worst |err| / hard bound"))
        for case, r in TABLE:
            print("%-64s %.3e" % (case, r))


def fixture(tag):
    return spec64.load_fixture(os.path.join(GOLD, "ref_lps_%s.npz" % tag))


synthesis_bound = spec64.synthesis_bound   # derivation there; sound and sharp on the CPU (tests/test_spec64.py)


@pytest.mark.parametrize("tag", ["sx289", "sx379"])
def test_analysis_within_the_bound_of_float64_on_the_recorded_utterances(pkg, tag):
    f = fixture(tag)
    got = pkg.wave_to_lps(f["samples"])
    lps64, X, E = spec64.analysis64(f["samples"])
    assert got.shape == lps64.shape == (56, 257) and got.dtype == np.float32
    assert spec64.lps_ok(got, X, E).all()
    assert np.median(np.abs(got - lps64)) <= 1e-5
    # and the original's recorded rows lie within the same bound (both are fp32 FFTs of the same frames)
    assert np.abs(got - f["lps"]).max() < 5e-3


@pytest.mark.parametrize("fs", [8, 11, 16])
def test_analysis_within_the_bound_at_every_rate(pkg, fs):
    w = spec64.synth_speech(fs * 1000 + 123, fs, seed=fs)
    got = pkg.wave_to_lps(w, fs_khz=fs)
    lps64, X, E = spec64.analysis64(w, fs)
    assert got.shape == lps64.shape
    assert spec64.lps_ok(got, X, E).all()
    assert np.median(np.abs(got - lps64)) <= 1e-5


def check_synthesis(pkg, noisy, lps, fs=16):
    out, outf = pkg.lps_to_wave(noisy, lps, fs_khz=fs, return_float=True)
    want = spec64.synthesis64(noisy, lps, fs)
    assert out.shape == outf.shape == want.shape
    assert np.all(np.abs(outf.astype(np.float64) - want) <= synthesis_bound(noisy, lps, fs))
    assert np.array_equal(out, spec64.trunc_sat(outf))           # trunc toward zero, saturated: exactly
    return out, outf


@pytest.mark.parametrize("fs", [8, 11, 16])
def test_synthesis_within_the_bound_and_round_trip(pkg, fs):
    w = spec64.synth_speech(fs * 900 + 77, fs, seed=fs + 1)
    lps = pkg.wave_to_lps(w, fs_khz=fs)
    out, _ = check_synthesis(pkg, w, lps, fs)
    assert np.abs(out.astype(np.int64) - w[:out.size].astype(np.int64)).max() <= 1   # own LPS: the wave again
    lowered = (lps - np.float32(np.log(2.0))).astype(np.float32)
    check_synthesis(pkg, w, lowered, fs)


def test_synthesis_round_trip_on_the_recorded_utterance(pkg):
    w = fixture("sx289")["samples"]
    out = pkg.lps_to_wave(w, pkg.wave_to_lps(w))
    d = out.astype(np.int64) - w.astype(np.int64)
    assert np.abs(d).max() <= 1


def test_synthesis_saturates_clipping_output(pkg):
    rng = np.random.default_rng(5)
    t = np.arange(16000)
    w = np.clip(np.round(30000 * np.sign(np.sin(2 * np.pi * 220 * t / 16000)) + rng.normal(0, 500, t.size)),
                -32768, 32767).astype(np.int16)
    lps = (pkg.wave_to_lps(w) + np.float32(np.log(4.0))).astype(np.float32)    # twice the amplitude
    out, outf = check_synthesis(pkg, w, lps)
    assert (out == 32767).sum() > 100 and (out == -32768).sum() > 100
    assert np.abs(outf).max() > 40000


def test_digital_silence_floors_and_takes_phase_zero(pkg):
    w = spec64.synth_speech(16000, 16, seed=9)
    w[4000:9000] = 0                                             # frames 16..33 are all zeros
    lps = pkg.wave_to_lps(w)
    assert np.all(lps[16:34] == -50.0)
    out, outf = check_synthesis(pkg, w, lps)
    assert np.all(out[4608:8704] == 0) and np.all(np.isfinite(outf))
    # a non-floor target on a silent frame: magnitude with phase 0
    lps2 = lps.copy()
    lps2[20:24] = 12.0
    out2, _ = check_synthesis(pkg, w, lps2)
    assert np.any(out2[5120:6400] != 0)


@pytest.mark.parametrize("extra", [0, 1, 255])
def test_trailing_samples_are_dropped(pkg, extra):
    F = 40
    n = F * 256 + 256 + extra
    w = spec64.synth_speech(n, 16, seed=extra)
    lps = pkg.wave_to_lps(w)
    assert lps.shape == (F, 257)
    out, _ = check_synthesis(pkg, w, lps)
    assert out.size == F * 256 + 256


def small_net(rng, ctx=7, hidden=(64, 48), D=257):
    ls = [ctx * D, *hidden, D]
    ws = [rng.normal(0, 0.05, (ls[i], ls[i + 1])).astype(np.float32) for i in range(len(ls) - 1)]
    bs = [rng.normal(0, 0.1, ls[i + 1]).astype(np.float32) for i in range(len(ls) - 1)]
    return ls, ws, bs


def norm_stats(rng, D=257):
    mean = rng.normal(10, 2, D).astype(np.float32)
    inv = (1.0 / rng.uniform(2, 4, D)).astype(np.float32)
    return mean, inv


def chain_from_pieces(pkg, eng, noisy, mean, inv, ctx, fs=16):
    """decode.m from the public pieces: wave_to_lps, norm, edge-replicated context, forward_frames, de-norm,
    lps_to_wave -- every elementwise step one IEEE fp32 operation."""
    lps = pkg.wave_to_lps(noisy, fs_khz=fs)
    F, half = lps.shape[0], (ctx - 1) // 2
    x = ((lps - mean) * inv).astype(np.float32)
    stream = x[np.clip(np.arange(F + 2 * half) - half, 0, F - 1)]
    y = eng.forward_frames(stream, np.arange(F, dtype=np.int32), ctx)
    den = (y / inv + mean).astype(np.float32)
    return pkg.lps_to_wave(noisy, den, fs_khz=fs, return_float=True), lps, den


def test_enhance_wave_equals_the_public_pieces_small_net(pkg):
    rng = np.random.default_rng(11)
    ls, ws, bs = small_net(rng)
    mean, inv = norm_stats(rng)
    eng = pkg.BPGpu(1, 0, ls, 128, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    noisy = spec64.synth_speech(3 * 16000 + 17, 16, seed=4)
    out, outf = eng.enhance_wave(noisy, mean, inv, fea_context=7, return_float=True)
    (pout, poutf), _, _ = chain_from_pieces(pkg, eng, noisy, mean, inv, 7)
    assert np.array_equal(outf, poutf) and np.array_equal(out, pout)
    assert np.array_equal(out, eng.enhance_wave(noisy, mean, inv))   # deterministic, repeatable
    eng.close()


def test_enhance_wave_equals_the_public_pieces_shipped_shape(pkg):
    rng = np.random.default_rng(12)
    ls, ws, bs = small_net(rng, hidden=(2048, 2048, 2048))
    ws = [(w * np.float32(0.4)).astype(np.float32) for w in ws]
    mean, inv = norm_stats(rng)
    eng = pkg.BPGpu(1, 0, ls, 512, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    noisy = spec64.synth_speech(5 * 16000, 16, seed=6)
    out, outf = eng.enhance_wave(noisy, mean, inv, fea_context=7, return_float=True)
    (pout, poutf), _, _ = chain_from_pieces(pkg, eng, noisy, mean, inv, 7)
    assert np.array_equal(outf, poutf) and np.array_equal(out, pout)
    eng.close()


def test_chunked_enhance_wave_equals_one_shot(pkg):
    rng = np.random.default_rng(13)
    ls, ws, bs = small_net(rng)
    mean, inv = norm_stats(rng)
    noisy = spec64.synth_speech(300 * 256 + 256, 16, seed=8)      # 300 frames: chunks of 64 + a partial one
    one = pkg.BPGpu(1, 0, ls, 64, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    chunked = pkg.BPGpu(1, 0, ls, 64, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0, max_cache_frames=64)
    a = one.enhance_wave(noisy, mean, inv, return_float=True)
    b = chunked.enhance_wave(noisy, mean, inv, return_float=True)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
    one.close()
    chunked.close()


def test_enhance_wave_matches_a_float64_decode_m(pkg):
    """Downstream of the analysis (checked above on its own), decode.m in float64: norm, context, MLP, de-norm,
    synthesis.  The network's fp32 error is taken, as in test_enhance_lps_tool_matches_decode_m_math, as 2e-4 of the
    largest output in the log domain, and propagated through the synthesis bound."""
    rng = np.random.default_rng(14)
    ctx = 7
    ls, ws, bs = small_net(rng)
    mean, inv = norm_stats(rng)
    eng = pkg.BPGpu(1, 0, ls, 128, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    noisy = spec64.synth_speech(2 * 16000, 16, seed=15)
    outf = eng.enhance_wave(noisy, mean, inv, fea_context=ctx, return_float=True)[1]
    lps = pkg.wave_to_lps(noisy).astype(np.float64)
    F = lps.shape[0]
    x = (lps - mean) * inv
    idx = np.clip(np.arange(F)[:, None] + np.arange(-3, 4)[None, :], 0, F - 1)
    a = x[idx].reshape(F, ctx * 257)
    for i in range(3):
        a = a @ ws[i].astype(np.float64) + bs[i]
        if i < 2:
            a = 1.0 / (1.0 + np.exp(-a))
    want_lps = a / inv.astype(np.float64) + mean
    want = spec64.synthesis64(noisy, want_lps)
    eps = 2e-4 * np.abs(want_lps).max()
    assert np.all(np.abs(outf - want) <= synthesis_bound(noisy, want_lps, lps_eps=eps))
    # and per element: decode64's propagated bound of the chain
    want64, eps64 = spec64.decode64(lps, mean, inv, ctx, ws, bs, slabs=eng.out_slabs())
    assert np.allclose(want64, want_lps, rtol=1e-12, atol=1e-9)
    r = spec64.synthesis_ratio(outf, noisy, want64, 16, lps_eps=eps64)
    record("decode.m 16 kHz ctx 7 F %d (per element)" % F, r)
    assert r <= 1.0
    eng.close()


def test_enhance_wave_argument_errors(pkg):
    rng = np.random.default_rng(16)
    ls, ws, bs = small_net(rng)
    mean, inv = norm_stats(rng)
    eng = pkg.BPGpu(1, 0, ls, 64, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    noisy = spec64.synth_speech(8000, 16, seed=1)
    with pytest.raises(pkg.MlggdError, match=r"error 1: fea_context 5"):
        eng.enhance_wave(noisy, mean, inv, fea_context=5)
    with pytest.raises(pkg.MlggdError, match=r"error 1: .*shorter than one frame"):
        eng.enhance_wave(noisy[:511], mean, inv)
    eng.close()
    ls2, ws2, bs2 = small_net(rng, ctx=7, D=129)                   # 8 kHz bins on a 16 kHz input
    eng2 = pkg.BPGpu(1, 0, ls2, 64, 0.1, 0.9, 1e-5, ws2, bs2, 2.0, 0)
    with pytest.raises(pkg.MlggdError, match=r"error 1: fea_context 7 x 257 bins"):
        eng2.enhance_wave(noisy, mean, inv, fs_khz=16)
    eng2.close()
    with pytest.raises(pkg.MlggdError, match="error 1"):
        pkg.lps_to_wave(noisy, np.zeros((5, 257), np.float32))      # frame count does not match the wave


# ---- enhance_wave against float64 at every rate, context, length and chunk capacity
def frames_wave(F, fs, seed):
    """an int16 speech-like wave of exactly F frames plus a few trailing samples (dropped)"""
    L, S, _ = spec64.params(fs)
    return spec64.synth_speech(F * S + L - S + 7, fs, seed=seed)


def check_enhance(pkg, case, fs, ctx, F, B, caps, ls=None, ws=None, bs=None, seed=0):
    """enhance_wave on a one-shot engine: bit-equal to the public pieces (chain_from_pieces), and against decode64 +
    synthesis_bound element by element; then the same weights on engines of each chunk capacity in `caps`: bit-equal
    to the one-shot output"""
    D = spec64.params(fs)[2] // 2 + 1
    rng = np.random.default_rng(seed)
    if ls is None:
        ls, ws, bs = small_net(rng, ctx=ctx, hidden=(40, 24), D=D)
    mean, inv = norm_stats(rng, D)
    noisy = frames_wave(F, fs, seed + 1)
    eng = pkg.BPGpu(1, 0, ls, B, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    out, outf = eng.enhance_wave(noisy, mean, inv, fea_context=ctx, fs_khz=fs, return_float=True)
    slabs = eng.out_slabs()
    # exact: the public pieces with the context formed in numpy -- a shifted or wrapped context stream, which the
    # float64 wave bound below is too wide to see on these nets (tests/test_spec64.py), fails here
    (pout, poutf), _, _ = chain_from_pieces(pkg, eng, noisy, mean, inv, ctx, fs)
    eng.close()
    assert np.array_equal(outf, poutf) and np.array_equal(out, pout)
    lps = pkg.wave_to_lps(noisy, fs_khz=fs)
    assert lps.shape == (F, D)
    L, S, _ = spec64.params(fs)
    assert out.shape == outf.shape == (F * S + L - S,)
    assert np.array_equal(out, spec64.trunc_sat(outf))
    want, eps = spec64.decode64(lps, mean, inv, ctx, ws, bs, slabs=slabs)
    r = spec64.synthesis_ratio(outf, noisy, want, fs, lps_eps=eps)
    record("%s: %d kHz ctx %d F %d B %d" % (case, fs, ctx, F, B), r)
    assert r <= 1.0, r
    for cap in sorted(set(c for c in caps if c >= 1)):
        ch = pkg.BPGpu(1, 0, ls, B, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0, max_cache_frames=cap)
        o2, f2 = ch.enhance_wave(noisy, mean, inv, fea_context=ctx, fs_khz=fs, return_float=True)
        ch.close()
        assert np.array_equal(f2, outf) and np.array_equal(o2, out), "capacity %d" % cap


def capacities(ctx, B, F):
    return [1, 2, ctx - 1, ctx, B - 1, B + 1, F - 1]


@pytest.mark.parametrize("ctx", [1, 3, 7, 11])
@pytest.mark.parametrize("fs", [8, 11, 16])
def test_enhance_wave_rates_and_contexts_against_float64(pkg, fs, ctx):
    B, F = 16, 37
    check_enhance(pkg, "rate x context", fs, ctx, F, B, capacities(ctx, B, F), seed=fs * 10 + ctx)


@pytest.mark.parametrize("F", [1, 2, 3, 5, 15, 17, 300])
@pytest.mark.parametrize("fs,ctx", [(16, 11), (11, 11), (8, 3)])
def test_enhance_wave_utterance_lengths_against_float64(pkg, fs, ctx, F):
    """F = 1..5 leave dead waves in a SPEC_FRAMES = 4 workgroup; F < fea_context replicates both edges into the same
    frames; F = B -/+ 1 around one bunch; 300 frames over many chunks"""
    B = 16
    caps = capacities(ctx, B, F) if F < 300 else [1, ctx, B + 1, F - 1]
    check_enhance(pkg, "length", fs, ctx, F, B, caps, seed=F * 7 + ctx)


def test_enhance_wave_config4_shape_against_float64(pkg):
    """2827-2048^3-257 (BASELINE configs 1, 4, 5: context 11 at 16 kHz), B = 128: bit-equal to the public pieces and
    to a chunked engine; the float64 check is as wide as at the shipped shape (below)"""
    rng = np.random.default_rng(31)
    ls, ws, bs = small_net(rng, ctx=11, hidden=(2048, 2048, 2048))
    ws = [(w * np.float32(0.4)).astype(np.float32) for w in ws]
    check_enhance(pkg, "config 4 net", 16, 11, 150, 128, [129], ls=ls, ws=ws, bs=bs, seed=32)


def test_enhance_wave_shipped_shape_against_float64(pkg):
    """1799-2048^3-257 at context 7 (the shipped net), B = 512: bit-equal to the public pieces and against decode64.  At
    the 2048-wide nets the network's propagated worst-case bound is wide (ratios near 1e-8 in the table), so the float64
    check only guards against gross slips; the precision rests on the bit-equality with the public pieces, whose
    forward pass tests/test_gpu_vs_float64.py checks per layer at these shapes"""
    rng = np.random.default_rng(33)
    ls, ws, bs = small_net(rng, ctx=7, hidden=(2048, 2048, 2048))
    ws = [(w * np.float32(0.4)).astype(np.float32) for w in ws]
    check_enhance(pkg, "shipped net", 16, 7, 200, 512, [], ls=ls, ws=ws, bs=bs, seed=34)


# ---- analysis and synthesis edges at every rate
@pytest.mark.parametrize("fs", [8, 11, 16])
def test_analysis_edges_at_every_rate(pkg, fs):
    L, S, N = spec64.params(fs)
    for F in range(1, 6):
        w = frames_wave(F, fs, seed=F)
        got = pkg.wave_to_lps(w, fs_khz=fs)
        _, X, E = spec64.analysis64(w, fs)
        assert got.shape == (F, N // 2 + 1)
        assert spec64.lps_ok(got, X, E).all(), F
    n = 20 * S + L
    sq = np.where((np.arange(n) // 37) % 2 == 0, 32767, -32768).astype(np.int16)
    sq[::101] = -32767
    got = pkg.wave_to_lps(sq, fs_khz=fs)
    _, X, E = spec64.analysis64(sq, fs)
    assert spec64.lps_ok(got, X, E).all()
    assert np.isfinite(got).all() and got.max() > 25.0                # full scale: e^25 and more at every rate
    k = N // 8                                                   # a pure tone on the centre of bin k: the other
    tone = np.round(10000 * np.sin(2 * np.pi * k * np.arange(n) / N)).astype(np.int16)   # bins near the FFT noise
    got = pkg.wave_to_lps(tone, fs_khz=fs)
    lps64, X, E = spec64.analysis64(tone, fs)
    assert spec64.lps_ok(got, X, E).all()
    assert np.all(np.argmax(got, axis=1) == k)


@pytest.mark.parametrize("fs", [8, 11])
def test_synthesis_silence_and_clipping_at_8_and_11_khz(pkg, fs):
    L, S, _ = spec64.params(fs)
    w = spec64.synth_speech(fs * 1000, fs, seed=fs + 40)
    w[10 * S:10 * S + 8 * S + L] = 0
    lps = pkg.wave_to_lps(w, fs_khz=fs)
    assert np.all(lps[11:18] == -50.0)
    out, outf = check_synthesis(pkg, w, lps, fs)
    assert np.all(out[11 * S + L - S:18 * S] == 0) and np.all(np.isfinite(outf))
    lps[12:16] = 12.0
    out2, outf2 = check_synthesis(pkg, w, lps, fs)
    assert np.any(out2[12 * S + L - S:15 * S] != 0)
    record("synthesis %d kHz silence, target 12" % fs, spec64.synthesis_ratio(outf2, w, lps, fs))
    rng = np.random.default_rng(fs)
    t = np.arange(fs * 1000)
    clip = np.clip(np.round(30000 * np.sign(np.sin(2 * np.pi * 220 * t / (fs * 1000.0))) + rng.normal(0, 500, t.size)),
                   -32768, 32767).astype(np.int16)
    lps_c = (pkg.wave_to_lps(clip, fs_khz=fs) + np.float32(np.log(4.0))).astype(np.float32)
    out3, outf3 = check_synthesis(pkg, clip, lps_c, fs)
    assert (out3 == 32767).sum() > 50 and (out3 == -32768).sum() > 50
    record("synthesis %d kHz clipping x2" % fs, spec64.synthesis_ratio(outf3, clip, lps_c, fs))


# ---- tools
def tool(name):
    return os.path.join(hostlib.HOST, name)


def write_wav(path, w, rate=16000):
    w = np.asarray(w, "<i2")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + 2 * w.size) + b"WAVEfmt " +
                struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16) + b"data" + struct.pack("<I", 2 * w.size) +
                w.tobytes())


def read_wav(path):
    d = open(path, "rb").read()
    assert d[:4] == b"RIFF" and d[8:16] == b"WAVEfmt " and d[36:40] == b"data"
    return np.frombuffer(d[44:], "<i2").astype(np.int16), struct.unpack("<I", d[24:28])[0]


def run(args):
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def test_wav2lps_writes_the_reference_header_and_body(pkg, tmp_path):
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    f = fixture("sx289")
    w = f["samples"]
    w.astype("<i2").tofile(tmp_path / "x.raw")
    run([tool("wav2lps"), "-F", "RAW", "-fs", "16", str(tmp_path / "x.raw"), str(tmp_path / "x.lps")])
    raw = open(tmp_path / "x.lps", "rb").read()
    ref_hdr = bytes(f["header"])
    assert raw[:12] == struct.pack(">i", 56) + ref_hdr[4:]             # the original's header, 56 frames of it
    got = np.frombuffer(raw[12:], ">f4").reshape(56, 257)
    _, X, E = spec64.analysis64(w)
    assert spec64.lps_ok(got, X, E).all()
    assert np.array_equal(got.astype(np.float32), pkg.wave_to_lps(w))
    write_wav(tmp_path / "x.wav", w)
    run([tool("wav2lps"), "-q", "-F", "WAV", str(tmp_path / "x.wav"), str(tmp_path / "y.lps")])
    assert open(tmp_path / "y.lps", "rb").read() == raw
    r = subprocess.run([tool("wav2lps"), "-F", "NIST", str(tmp_path / "x.wav"), str(tmp_path / "z.lps")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "not supported" in r.stderr


def test_enhance_wav_equals_enhance_wave(pkg, tmp_path):
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    rng = np.random.default_rng(17)
    ls, ws, bs = small_net(rng)
    mean, inv = norm_stats(rng)
    hostlib.write_wts(str(tmp_path / "mlp.wts"), ws, bs)
    hostlib.write_norm(str(tmp_path / "n.norm"), mean, inv)
    norm_mean, norm_inv = hostlib.HostNorm.read(str(tmp_path / "n.norm"), 257)   # what the tool parses
    norm_mean, norm_inv = np.asarray(norm_mean, np.float32), np.asarray(norm_inv, np.float32)
    waves = [spec64.synth_speech(16000 + 333 * i, 16, seed=20 + i) for i in range(2)]
    for i, w in enumerate(waves):
        write_wav(tmp_path / ("n%d.wav" % i), w)
    common = [tool("enhance_wav"), "wts=%s" % (tmp_path / "mlp.wts"), "norm_file=%s" % (tmp_path / "n.norm"),
              "fea_context=7", "bunchsize=512"]
    run(common + ["in=%s" % (tmp_path / "n0.wav"), "out=%s" % (tmp_path / "e0.wav")])
    with open(tmp_path / "list.scp", "w") as f:
        for i in range(2):
            f.write("%s %s\n" % (tmp_path / ("n%d.wav" % i), tmp_path / ("s%d.wav" % i)))
    run(common + ["scp=%s" % (tmp_path / "list.scp")])
    eng = pkg.BPGpu(1, 0, ls, 512, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    for i, w in enumerate(waves):
        want = eng.enhance_wave(w, norm_mean, norm_inv)
        got, rate = read_wav(tmp_path / ("s%d.wav" % i))
        assert rate == 16000 and np.array_equal(got, want)
        if i == 0:
            assert np.array_equal(read_wav(tmp_path / "e0.wav")[0], want)
    eng.close()


def test_lps2wav_writes_the_wave_and_the_quality_report(pkg, tmp_path):
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    clean = fixture("sx379")["samples"]
    noisy = np.clip(clean + np.random.default_rng(18).normal(0, 300, clean.size), -32768, 32767).astype(np.int16)
    lps = (pkg.wave_to_lps(noisy) - np.float32(0.3)).astype(np.float32)
    clean.astype("<i2").tofile(tmp_path / "c.raw")
    noisy.astype("<i2").tofile(tmp_path / "n.raw")
    with open(tmp_path / "f.htk", "wb") as f:
        f.write(struct.pack(">iihh", lps.shape[0], 160000, 257 * 4, 9) + lps.astype(">f4").tobytes())
    run([tool("lps2wav"), str(tmp_path / "c.raw"), str(tmp_path / "n.raw"), str(tmp_path / "f.htk"),
         str(tmp_path / "info.txt"), str(tmp_path / "o.raw"), "-F", "RAW", "-fs", "16"])
    got = np.fromfile(tmp_path / "o.raw", "<i2")
    assert np.array_equal(got, pkg.lps_to_wave(noisy, lps))
    lines = open(tmp_path / "info.txt").read().split("\n")
    assert lines[0] == "Segmental SNR:" and lines[2] == "Log-Spectral Distortion:" and lines[4] == ""
    snr, lsd = spec64.quality64(clean, noisy, lps)
    assert abs(float(lines[1]) - snr) <= 1e-4 and abs(float(lines[3]) - lsd) <= 1e-4
    assert len(lines[1].split(".")[1]) == 6                          # "%f"


@pytest.mark.parametrize("rate", [8000, 11000])
def test_enhance_wav_at_8_and_11_khz(pkg, tmp_path, rate):
    """the tool on 8000 / 11000 Hz RIFF files with a 129-bin net at context 11: the output equals enhance_wave at that
    rate and keeps the input's rate"""
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    fs = rate // 1000
    rng = np.random.default_rng(rate)
    ls, ws, bs = small_net(rng, ctx=11, D=129)
    mean, inv = norm_stats(rng, 129)
    hostlib.write_wts(str(tmp_path / "mlp.wts"), ws, bs)
    hostlib.write_norm(str(tmp_path / "n.norm"), mean, inv)
    norm_mean, norm_inv = hostlib.HostNorm.read(str(tmp_path / "n.norm"), 129)
    norm_mean, norm_inv = np.asarray(norm_mean, np.float32), np.asarray(norm_inv, np.float32)
    w = spec64.synth_speech(rate + 555, fs, seed=rate)
    write_wav(tmp_path / "n.wav", w, rate)
    run([tool("enhance_wav"), "wts=%s" % (tmp_path / "mlp.wts"), "norm_file=%s" % (tmp_path / "n.norm"),
         "fea_context=11", "bunchsize=64", "in=%s" % (tmp_path / "n.wav"), "out=%s" % (tmp_path / "e.wav")])
    eng = pkg.BPGpu(1, 0, ls, 64, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    want = eng.enhance_wave(w, norm_mean, norm_inv, fea_context=11, fs_khz=fs)
    eng.close()
    got, got_rate = read_wav(tmp_path / "e.wav")
    assert got_rate == rate and np.array_equal(got, want)
