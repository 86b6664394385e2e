"""GPU: BPGpu.enhance_waves (mlggd_enhance_waves) -- a list of utterances packed into one frame stream -- against the
per-utterance call enhance_wave, bit for bit on the int16 wave, the float32 wave and the de-normalised LPS rows:
whatever the neighbours, the position in the batch, the batch and the chunk capacity; against float64 per element; its
workspace reuse and argument checks; and the enhance_wav tool's batched lists against its per-utterance loop."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import hostlib
import spec64

pytestmark = pytest.mark.gpu
MIXED_F = [1, 2, 3, 5, 17, 300]


def small_net(rng, ctx=7, hidden=(40, 24), D=257):
    ls = [ctx * D, *hidden, D]
    ws = [rng.normal(0, 0.05, (ls[i], ls[i + 1])).astype(np.float32) for i in range(len(ls) - 1)]
    bs = [rng.normal(0, 0.1, ls[i + 1]).astype(np.float32) for i in range(len(ls) - 1)]
    return ls, ws, bs


def norm_stats(rng, D=257):
    mean = rng.normal(10, 2, D).astype(np.float32)
    inv = (1.0 / rng.uniform(2, 4, D)).astype(np.float32)
    return mean, inv


def frames_wave(F, fs, seed, extra=7):
    """an int16 speech-like wave of exactly F frames plus a few trailing samples (dropped)"""
    L, S, _ = spec64.params(fs)
    return spec64.synth_speech(F * S + L - S + extra, fs, seed=seed)


def engine(pkg, ls, ws, bs, B, cap=0):
    return pkg.BPGpu(1, 0, ls, B, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0, max_cache_frames=cap)


def lps_from_pieces(pkg, eng, noisy, mean, inv, ctx, fs):
    """the enhanced LPS rows as enhance_wav.cc forms them for one pair: wave_to_lps, normalise, edge-replicated
    context, forward_frames, y / inv + mean -- every elementwise step one IEEE fp32 operation"""
    lps = pkg.wave_to_lps(noisy, fs_khz=fs)
    F, half = lps.shape[0], (ctx - 1) // 2
    x = ((lps - mean) * inv).astype(np.float32)
    stream = x[np.clip(np.arange(F + 2 * half) - half, 0, F - 1)]
    y = eng.forward_frames(stream, np.arange(F, dtype=np.int32), ctx)
    return (y / inv + mean).astype(np.float32)


def same(got, want):
    """lists of arrays equal in every bit (and in shape and type)"""
    assert len(got) == len(want)
    for u, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), "utterance %d" % u


def check_equals_single(pkg, eng, waves, mean, inv, ctx, fs, lps=True):
    out, outf, den = eng.enhance_waves(waves, mean, inv, fs_khz=fs, fea_context=ctx, return_f32=True, return_lps=True)
    singles = [eng.enhance_wave(w, mean, inv, fea_context=ctx, fs_khz=fs, return_float=True) for w in waves]
    same(out, [s[0] for s in singles])
    same(outf, [s[1] for s in singles])
    if lps:
        same(den, [lps_from_pieces(pkg, eng, w, mean, inv, ctx, fs) for w in waves])
    return out, outf, den


# ---- equals the single call
@pytest.mark.parametrize("ctx", [11, 1, 7])
@pytest.mark.parametrize("fs", [8, 11, 16])
def test_mixed_lengths_equal_the_single_call(pkg, fs, ctx):
    """F = 1, 2, 3, 5 are shorter than the half context of 11 (and leave dead waves in a 4-frame workgroup); the bunches
    of 16 run across every utterance boundary"""
    D = spec64.params(fs)[2] // 2 + 1
    rng = np.random.default_rng(100 * fs + ctx)
    ls, ws, bs = small_net(rng, ctx=ctx, D=D)
    mean, inv = norm_stats(rng, D)
    waves = [frames_wave(F, fs, seed=fs + 10 * i, extra=3 * i) for i, F in enumerate(MIXED_F)]
    frames = pkg.enhance_waves_layout([w.size for w in waves], fs)[0]
    assert frames.tolist() == MIXED_F
    eng = engine(pkg, ls, ws, bs, 16)
    out, outf, den = check_equals_single(pkg, eng, waves, mean, inv, ctx, fs)
    L, S, _ = spec64.params(fs)
    for F, o, f, d in zip(MIXED_F, out, outf, den):
        assert o.shape == f.shape == (F * S + L - S,) and d.shape == (F, D)
        assert np.array_equal(o, spec64.trunc_sat(f))
    same(eng.enhance_waves(waves, mean, inv, fs_khz=fs), out)       # fea_context from the shape; int16 output alone
    eng.close()


def test_shipped_shape_equals_the_single_call(pkg):
    """1799-2048^3-257, bunches of 512, twenty utterances of 2 to 4 s"""
    rng = np.random.default_rng(41)
    ls, ws, bs = small_net(rng, ctx=7, hidden=(2048, 2048, 2048))
    ws = [(w * np.float32(0.4)).astype(np.float32) for w in ws]
    mean, inv = norm_stats(rng)
    waves = [spec64.synth_speech(int(n), 16, seed=50 + i) for i, n in enumerate(rng.integers(2 * 16000, 4 * 16000, 20))]
    eng = engine(pkg, ls, ws, bs, 512)
    check_equals_single(pkg, eng, waves, mean, inv, 7, 16)
    eng.close()


# ---- neighbour and order independence
def test_an_utterance_does_not_see_its_neighbours_or_its_position(pkg):
    fs, ctx = 16, 11
    rng = np.random.default_rng(42)
    ls, ws, bs = small_net(rng, ctx=ctx)
    mean, inv = norm_stats(rng)
    A = frames_wave(23, fs, seed=3)
    silence = [np.zeros(n, np.int16) for n in (512 + 256 * 4, 512 + 256 * 9 + 100)]
    noise = [rng.choice(np.array([-32768, 32767], np.int16), n) for n in (512 + 256 * 4, 512 + 256 * 9 + 100)]
    other = [frames_wave(F, fs, seed=60 + F) for F in (2, 40, 7)]
    eng = engine(pkg, ls, ws, bs, 16)

    def run(waves):
        return eng.enhance_waves(waves, mean, inv, fs_khz=fs, fea_context=ctx, return_f32=True, return_lps=True)

    alone = [r[0] for r in run([A])]
    for batch, at in (([silence[0], A, silence[1]], 1), ([noise[0], A, noise[1]], 1), ([A] + other, 0),
                      (other + [A], 3), ([noise[1], A], 1)):
        got = [r[at] for r in run(batch)]
        same(got, alone)
    same(alone[:2], list(eng.enhance_wave(A, mean, inv, fea_context=ctx, fs_khz=fs, return_float=True)))
    batch = other + [A] + silence + noise
    base = run(batch)
    perm = rng.permutation(len(batch))
    assert not np.array_equal(perm, np.arange(len(batch)))
    shuffled = run([batch[i] for i in perm])
    for b, s in zip(base, shuffled):
        same(s, [b[i] for i in perm])
    eng.close()


# ---- chunk independence
def test_chunk_boundaries_anywhere_give_the_same_bits(pkg):
    """frame offsets 0 10 30 35 65 66 80 at context 7 (half = 3): capacity 10 cuts on utterance boundaries (10, 30) and
    inside (20, 40, ...); 7 and 1 inside everywhere; 32 cuts 2 frames after the boundary 30 and 1 before 65; 33 cuts 2
    before 35 and on 66; 13 cuts 1 after 65; 1000 holds all 80 frames in one chunk"""
    fs, ctx, B = 16, 7, 16
    frames = [10, 20, 5, 30, 1, 14]
    rng = np.random.default_rng(43)
    ls, ws, bs = small_net(rng, ctx=ctx)
    mean, inv = norm_stats(rng)
    waves = [frames_wave(F, fs, seed=70 + i) for i, F in enumerate(frames)]
    assert pkg.enhance_waves_layout([w.size for w in waves], fs)[1].tolist() == [0, 10, 30, 35, 65, 66, 80]
    one = engine(pkg, ls, ws, bs, B, cap=1000)
    base = check_equals_single(pkg, one, waves, mean, inv, ctx, fs)
    one.close()
    for cap in (10, 7, 1, 32, 33, 13, 80, 79):
        eng = engine(pkg, ls, ws, bs, B, cap=cap)
        got = eng.enhance_waves(waves, mean, inv, fs_khz=fs, fea_context=ctx, return_f32=True, return_lps=True)
        eng.close()
        for g, b in zip(got, base):
            same(g, b)
    default = engine(pkg, ls, ws, bs, B)
    got = default.enhance_waves(waves, mean, inv, fs_khz=fs, fea_context=ctx, return_f32=True, return_lps=True)
    default.close()
    for g, b in zip(got, base):
        same(g, b)


# ---- float64
@pytest.mark.parametrize("fs,ctx", [(16, 11), (11, 7), (8, 3)])
def test_a_mixed_batch_against_float64(pkg, fs, ctx):
    """per utterance, as check_enhance of test_gpu_spectral.py does for the single call: decode64 on the utterance's
    own LPS and its propagated bound, every output sample inside it"""
    D = spec64.params(fs)[2] // 2 + 1
    rng = np.random.default_rng(44 + fs)
    ls, ws, bs = small_net(rng, ctx=ctx, D=D)
    mean, inv = norm_stats(rng, D)
    waves = [frames_wave(F, fs, seed=80 + i) for i, F in enumerate(MIXED_F)]
    eng = engine(pkg, ls, ws, bs, 16)
    _, outf = eng.enhance_waves(waves, mean, inv, fs_khz=fs, fea_context=ctx, return_f32=True)
    slabs = eng.out_slabs()
    eng.close()
    for F, w, f in zip(MIXED_F, waves, outf):
        lps = pkg.wave_to_lps(w, fs_khz=fs)
        want, eps = spec64.decode64(lps, mean, inv, ctx, ws, bs, slabs=slabs)
        r = spec64.synthesis_ratio(f, w, want, fs, lps_eps=eps)
        print("enhance_waves vs float64: %d kHz ctx %d F %d ratio %.3g" % (fs, ctx, F, r))
        assert r <= 1.0, (F, r)


# ---- repeatability and the workspace
def test_repeated_calls_and_a_small_batch_in_the_grown_workspace(pkg):
    fs, ctx = 16, 7
    rng = np.random.default_rng(45)
    ls, ws, bs = small_net(rng, ctx=ctx)
    mean, inv = norm_stats(rng)
    large = [frames_wave(F, fs, seed=90 + i) for i, F in enumerate([300, 120, 64, 200, 33])]
    small = [frames_wave(F, fs, seed=95 + i) for i, F in enumerate([4, 1, 19])]
    eng = engine(pkg, ls, ws, bs, 32)
    a = check_equals_single(pkg, eng, large, mean, inv, ctx, fs)
    b = eng.enhance_waves(large, mean, inv, fs_khz=fs, fea_context=ctx, return_f32=True, return_lps=True)
    for x, y in zip(a, b):
        same(y, x)
    check_equals_single(pkg, eng, small, mean, inv, ctx, fs)           # every buffer is larger than this batch needs
    mean2, inv2 = norm_stats(rng)                                       # other norm vectors on the same engine
    check_equals_single(pkg, eng, small, mean2, inv2, ctx, fs)
    check_equals_single(pkg, eng, small, mean, inv, ctx, fs)
    same(eng.enhance_waves(large, mean, inv, fs_khz=fs), a[0])
    eng.close()


# ---- errors: every one is found on the host, before any launch
def test_argument_errors(pkg):
    fs, ctx = 16, 7
    rng = np.random.default_rng(46)
    ls, ws, bs = small_net(rng, ctx=ctx)
    mean, inv = norm_stats(rng)
    waves = [frames_wave(F, fs, seed=F) for F in (3, 9)]
    eng = engine(pkg, ls, ws, bs, 16)
    assert eng.enhance_waves([], mean, inv) == []                       # n_utts = 0: nothing to do
    assert eng.enhance_waves([], mean, inv, return_f32=True, return_lps=True) == ([], [], [])
    with pytest.raises(pkg.MlggdError, match=r"error 1: utterance 2: 511 samples is shorter than one frame \(512\)"):
        eng.enhance_waves(waves + [waves[0][:511]] + waves, mean, inv)
    with pytest.raises(pkg.MlggdError, match=r"error 1: fea_context 5"):
        eng.enhance_waves(waves, mean, inv, fea_context=5)
    with pytest.raises(pkg.MlggdError, match=r"error 1: fea_context 4 must be odd"):
        eng.enhance_waves(waves, mean, inv, fea_context=4)
    with pytest.raises(pkg.MlggdError, match=r"error 1: fs_khz 12"):
        pkg._check(raw_call(pkg, eng, waves, mean, inv, fs=12))
    # NULL arguments
    for null in ("mean", "inv", "noisy", "offsets", "out"):
        assert raw_call(pkg, eng, waves, mean, inv, null=null) == 1, null
        assert "NULL" in pkg.load().mlggd_last_error().decode()
    assert raw_call(pkg, None, waves, mean, inv) == 1
    assert raw_call(pkg, eng, waves, mean, inv, n_utts=-1) == 1
    assert raw_call(pkg, eng, waves, mean, inv, offsets=[0, 5000, 4000]) == 1
    assert "offsets decrease at utterance 1" in pkg.load().mlggd_last_error().decode()
    assert raw_call(pkg, eng, waves, mean, inv) == 0                    # the same call with nothing wrong
    eng.close()
    ls2, ws2, bs2 = small_net(rng, ctx=7, D=129)                        # 8 kHz bins on a 16 kHz batch
    eng2 = engine(pkg, ls2, ws2, bs2, 16)
    with pytest.raises(pkg.MlggdError, match=r"error 1: fea_context 7 x 257 bins"):
        eng2.enhance_waves(waves, mean, inv, fs_khz=16, fea_context=7)
    eng2.close()


def raw_call(pkg, eng, waves, mean, inv, fs=16, ctx=7, null=None, n_utts=None, offsets=None):
    packed = np.concatenate(waves)
    off = np.asarray(offsets if offsets is not None else np.concatenate([[0], np.cumsum([w.size for w in waves])]),
                     np.int64)
    out = np.zeros(packed.size, np.int16)
    fp, sp, lp = C.POINTER(C.c_float), C.POINTER(C.c_int16), C.POINTER(C.c_int64)
    args = {"mean": mean.ctypes.data_as(fp), "inv": inv.ctypes.data_as(fp), "noisy": packed.ctypes.data_as(sp),
            "offsets": off.ctypes.data_as(lp), "out": out.ctypes.data_as(sp)}
    if null:
        args[null] = None
    return pkg.load().mlggd_enhance_waves(eng._h if eng is not None else None, fs, ctx, args["mean"], args["inv"],
                                          len(waves) if n_utts is None else n_utts, args["noisy"], args["offsets"],
                                          args["out"], None, None)


def test_an_emulated_world_is_refused(pkg):
    rng = np.random.default_rng(47)
    ls, ws, bs = small_net(rng, ctx=7)
    mean, inv = norm_stats(rng)
    eng = engine(pkg, ls, ws, bs, 32)
    eng.fake_world(2, allreduce=True)
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_enhance_waves runs on a single-device engine"):
        eng.enhance_waves([frames_wave(5, 16, seed=1)], mean, inv)
    eng.close()


# ---- the tool
def tool(name):
    return os.path.join(hostlib.HOST, name)


def write_wav(path, w, rate=16000):
    w = np.asarray(w, "<i2")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + 2 * w.size) + b"WAVEfmt " +
                struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16) + b"data" + struct.pack("<I", 2 * w.size) +
                w.tobytes())


def tool_setup(tmp_path, D, ctx, seed):
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    rng = np.random.default_rng(seed)
    ls, ws, bs = small_net(rng, ctx=ctx, D=D)
    mean, inv = norm_stats(rng, D)
    hostlib.write_wts(str(tmp_path / "mlp.wts"), ws, bs)
    hostlib.write_norm(str(tmp_path / "n.norm"), mean, inv)
    return [tool("enhance_wav"), "wts=%s" % (tmp_path / "mlp.wts"), "norm_file=%s" % (tmp_path / "n.norm"),
            "fea_context=%d" % ctx, "bunchsize=64"]


def run_list(common, tmp_path, tag, lines, extra=()):
    """the tool on an scp of `lines` = (input, clean or None); outputs and info files go to tmp_path/tag"""
    d = tmp_path / tag
    d.mkdir()
    with open(d / "list.scp", "w") as f:
        for i, (src, clean) in enumerate(lines):
            f.write("%s %s" % (src, tmp_path / ("out%d.wav" % i)))
            f.write(" %s %s\n" % (clean, tmp_path / ("info%d.txt" % i)) if clean else "\n")
    r = subprocess.run(common + ["scp=%s" % (d / "list.scp"), *extra], capture_output=True, text=True, timeout=600)
    files = {}
    for i in range(len(lines)):
        for name in ("out%d.wav" % i, "info%d.txt" % i):
            if (tmp_path / name).exists():
                files[name] = open(tmp_path / name, "rb").read()
                os.remove(tmp_path / name)
    return r, files


def six_waves(tmp_path, rates):
    lines = []
    for i, rate in enumerate(rates):
        fs = rate // 1000
        n = rate + 777 * i + (0 if i != 2 else -rate // 2)
        noisy = spec64.synth_speech(n, fs, seed=200 + i)
        clean = spec64.synth_speech(n - 50 * i, fs, seed=300 + i)
        write_wav(tmp_path / ("n%d.wav" % i), noisy, rate)
        write_wav(tmp_path / ("c%d.wav" % i), clean, rate)
        lines.append((tmp_path / ("n%d.wav" % i), tmp_path / ("c%d.wav" % i)))
    return lines


def test_tool_batches_a_list_of_16_and_8_khz_files_like_the_loop(pkg, tmp_path):
    """Six lines, 16 kHz and 8 kHz mixed.  One net has one number of bins, so the 257-bin engine decodes the 16 kHz
    lines and stops at the first 8 kHz line, in both forms at the same place: the batch is flushed where the rate
    changes, so the WAVs written up to there, stdout and the exit status are the same as with batch_s=0."""
    common = tool_setup(tmp_path, 257, 7, 48)
    lines = [(p, None) for p, _ in six_waves(tmp_path, [16000, 16000, 16000, 8000, 16000, 8000])]
    loop, loop_files = run_list(common, tmp_path, "loop", lines, ["batch_s=0"])
    for tag, extra in (("default", []), ("tiny", ["batch_s=0.5"]), ("two", ["batch_s=2"])):
        got, got_files = run_list(common, tmp_path, tag, lines, extra)
        assert got.stdout == loop.stdout and got.returncode == loop.returncode
        assert got_files == loop_files
    assert sorted(loop_files) == ["out0.wav", "out1.wav", "out2.wav"] and loop.stdout.count("\n") == 3
    assert loop.returncode == 1 and "129 bins" in loop.stderr


def test_tool_batches_a_list_of_two_rates_that_share_a_net(pkg, tmp_path):
    """8000 and 11000 Hz files both have 129 bins: all six lines decode, the batch being flushed at each change of
    rate; WAVs and stdout byte-identical to batch_s=0, and equal to enhance_wave"""
    common = tool_setup(tmp_path, 129, 11, 49)
    rates = [8000, 8000, 11000, 8000, 11000, 11000]
    lines = [(p, None) for p, _ in six_waves(tmp_path, rates)]
    loop, loop_files = run_list(common, tmp_path, "loop", lines, ["batch_s=0"])
    assert loop.returncode == 0, loop.stderr
    assert len(loop_files) == 6 and loop.stdout.count("\n") == 6
    for tag, extra in (("default", []), ("tiny", ["batch_s=0.5"]), ("two", ["batch_s=2.5"])):
        got, got_files = run_list(common, tmp_path, tag, lines, extra)
        assert got.returncode == 0, got.stderr
        assert got.stdout == loop.stdout and got_files == loop_files


def test_tool_four_field_lines_write_the_single_pair_reports(pkg, tmp_path):
    common = tool_setup(tmp_path, 257, 7, 50)
    lines = six_waves(tmp_path, [16000] * 6)
    want = {}
    for i, (noisy, clean) in enumerate(lines):
        r = subprocess.run(common + ["in=%s" % noisy, "out=%s" % (tmp_path / "single.wav"), "clean=%s" % clean,
                                     "info=%s" % (tmp_path / "single.txt")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        want["out%d.wav" % i] = open(tmp_path / "single.wav", "rb").read()
        want["info%d.txt" % i] = open(tmp_path / "single.txt", "rb").read()
        assert want["info%d.txt" % i].startswith(b"Segmental SNR:\n")
    assert len(set(want[k] for k in want if k.startswith("info"))) == 6      # six different reports
    for tag, extra in (("default", []), ("loop", ["batch_s=0"]), ("two", ["batch_s=2"])):
        got, files = run_list(common, tmp_path, tag, lines, extra)
        assert got.returncode == 0, got.stderr
        assert files == want
    mixed = [(n, c if i % 2 else None) for i, (n, c) in enumerate(lines)]     # two- and four-field lines in one list
    got, files = run_list(common, tmp_path, "mixed", mixed)
    assert got.returncode == 0, got.stderr
    assert files == {k: v for k, v in want.items() if k.endswith(".wav") or int(k[4]) % 2}
