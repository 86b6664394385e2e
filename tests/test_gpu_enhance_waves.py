"""GPU: BPGpu.enhance_waves (mlggd_enhance_waves) -- a list of utterances packed into one frame stream -- against the
per-utterance call enhance_wave, bit for bit on the int16 wave, the float32 wave and the de-normalised LPS rows:
whatever the neighbours, the position in the batch, the batch and the chunk capacity; against float64 per element; its
workspace reuse and argument checks; and the enhance_wav tool's batched lists against its per-utterance loop.

The batches of the later tests (table lookup, thousands of utterances, wave base, degenerate subjects) are those of
spec64.waves_gpu_configs(); tests/test_enhance_waves_model.py shows on the CPU which planted index slips each of them
would see, and the docstrings here name them."""
import ctypes as C
import os
import struct
import subprocess
import time

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


def raw_call(pkg, eng, waves, mean, inv, fs=16, ctx=7, null=None, n_utts=None, offsets=None, base=None):
    """mlggd_enhance_waves through ctypes; returns its status.  With base (>= 0): the packed buffer starts with `base`
    samples of +-32767 garbage, so offsets[0] = base, and ends with a gap of the same garbage after the last offset;
    out_f32 and lps_out are asked for too and (status, out, out_f32, lps_out) is returned."""
    packed = np.concatenate(waves)
    off = np.asarray(offsets if offsets is not None else np.concatenate([[0], np.cumsum([w.size for w in waves])]),
                     np.int64)
    out = np.zeros(packed.size, np.int16)
    outf = lps = None
    fp, sp, lp = C.POINTER(C.c_float), C.POINTER(C.c_int16), C.POINTER(C.c_int64)
    if base is not None:
        garbage = np.tile(np.array([32767, -32767], np.int16), (base + 778) // 2 + 1)
        packed = np.concatenate([garbage[:base], packed, garbage[1:778]])
        off = off + base
        _, frame_off, out_off = pkg.enhance_waves_layout([w.size for w in waves], fs)
        out = np.zeros(int(out_off[-1]), np.int16)
        outf = np.zeros(out.size, np.float32)
        lps = np.zeros((int(frame_off[-1]), mean.size), np.float32)
    args = {"mean": mean.ctypes.data_as(fp), "inv": inv.ctypes.data_as(fp), "noisy": packed.ctypes.data_as(sp),
            "offsets": off.ctypes.data_as(lp), "out": out.ctypes.data_as(sp)}
    if null:
        args[null] = None
    rc = pkg.load().mlggd_enhance_waves(eng._h if eng is not None else None, fs, ctx, args["mean"], args["inv"],
                                        len(waves) if n_utts is None else n_utts, args["noisy"], args["offsets"],
                                        args["out"], outf.ctypes.data_as(fp) if outf is not None else None,
                                        lps.ctypes.data_as(fp) if lps is not None else None)
    return rc if base is None else (rc, out, outf, lps)


def test_an_emulated_world_is_refused(pkg):
    rng = np.random.default_rng(47)
    ls, ws, bs = small_net(rng, ctx=7)
    mean, inv = norm_stats(rng)
    eng = engine(pkg, ls, ws, bs, 32)
    eng.fake_world(2, allreduce=True)
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_enhance_waves runs on a single-device engine"):
        eng.enhance_waves([frames_wave(5, 16, seed=1)], mean, inv)
    eng.close()


def test_a_communicator_of_one_rank_may_decode_but_not_load_or_go_live(pkg):
    """The wave entries share one engine check but not one single-device rule: an engine that has joined a communicator
    of one rank still decodes (the same bytes as one that has not), while the wave loader and a live group refuse it."""
    rng = np.random.default_rng(48)
    ls, ws, bs = small_net(rng, ctx=1, hidden=(32,), D=129)
    mean, inv = norm_stats(rng, D=129)
    wave = frames_wave(1, 8, seed=2, extra=0)
    assert wave.size == 256
    plain, joined = engine(pkg, ls, ws, bs, 32), engine(pkg, ls, ws, bs, 32)
    joined.comm_init(pkg.comm_unique_id(), 1, 0)
    want = plain.enhance_waves([wave], mean, inv, fs_khz=8, fea_context=1, return_f32=True, return_lps=True)
    got = joined.enhance_waves([wave], mean, inv, fs_khz=8, fea_context=1, return_f32=True, return_lps=True)
    for g, w in zip(got, want):
        same(g, w)
    first = np.zeros(1, np.int32)
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_load_waves runs on a single-device engine"):
        joined.load_waves([wave], [wave], mean, inv, first, 0, fea_context=1, fs_khz=8)
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_live_open runs on a single-device engine"):
        joined.live(mean, inv, 1, fs_khz=8, fea_context=1)
    plain.load_waves([wave], [wave], mean, inv, first, 0, fea_context=1, fs_khz=8)   # the engine that stands alone may
    plain.live(mean, inv, 1, fs_khz=8, fea_context=1).close()
    plain.close()
    joined.close()


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


# ---- the batches of spec64.waves_gpu_configs(): table lookup, thousands of utterances, wave base, degenerate subjects
def config_waves(name, seed):
    """the configuration and int16 waves of exactly its frame counts (no trailing samples: the packed layout is the
    one the CPU model was checked on)"""
    cfg = spec64.waves_gpu_configs()[name]
    return cfg, [frames_wave(F, cfg["fs"], seed=seed + u, extra=0) for u, F in enumerate(cfg["frames"])]


def run_all(eng, waves, mean, inv, ctx, fs):
    return eng.enhance_waves(waves, mean, inv, fs_khz=fs, fea_context=ctx, return_f32=True, return_lps=True)


def same3(got, want):
    for g, w in zip(got, want):
        same(g, w)


def test_table_lookup_equals_the_search_and_the_single_call(pkg, monkeypatch):
    """MLGGD_WAVES_LOOKUP=table, set before the engine is created: seg_of_frame returns utt_of[g] in
    k_lps_analysis_seg and k_lps_stream_seg.  Configurations table_mixed (the mixed lengths at 16 kHz, context 7) and
    table_chunks (the chunk-boundary batch with capacities 1, 7, 33, 1000); every output bit-equal to the search
    engine's and to the single call; then one table engine on a large batch and a small one (h_utt_of / utt_of larger
    than needed).  Planted slips these inputs discriminate: table_plus_1, ga_not_clamped (table_chunks),
    ctx_for_ctx_minus_1, fu_wrong_utterance, hi_not_clamped."""
    monkeypatch.delenv("MLGGD_WAVES_LOOKUP", raising=False)
    rng = np.random.default_rng(51)
    cfg, mixed = config_waves("table_mixed", 400)
    cfg2, cuts = config_waves("table_chunks", 420)
    fs, ctx = cfg["fs"], cfg["ctx"]
    assert (cfg2["fs"], cfg2["ctx"]) == (fs, ctx)
    assert pkg.enhance_waves_layout([w.size for w in cuts], fs)[1].tolist() == [0, 10, 30, 35, 65, 66, 80]
    ls, ws, bs = small_net(rng, ctx=ctx)
    mean, inv = norm_stats(rng)
    search = engine(pkg, ls, ws, bs, 16)
    want_mixed = check_equals_single(pkg, search, mixed, mean, inv, ctx, fs)
    search.close()
    search = engine(pkg, ls, ws, bs, 16, cap=1000)
    want_cuts = check_equals_single(pkg, search, cuts, mean, inv, ctx, fs)
    search.close()
    monkeypatch.setenv("MLGGD_WAVES_LOOKUP", "table")
    table = engine(pkg, ls, ws, bs, 16)
    same3(check_equals_single(pkg, table, mixed, mean, inv, ctx, fs), want_mixed)
    table.close()
    for cap in cfg2["caps"]:
        table = engine(pkg, ls, ws, bs, 16, cap=cap)
        same3(run_all(table, cuts, mean, inv, ctx, fs), want_cuts)
        if cap == 7:              # forward_frames takes no utterance beyond the capacity: the LPS rows by want_cuts
            same3(check_equals_single(pkg, table, cuts, mean, inv, ctx, fs, lps=False), want_cuts)
        table.close()
    table = engine(pkg, ls, ws, bs, 16)                               # a large batch, then small ones in its tables
    large = [frames_wave(F, fs, seed=440 + i) for i, F in enumerate([300, 120, 64, 200, 33])]
    a = check_equals_single(pkg, table, large, mean, inv, ctx, fs)
    same3(check_equals_single(pkg, table, cuts, mean, inv, ctx, fs), want_cuts)
    same3(check_equals_single(pkg, table, mixed[:3], mean, inv, ctx, fs), [w[:3] for w in want_mixed])
    same(table.enhance_waves(large, mean, inv, fs_khz=fs), a[0])
    table.close()


@pytest.mark.parametrize("name", ["many_odd", "many_even"])
def test_thousands_of_utterances(pkg, monkeypatch, name):
    """8 kHz, 129 bins, context 11, bunches of 64: 2187 (odd) and 2048 (even) utterances of 1 to 4 frames with six of
    200 to 400 frames between them.  The three searches run 11 to 12 levels deep; with capacities 257 and 1000 a chunk
    touches hundreds of utterances, with 257 its stream is more than five times its frames (asserted from the layout
    and the CPU model) and u0 / u1 advance over hundreds of utterances from chunk to chunk; 257 is a multiple of nothing in
    the layout; capacity 1 runs on the first 300 / 301 utterances.  Both lookups.  int16, float32 and the LPS rows
    bit-equal to the single call per utterance; at least 50 utterances -- the first, the last, every long one and its
    neighbours, and a seeded draw -- against float64.  Planted slips these inputs discriminate: search_bias,
    lt_for_le, ctx_for_ctx_minus_1, ga_not_clamped, fu_wrong_utterance, hi_not_clamped, table_plus_1."""
    t_start = time.time()
    monkeypatch.delenv("MLGGD_WAVES_LOOKUP", raising=False)
    cfg, waves = config_waves(name, 1000)
    fs, ctx, B, frames = cfg["fs"], cfg["ctx"], 64, cfg["frames"]
    n_utts = len(waves)
    D = spec64.params(fs)[2] // 2 + 1
    got_frames, frame_off, _ = pkg.enhance_waves_layout([w.size for w in waves], fs)
    assert got_frames.tolist() == frames and n_utts >= 2048
    # the regime is really reached: a full chunk of 257 frames over 100 utterances and more whose stream is five times
    # its frames, and a chunk of 1000 over 300 and more (the long utterances keep some of those just below 5 n)
    assert any(n == 257 and rows >= 5 * n and touched >= 100
               for n, rows, touched in spec64.waves_rows_per_chunk(frame_off, ctx, 257))
    assert any(n == 1000 and touched >= 300 for n, _, touched in spec64.waves_rows_per_chunk(frame_off, ctx, 1000))
    rng = np.random.default_rng(52 + n_utts)
    ls, ws, bs = small_net(rng, ctx=ctx, D=D)
    mean, inv = norm_stats(rng, D)
    eng = engine(pkg, ls, ws, bs, B)
    t0 = time.time()
    base = check_equals_single(pkg, eng, waves, mean, inv, ctx, fs)
    t_single = time.time() - t0
    slabs = eng.out_slabs()
    eng.close()
    sub = len(spec64.waves_gpu_configs()[name + "_cap1"]["frames"])
    assert frames[:sub] == spec64.waves_gpu_configs()[name + "_cap1"]["frames"] and sub >= 300
    for lookup in cfg["lookups"]:
        if lookup == "table":
            monkeypatch.setenv("MLGGD_WAVES_LOOKUP", "table")
        for cap in cfg["caps"]:
            if (lookup, cap) == ("search", 0):
                continue                                               # base itself
            eng = engine(pkg, ls, ws, bs, B, cap=cap)
            same3(run_all(eng, waves, mean, inv, ctx, fs), base)
            eng.close()
        eng = engine(pkg, ls, ws, bs, B, cap=1)
        same3(run_all(eng, waves[:sub], mean, inv, ctx, fs), [b[:sub] for b in base])
        eng.close()
    long_ones = [u for u, F in enumerate(frames) if F >= 200]
    assert len(long_ones) >= 5 and 0 < min(long_ones) and max(long_ones) < n_utts - 1
    pick = {0, n_utts - 1}
    for u in long_ones:
        pick |= {u - 1, u, u + 1}
    pick |= set(np.random.default_rng(53).choice(n_utts, 40, replace=False).tolist())
    assert len(pick) >= 50
    worst = 0.0
    for u in sorted(pick):
        want, eps = spec64.decode64(pkg.wave_to_lps(waves[u], fs_khz=fs), mean, inv, ctx, ws, bs, slabs=slabs)
        r = spec64.synthesis_ratio(base[1][u], waves[u], want, fs, lps_eps=eps)
        worst = max(worst, r)
        assert r <= 1.0, (u, frames[u], r)
    print("enhance_waves vs float64: %s, %d utterances of %d checked, worst ratio %.3g" % (name, len(pick), n_utts, worst))
    print("enhance_waves %s: wall time %.1f s (%.1f s of it the batch + %d single calls + their LPS pieces)"
          % (name, time.time() - t_start, t_single, n_utts))


def test_a_wave_base_other_than_zero(pkg):
    """mlggd_enhance_waves through ctypes with offsets[0] = 1, 1000 and 12345 (odd: the int16 upload source is 2-byte
    but not 4-byte aligned), the pad before and the gap after the utterances filled with +-32767: the engine uploads
    noisy + offsets[0] and indexes it with wave_off[u] = offsets[u] - offsets[0].  int16, float32 and LPS outputs
    bit-equal to the offsets[0] = 0 call and to BPGpu.enhance_waves.  Planted slip these inputs discriminate:
    wave_off_not_rebased."""
    cfg, waves = config_waves("wave_base", 500)
    fs, ctx = cfg["fs"], cfg["ctx"]
    rng = np.random.default_rng(54)
    ls, ws, bs = small_net(rng, ctx=ctx)
    mean, inv = norm_stats(rng)
    eng = engine(pkg, ls, ws, bs, 16)
    want = check_equals_single(pkg, eng, waves, mean, inv, ctx, fs)
    rc, out, outf, lps = raw_call(pkg, eng, waves, mean, inv, fs=fs, ctx=ctx, base=0)
    assert rc == 0
    assert np.array_equal(out, np.concatenate(want[0])) and np.array_equal(outf, np.concatenate(want[1]))
    assert np.array_equal(lps, np.concatenate(want[2]))
    for base in cfg["bases"]:
        rc, o, f, p = raw_call(pkg, eng, waves, mean, inv, fs=fs, ctx=ctx, base=base)
        assert rc == 0, pkg.load().mlggd_last_error().decode()
        assert np.array_equal(o, out) and np.array_equal(f, outf) and np.array_equal(p, lps), base
    assert 12345 in cfg["bases"] and 1 in cfg["bases"] and 1000 in cfg["bases"]
    eng.close()


def test_workspace_across_rates_outputs_norms_and_training(pkg):
    """one 129-bin engine (context 7, bunches of 16): a large 8 kHz batch, a small 11 kHz batch (same L and D, another
    S: another layout in the same buffers), 8 kHz again asking for out_f32 for the first time, then lps_out for the
    first time on a smaller call; one element of inv_std changed, then one of mean, then both restored (the upload
    rests on the memcmp); then two training steps and a forward() between decodes (raw sets, chunk_out and toff are
    shared with training).  Every result bit-equal to a fresh engine's; the trained weights and forward() equal those
    of an engine that only trained."""
    ctx, D, B = 7, 129, 16
    rng = np.random.default_rng(55)
    ls, ws, bs = small_net(rng, ctx=ctx, D=D)
    mean, inv = norm_stats(rng, D)
    large8 = [frames_wave(F, 8, seed=600 + i) for i, F in enumerate([300, 2, 120, 64, 1, 200, 33])]
    small11 = [frames_wave(F, 11, seed=610 + i) for i, F in enumerate([4, 1, 19])]
    mid8 = [frames_wave(F, 8, seed=620 + i) for i, F in enumerate([40, 3, 25])]
    tiny11 = [frames_wave(F, 11, seed=630 + i) for i, F in enumerate([2, 6])]

    def fresh(waves, fs, mean, inv, ws=ws, bs=bs, **kw):
        e = engine(pkg, ls, ws, bs, B)
        r = e.enhance_waves(waves, mean, inv, fs_khz=fs, fea_context=ctx, **kw)
        e.close()
        return r

    def agree(got, want):
        if isinstance(got, tuple):
            assert len(got) == len(want)
            same3(got, want)
        else:
            same(got, want)

    eng = engine(pkg, ls, ws, bs, B)
    agree(eng.enhance_waves(large8, mean, inv, fs_khz=8, fea_context=ctx), fresh(large8, 8, mean, inv))
    agree(eng.enhance_waves(small11, mean, inv, fs_khz=11, fea_context=ctx), fresh(small11, 11, mean, inv))
    agree(eng.enhance_waves(mid8, mean, inv, fs_khz=8, fea_context=ctx, return_f32=True),
          fresh(mid8, 8, mean, inv, return_f32=True))                  # out_f32 grown while the rest is oversized
    agree(eng.enhance_waves(tiny11, mean, inv, fs_khz=11, fea_context=ctx, return_f32=True, return_lps=True),
          fresh(tiny11, 11, mean, inv, return_f32=True, return_lps=True))
    agree(eng.enhance_waves(large8, mean, inv, fs_khz=8, fea_context=ctx, return_f32=True, return_lps=True),
          fresh(large8, 8, mean, inv, return_f32=True, return_lps=True))
    check_equals_single(pkg, eng, small11, mean, inv, ctx, 11)
    # the workspace no longer grows: the norm upload rests on the comparison with the last vectors alone
    inv2, mean2 = inv.copy(), mean.copy()
    inv2[D - 1] = np.float32(inv2[D - 1] * 1.25)
    mean2[0] = np.float32(mean2[0] + 0.5)
    kw = dict(return_f32=True, return_lps=True)
    before = eng.enhance_waves(mid8, mean, inv, fs_khz=8, fea_context=ctx, **kw)
    for m, v in ((mean, inv2), (mean2, inv2), (mean2, inv), (mean, inv)):
        got = eng.enhance_waves(mid8, m, v, fs_khz=8, fea_context=ctx, **kw)
        agree(got, fresh(mid8, 8, m, v, **kw))
        differs = not np.array_equal(got[2][0], before[2][0])
        assert differs == (m is not mean or v is not inv)              # one element is enough to change the rows
    # training between decodes
    inp = [rng.normal(0, 1, (B, ctx * D)).astype(np.float32) for _ in range(2)]
    targ = [rng.normal(0, 0.5, (B, D)).astype(np.float32) for _ in range(2)]
    only = engine(pkg, ls, ws, bs, B)
    assert only.train(inp[0], targ[0]) == 1 and only.train(inp[1], targ[1]) == 1
    only_fwd = only.forward(inp[0])
    only_w, only_b = only.returnWeights()
    only.close()
    assert eng.train(inp[0], targ[0]) == 1
    w1, b1 = eng.returnWeights()
    agree(eng.enhance_waves(small11, mean, inv, fs_khz=11, fea_context=ctx, **kw),
          fresh(small11, 11, mean, inv, ws=w1, bs=b1, **kw))
    assert eng.train(inp[1], targ[1]) == 1
    fwd = eng.forward(inp[0])
    w2, b2 = eng.returnWeights()
    agree(eng.enhance_waves(large8, mean, inv, fs_khz=8, fea_context=ctx, **kw),
          fresh(large8, 8, mean, inv, ws=w2, bs=b2, **kw))
    assert np.array_equal(eng.forward(inp[0]), fwd)                    # forward() after a decode
    check_equals_single(pkg, eng, mid8, mean, inv, ctx, 8)
    same(w2, only_w)
    same(b2, only_b)
    assert np.array_equal(fwd, only_fwd)
    assert not np.array_equal(w2[-1], ws[-1])                          # the steps did train
    eng.close()


def degenerate_waves(cfg):
    fs = cfg["fs"]
    L, S, _ = spec64.params(fs)
    F = cfg["frames"]
    n = [f * S + L - S for f in F]
    t = np.arange(n[5])
    loud = np.clip(np.round(30000 * np.sign(np.sin(2 * np.pi * 220 * t / 16000)) +
                            np.random.default_rng(5).normal(0, 500, t.size)), -32768, 32767).astype(np.int16)
    return [frames_wave(F[0], fs, seed=700, extra=0), np.zeros(n[1], np.int16), frames_wave(F[2], fs, seed=702, extra=0),
            np.zeros(n[3], np.int16), np.tile(np.array([32767, -32768], np.int16), n[4] // 2), loud,
            frames_wave(F[6], fs, seed=706, extra=0)]


def hot_bias(bs, mean, inv, level=25.5):
    """the output layer's bias raised so the de-normalised rows lie around `level` in every bin: a flat spectrum whose
    wave peaks several times beyond int16, as the + log 4 of test_synthesis_saturates_clipping_output in
    test_gpu_spectral.py puts its wave"""
    return bs[:-1] + [(bs[-1] + (np.float32(level) - mean) * inv).astype(np.float32)]


def test_degenerate_utterances_as_subjects(pkg):
    """configuration degenerate: speech, digital silence (9 frames), speech, one frame of silence, alternating
    +-full scale, a loud square wave, speech -- each one compared with the single call, under an ordinary net and under
    one whose output layer makes the enhanced wave clip, in one chunk and in chunks of 16 frames.  The silence takes
    the floor path (its analysis rows are all -50, |X| = 0: phase 0 in the synthesis) and the loud wave's output holds
    both 32767 and -32768 (the saturation inside k_ola_seg).  Planted slips these inputs discriminate: hi_not_clamped,
    fu_wrong_utterance, ga_not_clamped."""
    cfg = spec64.waves_gpu_configs()["degenerate"]
    fs, ctx = cfg["fs"], cfg["ctx"]
    waves = degenerate_waves(cfg)
    assert pkg.enhance_waves_layout([w.size for w in waves], fs)[0].tolist() == cfg["frames"] and cfg["frames"][3] == 1
    rng = np.random.default_rng(56)
    ls, ws, bs = small_net(rng, ctx=ctx)
    mean, inv = norm_stats(rng)
    for u in (1, 3):
        assert np.all(pkg.wave_to_lps(waves[u], fs_khz=fs) == -50.0)
    results = {}
    for net, bias in (("ordinary", bs), ("hot", hot_bias(bs, mean, inv))):
        for cap in cfg["caps"]:
            eng = engine(pkg, ls, ws, bias, 16, cap=cap)
            # the LPS pieces need a capacity of a whole utterance: with 16 the rows are held to the one-chunk engine's
            results[net, cap] = check_equals_single(pkg, eng, waves, mean, inv, ctx, fs, lps=cap == 0)
            eng.close()
        same3(results[net, cfg["caps"][1]], results[net, cfg["caps"][0]])
    out, outf, _ = results["hot", 0]
    assert (out[5] == 32767).sum() > 100 and (out[5] == -32768).sum() > 100 and np.abs(outf[5]).max() > 40000
    for u in range(len(waves)):
        assert np.array_equal(out[u], spec64.trunc_sat(outf[u])) and np.all(np.isfinite(outf[u]))
    quiet = results["ordinary", 0][0]
    assert any(o.max() < 32767 and o.min() > -32768 and np.any(o != 0) for o in quiet)   # the ordinary net does not clip
