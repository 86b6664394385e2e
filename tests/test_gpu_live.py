"""GPU: BPGpu.live (mlggd_live_*) -- sessions decoded block by block with their state resident on the device.  The one
yardstick is the project's own single call: whatever a session emitted from its first sample to its end, concatenated,
is enhance_wave of the whole recording in every bit of the int16 and the float32 wave, however the recording was cut,
whatever its neighbours, its slot, the group's size, the chunk capacity and what the slot decoded before.  No test has
a tolerance.  Nets, norm vectors and waves as in tests/test_gpu_enhance_waves.py."""
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


def engine(pkg, ls, ws, bs, B=16, cap=0):
    return pkg.BPGpu(1, 0, ls, B, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0, max_cache_frames=cap)


def setup(pkg, fs, ctx, seed, B=16, cap=0):
    D = spec64.params(fs)[2] // 2 + 1
    rng = np.random.default_rng(seed)
    ls, ws, bs = small_net(rng, ctx=ctx, D=D)
    mean, inv = norm_stats(rng, D)
    return engine(pkg, ls, ws, bs, B, cap), mean, inv, (ls, ws, bs)


def blocks_of(n, size):
    """steps (block length, end) that cut n samples into blocks of `size`, the end on the last block"""
    sizes = [size] * (n // size) + ([n % size] if n % size else [])
    return [(s, i == len(sizes) - 1) for i, s in enumerate(sizes)] if sizes else [(0, True)]


def feed(live, waves, steps, slots=None):
    """Feeds waves[k] to slot slots[k] (default k) by steps[k] = [(block length, end), ...], step i of every session in
    push i; a session whose steps are used up idles with empty blocks.  Returns per session the concatenation of what
    it emitted (int16, float32) and the per-push counts."""
    n = live.n_sessions
    slots = list(range(len(waves))) if slots is None else slots
    at = [0] * len(waves)
    got = [([], [], []) for _ in waves]
    empty = np.zeros(0, np.int16)
    for i in range(max(len(s) for s in steps)):
        blocks, end = [empty] * n, [0] * n
        for k, w in enumerate(waves):
            if i < len(steps[k]):
                size, e = steps[k][i]
                blocks[slots[k]] = w[at[k]:at[k] + size]
                assert blocks[slots[k]].size == size
                at[k] += size
                end[slots[k]] = int(e)
        out, outf = live.push(blocks, end, return_f32=True)
        for k in range(len(waves)):
            got[k][0].append(out[slots[k]]), got[k][1].append(outf[slots[k]]), got[k][2].append(out[slots[k]].size)
    assert all(a == w.size for a, w in zip(at, waves))
    return [(np.concatenate(g[0]), np.concatenate(g[1]), g[2]) for g in got]


def single(eng, w, mean, inv, ctx, fs):
    return eng.enhance_wave(w, mean, inv, fea_context=ctx, fs_khz=fs, return_float=True)


def same_as(got, want):
    assert got[0].dtype == np.int16 and got[1].dtype == np.float32
    assert got[0].shape == want[0].shape and np.array_equal(got[0], want[0])
    assert got[1].shape == want[1].shape and np.array_equal(got[1], want[1])


# ---- 1. every cut, every rate
@pytest.mark.parametrize("ctx", [1, 7, 11])
@pytest.mark.parametrize("fs", [8, 11, 16])
def test_every_cut_equals_the_single_call(pkg, fs, ctx):
    """one session, 17 frames + 5 dropped samples; the whole recording with its end in one push; blocks of S, S + 1,
    L - 1, 2 L + 3; random blocks in [0, 2 S] with empty ones among them and the end sent alone in an empty push.  At 11
    kHz three frames cover a sample (two time blocks are carried); context 1 carries no rows; with context 11 a short
    push has fewer frames than half a context."""
    L, S, _ = spec64.params(fs)
    eng, mean, inv, _ = setup(pkg, fs, ctx, 100 * fs + ctx)
    w = frames_wave(17, fs, seed=fs + ctx, extra=5)
    want = single(eng, w, mean, inv, ctx, fs)
    assert want[0].size == 17 * S + L - S
    live = eng.live(mean, inv, 1, fs_khz=fs, fea_context=ctx)
    rng = np.random.default_rng(fs * ctx)
    rand = [0]
    while sum(rand) < w.size:
        rand.append(min(int(rng.integers(0, 2 * S + 1)), w.size - sum(rand)))
        if len(rand) % 4 == 0:
            rand.append(0)
    cuttings = [[(w.size, True)]] + [blocks_of(w.size, b) for b in (S, S + 1, L - 1, 2 * L + 3)]
    cuttings.append([(r, False) for r in rand] + [(0, True)])
    for steps in cuttings:
        got = feed(live, [w], [steps])[0]
        same_as(got, want)
        assert live.received().tolist() == [0]                       # the slot is empty again
    live.close()
    eng.close()


# ---- 2. one sample at a time
def test_one_sample_at_a_time(pkg):
    fs, ctx = 8, 7
    L, S, _ = spec64.params(fs)
    eng, mean, inv, _ = setup(pkg, fs, ctx, 21)
    w = frames_wave(5, fs, seed=22, extra=3)
    want = single(eng, w, mean, inv, ctx, fs)
    live = eng.live(mean, inv, 1, fs_khz=fs, fea_context=ctx)
    steps = [(1, i == w.size - 1) for i in range(w.size)]
    got = feed(live, [w], [steps])[0]
    same_as(got, want)
    counts = [int(pkg.live_layout([i], [1], [i == w.size - 1], fs, ctx)[1]) for i in range(w.size)]
    assert got[2] == counts and sorted(set(counts[:-1])) == [0, S]
    live.close()
    eng.close()


# ---- 3. short recordings
def test_short_recordings_at_context_11(pkg):
    """1, 2, 3 and 5 frames are never decodable before the end (half = 5): the ending push clamps them on both sides at
    once.  L - 1 samples emit nothing, and the next recording in the slot is still right."""
    fs, ctx = 16, 11
    L, S, _ = spec64.params(fs)
    eng, mean, inv, _ = setup(pkg, fs, ctx, 31)
    live = eng.live(mean, inv, 1, fs_khz=fs, fea_context=ctx)
    for F in (1, 2, 3, 5):
        w = frames_wave(F, fs, seed=30 + F)
        want = single(eng, w, mean, inv, ctx, fs)
        for steps in (blocks_of(w.size, 200), [(w.size, False), (0, True)], [(w.size, True)]):
            got = feed(live, [w], [steps])[0]
            same_as(got, want)
            assert all(c == 0 for c in got[2][:-1])
    stub = frames_wave(1, fs, seed=39)[:L - 1]
    got = feed(live, [stub], [blocks_of(stub.size, 100)])[0]
    assert got[0].size == 0 and got[1].size == 0 and live.received().tolist() == [0]
    w = frames_wave(9, fs, seed=38)
    same_as(feed(live, [w], [blocks_of(w.size, 300)])[0], single(eng, w, mean, inv, ctx, fs))
    live.close()
    eng.close()


# ---- 4. neighbours and slots
def test_neighbours_slots_and_group_size(pkg):
    """six sessions of 1, 2, 3, 5, 17 and 300 frames fed different block sizes in the same pushes, ending in different
    pushes; the same recordings permuted over the slots; one of them alone in a group of one"""
    fs, ctx = 16, 7
    L, S, _ = spec64.params(fs)
    eng, mean, inv, _ = setup(pkg, fs, ctx, 41)
    waves = [frames_wave(F, fs, seed=40 + i, extra=3 * i) for i, F in enumerate(MIXED_F)]
    want = [single(eng, w, mean, inv, ctx, fs) for w in waves]
    sizes = [100, 300, S, S + 1, L - 1, 4000]
    steps = [blocks_of(w.size, b) for w, b in zip(waves, sizes)]
    assert len(set(len(s) for s in steps)) >= 4                      # they end in different pushes
    live = eng.live(mean, inv, 6, fs_khz=fs, fea_context=ctx)
    base = feed(live, waves, steps)
    for g, w in zip(base, want):
        same_as(g, w)
    perm = [3, 5, 0, 4, 1, 2]
    for g, w in zip(feed(live, waves, steps, slots=perm), want):
        same_as(g, w)
    steps2 = [blocks_of(w.size, b) for w, b in zip(waves, reversed(sizes))]
    for g, w in zip(feed(live, waves, steps2, slots=perm[::-1]), want):
        same_as(g, w)
    live.close()
    alone = eng.live(mean, inv, 1, fs_khz=fs, fea_context=ctx)
    same_as(feed(alone, [waves[4]], [steps[4]])[0], want[4])
    alone.close()
    wide = eng.live(mean, inv, 9, fs_khz=fs, fea_context=ctx)      # another group size; slots 2 and 7, the rest idle
    got = feed(wide, [waves[4], waves[5]], [steps[4], steps[5]], slots=[7, 2])
    same_as(got[0], want[4])
    same_as(got[1], want[5])
    wide.close()
    eng.close()


# ---- 5. slot reuse
def test_slot_reuse_reads_nothing_stale(pkg):
    """11 kHz, context 7: a session of 20 frames in blocks of 3 S + 7 leaves full carries (two time blocks, six LPS
    rows, three spectra, a long tail) right up to its end; then other recordings in the same slot, a short one among
    them; the whole sequence twice on one group"""
    fs, ctx = 11, 7
    L, S, _ = spec64.params(fs)
    eng, mean, inv, _ = setup(pkg, fs, ctx, 51)
    recs = [frames_wave(F, fs, seed=50 + i, extra=i) for i, F in enumerate([20, 6, 2, 13])]
    want = [single(eng, w, mean, inv, ctx, fs) for w in recs]
    live = eng.live(mean, inv, 2, fs_khz=fs, fea_context=ctx)
    rounds = []
    for _ in range(2):
        got = []
        for k, w in enumerate(recs):
            other = recs[(k + 1) % len(recs)]                          # the neighbour slot is busy with another one
            got.append(feed(live, [w, other], [blocks_of(w.size, 3 * S + 7), blocks_of(other.size, S + 3)]))
        rounds.append(got)
    for got in rounds:
        for k in range(len(recs)):
            same_as(got[k][0], want[k])
            same_as(got[k][1], want[(k + 1) % len(recs)])
    live.close()
    eng.close()


# ---- 6. chunk capacity
def test_chunk_capacity_does_not_change_a_bit(pkg):
    """max_cache_frames = 5, bunches of 16: pushes of ten frames to each of four sessions make about 40 decodable frames,
    eight chunks that cut inside and between the sessions' sections"""
    fs, ctx = 16, 7
    L, S, _ = spec64.params(fs)
    results = []
    for cap in (0, 5):
        eng, mean, inv, _ = setup(pkg, fs, ctx, 61, cap=cap)
        waves = [frames_wave(F, fs, seed=60 + i) for i, F in enumerate([31, 24, 40, 12])]
        live = eng.live(mean, inv, 4, fs_khz=fs, fea_context=ctx)
        got = feed(live, waves, [blocks_of(w.size, 10 * S) for w in waves])
        live.close()
        if cap == 0:
            for g, w in zip(got, waves):
                same_as(g, single(eng, w, mean, inv, ctx, fs))
        eng.close()
        results.append(got)
    for a, b in zip(*results):
        same_as(b, a)
        assert a[2] == b[2]


# ---- 7. other calls in between
def test_other_engine_calls_between_pushes(pkg):
    """between two pushes: an enhance_waves call, a training step on frame streams (the engine's raw sets and chunk
    buffers), set_weights back to the original weights"""
    fs, ctx, B = 16, 7, 16
    L, S, _ = spec64.params(fs)
    eng, mean, inv, (ls, ws, bs) = setup(pkg, fs, ctx, 71, B=B)
    waves = [frames_wave(F, fs, seed=70 + i) for i, F in enumerate([14, 9])]
    want = [single(eng, w, mean, inv, ctx, fs) for w in waves]
    live = eng.live(mean, inv, 2, fs_khz=fs, fea_context=ctx)
    rng = np.random.default_rng(72)
    feat = rng.normal(0, 1, (B + ctx - 1, 257)).astype(np.float32)
    targ = rng.normal(0, 0.5, (B + ctx - 1, 257)).astype(np.float32)
    parts = [[], []], [[], []]
    at, done = [0, 0], [False, False]
    step = 3 * S + 11
    while not all(done):
        blocks = [w[a:a + step] for a, w in zip(at, waves)]
        at = [a + b.size for a, b in zip(at, blocks)]
        end = [int(a == w.size and not d) for a, d, w in zip(at, done, waves)]
        done = [a == w.size for a, w in zip(at, waves)]
        out, outf = live.push(blocks, end, return_f32=True)
        for u in range(2):
            parts[0][u].append(out[u]), parts[1][u].append(outf[u])
        other = eng.enhance_waves([waves[1], waves[0]], mean, inv, fs_khz=fs, fea_context=ctx)
        assert np.array_equal(other[0], want[1][0])
        assert eng.train_frames(feat, targ, np.arange(B, dtype=np.int32), ctx, (ctx - 1) // 2) == 1
        assert not np.array_equal(eng.returnWeights()[0][-1], ws[-1])
        eng.set_weights(ws, bs)
    for u in range(2):
        same_as((np.concatenate(parts[0][u]), np.concatenate(parts[1][u])), want[u])
    live.close()
    eng.close()


# ---- 8. state errors
def test_state_and_capacity_errors(pkg):
    fs, ctx = 16, 7
    L, S, _ = spec64.params(fs)
    eng, mean, inv, (ls, ws, bs) = setup(pkg, fs, ctx, 81)
    fake = engine(pkg, ls, ws, bs, B=32)
    fake.fake_world(2, allreduce=True)
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_live_open runs on a single-device engine"):
        fake.live(mean, inv, 1)
    fake.close()
    with pytest.raises(pkg.MlggdError, match=r"error 1: fea_context 4 must be odd"):
        eng.live(mean, inv, 1, fea_context=4)
    with pytest.raises(pkg.MlggdError, match=r"error 1: fea_context 5 x 257"):
        eng.live(mean, inv, 1, fea_context=5)
    with pytest.raises(pkg.MlggdError, match=r"error 1: n_sessions 0 < 1"):
        eng.live(mean, inv, 0)
    with pytest.raises(pkg.MlggdError, match=r"error 1: fs_khz 12"):
        eng.live(mean, inv, 1, fs_khz=12, fea_context=7)
    lib = pkg.load()
    live = eng.live(mean, inv, 2)
    assert lib.mlggd_destroy(eng._h) == 4 and "live group" in lib.mlggd_last_error().decode()
    w = frames_wave(12, fs, seed=82)
    want = single(eng, w, mean, inv, ctx, fs)                          # the engine is still usable
    # a raw push whose out_capacity is one sample short, then NULL / decreasing offsets: refused, state untouched
    first = w[:L + 5 * S]
    k = int(pkg.live_layout([0], [first.size], None, fs, ctx)[1])
    assert k == 3 * S
    assert feed(live, [first], [[(first.size, False)]], slots=[1])[0][0].size == k
    rest = w[first.size:]
    need = int(pkg.live_layout([0, first.size], [0, rest.size], [0, 1], fs, ctx)[-1])
    sp, lp, bp = C.POINTER(C.c_int16), C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
    off = np.array([0, 0, rest.size], np.int64)
    end = np.array([0, 1], np.uint8)
    out = np.zeros(need, np.int16)
    out_off = np.zeros(3, np.int64)

    def raw(offsets=off, cap=need, samples=rest):
        return lib.mlggd_live_push(live._s, samples.ctypes.data_as(sp) if samples is not None else None,
                                   offsets.ctypes.data_as(lp) if offsets is not None else None, end.ctypes.data_as(bp),
                                   out.ctypes.data_as(sp), None, cap, out_off.ctypes.data_as(lp))

    assert raw(cap=need - 1) == 1 and "out_capacity" in lib.mlggd_last_error().decode()
    assert raw(offsets=np.array([0, rest.size, 0], np.int64)) == 1
    assert "offsets decrease at session 1" in lib.mlggd_last_error().decode()
    assert raw(offsets=None) == 1 and raw(samples=None) == 1
    assert live.received().tolist() == [0, first.size]
    assert raw() == 0 and out_off.tolist() == [0, 0, need]
    assert np.array_equal(np.concatenate([want[0][:k], out]), want[0])
    live.close()
    assert lib.mlggd_destroy(eng._h) == 0
    eng._h = None
    eng2 = engine(pkg, ls, ws, bs)
    g = eng2.live(mean, inv, 1)
    eng2.close()                                                        # closes its group first
    assert g._s is None


# ---- 9. the tool
def write_wav(path, w, rate=16000):
    w = np.asarray(w, "<i2")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + 2 * w.size) + b"WAVEfmt " +
                struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16) + b"data" + struct.pack("<I", 2 * w.size) +
                w.tobytes())


def test_tool_live_writes_the_default_modes_bytes(pkg, tmp_path):
    """enhance_wav scp=LIST live=200 sessions=3 over seven short waves: three slots refilled from the list as they free
    up; every file byte-identical to the list decoded without live="""
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    rng = np.random.default_rng(91)
    ls, ws, bs = small_net(rng, ctx=7)
    mean, inv = norm_stats(rng)
    hostlib.write_wts(str(tmp_path / "mlp.wts"), ws, bs)
    hostlib.write_norm(str(tmp_path / "n.norm"), mean, inv)
    common = [os.path.join(hostlib.HOST, "enhance_wav"), "wts=%s" % (tmp_path / "mlp.wts"),
              "norm_file=%s" % (tmp_path / "n.norm"), "fea_context=7", "bunchsize=64"]
    frames = [3, 11, 1, 7, 20, 2, 9]
    for i, F in enumerate(frames):
        write_wav(tmp_path / ("n%d.wav" % i), frames_wave(F, 16, seed=90 + i, extra=11 * i))

    def run(tag, extra):
        d = tmp_path / tag
        d.mkdir()
        with open(d / "list.scp", "w") as f:
            for i in range(len(frames)):
                f.write("%s %s\n" % (tmp_path / ("n%d.wav" % i), d / ("out%d.wav" % i)))
        r = subprocess.run(common + ["scp=%s" % (d / "list.scp"), *extra], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return [open(d / ("out%d.wav" % i), "rb").read() for i in range(len(frames))], r.stdout

    want, want_out = run("default", [])
    got, got_out = run("live", ["live=200", "sessions=3"])
    assert got == want and len(set(want)) == len(frames)
    assert sorted(l.replace("/live/", "/default/") for l in got_out.splitlines()) == sorted(want_out.splitlines())
    r = subprocess.run(common + ["scp=%s" % (tmp_path / "live" / "list.scp"), "live=200", "score=device"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "live=" in r.stderr and "score=" in r.stderr
