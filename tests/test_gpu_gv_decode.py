"""GPU: global variance equalisation in the decoders (BPGpu.set_gv, csrc/gv_rule.h, k_lps_synthesis_gv).

Decoding with factors is pinned from the public pieces, as tests/test_gpu_spectral.py pins enhance_wave: wave_to_lps,
(lps - mean) * inv_std, edge-replicated windows, forward_frames, v = ((y * eta) / inv_std) + mean in NumPy float32 one
operation at a time (tests/gv64.apply32), lps_to_wave -- every bit of the int16 wave, the float32 wave and the rows.
Every decoder is then held to that composition: enhance_wave (one shot and chunked), enhance_waves with its rows, the
scored pass (whose scores are those of the equalised rows), a live group, a NAT and a ReLU engine.  Ones and None are
the engine without factors, bit for bit.

Shapes: a 771-64-257 net at 16 kHz and a 387-32-129 net at 8 kHz, both context 3; utterances of 1, 2, 9 and 40 frames;
eta drawn in [0.5, 2] per bin.  The compositions are computed once per rate and shared."""
import numpy as np
import pytest

import gv64
import nat_model
import spec64

pytestmark = pytest.mark.gpu
CTX, B = 3, 16
HIDDEN = {16: 64, 8: 32}
FRAMES = [1, 2, 9, 40]


def frames_wave(F, fs, seed, extra=5):
    L, S, _ = spec64.params(fs)
    return spec64.synth_speech(F * S + L - S + extra, fs, seed=seed)


def compose(pkg, eng, w, mean, inv, eta, fs, ctx=CTX):
    """(int16 wave, float32 wave, rows v) of one utterance from the public pieces"""
    lps = pkg.wave_to_lps(w, fs_khz=fs)
    F, half = lps.shape[0], (ctx - 1) // 2
    x = ((lps - mean) * inv).astype(np.float32)
    stream = x[np.clip(np.arange(F + 2 * half) - half, 0, F - 1)]
    y = eng.forward_frames(stream, np.arange(F, dtype=np.int32), ctx)
    v = gv64.apply32(y, eta, inv, mean)
    out, outf = pkg.lps_to_wave(w, v, fs_khz=fs, return_float=True)
    return out, outf, v


class Case:
    def __init__(self, pkg, fs):
        self.pkg, self.fs = pkg, fs
        D = self.D = spec64.params(fs)[2] // 2 + 1
        rng = np.random.default_rng(100 + fs)
        self.ls = [CTX * D, HIDDEN[fs], D]
        self.ws = [rng.normal(0, 0.05, (self.ls[i], self.ls[i + 1])).astype(np.float32) for i in range(2)]
        self.bs = [rng.normal(0, 0.1, self.ls[i + 1]).astype(np.float32) for i in range(2)]
        self.mean = rng.normal(10, 2, D).astype(np.float32)
        self.inv = (1.0 / rng.uniform(2, 4, D)).astype(np.float32)
        self.eta = gv64.draw_eta(D, 7 + fs)
        assert self.eta.min() >= 0.5 and self.eta.max() <= 2.0 and (self.eta != 1).all()
        self.waves = [frames_wave(F, fs, seed=30 + i, extra=3 * i) for i, F in enumerate(FRAMES)]
        assert pkg.enhance_waves_layout([w.size for w in self.waves], fs)[0].tolist() == FRAMES
        eng = self.engine()
        self.gv = [compose(pkg, eng, w, self.mean, self.inv, self.eta, fs) for w in self.waves]      # with factors
        self.plain = [compose(pkg, eng, w, self.mean, self.inv, None, fs) for w in self.waves]       # without
        eng.close()

    def engine(self, cap=0, **kw):
        return self.pkg.BPGpu(1, 0, self.ls, B, 0.1, 0.9, 1e-5, self.ws, self.bs, 2.0, 0, max_cache_frames=cap, **kw)

    def wave(self, eng, w):
        return eng.enhance_wave(w, self.mean, self.inv, fea_context=CTX, fs_khz=self.fs, return_float=True)


@pytest.fixture(scope="module")
def cases(pkg):
    return {fs: Case(pkg, fs) for fs in (16, 8)}


def same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("fs", [16, 8])
def test_enhance_wave_with_factors_equals_the_composition(cases, fs):
    c = cases[fs]
    eng = c.engine()
    eng.set_gv(c.eta)
    for u, w in enumerate(c.waves):
        out, outf = c.wave(eng, w)
        same(outf, c.gv[u][1], "F %d" % FRAMES[u])
        same(out, c.gv[u][0], "F %d" % FRAMES[u])
        assert outf.tobytes() != c.plain[u][1].tobytes()          # the factors are in the result
    eng.close()


@pytest.mark.parametrize("fs", [16, 8])
def test_ones_and_none_are_the_engine_without_factors(cases, fs):
    c = cases[fs]
    eng = c.engine()
    ones = np.ones(c.D, np.float32)
    assert np.array_equal(eng.gv(), ones)                         # off: ones
    before = [c.wave(eng, w) for w in c.waves]
    for u in range(len(FRAMES)):
        same(before[u][1], c.plain[u][1]), same(before[u][0], c.plain[u][0])
    eng.set_gv(ones)
    assert np.array_equal(eng.gv(), ones)
    for u, w in enumerate(c.waves):
        out, outf = c.wave(eng, w)
        same(outf, before[u][1]), same(out, before[u][0])
    eng.set_gv(c.eta)
    assert eng.gv().tobytes() == c.eta.tobytes()                  # on: the vector
    same(c.wave(eng, c.waves[2])[1], c.gv[2][1])
    eng.set_gv(None)
    assert np.array_equal(eng.gv(), ones)
    for u, w in enumerate(c.waves):
        out, outf = c.wave(eng, w)
        same(outf, before[u][1]), same(out, before[u][0])
    rows = eng.enhance_waves(c.waves, c.mean, c.inv, fs_khz=fs, fea_context=CTX, return_lps=True)[1]
    for u in range(len(FRAMES)):
        same(rows[u], c.plain[u][2])
    eng.close()


@pytest.mark.parametrize("fs", [16, 8])
def test_chunked_decoding_equals_one_shot(cases, fs):
    """40 frames through a capacity of 16: three chunks"""
    c = cases[fs]
    eng = c.engine(cap=16)
    eng.set_gv(c.eta)
    out, outf = c.wave(eng, c.waves[3])
    same(outf, c.gv[3][1]), same(out, c.gv[3][0])
    got = eng.enhance_waves(c.waves, c.mean, c.inv, fs_khz=fs, fea_context=CTX, return_f32=True, return_lps=True)
    for u in range(len(FRAMES)):
        same(got[0][u], c.gv[u][0]), same(got[1][u], c.gv[u][1]), same(got[2][u], c.gv[u][2])
    eng.close()


@pytest.mark.parametrize("fs", [16, 8])
def test_enhance_waves_equals_the_single_calls_and_its_rows_the_composition(cases, fs):
    """five utterances, one of them a single frame, not in the order of their lengths"""
    c = cases[fs]
    order = [2, 0, 3, 1, 2]
    eng = c.engine()
    eng.set_gv(c.eta)
    singles = [c.wave(eng, c.waves[u]) for u in order]
    out, outf, rows = eng.enhance_waves([c.waves[u] for u in order], c.mean, c.inv, fs_khz=fs, fea_context=CTX,
                                        return_f32=True, return_lps=True)
    for k, u in enumerate(order):
        same(out[k], singles[k][0]), same(outf[k], singles[k][1])
        same(out[k], c.gv[u][0]), same(outf[k], c.gv[u][1])
        same(rows[k], c.gv[u][2], "rows of utterance %d" % k)
    eng.close()


@pytest.mark.parametrize("fs", [16, 8])
def test_the_scores_are_those_of_the_equalised_rows(pkg, cases, fs):
    c = cases[fs]
    order = [2, 0, 3, 1, 2]
    waves = [c.waves[u] for u in order]
    cleans = [frames_wave(FRAMES[u], fs, seed=60 + k, extra=3 * u) for k, u in enumerate(order)]
    eng = c.engine()
    run = lambda: eng.enhance_waves(waves, c.mean, c.inv, fs_khz=fs, fea_context=CTX, return_lps=True, cleans=cleans,
                                    stoi=True)
    out0, rows0, segsnr0, lsd0, stoi0 = run()
    eng.set_gv(c.eta)
    out, rows, segsnr, lsd, stoi = run()
    for k, u in enumerate(order):
        same(out[k], c.gv[u][0]), same(rows[k], c.gv[u][2])
    want_snr, want_lsd = pkg.score_waves(cleans, waves, rows, fs_khz=fs)
    assert segsnr.tobytes() == want_snr.tobytes() and lsd.tobytes() == want_lsd.tobytes()
    want_stoi = pkg.stoi_waves(cleans, out, fs_khz=fs)
    assert np.array_equal(stoi, want_stoi, equal_nan=True) and np.isfinite(stoi[2])     # the 40-frame utterance has one
    print("fs %d: lsd without factors %s, with %s" % (fs, lsd0, lsd))
    assert (lsd != lsd0).all()                                    # the filter reaches the scores
    eng.close()


def test_a_live_group_emits_enhance_wave_with_factors(cases):
    """blocks of 1, 160 and 1000 samples in one group, with empty pushes in between and idle sessions at the end"""
    fs = 8
    c = cases[fs]
    eng = c.engine()
    eng.set_gv(c.eta)
    live = eng.live(c.mean, c.inv, 3, fs_khz=fs, fea_context=CTX)
    feeds = [(c.waves[1], 1, 1), (c.waves[2], 160, 2), (c.waves[3], 1000, 3)]     # (wave, block, utterance)
    at, done = [0, 0, 0], [False, False, False]
    parts = [([], []) for _ in feeds]
    empty = np.zeros(0, np.int16)
    i = 0
    while not all(done):
        blocks, end = [], []
        for k, (w, blk, _) in enumerate(feeds):
            n = 0 if done[k] or i % 7 == 3 else min(blk, w.size - at[k])
            blocks.append(w[at[k]:at[k] + n] if n else empty)
            at[k] += n
            fin = n > 0 and at[k] == w.size
            end.append(int(fin))
            done[k] = done[k] or fin
        out, outf = live.push(blocks, end, return_f32=True)
        for k in range(3):
            parts[k][0].append(out[k]), parts[k][1].append(outf[k])
        i += 1
    for k, (_, _, u) in enumerate(feeds):
        same(np.concatenate(parts[k][1]), c.gv[u][1], "session %d" % k)
        same(np.concatenate(parts[k][0]), c.gv[u][0], "session %d" % k)
    live.close()
    eng.close()


def test_a_relu_and_a_nat_engine(pkg, cases):
    fs = 8
    c = cases[fs]
    w = c.waves[2]
    relu = c.engine(activation="relu")
    want = compose(pkg, relu, w, c.mean, c.inv, c.eta, fs)
    assert want[2].tobytes() != c.gv[2][2].tobytes()              # other units, other rows
    relu.set_gv(c.eta)
    out, outf = c.wave(relu, w)
    same(outf, want[1]), same(out, want[0])
    relu.close()
    # NAT: the rows through the expanded entry, as tests/test_gpu_nat_decode.py forms them
    T, D = 4, c.D
    rng = np.random.default_rng(5)
    ls = [(CTX + 1) * D, 32, D]
    ws = [rng.normal(0, 0.05, (ls[i], ls[i + 1])).astype(np.float32) for i in range(2)]
    bs = [rng.normal(0, 0.1, ls[i + 1]).astype(np.float32) for i in range(2)]
    nat = pkg.BPGpu(1, 0, ls, B, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0, nat_frames=T)
    x = nat_model.normalise(pkg.wave_to_lps(w, fs_khz=fs), c.mean, c.inv)
    F = x.shape[0]
    z = nat_model.noise_rows(x, [0, F], T)
    y = nat.forward(nat_model.expand(nat_model.edge_stream(x, CTX), np.arange(F), CTX, z, np.zeros(F, np.int32)))
    v = gv64.apply32(y, c.eta, c.inv, c.mean)
    wout, woutf = pkg.lps_to_wave(w, v, fs_khz=fs, return_float=True)
    nat.set_gv(c.eta)
    out, outf = c.wave(nat, w)
    same(outf, woutf), same(out, wout)
    rows = nat.enhance_waves([w], c.mean, c.inv, fs_khz=fs, fea_context=CTX, return_lps=True)[1]
    same(rows[0], v)
    nat.close()


def test_a_bad_factor_is_refused_naming_the_bin(pkg, cases):
    c = cases[8]
    eng = c.engine()
    eng.set_gv(c.eta)
    before = c.wave(eng, c.waves[2])
    for d, bad in ((0, 0.0), (5, -1.5), (c.D - 1, float("nan")), (17, float("inf")), (3, -0.0)):
        e = c.eta.copy()
        e[d] = bad
        with pytest.raises(pkg.MlggdError, match=r"error 1: eta\[%d\]" % d):
            eng.set_gv(e)
        assert eng.gv().tobytes() == c.eta.tobytes()
    with pytest.raises(ValueError):
        eng.set_gv(c.eta[:-1])
    after = c.wave(eng, c.waves[2])
    same(after[1], before[1]), same(after[0], before[0])
    same(after[1], c.gv[2][1])
    L = pkg.load()
    assert L.mlggd_set_gv(None, None) == 1 and L.mlggd_get_gv(eng._h, None) == 1
    # an engine without factors stays without them
    fresh = c.engine()
    e = np.ones(c.D, np.float32)
    e[1] = 0
    with pytest.raises(pkg.MlggdError, match=r"error 1: eta\[1\]"):
        fresh.set_gv(e)
    same(c.wave(fresh, c.waves[2])[1], c.plain[2][1])
    fresh.close()
    eng.close()


def test_one_factor_changes_one_column(cases):
    c = cases[8]
    eng = c.engine()
    k = 37
    e = np.ones(c.D, np.float32)
    e[k] = 1.75
    eng.set_gv(e)
    rows = eng.enhance_waves(c.waves, c.mean, c.inv, fs_khz=8, fea_context=CTX, return_lps=True)[1]
    for u in range(len(FRAMES)):
        diff = rows[u] != c.plain[u][2]
        assert diff[:, k].all() and not np.delete(diff, k, axis=1).any(), u
    eng.close()
