"""GPU: the error statistics of a CV chunk (BPGpu.error_stats / error_stats_frames, csrc/colstats.hip.h).

The pin: out = eng.forward(inp), e = out - targ in float32, the four moment terms in float64 from that e, the power
terms from oracle/pyoracle.pow_det (cross-checked once against the device's own pow_det) widened to float64, every sum
by math.fsum.  A double sum of n terms in ANY order is within 2 n 2^-53 sum|term| of that, and nothing else separates
the two sides, so that is the bound of every entry.  Beyond the pin: the two entries return the same bits for the same
rows, a call repeats its bits -- also after other calls have used the engine's workspaces --, chunks add up, the ML
scale of ggd_fit is the trainer's scalefactor, and every refusal leaves a usable engine.

Shapes: D = 33 (one bin past a 32-bin strip), context 3, net 99-64-33, B = 32 and 128 (one and four 32-row tiles),
n in {0, 1, 31, 32, 33, 2B + 7}; one net whose output layer is summed from several split-K slabs."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HP = (0.1, 0.9, 1e-5)
FDIM, CTX, TOFF = 33, 3, 2
LS = [FDIM * CTX, 64, FDIM]
GRIDS = {
    "one": np.array([1.0], np.float32),                                       # pow_or_self's shortcut alone
    "six": np.array([0.5, 0.9, 1.0, 1.2, 2.0, 2.5], np.float32),
    "full": (0.3 + 0.075 * np.arange(32)).astype(np.float32),                 # 32 shapes, 0.3 .. 2.625
}


def make_engine(pkg, synth, ls, B, beta=1.2, ML=1, seed=3, **kw):
    ws, bs = synth.make_weights(ls, seed=seed)
    bs = [np.random.default_rng(seed + 1 + i).uniform(-0.3, 0.3, b.size).astype(np.float32) for i, b in enumerate(bs)]
    return pkg.BPGpu(1, 0, ls, B, *HP, ws, bs, beta, ML, **kw), ws, bs


def make_chunk(n, seed, fdim=FDIM, ctx=CTX, toff=TOFF):
    """a frame stream, shuffled first frames of n samples and the expanded rows they stand for"""
    rng = np.random.default_rng(seed)
    F = n + ctx + 5
    feat = rng.standard_normal((F, fdim), dtype=np.float32)
    tstream = (0.5 * feat + 0.5 * rng.standard_normal((F, fdim), dtype=np.float32)).astype(np.float32)
    first = rng.permutation(F - ctx + 1)[:n].astype(np.int32)
    idx = first[:, None] + np.arange(ctx)[None, :]
    inp = np.ascontiguousarray(feat[idx].reshape(n, ctx * fdim))
    targ = np.ascontiguousarray(tstream[first + toff])
    return feat, tstream, first, inp, targ


def pow_or_self(pyoracle, a, b):
    return a.copy() if b == np.float32(1.0) else pyoracle.pow_det(a, np.float32(b))


def pin(pyoracle, out, targ, betas):
    """(want [4 + K][D], bound [4 + K][D]) from the network outputs"""
    if out.shape[0] == 0:
        z = np.zeros((4 + len(betas), targ.shape[1]))
        return z, z.copy()
    e = (out.astype(np.float32) - targ.astype(np.float32)).astype(np.float32)
    e1 = e.astype(np.float64)
    e2 = e1 * e1
    a = np.abs(e)
    terms = [e1, e2, e2 * e1, e2 * e2]
    for b in betas:
        terms.append(pow_or_self(pyoracle, a.ravel(), b).reshape(a.shape).astype(np.float64))
    n, D = e.shape
    want = np.array([[math.fsum(t[:, d]) for d in range(D)] for t in terms], np.float64).reshape(len(terms), D)
    mag = np.array([[math.fsum(np.abs(t[:, d])) for d in range(D)] for t in terms], np.float64).reshape(len(terms), D)
    return want, 2.0 * n * 2.0 ** -53 * mag


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def engines(pkg, synth):
    made = {B: make_engine(pkg, synth, LS, B)[0] for B in (32, 128)}
    yield made
    for e in made.values():
        e.close()


def test_the_oracle_s_power_is_the_device_s(pkg, pyoracle, engines):
    x = np.abs(np.random.default_rng(0).standard_normal(4096)).astype(np.float32)
    x[:3] = [0.0, 1e-30, 40.0]
    for b in GRIDS["full"][::5]:
        dev = engines[32].debug_math("pow_det", x, np.float32(b))
        assert np.array_equal(dev.view(np.uint32), pyoracle.pow_det(x, np.float32(b)).view(np.uint32)), b


@pytest.mark.parametrize("B", [32, 128])
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, "2B+7"])
def test_sums_against_the_pin_and_both_entries_agree(pkg, pyoracle, engines, B, n):
    eng = engines[B]
    n = 2 * B + 7 if n == "2B+7" else n
    feat, tstream, first, inp, targ = make_chunk(n, seed=100 + n)
    out = eng.forward(inp) if n else np.zeros((0, FDIM), np.float32)
    for name, betas in GRIDS.items():
        got = eng.error_stats(inp, targ, betas)
        assert got.shape == (4 + betas.size, FDIM) and got.dtype == np.float64
        want, bound = pin(pyoracle, out, targ, betas)
        err = np.abs(got - want)
        print("B %d n %d grid %s: max |got - want| / bound = %.3g" % (B, n, name, (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (name, np.argwhere(err > bound)[:5])
        assert same_bits(got, eng.error_stats(inp, targ, betas))                               # a call repeats its bits
        assert same_bits(got, eng.error_stats_frames(feat, tstream, first, CTX, TOFF, betas))  # the same rows
    if n == 0:
        assert not got.any()


def test_an_output_layer_of_several_slabs(pkg, synth, pyoracle):
    B = 32
    eng, _, _ = make_engine(pkg, synth, [FDIM * CTX, 512, FDIM], B)
    try:
        assert eng.out_slabs() > 1
        n = B + 5
        feat, tstream, first, inp, targ = make_chunk(n, seed=7)
        out = eng.forward(inp)
        got = eng.error_stats(inp, targ, GRIDS["six"])
        want, bound = pin(pyoracle, out, targ, GRIDS["six"])
        assert (np.abs(got - want) <= bound).all()
        assert same_bits(got, eng.error_stats_frames(feat, tstream, first, CTX, TOFF, GRIDS["six"]))
    finally:
        eng.close()


def test_chunks_add_up(pkg, pyoracle, engines):
    B = 32
    eng = engines[B]
    n = 3 * B + 9
    _, _, _, inp, targ = make_chunk(n, seed=8)
    betas = GRIDS["six"]
    whole = eng.error_stats(inp, targ, betas)
    cut = 2 * B
    parts = eng.error_stats(inp[:cut], targ[:cut], betas) + eng.error_stats(inp[cut:], targ[cut:], betas)
    _, bound = pin(pyoracle, eng.forward(inp), targ, betas)
    assert (np.abs(parts - whole) <= bound).all()


def test_the_same_bits_after_other_calls_used_the_workspaces(pkg, synth):
    """cv_all, an enhance_waves call and a train + set_weights round trip back to the same weights in between"""
    fs, ctx, D, B = 8, 3, 129, 32
    eng, ws, bs = make_engine(pkg, synth, [D * ctx, 64, D], B)
    try:
        n = 2 * B + 7
        feat, tstream, first, inp, targ = make_chunk(n, seed=9, fdim=D, ctx=ctx, toff=1)
        betas = GRIDS["six"]
        eng.set_scalefactor(np.full(D, 0.7, np.float32))              # a finite log-likelihood to compare
        first_cv = eng.cv_all(inp, targ)
        want = eng.error_stats(inp, targ, betas)
        assert eng.cv_all(inp, targ) == first_cv                      # error_stats leaves cv_all's results alone
        assert same_bits(eng.error_stats(inp, targ, betas), want)
        eng.set_cv_device_reduce(True)
        dev_cv = eng.cv_all(inp, targ)
        assert same_bits(eng.error_stats_frames(feat, tstream, first, ctx, 1, betas), want)
        assert eng.cv_all(inp, targ) == dev_cv
        eng.set_cv_device_reduce(False)
        rng = np.random.default_rng(10)
        waves = [(3000 * rng.standard_normal(m)).astype(np.int16) for m in (2100, 900)]
        eng.enhance_waves(waves, np.zeros(D, np.float32), np.ones(D, np.float32), fs_khz=fs, fea_context=ctx)
        assert same_bits(eng.error_stats(inp, targ, betas), want)
        assert eng.train(inp, targ) == 2
        assert not same_bits(eng.error_stats(inp, targ, betas), want)  # other weights, other errors
        eng.set_weights(ws, bs)
        assert same_bits(eng.error_stats(inp, targ, betas), want)
        assert same_bits(eng.error_stats_frames(feat, tstream, first, ctx, 1, betas), want)
    finally:
        eng.close()


@pytest.mark.parametrize("beta", [0.9, 1.0, 1.2, 2.0])
def test_the_fitted_scale_is_the_trainer_s_scalefactor(pkg, synth, beta):
    """One bunch: alpha of ggd_fit at beta = shapefactor against the scalefactor the training step on the same rows
    leaves.  The trainer forms it in fp32 -- colsum of B non-negative terms (B - 1 roundings), / n, * beta, then the
    1/beta power: a divide, a multiply, the power's own rounding and the rounding of 1/beta, 4 in all, each worth up
    to max(1, 1/beta) through the power; p = 1 is pow_det's distance from the rounded exact power, the `max 1 ulp`
    tests/test_gpu_loss_ulps.py asserts and prints for this device -- and ggd_fit in double from the same fp32 terms."""
    B, p = 32, 1
    eng, _, _ = make_engine(pkg, synth, LS, B, beta=beta)
    try:
        _, _, _, inp, targ = make_chunk(B, seed=11)
        b32 = np.array([beta], np.float32)
        fit = pkg.ggd_fit(B, eng.error_stats(inp, targ, b32), b32)
        assert eng.train(inp, targ) == 1
        alpha = eng.scalefactor().astype(np.float64)
        rel = np.abs(alpha - fit.alpha[0]) / fit.alpha[0]
        bound = ((B - 1) + 4 + p) * 2.0 ** -24 * max(1.0, 1.0 / beta)
        print("beta %.1f: max relative distance %.3g, bound %.3g" % (beta, rel.max(), bound))
        assert (rel <= bound).all()
    finally:
        eng.close()


def test_every_refusal_leaves_a_usable_engine(pkg, synth, engines):
    B = 32
    _, _, _, inp, targ = make_chunk(B + 3, seed=12)
    feat, tstream, first, _, _ = make_chunk(B + 3, seed=12)
    betas = GRIDS["six"]
    # an emulated world
    fake, _, _ = make_engine(pkg, synth, LS, B)
    fake.fake_world(2, allreduce=True)
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_error_stats runs on a single-device engine"):
        fake.error_stats(inp, targ, betas)
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_error_stats_frames runs on a single-device engine"):
        fake.error_stats_frames(feat, tstream, first, CTX, TOFF, betas)
    assert fake.train(np.tile(inp, (2, 1)), np.tile(targ, (2, 1))) == 1      # one global minibatch of 2 x B rows
    fake.close()
    # dropout
    drop, _, _ = make_engine(pkg, synth, LS, B, dropoutflag=1, visible_omit=0.1, hid_omit=0.2)
    with pytest.raises(pkg.MlggdError, match=r"error 4: .*not available with dropoutflag"):
        drop.error_stats(inp, targ, betas)
    assert np.isfinite(drop.cv_all(inp, targ)[0]) and drop.train(inp, targ) == 1
    drop.close()
    # bad arguments
    eng = engines[B]
    want = eng.error_stats(inp, targ, betas)
    for bad, msg in ((np.zeros(0, np.float32), "n_betas 0"), (np.ones(33, np.float32), "n_betas 33"),
                     ([1.0, 0.0], r"betas\[1\]"), ([-0.5], r"betas\[0\]"), ([1.0, float("nan")], r"betas\[1\]"),
                     ([float("inf")], r"betas\[0\]")):
        with pytest.raises(pkg.MlggdError, match="error 1: " + msg):
            eng.error_stats(inp, targ, bad)
        with pytest.raises(pkg.MlggdError, match="error 1: " + msg):
            eng.error_stats_frames(feat, tstream, first, CTX, TOFF, bad)
    with pytest.raises(pkg.MlggdError, match=r"error 1: targ_offset 3"):
        eng.error_stats_frames(feat, tstream, first, CTX, 3, betas)
    with pytest.raises(pkg.MlggdError, match=r"error 1: sample 0: window"):
        eng.error_stats_frames(feat, tstream, first + 1000, CTX, TOFF, betas)
    with pytest.raises(ValueError):
        eng.error_stats(inp[:, :-1], targ, betas)
    L = pkg.load()
    assert L.mlggd_error_stats(eng._h, 4, None, None, 1, None, None) == 1 and "NULL" in L.mlggd_last_error().decode()
    assert L.mlggd_error_stats(None, 4, None, None, 1, None, None) == 1
    assert same_bits(eng.error_stats(inp, targ, betas), want)
