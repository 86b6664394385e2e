"""GPU: the signed error statistics of a CV chunk (BPGpu.error_stats_signed / error_stats_signed_frames,
k_err_stats_signed in csrc/colstats.hip.h): per bin and grid shape P+ = sum_{e>0} e^beta and P- = sum_{e<0} (-e)^beta.

The pin is that of tests/test_gpu_error_stats.py: out = eng.forward(inp), e = out - targ in float32, the power terms
from oracle/pyoracle.pow_det widened to float64 and sent to the side of e's sign, every sum by math.fsum; a double sum
of n terms in any order is within 2 n 2^-53 sum|term| of that.  Beyond the pin: the two entries return the same bits
for the same rows, a call repeats its bits, chunks add up, P+ + P- is error_stats' row 4 + k to double rounding (each a
sum of at most n non-negative terms: gamma_n in double on either side, one more rounding for the addition), the
vectors in effect do not matter, and every refusal leaves a usable engine.

Shapes: D = 33 (one bin past a 32-bin strip), context 3, net 99-64-33, B = 32 and 128; n in {0, 1, 31, 33, 2B + 7}:
row counts that are no multiple of 32 and a trailing partial bunch."""
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
    "full": (0.3 + 0.075 * np.arange(32)).astype(np.float32),                 # 32 shapes: all 64 accumulators
}


def make_engine(pkg, synth, ls, B, beta=1.2, seed=3):
    ws, bs = synth.make_weights(ls, seed=seed)
    bs = [np.random.default_rng(seed + 1 + i).uniform(-0.3, 0.3, b.size).astype(np.float32) for i, b in enumerate(bs)]
    return pkg.BPGpu(1, 0, ls, B, *HP, ws, bs, beta, 1)


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


def pin(pyoracle, out, targ, betas):
    """(want [2 K][D], bound [2 K][D]) from the network outputs"""
    K, D = len(betas), targ.shape[1]
    if out.shape[0] == 0:
        z = np.zeros((2 * K, D))
        return z, z.copy()
    e = (out.astype(np.float32) - targ.astype(np.float32)).astype(np.float32)
    a = np.abs(e)
    plus, minus = [], []
    for b in betas:
        p = (a.ravel().copy() if b == np.float32(1.0) else pyoracle.pow_det(a.ravel(), np.float32(b))).reshape(a.shape)
        p = p.astype(np.float64)
        plus.append(np.where(e > 0, p, 0.0))
        minus.append(np.where(e < 0, p, 0.0))
    terms = plus + minus
    n = e.shape[0]
    want = np.array([[math.fsum(t[:, d]) for d in range(D)] for t in terms], np.float64).reshape(2 * K, D)
    return want, 2.0 * n * 2.0 ** -53 * want


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def engines(pkg, synth):
    made = {B: make_engine(pkg, synth, LS, B) for B in (32, 128)}
    yield made
    for e in made.values():
        e.close()


@pytest.mark.parametrize("B", [32, 128])
@pytest.mark.parametrize("n", [0, 1, 31, 33, "2B+7"])
def test_sums_against_the_pin_and_both_entries_agree(pkg, pyoracle, engines, B, n):
    eng = engines[B]
    n = 2 * B + 7 if n == "2B+7" else n
    feat, tstream, first, inp, targ = make_chunk(n, seed=100 + n)
    out = eng.forward(inp) if n else np.zeros((0, FDIM), np.float32)
    for name, betas in GRIDS.items():
        K = betas.size
        got = eng.error_stats_signed(inp, targ, betas)
        assert got.shape == (2 * K, FDIM) and got.dtype == np.float64
        want, bound = pin(pyoracle, out, targ, betas)
        err = np.abs(got - want)
        print("B %d n %d grid %s: max |got - want| / bound = %.3g" % (B, n, name, (err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (name, np.argwhere(err > bound)[:5])
        assert same_bits(got, eng.error_stats_signed(inp, targ, betas))                               # a call repeats its bits
        assert same_bits(got, eng.error_stats_signed_frames(feat, tstream, first, CTX, TOFF, betas))  # the same rows
        # P+ + P- against the unsigned sums: gamma_n in double on either side, one rounding for the addition
        both = eng.error_stats(inp, targ, betas)[4:]
        gn = n * 2.0 ** -53 / (1.0 - n * 2.0 ** -53)
        assert (np.abs((got[:K] + got[K:]) - both) <= (2.0 * gn + 2.0 ** -53) * both).all(), name
    if n == 0:
        assert not got.any()
    elif n > 1:
        assert (got[:K] > 0).any() and (got[K:] > 0).any()                 # both signs occur


def test_chunks_add_up_and_the_vectors_in_effect_do_not_matter(pkg, pyoracle, engines):
    B = 32
    eng = engines[B]
    n = 3 * B + 9
    _, _, _, inp, targ = make_chunk(n, seed=8)
    betas = GRIDS["six"]
    whole = eng.error_stats_signed(inp, targ, betas)
    cut = 2 * B
    parts = eng.error_stats_signed(inp[:cut], targ[:cut], betas) + eng.error_stats_signed(inp[cut:], targ[cut:], betas)
    _, bound = pin(pyoracle, eng.forward(inp), targ, betas)
    assert (np.abs(parts - whole) <= bound).all()
    try:
        eng.set_shapefactors(np.linspace(0.6, 2.0, FDIM).astype(np.float32))
        eng.set_asymmetry(np.linspace(0.5, 2.0, FDIM).astype(np.float32))
        assert same_bits(eng.error_stats_signed(inp, targ, betas), whole)
    finally:
        eng.set_shapefactors(None)
        eng.set_asymmetry(None)
    assert same_bits(eng.error_stats_signed(inp, targ, betas), whole)


def test_the_fitted_model_is_the_trainer_s(pkg, synth):
    """One bunch: with the skew of asym_fit set on the engine, alpha of asym_fit at beta = shapefactor against the
    scalefactor the training step on the same rows leaves.  The trainer forms it in fp32: the rounding of kappa to
    fp32 (1, through s), s itself (1), the power (1 ulp = 2 roundings' worth at most, beta of it through the
    argument), the colsum of B non-negative terms (B - 1), / n, * beta, the 1/beta power and the rounding of 1/beta
    (4), each worth up to max(1, 1/beta) through the last power once the argument's roundings are scaled by beta."""
    B, beta = 32, 1.2
    eng = make_engine(pkg, synth, LS, B, beta=beta)
    try:
        _, _, _, inp, targ = make_chunk(B, seed=11)
        b32 = np.array([beta], np.float32)
        fit = pkg.asym_fit(B, eng.error_stats_signed(inp, targ, b32), b32)
        ok = fit.best == 0                                 # a bin whose 32 errors share one sign has no fit: it keeps 1
        assert ok.sum() > FDIM // 2 and np.isfinite(fit.kappa[0][ok]).all() and np.isnan(fit.kappa[0][~ok]).all()
        eng.set_asymmetry(np.where(ok, fit.kappa[0], 1.0).astype(np.float32))
        assert eng.train(inp, targ) == 1
        alpha = eng.scalefactor().astype(np.float64)
        rel = (np.abs(alpha - fit.alpha[0]) / np.where(ok, fit.alpha[0], 1.0))[ok]
        # d ln alpha / d ln kappa is at most 1 in magnitude (alpha^beta = (beta/n)(kappa^beta P+ + kappa^-beta P-))
        bound = ((B - 1) + 4 + 2 + 2 * beta + 1) * 2.0 ** -24 * max(1.0, 1.0 / beta)
        print("max relative distance %.3g, bound %.3g" % (rel.max(), bound))
        assert (rel <= bound).all()
    finally:
        eng.close()


def test_every_refusal_leaves_a_usable_engine(pkg, synth, engines):
    B = 32
    feat, tstream, first, inp, targ = make_chunk(B + 3, seed=12)
    betas = GRIDS["six"]
    fake = make_engine(pkg, synth, LS, B)
    fake.fake_world(2, allreduce=True)
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_error_stats_signed runs on a single-device engine"):
        fake.error_stats_signed(inp, targ, betas)
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_error_stats_signed_frames runs on a single-device engine"):
        fake.error_stats_signed_frames(feat, tstream, first, CTX, TOFF, betas)
    fake.close()
    eng = engines[B]
    want = eng.error_stats_signed(inp, targ, betas)
    for bad, msg in ((np.zeros(0, np.float32), "n_betas 0"), (np.ones(33, np.float32), "n_betas 33"),
                     ([1.0, 0.0], r"betas\[1\]"), ([-0.5], r"betas\[0\]"), ([1.0, float("nan")], r"betas\[1\]"),
                     ([float("inf")], r"betas\[0\]")):
        with pytest.raises(pkg.MlggdError, match="error 1: " + msg):
            eng.error_stats_signed(inp, targ, bad)
        with pytest.raises(pkg.MlggdError, match="error 1: " + msg):
            eng.error_stats_signed_frames(feat, tstream, first, CTX, TOFF, bad)
    with pytest.raises(pkg.MlggdError, match=r"error 1: targ_offset 3"):
        eng.error_stats_signed_frames(feat, tstream, first, CTX, 3, betas)
    with pytest.raises(ValueError):
        eng.error_stats_signed(inp[:, :-1], targ, betas)
    L = pkg.load()
    assert L.mlggd_error_stats_signed(eng._h, 4, None, None, 1, None, None) == 1 and "NULL" in L.mlggd_last_error().decode()
    assert L.mlggd_error_stats_signed(None, 4, None, None, 1, None, None) == 1
    assert same_bits(eng.error_stats_signed(inp, targ, betas), want)
