"""GPU: one shape factor per output bin (BPGpu.set_shapefactors) through every loss path.

Column d of the ML-GGD loss chain depends on column d's errors and on beta_d alone, and the vector kernels keep the
scalar kernels' expressions and order, which gives two checks that need no tolerance: a uniform vector leaves the bits
of the scalar engine, and under a mixed vector the columns of one value carry the bits of a scalar engine at that
value.  The float64 checks are those of tests/test_gpu_vs_float64.py with the loss bound applied per group of columns
of equal beta (tests/shapes64.py).

Shapes: 40-64-D with D = 19 (Dp 32: a partly filled group of 8 units and an empty one) and D = 257 (Dp 288: a last
group with one live unit); B = 32 and B = 160 (the fused kernel's 128-frame loop runs a second, partial pass).  The
emulated worlds run at 32 frames per rank (2 x 32 = one 64-frame unit of the factor exchange), the all-reduce form
also at 160."""
import numpy as np
import pytest

import bounds64 as b6
import shapes64 as s6
import spec64

pytestmark = pytest.mark.gpu

HP = (0.1, 0.9, 1e-5)
NO_MOM = (0.05, 0.0, 1e-5)
KNOBS = ("MLGGD_TILE64", "MLGGD_S_OUT", "MLGGD_LOSS_FUSE", "MLGGD_DW_MERGE", "MLGGD_STAGE_AHEAD", "MLGGD_CV_DEVICE",
         "MLGGD_DW_TILE", "MLGGD_DW_PERSIST", "MLGGD_DWP_PER_CU", "MLGGD_TILE_MAP")
SHAPES = [(19, 32), (19, 160), (257, 32), (257, 160)]
# (mode, D, B): fused and unfused on one device at every shape; the emulated worlds where the exchange exists
SINGLE = [(m, D, B) for m in ("fused", "unfused") for D, B in SHAPES]
WORLDS = [("gather", D, 32) for D in (19, 257)] + [("allreduce", D, B) for D, B in SHAPES]
_CACHE = {}


def ls_of(D):
    return [40, 64, D]


def net(D):
    if ("net", D) not in _CACHE:
        _CACHE["net", D] = b6.make_net(ls_of(D), 100 + D)
    return _CACHE["net", D]


def frames(D, n, seed=0):
    """n rows of inputs and targets, computed once per (D, n, seed) and never written to"""
    key = ("frames", D, n, seed)
    if key not in _CACHE:
        x, t = b6.make_data(ls_of(D), n, 200 + D + seed)
        x.setflags(write=False)
        t.setflags(write=False)
        _CACHE[key] = (x, t)
    return _CACHE[key]


def rows_per_step(mode, B):
    return 2 * B if mode in ("gather", "allreduce") else B


def engine(pkg, monkeypatch, mode, D, B, beta, ml=1, hp=HP, W=None, b=None):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if mode == "unfused":
        monkeypatch.setenv("MLGGD_LOSS_FUSE", "0")
    if W is None:
        W, b = net(D)
    eng = pkg.BPGpu(1, 0, ls_of(D), B, *hp, W, b, beta, ml)
    if mode == "gather":
        eng.fake_world(2)                     # the factor all-gather: CS_ACCUMULATE, then CS_GIVEN on the last rank
    elif mode == "allreduce":
        eng.fake_world(2, allreduce=True)     # the gradient all-reduce
    return eng


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def snapshot(eng, L=3):
    W, b = eng.returnWeights()
    return ([bits(w) for w in W], [bits(v) for v in b], [bits(eng.debug_tensor("delta_w", l)) for l in range(1, L)],
            [bits(eng.debug_tensor("delta_b", l)) for l in range(1, L)], bits(eng.scalefactor()))


def same(a, b):
    names = ("weights", "bias", "delta_w", "delta_b")
    for name, xs, ys in zip(names, a[:4], b[:4]):
        for l, (x, y) in enumerate(zip(xs, ys)):
            assert np.array_equal(x, y), "%s of layer %d differ in %d bits" % (name, l + 1, int((x != y).sum()))
    assert np.array_equal(a[4], b[4]), "scalefactor"


# ---------------------------------------------------------------------------------------------------------------------
# 1. a uniform vector is the scalar engine, bit for bit
@pytest.mark.parametrize("beta", [0.9, 1.0, 2.0])
@pytest.mark.parametrize("mode,D,B", SINGLE + WORLDS)
def test_uniform_vector_equals_scalar(pkg, monkeypatch, mode, D, B, beta):
    x, t = frames(D, 6 * rows_per_step(mode, B))
    vec = engine(pkg, monkeypatch, mode, D, B, 1.7)        # its own shapefactor is NOT beta: the vector must be what counts
    sca = engine(pkg, monkeypatch, mode, D, B, beta)
    try:
        vec.set_shapefactors(np.full(D, beta, np.float32))
        assert vec.train(x, t) == 6 and sca.train(x, t) == 6
        same(snapshot(vec), snapshot(sca))
    finally:
        vec.close()
        sca.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. under a mixed vector the columns of one value are a scalar engine's at that value, bit for bit
@pytest.mark.parametrize("mode,D,B", SINGLE + WORLDS)
def test_columns_are_independent(pkg, monkeypatch, mode, D, B):
    x, t = frames(D, rows_per_step(mode, B), seed=1)
    betas = s6.mixed(D)
    vec = engine(pkg, monkeypatch, mode, D, B, 1.7)
    try:
        vec.set_shapefactors(betas)
        assert vec.train(x, t) == 1
        out, dedx, alpha = bits(vec.debug_tensor("out")), bits(vec.debug_tensor("dedx", 2)), bits(vec.scalefactor())
    finally:
        vec.close()
    assert len(s6.groups(betas)) == len(s6.CYCLE)
    for v, cols in s6.groups(betas):
        sca = engine(pkg, monkeypatch, mode, D, B, v)
        try:
            assert sca.train(x, t) == 1
            assert np.array_equal(out, bits(sca.debug_tensor("out"))), v            # the forward pass knows no shape
            got = bits(sca.debug_tensor("dedx", 2))
            assert np.array_equal(dedx[:, cols], got[:, cols]), "dedx, columns of beta %g" % v
            assert np.array_equal(alpha[cols], bits(sca.scalefactor())[cols]), "scalefactor, columns of beta %g" % v
            other = ~cols
            assert not np.array_equal(dedx[:, other], got[:, other])               # ... and the others are not its
        finally:
            sca.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. against float64
def state(eng, L=3):
    W, b = eng.returnWeights()
    return W, b, [eng.debug_tensor("delta_w", l) for l in range(1, L)], [eng.debug_tensor("delta_b", l) for l in range(1, L)]


@pytest.mark.parametrize("mode,D,B", SINGLE)
def test_mixed_vector_against_float64(pkg, monkeypatch, mode, D, B):
    """4 steps, every operation against its own fp32 inputs as tests/test_gpu_vs_float64.py does it for a scalar step;
    bounds64.expect_loss per group of columns of equal beta (shapes64.check_step_bins), no new tolerance"""
    L = 3
    x, t = frames(D, 4 * B, seed=2)
    betas = s6.mixed(D)
    eng = engine(pkg, monkeypatch, mode, D, B, 1.7)
    bad = []
    try:
        eng.set_shapefactors(betas)
        for k in range(4):
            W, b, dW, db = state(eng)
            xb, tb = x[k * B:(k + 1) * B], t[k * B:(k + 1) * B]
            assert eng.train(xb, tb) == 1
            Wn, bn, dWn, dbn = state(eng)
            s = b6.Step(xb, tb, W, b, dW, db, {l: eng.debug_tensor("y", l) for l in range(1, L - 1)},
                        eng.debug_tensor("out"), {l: eng.debug_tensor("dedx", l) for l in range(1, L)}, dWn, dbn, Wn, bn,
                        HP[0], HP[1], HP[2], 1.7, 1, eng.out_slabs(), eng.scalefactor())
            reps = s6.check_step_bins(s, betas)
            assert sum(r.name.startswith("loss ML beta_d") for r in reps) == len(s6.CYCLE)
            for r in reps:
                print("step %d %s" % (k + 1, r.line()))
            bad += ["step %d %s" % (k + 1, r.line()) for r in reps if not r.ok]
    finally:
        eng.close()
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the CV log-likelihood under the mixed vector
@pytest.mark.parametrize("device_reduce", [False, True], ids=["host_order", "device_reduce"])
@pytest.mark.parametrize("D,B", SHAPES)
def test_cv_loglik_with_a_mixed_vector(pkg, monkeypatch, D, B, device_reduce):
    """The log-likelihood of cv_all on n = B + 7 frames (a whole bunch and a partial one) against the float64 formula with
    beta_d per column, under bounds64.expect_cv's bound generalised term by term in shapes64.expect_cv_bins"""
    x, t = frames(D, 2 * B, seed=3)
    cx, ct = frames(D, B + 7, seed=4)
    betas = s6.mixed(D)
    eng = engine(pkg, monkeypatch, "fused", D, B, 1.7)
    try:
        eng.set_shapefactors(betas)
        assert eng.train(x, t) == 2
        eng.set_cv_device_reduce(device_reduce)
        sq, ab, ll = eng.cv_all(cx, ct)
        ex = s6.expect_cv_bins(eng.forward(cx), ct, betas, eng.scalefactor(), pkg.gamma)
        eng.set_shapefactors(None)
        sq0, ab0, ll0 = eng.cv_all(cx, ct)
    finally:
        eng.close()
    r = b6.compare("loglik", np.array(ll), ex["loglik"])
    print(r.line())
    assert r.ok, r.line()
    assert ll0 != ll                                        # the vector is what the number was formed with
    # the two sums that know no shape are bystanders: the bits of the same engine without the vector
    assert bits(np.float32([sq, ab])).tolist() == bits(np.float32([sq0, ab0])).tolist()


# ---------------------------------------------------------------------------------------------------------------------
# 5. state
@pytest.mark.parametrize("mode", ["fused", "unfused"])
def test_set_and_reset_before_the_first_step_leave_a_scalar_run(pkg, monkeypatch, mode):
    D, B = 257, 160
    x, t = frames(D, 3 * B)
    a = engine(pkg, monkeypatch, mode, D, B, 1.2)
    ref = engine(pkg, monkeypatch, mode, D, B, 1.2)
    try:
        assert np.array_equal(a.shapefactors(), np.full(D, 1.2, np.float32))
        a.set_shapefactors(s6.mixed(D))
        assert np.array_equal(a.shapefactors(), s6.mixed(D))                       # round trip
        a.set_shapefactors(None)
        assert np.array_equal(a.shapefactors(), np.full(D, 1.2, np.float32))
        assert a.train(x, t) == 3 and ref.train(x, t) == 3
        same(snapshot(a), snapshot(ref))
    finally:
        a.close()
        ref.close()


def test_reset_after_training_continues_as_a_scalar_engine(pkg, monkeypatch):
    """The momentum buffers cannot be set from outside, so this run has momentum 0: the next delta is then
    0 * delta - lrate * (...), whatever delta holds.  Two steps under a mixed vector, reset, two more steps -- beside a
    scalar engine created from the weights and the scalefactor read back at the reset.  (With momentum, the set and
    reset before the first step above compares whole runs.)"""
    D, B = 257, 160
    x, t = frames(D, 4 * B)
    a = engine(pkg, monkeypatch, "fused", D, B, 1.2, hp=NO_MOM)
    try:
        a.set_shapefactors(s6.mixed(D))
        assert a.train(x[:2 * B], t[:2 * B]) == 2
        a.set_shapefactors(None)
        W, b = a.returnWeights()
        alpha = a.scalefactor()
        c = engine(pkg, monkeypatch, "fused", D, B, 1.2, hp=NO_MOM, W=W, b=b)
        try:
            c.set_scalefactor(alpha)
            cx, ct = frames(D, B + 7, seed=4)
            assert bits(np.float32(a.cv_all(cx, ct))).tolist() == bits(np.float32(c.cv_all(cx, ct))).tolist()
            assert a.train(x[2 * B:], t[2 * B:]) == 2 and c.train(x[2 * B:], t[2 * B:]) == 2
            sa, sc = snapshot(a), snapshot(c)
            for xs, ys in zip(sa[:2], sc[:2]):
                for p, q in zip(xs, ys):
                    assert np.array_equal(p, q)
            assert np.array_equal(sa[4], sc[4])
            for l in (1, 2):                               # 0 * delta may be -0: equal as numbers
                assert np.array_equal(a.debug_tensor("delta_w", l), c.debug_tensor("delta_w", l))
        finally:
            c.close()
    finally:
        a.close()


@pytest.mark.parametrize("bad", [0.0, float("nan"), float("inf"), -1.0])
@pytest.mark.parametrize("with_vector", [False, True])
def test_a_bad_vector_is_refused_and_changes_nothing(pkg, monkeypatch, bad, with_vector):
    D, B = 19, 32
    x, t = frames(D, B)
    a = engine(pkg, monkeypatch, "fused", D, B, 1.2)
    ref = engine(pkg, monkeypatch, "fused", D, B, 1.2)
    try:
        if with_vector:
            a.set_shapefactors(s6.mixed(D))
            ref.set_shapefactors(s6.mixed(D))
        v = s6.mixed(D)[::-1].copy()
        v[3] = bad
        with pytest.raises(pkg.MlggdError, match=r"mlggd error 1: .*\b3\b"):
            a.set_shapefactors(v)
        assert np.array_equal(a.shapefactors(), ref.shapefactors())
        assert a.train(x, t) == 1 and ref.train(x, t) == 1
        same(snapshot(a), snapshot(ref))
    finally:
        a.close()
        ref.close()


def test_a_beta_norm_engine_refuses_a_vector(pkg, monkeypatch):
    D, B = 19, 32
    x, t = frames(D, B)
    a = engine(pkg, monkeypatch, "fused", D, B, 2.0, ml=0)
    ref = engine(pkg, monkeypatch, "fused", D, B, 2.0, ml=0)
    try:
        with pytest.raises(pkg.MlggdError, match="mlggd error 4: .*MLflag"):
            a.set_shapefactors(s6.mixed(D))
        a.set_shapefactors(None)                                                   # nothing to undo: accepted
        assert np.array_equal(a.shapefactors(), np.full(D, 2.0, np.float32))
        assert a.train(x, t) == 1 and ref.train(x, t) == 1
        same(snapshot(a), snapshot(ref))
    finally:
        a.close()
        ref.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. bystanders
def test_entry_points_that_do_not_know_the_vector(pkg, monkeypatch):
    """error_stats (its own grid), forward and enhance_wave return the same bits with and without a vector set"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    D, ctx, B = 257, 3, 32
    ls = [D * ctx, 64, D]
    W, b = b6.make_net(ls, 7)
    x, t = b6.make_data(ls, 2 * B + 5, 8)
    rng = np.random.default_rng(9)
    mean = rng.normal(5, 1, D).astype(np.float32)
    inv = (1.0 / rng.uniform(1, 3, D)).astype(np.float32)
    wave = spec64.synth_speech(16000, 16, seed=10)
    grid = np.float32([0.5, 1.0, 1.3, 2.0])
    eng = pkg.BPGpu(1, 0, ls, B, *HP, W, b, 1.2, 1)
    try:
        def calls():
            return [eng.error_stats(x, t, grid).view(np.uint64), bits(eng.forward(x)),
                    eng.enhance_wave(wave, mean, inv, fea_context=ctx), bits(eng.enhance_wave(wave, mean, inv, fea_context=ctx,
                                                                                                return_float=True)[1])]
        before = calls()
        eng.set_shapefactors(s6.mixed(D))
        during = calls()
        eng.set_shapefactors(None)
        after = calls()
    finally:
        eng.close()
    for p, q, r in zip(before, during, after):
        assert np.array_equal(p, q) and np.array_equal(p, r)
