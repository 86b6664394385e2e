"""GPU: the asymmetric GGD error model, a skew per output bin (BPGpu.set_asymmetry), through every loss path.

The rule (csrc/asym_rule.h) charges e = out - targ through s(e) = kappa e (e > 0), -e / kappa (e < 0) in the place of
|e|, with x * 1.0f and x / 1.0f exact, which gives three checks that need no tolerance:
  1. a vector of ones leaves the bits of the engine without a vector -- weights, momentum, scalefactor, CV sums;
  2. under mixed vectors the columns of one (beta, kappa) pair carry the bits of an engine with that pair everywhere;
  3. for kappa a power of two, kappa e and e / (1 / kappa) are the same float: the engine with 1 / kappa, the negated
     last layer and negated targets is the exact mirror image, step after step.
The float64 checks (4) are those of tests/test_gpu_shapefactors.py with the loss bound applied per group of columns
of equal (beta, kappa) and extended by the rule's two roundings (tests/asym64.py).

Shapes as in tests/test_gpu_shapefactors.py: 40-64-D with D = 19 (Dp 32: a partly filled group of 8 units and an empty
one) and D = 257 (a last group with one live unit); B = 32 and B = 160 (the fused kernel's 128-frame loop runs a second,
partial pass); fused, MLGGD_LOSS_FUSE=0, fake_world(2) and fake_world(2, allreduce=True)."""
import numpy as np
import pytest

import asym64 as a6
import bounds64 as b6
import shapes64 as s6

pytestmark = pytest.mark.gpu

HP = (0.1, 0.9, 1e-5)
KNOBS = ("MLGGD_TILE64", "MLGGD_S_OUT", "MLGGD_LOSS_FUSE", "MLGGD_DW_MERGE", "MLGGD_STAGE_AHEAD", "MLGGD_CV_DEVICE",
         "MLGGD_DW_TILE", "MLGGD_DW_PERSIST", "MLGGD_DWP_PER_CU", "MLGGD_TILE_MAP")
SHAPES = [(19, 32), (19, 160), (257, 32), (257, 160)]
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
        x, t = b6.make_data(ls_of(D), n, 300 + D + seed)
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


def cv_bits(eng, cx, ct):
    """the three CV sums under the host-order and the device reduce, as bits"""
    got = []
    for dev in (False, True):
        eng.set_cv_device_reduce(dev)
        got.append(bits(np.float32(eng.cv_all(cx, ct))).tolist())
    eng.set_cv_device_reduce(False)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# 1. kappa = 1 everywhere is the engine without a vector, bit for bit
@pytest.mark.parametrize("beta", [0.9, 1.0, 2.0, "mixed"])
@pytest.mark.parametrize("mode,D,B", SINGLE + WORLDS)
def test_ones_equal_the_engine_without_a_vector(pkg, monkeypatch, mode, D, B, beta):
    x, t = frames(D, 6 * rows_per_step(mode, B))
    shapes = s6.mixed(D) if beta == "mixed" else np.full(D, beta, np.float32)
    asy = engine(pkg, monkeypatch, mode, D, B, 1.7)        # its own shapefactor is NOT the vector's: the vector counts
    ref = engine(pkg, monkeypatch, mode, D, B, 1.4 if beta == "mixed" else beta)
    try:
        asy.set_shapefactors(shapes)
        asy.set_asymmetry(np.ones(D, np.float32))
        if beta == "mixed":
            ref.set_shapefactors(shapes)
        assert np.array_equal(asy.asymmetry(), np.ones(D, np.float32))
        assert asy.train(x, t) == 6 and ref.train(x, t) == 6
        same(snapshot(asy), snapshot(ref))
        if mode in ("fused", "unfused"):
            cx, ct = frames(D, B + 7, seed=4)
            assert cv_bits(asy, cx, ct) == cv_bits(ref, cx, ct)
    finally:
        asy.close()
        ref.close()


@pytest.mark.parametrize("mode", ["fused", "unfused", "allreduce"])
@pytest.mark.parametrize("order", ["kappa_first", "beta_first", "kappa_only"])
def test_ones_without_a_shape_vector_and_in_either_order(pkg, monkeypatch, mode, order):
    """an engine without a shape vector reads cfg.shapefactor through the kernels' beta array; set_asymmetry and
    set_shapefactors compose in either order"""
    D, B, beta = 19, 160, 1.2
    x, t = frames(D, 3 * rows_per_step(mode, B))
    asy = engine(pkg, monkeypatch, mode, D, B, beta)
    ref = engine(pkg, monkeypatch, mode, D, B, beta)
    try:
        if order == "kappa_first":
            asy.set_asymmetry(np.ones(D, np.float32))
            asy.set_shapefactors(s6.mixed(D))
        elif order == "beta_first":
            asy.set_shapefactors(s6.mixed(D))
            asy.set_asymmetry(np.ones(D, np.float32))
        else:
            asy.set_asymmetry(np.ones(D, np.float32))
        if order != "kappa_only":
            ref.set_shapefactors(s6.mixed(D))
            assert np.array_equal(asy.shapefactors(), s6.mixed(D))                 # the shape vector is left alone
        assert asy.train(x, t) == 3 and ref.train(x, t) == 3
        same(snapshot(asy), snapshot(ref))
    finally:
        asy.close()
        ref.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. under mixed vectors the columns of one (beta, kappa) pair are an engine's with that pair everywhere, bit for bit
@pytest.mark.parametrize("mode,D,B", SINGLE + WORLDS)
def test_columns_are_independent(pkg, monkeypatch, mode, D, B):
    x, t = frames(D, rows_per_step(mode, B), seed=1)
    betas, kaps = s6.mixed(D), a6.kappas(D)
    vec = engine(pkg, monkeypatch, mode, D, B, 1.7)
    try:
        vec.set_shapefactors(betas)
        vec.set_asymmetry(kaps)
        assert np.array_equal(vec.asymmetry(), kaps)
        assert vec.train(x, t) == 1
        out, dedx, alpha = bits(vec.debug_tensor("out")), bits(vec.debug_tensor("dedx", 2)), bits(vec.scalefactor())
    finally:
        vec.close()
    groups = a6.pairs(betas, kaps)
    assert len(groups) == len(a6.KCYCLE)
    for bv, kv, cols in groups:
        one = engine(pkg, monkeypatch, mode, D, B, bv)     # the shape through cfg.shapefactor, the skew uniform
        try:
            one.set_asymmetry(np.full(D, kv, np.float32))
            assert one.train(x, t) == 1
            assert np.array_equal(out, bits(one.debug_tensor("out"))), (bv, kv)     # the forward pass knows neither
            got = bits(one.debug_tensor("dedx", 2))
            assert np.array_equal(dedx[:, cols], got[:, cols]), "dedx, columns of (%g, %g)" % (bv, kv)
            assert np.array_equal(alpha[cols], bits(one.scalefactor())[cols]), "scalefactor, columns of (%g, %g)" % (bv, kv)
            other = ~cols
            assert not np.array_equal(dedx[:, other], got[:, other])               # ... and the others are not its
        finally:
            one.close()
        if kv == 1.0:                                      # ... and the kappa = 1 columns those of no kappa vector at all
            plain = engine(pkg, monkeypatch, mode, D, B, bv)
            try:
                assert plain.train(x, t) == 1
                got = bits(plain.debug_tensor("dedx", 2))
                assert np.array_equal(dedx[:, cols], got[:, cols]) and np.array_equal(alpha[cols], bits(plain.scalefactor())[cols])
            finally:
                plain.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the mirror identity
@pytest.mark.parametrize("kappa", [2.0, 0.5, "mixed"])
@pytest.mark.parametrize("mode,D,B", SINGLE + WORLDS)
def test_mirror_identity(pkg, monkeypatch, mode, D, B, kappa):
    """Engine A under kappa; engine B under 1 / kappa with the last layer's W and b and the targets negated: every
    error of B is the negation of A's, s is the same float (kappa a power of two), so after 6 steps with momentum B's
    last layer is the exact negation of A's and everything else is A's, bit for bit.  A few targets of the first step
    are set to the outputs themselves (single-device modes): exact-zero errors, which take the third branch."""
    L, rows = 3, rows_per_step(mode, B)
    x, t = frames(D, 6 * rows, seed=5)
    kaps = a6.pow2(D) if kappa == "mixed" else np.full(D, kappa, np.float32)
    betas = s6.mixed(D)
    W, b = net(D)
    Wn, bn = [W[0], -W[1]], [b[0], -b[1]]
    planted = []
    if mode in ("fused", "unfused"):
        probe = engine(pkg, monkeypatch, mode, D, B, 1.2)
        try:
            assert probe.train(x[:B], t[:B]) == 1
            out = probe.debug_tensor("out")
        finally:
            probe.close()
        t = t.copy()
        planted = [(0, 0), (1, D - 1), (B - 1, 3), (B // 2, D // 2)]
        for r, c in planted:
            t[r, c] = out[r, c]
    A = engine(pkg, monkeypatch, mode, D, B, 1.7)
    Bm = engine(pkg, monkeypatch, mode, D, B, 1.7, W=Wn, b=bn)
    try:
        for e, k in ((A, kaps), (Bm, (1.0 / kaps).astype(np.float32))):
            e.set_shapefactors(betas)
            e.set_asymmetry(k)
        tn = -t
        assert A.train(x[:rows], t[:rows]) == 1 and Bm.train(x[:rows], tn[:rows]) == 1
        da, db = A.debug_tensor("dedx", L - 1), Bm.debug_tensor("dedx", L - 1)
        assert np.array_equal(da, -db)                     # as numbers: a planted zero is +0 on both sides
        for r, c in planted:
            assert da[r, c] == 0.0 and db[r, c] == 0.0, (r, c)
        assert A.train(x[rows:], t[rows:]) == 5 and Bm.train(x[rows:], tn[rows:]) == 5
        sa, sb = snapshot(A), snapshot(Bm)
        for name, xs, ys in zip(("weights", "bias", "delta_w", "delta_b"), sa[:4], sb[:4]):
            assert np.array_equal(xs[0], ys[0]), "%s of layer 1" % name
            pa, pb = xs[1].view(np.float32), ys[1].view(np.float32)
            assert np.isfinite(pa).all() and np.array_equal(pa, -pb), \
                "%s of the last layer: %d are not the negation" % (name, int((pa != -pb).sum()))
        assert np.array_equal(sa[4], sb[4]), "scalefactor"
    finally:
        A.close()
        Bm.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. against float64
def state(eng, L=3):
    W, b = eng.returnWeights()
    return W, b, [eng.debug_tensor("delta_w", l) for l in range(1, L)], [eng.debug_tensor("delta_b", l) for l in range(1, L)]


@pytest.mark.parametrize("mode,D,B", SINGLE)
def test_mixed_vectors_against_float64(pkg, monkeypatch, mode, D, B):
    """4 steps, every operation against its own fp32 inputs; asym64.expect_loss per group of columns of equal
    (beta, kappa), bounds64.expect_loss's derivation plus the rule's two roundings, no measured tolerance"""
    L = 3
    x, t = frames(D, 4 * B, seed=2)
    betas, kaps = s6.mixed(D), a6.kappas(D)
    eng = engine(pkg, monkeypatch, mode, D, B, 1.7)
    bad = []
    try:
        eng.set_shapefactors(betas)
        eng.set_asymmetry(kaps)
        for k in range(4):
            W, b, dW, db = state(eng)
            xb, tb = x[k * B:(k + 1) * B], t[k * B:(k + 1) * B]
            assert eng.train(xb, tb) == 1
            Wn, bn, dWn, dbn = state(eng)
            s = b6.Step(xb, tb, W, b, dW, db, {l: eng.debug_tensor("y", l) for l in range(1, L - 1)},
                        eng.debug_tensor("out"), {l: eng.debug_tensor("dedx", l) for l in range(1, L)}, dWn, dbn, Wn, bn,
                        HP[0], HP[1], HP[2], 1.7, 1, eng.out_slabs(), eng.scalefactor())
            reps = a6.check_step(s, betas, kaps)
            assert sum(r.name.startswith("loss ML beta_d") for r in reps) == len(a6.KCYCLE)
            for r in reps:
                print("step %d %s" % (k + 1, r.line()))
            bad += ["step %d %s" % (k + 1, r.line()) for r in reps if not r.ok]
    finally:
        eng.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape_vector", [True, False], ids=["beta_d", "shapefactor"])
@pytest.mark.parametrize("device_reduce", [False, True], ids=["host_order", "device_reduce"])
@pytest.mark.parametrize("D,B", SHAPES)
def test_cv_loglik_under_a_skew(pkg, monkeypatch, D, B, device_reduce, shape_vector):
    """The log-likelihood of cv_all on n = B + 7 frames (a whole bunch and a partial one) against the float64 formula
    with s(o - t) and the ln((kappa + 1/kappa) / 2) term, under asym64.expect_cv's bound; with a shape per bin and with
    the engine's one shapefactor (density1 is then an fp32 product the term is taken off in fp32)"""
    x, t = frames(D, 2 * B, seed=3)
    cx, ct = frames(D, B + 7, seed=4)
    betas = s6.mixed(D) if shape_vector else np.full(D, 1.3, np.float32)
    kaps = a6.kappas(D)
    eng = engine(pkg, monkeypatch, "fused", D, B, 1.3)
    try:
        if shape_vector:
            eng.set_shapefactors(betas)
        eng.set_asymmetry(kaps)
        assert eng.train(x, t) == 2
        eng.set_cv_device_reduce(device_reduce)
        sq, ab, ll = eng.cv_all(cx, ct)
        ex = a6.expect_cv(eng.forward(cx), ct, betas, kaps, eng.scalefactor(), pkg.gamma)
        eng.set_asymmetry(None)
        assert np.array_equal(eng.asymmetry(), np.ones(D, np.float32))
        sq0, ab0, ll0 = eng.cv_all(cx, ct)
    finally:
        eng.close()
    r = b6.compare("loglik", np.array(ll), ex["loglik"])
    print(r.line())
    assert r.ok, r.line()
    assert ll0 != ll                                        # the vector is what the number was formed with
    # the two sums that know no skew are bystanders: the bits of the same engine without the vector
    assert bits(np.float32([sq, ab])).tolist() == bits(np.float32([sq0, ab0])).tolist()


# ---------------------------------------------------------------------------------------------------------------------
# state and refusals
@pytest.mark.parametrize("mode", ["fused", "unfused"])
def test_set_and_reset_before_the_first_step_leave_a_plain_run(pkg, monkeypatch, mode):
    D, B = 257, 160
    x, t = frames(D, 3 * B)
    a = engine(pkg, monkeypatch, mode, D, B, 1.2)
    ref = engine(pkg, monkeypatch, mode, D, B, 1.2)
    try:
        assert np.array_equal(a.asymmetry(), np.ones(D, np.float32))
        a.set_asymmetry(a6.kappas(D))
        assert np.array_equal(a.asymmetry(), a6.kappas(D))                         # round trip
        assert np.array_equal(a.shapefactors(), np.full(D, 1.2, np.float32))       # the shapes are left alone
        a.set_asymmetry(None)
        assert np.array_equal(a.asymmetry(), np.ones(D, np.float32))
        assert a.train(x, t) == 3 and ref.train(x, t) == 3
        same(snapshot(a), snapshot(ref))
    finally:
        a.close()
        ref.close()


def test_a_skew_changes_the_step_and_leaves_the_state_alone(pkg, monkeypatch):
    D, B = 19, 32
    x, t = frames(D, 2 * B)
    a = engine(pkg, monkeypatch, "fused", D, B, 1.2)
    ref = engine(pkg, monkeypatch, "fused", D, B, 1.2)
    try:
        assert a.train(x[:B], t[:B]) == 1 and ref.train(x[:B], t[:B]) == 1
        before = snapshot(a)
        a.set_asymmetry(a6.kappas(D))
        same(snapshot(a), before)                          # weights, momentum, scalefactor: untouched by the call
        assert a.train(x[B:], t[B:]) == 1 and ref.train(x[B:], t[B:]) == 1
        assert not np.array_equal(snapshot(a)[0][1], snapshot(ref)[0][1])
    finally:
        a.close()
        ref.close()


@pytest.mark.parametrize("bad", [0.0, float("nan"), float("inf"), -1.0])
@pytest.mark.parametrize("with_vector", [False, True])
def test_a_bad_vector_is_refused_and_changes_nothing(pkg, monkeypatch, bad, with_vector):
    D, B = 19, 32
    x, t = frames(D, B)
    a = engine(pkg, monkeypatch, "fused", D, B, 1.2)
    ref = engine(pkg, monkeypatch, "fused", D, B, 1.2)
    try:
        if with_vector:
            a.set_asymmetry(a6.kappas(D))
            ref.set_asymmetry(a6.kappas(D))
        v = a6.kappas(D)[::-1].copy()
        v[3] = bad
        with pytest.raises(pkg.MlggdError, match=r"mlggd error 1: .*\b3\b"):
            a.set_asymmetry(v)
        assert np.array_equal(a.asymmetry(), ref.asymmetry())
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
            a.set_asymmetry(a6.kappas(D))
        a.set_asymmetry(None)                                                      # nothing to undo: accepted
        assert np.array_equal(a.asymmetry(), np.ones(D, np.float32))
        assert a.train(x, t) == 1 and ref.train(x, t) == 1
        same(snapshot(a), snapshot(ref))
    finally:
        a.close()
        ref.close()
