"""GPU: the learned GGD scale, alpha_d as a state moved by SGD beside the weights (BPGpu.set_scale_mode), through every
loss path.

The rule (csrc/scale_rule.h) has two identities that need no tolerance -- a fresh engine's first step seeds alpha with
the alternating engine's bits; lrate = momentum = 0 keeps a given alpha bit for bit -- and a float32 model
(tests/scale_model.py) that the one-device paths equal bit for bit, and every path where the column sums are exact.  The
data-parallel paths sum the columns in another order: there (alpha, v) lie within the float64 bounds of scale_model.py.

Shapes as in tests/test_gpu_asymmetry.py: 40-64-D with D = 19 (Dp 32: a partly filled group of 8 units and an empty
one) and D = 257 (a last group with one live unit); B = 32 and B = 160 (the fused kernel's 128-frame loop runs a second,
partial pass); fused, MLGGD_LOSS_FUSE=0, fake_world(2) and fake_world(2, allreduce=True)."""
import math

import numpy as np
import pytest

import asym64 as a6
import bounds64 as b6
import scale_model as sm
import shapes64 as s6

pytestmark = pytest.mark.gpu

F = np.float32
HP = (0.1, 0.9, 1e-5)
KNOBS = ("MLGGD_TILE64", "MLGGD_S_OUT", "MLGGD_LOSS_FUSE", "MLGGD_DW_MERGE", "MLGGD_STAGE_AHEAD", "MLGGD_CV_DEVICE",
         "MLGGD_DW_TILE", "MLGGD_DW_PERSIST", "MLGGD_DWP_PER_CU", "MLGGD_TILE_MAP")
SHAPES = [(19, 32), (19, 160), (257, 32), (257, 160)]
SINGLE = [(m, D, B) for m in ("fused", "unfused") for D, B in SHAPES]
WORLDS = [("gather", D, 32) for D in (19, 257)] + [("allreduce", D, B) for D, B in SHAPES]
ETA, MU, VMAX = 0.05, 0.5, 1.0
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


def world(mode):
    return mode in ("gather", "allreduce")


def rows_per_step(mode, B):
    return 2 * B if world(mode) else B


def engine(pkg, monkeypatch, mode, D, B, beta, ml=1, hp=HP, W=None, b=None):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if mode == "unfused":
        monkeypatch.setenv("MLGGD_LOSS_FUSE", "0")
    if W is None:
        W, b = net(D)
    eng = pkg.BPGpu(1, 0, ls_of(D), B, *hp, W, b, beta, ml)
    if mode == "gather":
        eng.fake_world(2)                     # the factor all-gather: CS_ACCUMULATE, then CS_GIVEN on every rank
    elif mode == "allreduce":
        eng.fake_world(2, allreduce=True)     # the gradient all-reduce
    return eng


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


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


def vectors(eng, D, beta, skew):
    """the error model of a case on an engine: a shape vector for "mixed", a skew vector on request; returns (betas, kappas)"""
    betas = s6.mixed(D) if beta == "mixed" else np.full(D, beta, F)
    kaps = a6.kappas(D) if skew else np.ones(D, F)
    if beta == "mixed":
        eng.set_shapefactors(betas)
    if skew:
        eng.set_asymmetry(kaps)
    return betas, kaps


# ---------------------------------------------------------------------------------------------------------------------
# 1. seed: step 1 of a learned engine is step 1 of the plain engine, bit for bit
@pytest.mark.parametrize("beta", [0.9, 1.0, 2.0, "mixed"])
@pytest.mark.parametrize("mode,D,B", SINGLE + WORLDS)
def test_the_first_step_seeds_with_the_alternating_engines_bits(pkg, monkeypatch, mode, D, B, beta):
    x, t = frames(D, rows_per_step(mode, B))
    for skew in (False, True):
        lrn = engine(pkg, monkeypatch, mode, D, B, 1.4 if beta == "mixed" else beta)
        ref = engine(pkg, monkeypatch, mode, D, B, 1.4 if beta == "mixed" else beta)
        try:
            vectors(lrn, D, beta, skew)
            vectors(ref, D, beta, skew)
            lrn.set_scale_mode("learned", lrate=ETA, momentum=MU, vmax=VMAX)
            assert lrn.scale_mode()[:4] == ("learned", F(ETA), MU, VMAX) and lrn.scale_mode().steps == 0
            assert ref.scale_mode().mode == "alternating"
            a0, v0 = lrn.scale_state()
            assert not a0.any() and not v0.any()                                   # a fresh engine: every bin seeds
            assert lrn.train(x, t) == 1 and ref.train(x, t) == 1
            same(snapshot(lrn), snapshot(ref))
            a1, v1 = lrn.scale_state()
            assert np.array_equal(bits(a1), bits(ref.scalefactor())) and not v1.any() and (a1 > 0).all()
            assert lrn.scale_mode().steps == 1
        finally:
            lrn.close()
            ref.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. frozen: lrate = momentum = 0 trains under a given scale vector
@pytest.mark.parametrize("mode,D,B", SINGLE + WORLDS)
def test_frozen_keeps_the_given_scale_and_its_gradient_is_float64s(pkg, monkeypatch, mode, D, B):
    rows = rows_per_step(mode, B)
    x, t = frames(D, 5 * rows, seed=1)
    X = np.random.default_rng(D + B).uniform(0.3, 3.0, D).astype(F)
    eng = engine(pkg, monkeypatch, mode, D, B, 1.7)
    try:
        betas, kaps = vectors(eng, D, "mixed", True)
        eng.set_scale_mode("learned", lrate=0.0, momentum=0.0, vmax=VMAX)
        eng.set_scale_state(X, np.full(D, 0.3, F))                                 # a velocity to forget: mu = 0
        assert np.array_equal(bits(eng.scalefactor()), bits(X))
        assert eng.train(x, t) == 5
        a, v = eng.scale_state()
        assert np.array_equal(bits(a), bits(X)) and np.array_equal(bits(eng.scalefactor()), bits(X))
        assert (v == 0).all()
        assert eng.scale_mode().steps == 5
        out, dedx = eng.debug_tensor("out"), eng.debug_tensor("dedx", 2)           # of the last (emulated) rank
        tl = t[5 * rows - B:5 * rows]
    finally:
        eng.close()
    bad = []
    for bv, kv, cols in a6.pairs(betas, kaps):
        r = b6.compare("dE/dz beta_d %g kappa_d %g" % (bv, kv), dedx[:, cols],
                       sm.expect_grad_fixed(out[:, cols], tl[:, cols], bv, kv, X[cols], n=rows))
        print(r.line())
        bad += [r.line()] if not r.ok else []
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the rule, bit for bit, on one device
@pytest.mark.parametrize("mode,D,B", SINGLE)
def test_every_step_is_the_float32_model(pkg, monkeypatch, pyoracle, mode, D, B):
    steps = 5
    x, t = frames(D, steps * B, seed=2)
    eng = engine(pkg, monkeypatch, mode, D, B, 1.7)
    try:
        betas, kaps = vectors(eng, D, "mixed", True)
        eng.set_scale_mode("learned", lrate=ETA, momentum=MU, vmax=VMAX)
        a, v = eng.scale_state()
        for k in range(steps):
            tb = t[k * B:(k + 1) * B]
            assert eng.train(x[k * B:(k + 1) * B], tb) == 1
            want_a, want_v, _ = sm.step(a, v, sm.colsum(eng.debug_tensor("out"), tb, betas, kaps), B, betas, ETA, MU, VMAX)
            a, v = eng.scale_state()
            assert np.array_equal(bits(a), bits(want_a)), "alpha after step %d: %d bins differ" % (k + 1, (bits(a) != bits(want_a)).sum())
            assert np.array_equal(bits(v), bits(want_v)), "v after step %d" % (k + 1)
            assert np.array_equal(bits(eng.scalefactor()), bits(a))
        assert v.any() and eng.scale_mode().steps == steps
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. all paths agree, bit for bit, where the sums are exact
def exact_case(D, rows, seed):
    """targets that are multiples of 1/64 in [-4, 4] and a net whose output is 0 whatever the input: with beta = 1 every
    p = |t| and every column sum of at most 2^11 of them is exact in any order"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, 40)).astype(F)
    t = (rng.integers(-256, 257, (rows, D)) / 64.0).astype(F)
    W, b = net(D)
    return x, t, [W[0], np.zeros_like(W[1])], [b[0], np.zeros_like(b[1])]


def exact_sequence(pkg, monkeypatch, mode, D, B, x, t, W, b, steps):
    eng = engine(pkg, monkeypatch, mode, D, B, 1.0, hp=(0.0, 0.0, 0.0), W=W, b=b)
    seq = []
    try:
        eng.set_scale_mode("learned", lrate=ETA, momentum=MU, vmax=VMAX)
        rows = rows_per_step(mode, B)
        for k in range(steps):
            assert eng.train(x[k * rows:(k + 1) * rows], t[k * rows:(k + 1) * rows]) == 1
            assert not eng.debug_tensor("out").any()
            a, v = eng.scale_state()
            assert np.array_equal(bits(eng.scalefactor()), bits(a))
            seq.append((bits(a), bits(v)))
        assert eng.scale_mode().steps == steps                                     # one flip per step, not per launch
    finally:
        eng.close()
    return seq


@pytest.mark.parametrize("D,B", [(19, 32), (257, 32), (19, 160), (257, 160)])
def test_all_paths_give_one_sequence_where_the_sums_are_exact(pkg, monkeypatch, pyoracle, D, B):
    steps = 6
    x, t, W, b = exact_case(D, steps * 2 * B, D + B)
    betas = np.ones(D, F)
    a, v = np.zeros(D, F), np.zeros(D, F)
    model = []
    for k in range(steps):
        tb = t[k * 2 * B:(k + 1) * 2 * B]
        s = np.abs(tb).sum(axis=0, dtype=np.float64)
        assert np.array_equal(s.astype(F).astype(np.float64), s)                   # exact: the order cannot matter
        a, v, _ = sm.step(a, v, s.astype(F), 2 * B, betas, ETA, MU, VMAX)
        model.append((bits(a), bits(v)))
    assert len(set(m[0].tobytes() for m in model)) == steps and model[-1][1].any()  # the state moves at every step
    paths = [("fused", 2 * B), ("unfused", 2 * B), ("allreduce", B)] + ([("gather", B)] if B == 32 else [])
    for mode, bunch in paths:
        seq = exact_sequence(pkg, monkeypatch, mode, D, bunch, x, t, W, b, steps)
        for k, ((ga, gv), (wa, wv)) in enumerate(zip(seq, model)):
            assert np.array_equal(ga, wa), "%s: alpha after step %d, %d bins differ" % (mode, k + 1, (ga != wa).sum())
            assert np.array_equal(gv, wv), "%s: v after step %d, %d bins differ" % (mode, k + 1, (gv != wv).sum())


# ---------------------------------------------------------------------------------------------------------------------
# 5. general beta on the unfused and world paths, against float64
@pytest.mark.parametrize("mode,D,B", [c for c in SINGLE if c[0] == "unfused"] + WORLDS)
def test_the_state_lies_within_the_float64_bounds(pkg, monkeypatch, mode, D, B):
    steps, rows = 4, rows_per_step(mode, B)
    x, t = frames(D, steps * rows, seed=3)
    eng = engine(pkg, monkeypatch, mode, D, B, 1.7)
    bad = []
    try:
        betas, kaps = vectors(eng, D, "mixed", True)
        if world(mode):
            eng.keep_ranks(True)
        eng.set_scale_mode("learned", lrate=ETA, momentum=MU, vmax=VMAX)
        start = np.zeros(D, F)
        start[1::2] = np.random.default_rng(D).uniform(0.5, 2.0, D).astype(F)[1::2]    # every other bin seeds
        eng.set_scale_state(start)
        a, v = eng.scale_state()
        for k in range(steps):
            tb = t[k * rows:(k + 1) * rows]
            assert eng.train(x[k * rows:(k + 1) * rows], tb) == 1
            out = np.vstack([eng.rank_tensor("out", 0, r) for r in range(2)]) if world(mode) else eng.debug_tensor("out")
            an, vn = eng.scale_state()
            for bv, kv, cols in a6.pairs(betas, kaps):
                ea, ev = sm.expect_step(a[cols], v[cols], out[:, cols], tb[:, cols], bv, kv, ETA, MU, VMAX)
                for r in (b6.compare("alpha' beta_d %g kappa_d %g" % (bv, kv), an[cols], ea),
                          b6.compare("v' beta_d %g kappa_d %g" % (bv, kv), vn[cols], ev)):
                    print("step %d %s" % (k + 1, r.line()))
                    bad += ["step %d %s" % (k + 1, r.line())] if not r.ok else []
            a, v = an, vn
        assert v.any()
    finally:
        eng.close()
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# 6. column independence
@pytest.mark.parametrize("mode,D,B", SINGLE + WORLDS)
def test_columns_are_independent(pkg, monkeypatch, mode, D, B):
    steps = 3
    x, t = frames(D, steps * rows_per_step(mode, B), seed=4)
    betas, kaps = s6.mixed(D), a6.kappas(D)

    def run(beta, kappa_vec, shape_vec):
        e = engine(pkg, monkeypatch, mode, D, B, beta, hp=(0.0, 0.0, 0.0))         # the net stands still: the forward
        try:                                                                       # pass is the same on every engine
            if shape_vec is not None:
                e.set_shapefactors(shape_vec)
            e.set_asymmetry(kappa_vec)
            e.set_scale_mode("learned", lrate=ETA, momentum=MU, vmax=VMAX)
            assert e.train(x, t) == steps
            a, v = e.scale_state()
            return bits(a), bits(v), bits(e.debug_tensor("dedx", 2))
        finally:
            e.close()

    alpha, vel, dedx = run(1.7, kaps, betas)
    for bv, kv, cols in a6.pairs(betas, kaps):
        a1, v1, d1 = run(bv, np.full(D, kv, F), None)                              # the shape through cfg.shapefactor
        assert np.array_equal(alpha[cols], a1[cols]), "alpha, columns of (%g, %g)" % (bv, kv)
        assert np.array_equal(vel[cols], v1[cols]), "v, columns of (%g, %g)" % (bv, kv)
        assert np.array_equal(dedx[:, cols], d1[:, cols]), "dedx, columns of (%g, %g)" % (bv, kv)
        assert not np.array_equal(alpha[~cols], a1[~cols])                         # ... and the others are not its


# ---------------------------------------------------------------------------------------------------------------------
# 7. convergence on the device
@pytest.mark.parametrize("start", [3.0, 1.0 / 3.0], ids=["from_3x", "from_a_third"])
@pytest.mark.parametrize("D,B", [(19, 32), (257, 160)])
def test_a_repeated_minibatch_converges_to_the_closed_form(pkg, monkeypatch, pyoracle, D, B, start):
    eta, steps = 0.25, 200
    x, t = frames(D, B, seed=5)
    eng = engine(pkg, monkeypatch, "fused", D, B, 1.7, hp=(0.0, 0.0, 0.0))
    try:
        betas, kaps = vectors(eng, D, "mixed", True)
        eng.set_scale_mode("learned", lrate=eta, momentum=0.0, vmax=VMAX)
        assert eng.train(x, t) == 1                                                # seeds: the fp32 closed form
        s = sm.colsum(eng.debug_tensor("out"), t, betas, kaps)
        star = sm.beta_s32(s, B, betas).astype(np.float64) ** (1.0 / betas.astype(np.float64))
        closed = eng.scale_state()[0]
        eng.set_scale_state((closed * F(start)).astype(F))
        assert eng.train(np.tile(x, (steps, 1)), np.tile(t, (steps, 1))) == steps
        a, _ = eng.scale_state()
    finally:
        eng.close()
    dist = np.abs(np.log(a.astype(np.float64)) - np.log(star))
    for bv in np.unique(betas):
        c = betas == bv
        R = sm.stall(eta, float(bv))
        assert sm.steps_to_stall(math.log(start) * (1.0 + 1e-5), eta, float(bv), VMAX) <= steps   # fp32 closed form vs alpha*
        print("beta %g: worst |ln alpha - ln alpha*| %.3g, stall distance %.3g" % (bv, dist[c].max(), R))
        assert (dist[c] <= R).all(), (float(bv), dist[c].max(), R)


# ---------------------------------------------------------------------------------------------------------------------
# 8. CV reads the learned alpha
@pytest.mark.parametrize("device_reduce", [False, True], ids=["host_order", "device_reduce"])
@pytest.mark.parametrize("D,B", SHAPES)
def test_cv_loglik_is_evaluated_at_the_learned_scale(pkg, monkeypatch, D, B, device_reduce):
    x, t = frames(D, 3 * B, seed=6)
    cx, ct = frames(D, B + 7, seed=7)
    eng = engine(pkg, monkeypatch, "fused", D, B, 1.3)
    try:
        betas, kaps = vectors(eng, D, "mixed", True)
        eng.set_scale_mode("learned", lrate=0.25, momentum=MU, vmax=VMAX)
        assert eng.train(x, t) == 3
        alpha = eng.scale_state()[0]
        eng.set_cv_device_reduce(device_reduce)
        ll = eng.cv_all(cx, ct)[2]
        ex = a6.expect_cv(eng.forward(cx), ct, betas, kaps, alpha, pkg.gamma)
        eng.set_scale_state((alpha * F(1.5)).astype(F))
        ll2 = eng.cv_all(cx, ct)[2]
    finally:
        eng.close()
    r = b6.compare("loglik", np.array(ll), ex["loglik"])
    print(r.line())
    assert r.ok, r.line()
    assert ll2 != ll                                        # the state is what the number was formed with


# ---------------------------------------------------------------------------------------------------------------------
# 9. switching
@pytest.mark.parametrize("mode", ["fused", "unfused", "allreduce"])
def test_back_to_alternating_gives_the_plain_engines_scale(pkg, monkeypatch, mode):
    D, B = 19, 160
    rows = rows_per_step(mode, B)
    x, t = frames(D, 3 * rows, seed=8)
    lrn = engine(pkg, monkeypatch, mode, D, B, 1.2, hp=(0.0, 0.0, 0.0))            # the net stands still, so the third
    ref = engine(pkg, monkeypatch, mode, D, B, 1.2, hp=(0.0, 0.0, 0.0))            # minibatch's closed form is one value
    try:
        lrn.set_scale_mode("learned", lrate=0.25, momentum=MU, vmax=VMAX)
        assert lrn.train(x[:2 * rows], t[:2 * rows]) == 2
        learned = lrn.scalefactor()
        lrn.set_scale_mode("alternating")
        assert lrn.scale_mode().mode == "alternating"
        assert np.array_equal(bits(lrn.scalefactor()), bits(learned))              # the switch itself leaves it
        with pytest.raises(pkg.MlggdError, match="mlggd error 4: .*not learned"):
            lrn.scale_state()
        assert ref.train(x[:2 * rows], t[:2 * rows]) == 2
        assert not np.array_equal(bits(ref.scalefactor()), bits(learned))
        assert lrn.train(x[2 * rows:], t[2 * rows:]) == 1 and ref.train(x[2 * rows:], t[2 * rows:]) == 1
        assert np.array_equal(bits(lrn.scalefactor()), bits(ref.scalefactor()))
        # ... and entering again takes alpha from the scalefactor of that step, v = 0
        lrn.set_scale_mode("learned")
        a, v = lrn.scale_state()
        assert np.array_equal(bits(a), bits(ref.scalefactor())) and not v.any()
        assert lrn.scale_mode() == ("learned", F(0.05), 0.5, 1.0, 0)               # the defaults
    finally:
        lrn.close()
        ref.close()


@pytest.mark.parametrize("mode", ["fused", "unfused"])
def test_on_and_off_before_the_first_step_leave_a_plain_run(pkg, monkeypatch, mode):
    D, B = 257, 160
    x, t = frames(D, 3 * B)
    a = engine(pkg, monkeypatch, mode, D, B, 1.2)
    ref = engine(pkg, monkeypatch, mode, D, B, 1.2)
    try:
        a.set_scale_mode("learned", lrate=0.3, momentum=0.2, vmax=2.0)
        a.set_scale_mode("alternating")
        assert a.train(x, t) == 3 and ref.train(x, t) == 3
        same(snapshot(a), snapshot(ref))
    finally:
        a.close()
        ref.close()


def test_set_scalefactor_in_learned_mode_sets_alpha_and_leaves_v(pkg, monkeypatch, pyoracle):
    D, B = 19, 32
    x, t = frames(D, 3 * B, seed=9)
    eng = engine(pkg, monkeypatch, "fused", D, B, 1.2)
    try:
        eng.set_scale_mode("learned", lrate=ETA, momentum=MU, vmax=VMAX)
        assert eng.train(x[:2 * B], t[:2 * B]) == 2
        _, v = eng.scale_state()
        assert v.any()
        X = np.linspace(0.5, 2.0, D).astype(F)
        eng.set_scalefactor(X)
        a2, v2 = eng.scale_state()
        assert np.array_equal(bits(a2), bits(X)) and np.array_equal(bits(v2), bits(v))
        tb = t[2 * B:]
        assert eng.train(x[2 * B:], tb) == 1
        betas = np.full(D, 1.2, F)
        want_a, want_v, _ = sm.step(X, v, sm.colsum(eng.debug_tensor("out"), tb, betas), B, betas, ETA, MU, VMAX)
        a3, v3 = eng.scale_state()
        assert np.array_equal(bits(a3), bits(want_a)) and np.array_equal(bits(v3), bits(want_v))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 10. refusals
NAN, INF = float("nan"), float("inf")
BAD_MODES = [dict(lrate=NAN), dict(lrate=INF), dict(lrate=-0.01), dict(momentum=NAN), dict(momentum=-0.1), dict(momentum=1.0),
             dict(momentum=INF), dict(vmax=NAN), dict(vmax=INF), dict(vmax=0.0), dict(vmax=-1.0)]


@pytest.mark.parametrize("learned_before", [False, True])
def test_bad_parameters_are_refused_and_change_nothing(pkg, monkeypatch, learned_before):
    D, B = 19, 32
    x, t = frames(D, 2 * B)
    a = engine(pkg, monkeypatch, "fused", D, B, 1.2)
    ref = engine(pkg, monkeypatch, "fused", D, B, 1.2)
    try:
        if learned_before:
            a.set_scale_mode("learned", lrate=0.1, momentum=0.3, vmax=0.7)
            ref.set_scale_mode("learned", lrate=0.1, momentum=0.3, vmax=0.7)
        assert a.train(x[:B], t[:B]) == 1 and ref.train(x[:B], t[:B]) == 1
        for kw in BAD_MODES:
            args = dict(lrate=ETA, momentum=MU, vmax=VMAX)
            args.update(kw)
            with pytest.raises(pkg.MlggdError, match="mlggd error 1: scale lrate"):
                a.set_scale_mode("learned", **args)
        with pytest.raises(pkg.MlggdError, match="mlggd error 1: scale mode 2"):
            pkg._check(pkg.load().mlggd_set_scale_mode(a._h, 2, 0.05, 0.5, 1.0))
        with pytest.raises(ValueError):
            a.set_scale_mode("both")
        assert a.scale_mode() == ref.scale_mode()
        if learned_before:
            for bad in (-1.0, NAN, INF, -INF):
                v = np.ones(D, F)
                v[3] = bad
                with pytest.raises(pkg.MlggdError, match=r"mlggd error 1: alpha\[3\]"):
                    a.set_scale_state(v)
                with pytest.raises(pkg.MlggdError, match=r"mlggd error 1: alpha\[3\]"):
                    a.set_scalefactor(v)
                if bad != -1.0:
                    with pytest.raises(pkg.MlggdError, match=r"mlggd error 1: velocity\[3\]"):
                        a.set_scale_state(np.ones(D, F), v)
            for got, want in zip(a.scale_state(), ref.scale_state()):
                assert np.array_equal(bits(got), bits(want))
        else:
            with pytest.raises(pkg.MlggdError, match="mlggd error 4: .*not learned"):
                a.set_scale_state(np.ones(D, F))
        assert a.train(x[B:], t[B:]) == 1 and ref.train(x[B:], t[B:]) == 1
        same(snapshot(a), snapshot(ref))
    finally:
        a.close()
        ref.close()


def test_a_beta_norm_engine_refuses_the_mode(pkg, monkeypatch):
    D, B = 19, 32
    x, t = frames(D, B)
    a = engine(pkg, monkeypatch, "fused", D, B, 2.0, ml=0)
    ref = engine(pkg, monkeypatch, "fused", D, B, 2.0, ml=0)
    try:
        with pytest.raises(pkg.MlggdError, match="mlggd error 4: .*MLflag"):
            a.set_scale_mode("learned")
        assert a.scale_mode().mode == "alternating"
        assert a.train(x, t) == 1 and ref.train(x, t) == 1
        same(snapshot(a), snapshot(ref))
    finally:
        a.close()
        ref.close()
