"""CPU: the oracle's two per-net switches -- rectified-linear hidden units (OracleNet(activation="relu")) and a shape factor
per output bin (OracleNet.set_shapefactors) -- pinned before any GPU run compares the engine with them bit for bit
(tests/test_gpu_twin_relu_bins.py).

* the ReLU oracle in the documented order against the independent float64 model relu64.step64, at
  test_oracle_matches_float64_model's shape and limits;
* the per-bin oracle: a uniform vector is the scalar oracle in every bit, under a mixed vector the columns of one value
  are a scalar oracle's at that value, and a step and the CV log-likelihood are inside the project's float64 bounds
  (shapes64.check_step_bins / expect_cv_bins: nothing new);
* the twin is another order and the rectifier another function (other bits);
* tests/golden/mfma_order_twin_relu_bins.npz (oracle/make_golden.py twin_relu_bins()) is reproduced bit for bit;
* every ReLU case of the GPU file, run here with the twin alone, is not degenerate."""
import os

import numpy as np
import pytest

import bounds64 as b6
import relu64 as r6
import shapes64 as s6
import twin_cases as tc
from test_oracle import CASES, HP, relmax

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F64_SEED = 3


# ---------------------------------------------------------------------------------------------------------------------
# 1. ReLU, documented order, against float64
@pytest.mark.parametrize("ml,beta", CASES)
def test_relu_oracle_matches_the_float64_model(pyoracle, ml, beta):
    """[15, 8, 8, 8, 5], B = 8, three chained steps of relu64.step64 beside OracleNet(activation="relu"): W to 2e-6, b
    and delta_w to 2e-5 of their maximum (test_oracle_matches_float64_model's limits).  A pre-activation whose sign
    differs between fp32 and float64 would break the comparison for a reason that is no bug, so the float64 run first
    shows that every hidden |z| exceeds its bound E_z = gamma_{K+2} (sum |y||w| + |b|) (relu64.expect_relu_layer)."""
    ls, B = [15, 8, 8, 8, 5], 8
    W0, b0 = b6.make_net(ls, F64_SEED)
    x, t = tc.data(ls, 3 * B, F64_SEED)
    o = pyoracle.OracleNet(ls, B, *HP, beta, ml, W0, b0, activation="relu")
    assert o.train(x, t) == 3
    W, b = W0, b0
    dW, db = [np.zeros_like(w) for w in W], [np.zeros_like(v) for v in b]
    for k in range(3):
        xb, tb = x[k * B:(k + 1) * B], t[k * B:(k + 1) * B]
        a = b6._d(xb)
        for l in range(1, len(ls) - 1):                                  # no sign of z is in doubt
            z = a @ b6._d(W[l - 1]) + b6._d(b[l - 1])
            Ez = b6.gamma(ls[l - 1] + 2) * (np.abs(a) @ np.abs(b6._d(W[l - 1])) + np.abs(b6._d(b[l - 1])))
            assert (np.abs(z) > Ez).all(), (k, l, float((np.abs(z) / Ez).min()))
            a = np.maximum(z, 0.0)
        m = r6.step64(xb, tb, W, b, dW, db, *HP, beta, ml)
        for l, y in m["y"].items():
            assert 0.0 < (y == 0).mean() < 1.0, (k, l)                   # both arms of the rule in every layer
        W, b, dW, db = m["W_new"], m["b_new"], m["dW_new"], m["db_new"]
    w, bb = o.get_weights()
    for l in range(4):
        assert relmax(w[l], W[l]) < 2e-6, l
        assert relmax(bb[l], b[l]) < 2e-5, l
        assert relmax(o.tensor("delta_w", l + 1), dW[l]) < 2e-5, l
    o.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. a shape factor per bin
BIN_LS, BIN_B = [40, 64, 19], 32


def bin_net(pyoracle, order, beta, betas=None, B=BIN_B, ls=BIN_LS, steps=1, **kw):
    """(net, x, t) after `steps` ML-GGD steps; order "ref", or "hip" with 3 slabs"""
    W, b = b6.make_net(ls, 100 + ls[-1])
    x, t = tc.data(ls, steps * B, 200 + ls[-1])
    pyoracle.set_gemm_order(order, 3)
    try:
        o = pyoracle.OracleNet(ls, B, *HP, beta, 1, W, b, shapefactors=betas, **kw)
        assert o.train(x, t) == steps
    finally:
        pyoracle.set_gemm_order("ref")
    return o, x, t


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def snapshot(o, L):
    w, b = o.get_weights()
    return ([bits(v) for v in w + b] + [bits(o.tensor(n, l)) for l in range(1, L) for n in ("delta_w", "delta_b", "dedx")]
            + [bits(o.tensor("scalefactor"))])


@pytest.mark.parametrize("order", ["ref", "hip"])
@pytest.mark.parametrize("beta", [0.9, 1.0, 2.0])
def test_a_uniform_vector_is_the_scalar_oracle(pyoracle, order, beta):
    """3 steps; the net's own shapefactor is NOT beta, so the vector is what counts; set, reset and set again is the
    vector too.  The CV log-likelihood's first term is formed in another way with a vector (a double sum over the bins,
    as the engine forms it), so it is the one number held to closeness, not to bits."""
    vec, x, t = bin_net(pyoracle, order, 1.7, np.full(BIN_LS[-1], beta, np.float32), steps=3)
    sca, _, _ = bin_net(pyoracle, order, beta, steps=3)
    for p, q in zip(snapshot(vec, 3), snapshot(sca, 3)):
        assert np.array_equal(p, q)
    assert abs(vec.cv_loglik(x, t) - sca.cv_loglik(x, t)) <= 1e-5 * abs(sca.cv_loglik(x, t))
    vec.set_shapefactors(None)
    assert vec.cv_loglik(x, t) != sca.cv_loglik(x, t)                    # back to its scalar 1.7
    vec.close()
    sca.close()


@pytest.mark.parametrize("order", ["ref", "hip"])
@pytest.mark.parametrize("D,B", [(19, 32), (257, 160)])
def test_columns_of_one_value_are_a_scalar_oracle_s(pyoracle, order, D, B):
    """one step under shapes64.mixed(D): `out` knows no shape; dedx of the output layer and the scalefactor carry, in the
    columns of each value, the bits of a scalar oracle at that value -- and in the other columns they do not"""
    ls = [40, 64, D]
    betas = s6.mixed(D)
    vec, _, _ = bin_net(pyoracle, order, 1.7, betas, B=B, ls=ls)
    out, dedx, alpha = bits(vec.tensor("out", rows=B)), bits(vec.tensor("dedx", 2, rows=B)), bits(vec.tensor("scalefactor"))
    vec.close()
    assert len(s6.groups(betas)) == len(s6.CYCLE)
    for v, cols in s6.groups(betas):
        sca, _, _ = bin_net(pyoracle, order, v, B=B, ls=ls)
        got = bits(sca.tensor("dedx", 2, rows=B))
        assert np.array_equal(out, bits(sca.tensor("out", rows=B)))
        assert np.array_equal(dedx[:, cols], got[:, cols]), v
        assert np.array_equal(alpha[cols], bits(sca.tensor("scalefactor"))[cols]), v
        assert not np.array_equal(dedx[:, ~cols], got[:, ~cols])
        sca.close()


@pytest.mark.parametrize("order", ["ref", "hip"])
@pytest.mark.parametrize("D,B", [(19, 32), (257, 160)])
def test_a_step_and_the_loglik_under_a_mixed_vector_are_inside_the_float64_bounds(pyoracle, order, D, B):
    """shapes64.check_step_bins on one step of the oracle (every operation against its own fp32 inputs) and
    shapes64.expect_cv_bins on its CV log-likelihood over B + 7 frames: the bounds tests/test_gpu_shapefactors.py holds
    the engine to"""
    ls, L = [40, 64, D], 3
    betas = s6.mixed(D)
    W, b = b6.make_net(ls, 100 + D)
    x, t = tc.data(ls, 2 * B, 300 + D)
    cx, ct = tc.data(ls, B + 7, 400 + D)
    pyoracle.set_gemm_order(order, 3)
    try:
        o = pyoracle.OracleNet(ls, B, *HP, 1.7, 1, W, b, shapefactors=betas)
        assert o.train(x[:B], t[:B]) == 1                                # a first step: momentum at work in the second
        W1, b1 = o.get_weights()
        dW1, db1 = [o.tensor("delta_w", l) for l in (1, 2)], [o.tensor("delta_b", l) for l in (1, 2)]
        assert o.train(x[B:], t[B:]) == 1
        W2, b2 = o.get_weights()
        s = b6.Step(x[B:], t[B:], W1, b1, dW1, db1, {1: o.tensor("y", 1, rows=B)}, o.tensor("out", rows=B),
                    {l: o.tensor("dedx", l, rows=B) for l in (1, 2)}, [o.tensor("delta_w", l) for l in (1, 2)],
                    [o.tensor("delta_b", l) for l in (1, 2)], W2, b2, HP[0], HP[1], HP[2], 1.7, 1,
                    3 if order == "hip" else 1, o.tensor("scalefactor"))
        reps = s6.check_step_bins(s, betas)
        assert sum(r.name.startswith("loss ML beta_d") for r in reps) == len(s6.CYCLE)
        bad = [r.line() for r in reps if not r.ok]
        assert not bad, "\n".join(bad)
        ll = o.cv_loglik(cx, ct)
        ex = s6.expect_cv_bins(np.vstack([o.cv_forward(cx[:B]), o.cv_forward(cx[B:])]), ct, betas,
                               o.tensor("scalefactor"), pyoracle.gamma)
        r = b6.compare("loglik", np.array(ll), ex["loglik"])
        assert r.ok, r.line()
        o.set_shapefactors(None)
        assert o.cv_loglik(cx, ct) != ll
        o.close()
    finally:
        pyoracle.set_gemm_order("ref")


def test_the_data_parallel_twin_takes_beta_d_in_its_per_rank_column_sums(pyoracle):
    """ora_set_dp_twin with a vector: two ranks' wavefront sums of |e|^beta_d met in rank order -- the same statistic as
    the plain twin's up to rounding, in other bits, and a uniform vector is the scalar data-parallel twin in every bit"""
    ls, B = [40, 64, 19], 64
    W, b = b6.make_net(ls, 119)
    x, t = tc.data(ls, 2 * B, 219)

    def run(world, betas, beta=1.7):
        pyoracle.set_gemm_order("hip", 1, dp_world=world)
        try:
            o = pyoracle.OracleNet(ls, B, *HP, beta, 1, W, b, shapefactors=betas)
            assert o.train(x, t) == 2
            a = o.tensor("scalefactor")
            o.close()
            return a
        finally:
            pyoracle.set_gemm_order("ref")

    one, two = run(1, s6.mixed(19)), run(2, s6.mixed(19))
    assert relmax(two, one) < 1e-5 and not np.array_equal(one, two)
    assert np.array_equal(run(2, np.full(19, 0.9, np.float32)), run(2, None, 0.9))


# ---------------------------------------------------------------------------------------------------------------------
# 3. not vacuous
def test_the_relu_twin_is_another_order_and_the_rectifier_another_function(pyoracle):
    ls, B = r6.CASE_LS, 24
    W, b = tc.net(ls, 3)
    x, t = tc.data(ls, B, 3)

    def out(order, act):
        pyoracle.set_gemm_order(order, 1)
        try:
            o = pyoracle.OracleNet(ls, B, *tc.HP, 2.0, 0, W, b, activation=act)
            o.train(x, t)
            r = (o.tensor("out", rows=B), o.tensor("y", 1, rows=B), o.tensor("dedx", 1, rows=B))
            o.close()
            return r
        finally:
            pyoracle.set_gemm_order("ref")

    twin, ref, sig = out("hip", "relu"), out("ref", "relu"), out("hip", "sigmoid")
    assert not np.array_equal(twin[0], ref[0]) and relmax(twin[0], ref[0]) < 1e-5
    assert not np.array_equal(twin[0], sig[0]) and relmax(twin[0], sig[0]) > 1e-2
    assert (twin[1] == 0).any() and (twin[2][twin[1] == 0] == 0).all() and (sig[1] > 0).all()
    with pytest.raises(ValueError, match="activation"):
        pyoracle.OracleNet(ls, B, *tc.HP, 2.0, 0, W, b, activation="bogus")


# ---------------------------------------------------------------------------------------------------------------------
# 4. the new golden
def test_the_relu_and_bins_twin_matches_its_golden_bit_exact(pyoracle, synth):
    """tests/golden/mfma_order_twin_relu_bins.npz (oracle/make_golden.py twin_relu_bins()): three steps of twin()'s net
    under the MFMA-order twin (3 slabs) with rectified-linear hidden units, and with those and a mixed shape vector"""
    g = np.load(os.path.join(GOLD, "mfma_order_twin_relu_bins.npz"))
    ls, B = [15, 8, 8, 8, 5], 8
    for key, betas in (("relu", None), ("relu_bins", s6.mixed(5))):
        ws, bs = synth.make_weights(ls, seed=3)
        bs = [np.random.default_rng(30 + l).uniform(-0.5, 0.5, v.shape).astype(np.float32) for l, v in enumerate(bs)]
        inp, targ = synth.make_frames(3 * B, 5, 3, seed=4)
        pyoracle.set_gemm_order("hip", 3)
        try:
            o = pyoracle.OracleNet(ls, B, *HP, 1.2, 1, ws, bs, activation="relu", shapefactors=betas)
            assert o.train(inp, targ) == 3
            ll = o.cv_loglik(inp, targ)
        finally:
            pyoracle.set_gemm_order("ref")
        w, b = o.get_weights()
        for l in range(4):
            assert np.array_equal(w[l], g["%s_W%d" % (key, l + 1)]), (key, l)
            assert np.array_equal(b[l], g["%s_b%d" % (key, l + 1)]), (key, l)
        assert np.array_equal(o.tensor("scalefactor"), g[key + "_alpha"])
        assert np.array_equal(o.tensor("y", 3, rows=B), g[key + "_y3"])
        assert (g[key + "_y3"] == 0).any() and (g[key + "_y3"] > 0).any()
        assert np.float32(ll) == g[key + "_loglik"]
        o.close()
    assert not np.array_equal(g["relu_W4"], g["relu_bins_W4"])


# ---------------------------------------------------------------------------------------------------------------------
# 5. the GPU file's ReLU cases are not degenerate
@pytest.mark.parametrize("case", tc.relu_cases(), ids=lambda c: c[0])
def test_a_gpu_case_is_not_degenerate(pyoracle, case):
    """The case's net, data and seed under the twin (4-wave layers unless the case names a plan, one slab; the zero
    fraction does not hang on a summation order, and the GPU test asserts it again on the engine's own y): in the last
    step between 20 % and 80 % of every hidden layer's y are exactly 0, everything is finite, every layer's weights moved."""
    _, ls, n, steps, seed, ml, beta, kw, plan, world = case
    W, b = tc.net(ls, seed)
    x, t = tc.data(ls, steps * n, seed)
    pyoracle.set_gemm_order("hip", 1, plan=plan, dp_world=world)
    try:
        o = pyoracle.OracleNet(ls, n, *tc.HP, beta, ml, W, b, activation="relu", **kw)
        assert o.train(x, t) == steps
    finally:
        pyoracle.set_gemm_order("ref")
    fr = tc.zero_fractions(o, len(ls), n)
    print(case[0], fr)
    tc.assert_not_degenerate(fr)
    w, bb = o.get_weights()
    assert all(np.isfinite(v).all() for v in w + bb)
    assert all(not np.array_equal(p, q) for p, q in zip(w, W))
    o.close()
