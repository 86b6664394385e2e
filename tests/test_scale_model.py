"""CPU: the learned GGD scale's rule on its float32 model (tests/scale_model.py, the restatement of csrc/scale_rule.h the
GPU tests compare the engine with): the two identities, the stationary point with its derived stall distance, the
clamp, NaN, and the float64 statement's bounds holding for the model itself."""
import math

import numpy as np
import pytest

import asym64 as a6
import bounds64 as b6
import scale_model as sm
import shapes64 as s6

F = np.float32
BETAS = (0.6, 0.9, 1.0, 1.3, 2.0)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def batch(D, B, seed):
    rng = np.random.default_rng(seed)
    out = rng.standard_normal((B, D)).astype(F)
    targ = rng.standard_normal((B, D)).astype(F)
    targ[:, 0] *= F(1e3)
    return out, targ


@pytest.fixture(scope="module", autouse=True)
def _oracle(pyoracle):
    return pyoracle


@pytest.mark.parametrize("skew", [False, True])
def test_seed_is_the_closed_form(skew):
    """alpha == 0 everywhere: alpha' = pow_or_self(v2, 1/beta), v' = 0 and q = pow_or_self(alpha', beta), the alternating
    kernels' statements, whatever eta, mu and vmax are"""
    D, B = 19, 33
    out, targ = batch(D, B, 1)
    betas = s6.mixed(D)
    kaps = a6.kappas(D) if skew else None
    s = sm.colsum(out, targ, betas, kaps)
    for eta, mu, vmax in ((0.05, 0.5, 1.0), (0.0, 0.0, 1e-3), (3.0, 0.9, 10.0)):
        a, v, q = sm.step(np.zeros(D, F), np.zeros(D, F), s, B, betas, eta, mu, vmax)
        v2 = sm.beta_s32(s, B, betas)
        for bv in np.unique(betas):
            c = betas == bv
            want = sm.pow_or_self(v2[c], F(1.0) / bv)
            assert np.array_equal(bits(a[c]), bits(want))
            assert np.array_equal(bits(q[c]), bits(sm.pow_or_self(want, bv)))
        assert np.array_equal(bits(v), bits(np.zeros(D, F)))
    # ... and the closed form is within asym64's bound of the float64 one
    for bv, kv, cols in a6.pairs(betas, kaps if skew else np.ones(D, F)):
        _, ea = a6.expect_loss(out[:, cols], targ[:, cols], bv, kv)
        r = b6.compare("alpha", a[cols], ea)
        assert r.ok, r.line()


def test_frozen_keeps_alpha_bit_for_bit():
    D, B = 257, 40
    betas = s6.mixed(D)
    rng = np.random.default_rng(2)
    X = rng.uniform(0.05, 30.0, D).astype(F)
    v = rng.normal(0.0, 0.2, D).astype(F)
    a = X.copy()
    for k in range(5):
        out, targ = batch(D, B, 10 + k)
        a, v, q = sm.step(a, v, sm.colsum(out, targ, betas), B, betas, 0.0, 0.0, 1.0)
        assert np.array_equal(bits(a), bits(X))
        assert (v == 0).all()                                   # +-0
        for bv in np.unique(betas):
            c = betas == bv
            assert np.array_equal(bits(q[c]), bits(sm.pow_or_self(X[c], bv)))


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("start", [3.0, 1.0 / 3.0])
def test_a_repeated_minibatch_converges_to_the_closed_form_within_the_stall_distance(beta, start):
    D, B, eta, vmax, steps = 24, 64, 0.25, 1.0, 200
    out, targ = batch(D, B, 3)
    betas = np.full(D, beta, F)
    s = sm.colsum(out, targ, betas)
    v2 = sm.beta_s32(s, B, betas).astype(np.float64)
    star = v2 ** (1.0 / float(F(beta)))                         # alpha*: the float64 closed form of the fp32 v2
    assert sm.steps_to_stall(math.log(start), eta, float(F(beta)), vmax) <= steps
    a, v = (star * start).astype(F), np.zeros(D, F)
    for _ in range(steps):
        a, v, _ = sm.step(a, v, s, B, betas, eta, 0.0, vmax)
    dist = np.abs(np.log(a.astype(np.float64)) - np.log(star))
    R = sm.stall(eta, float(F(beta)))
    print("beta %g start %g: worst |ln alpha - ln alpha*| %.3g, stall distance %.3g" % (beta, start, dist.max(), R))
    assert (dist <= R).all(), (dist.max(), R)
    assert R < 3e-6 / min(1.0, beta)                            # the derived distance is a few ulps, not a tolerance
    a2, _, _ = sm.step(a, v, s, B, betas, eta, 0.0, vmax)       # ... and one more step stays inside
    assert (np.abs(np.log(a2.astype(np.float64)) - np.log(star)) <= R).all()


def test_the_clamp_holds_the_velocity():
    D, B = 8, 16
    out, targ = batch(D, B, 4)
    betas = np.full(D, 2.0, F)
    s = sm.colsum(out, targ, betas)
    cf, _, _ = sm.step(np.zeros(D, F), np.zeros(D, F), s, B, betas)
    # alpha far too small: gl = 1 - (cf / alpha)^2 is hugely negative, v' = +vmax; far too large: gl -> 1, v' = -eta
    lo, v_lo, _ = sm.step((cf * F(1e-3)).astype(F), np.zeros(D, F), s, B, betas, 0.25, 0.0, 0.125)
    assert (v_lo == F(0.125)).all()
    assert np.array_equal(bits(lo), bits(sm.advance32((cf * F(1e-3)).astype(F), sm.pyoracle.exp_det(np.full(D, 0.125, F)))))
    hi, v_hi, _ = sm.step((cf * F(1e3)).astype(F), np.zeros(D, F), s, B, betas, 0.25, 0.0, 0.125)
    assert (v_hi == F(-0.125)).all()
    _, v_free, _ = sm.step((cf * F(1e3)).astype(F), np.zeros(D, F), s, B, betas, 0.25, 0.0, 1.0)
    assert (np.abs(v_free + 0.25) < 1e-6).all()
    # momentum alone can reach the clamp as well
    _, v_m, _ = sm.step(cf, np.full(D, 5.0, F), s, B, betas, 0.0, 0.9, 1.0)
    assert (v_m == F(1.0)).all()


def test_a_nan_stays_a_nan():
    D, B = 5, 16
    out, targ = batch(D, B, 5)
    betas = np.full(D, 1.3, F)
    s = sm.colsum(out, targ, betas)
    cf, _, _ = sm.step(np.zeros(D, F), np.zeros(D, F), s, B, betas)
    s_bad = s.copy()
    s_bad[1] = np.nan
    a, v, q = sm.step(cf, np.zeros(D, F), s_bad, B, betas)
    assert np.isnan(a[1]) and np.isnan(v[1]) and np.isfinite(q[1])
    assert np.isfinite(np.delete(a, 1)).all()
    a_bad = cf.copy()
    a_bad[2] = np.nan
    a, v, q = sm.step(a_bad, np.zeros(D, F), s, B, betas)
    assert np.isnan(a[2]) and np.isnan(v[2]) and np.isnan(q[2])
    a, v, _ = sm.step(cf, np.array([0, 0, 0, np.nan, 0], F), s, B, betas)
    assert np.isnan(a[3]) and np.isnan(v[3]) and np.isfinite(np.delete(a, 3)).all()


@pytest.mark.parametrize("skew", [False, True])
def test_the_model_lies_within_the_float64_bounds(skew):
    """several steps on changing minibatches, seeds among the bins: the fp32 model against expect_step"""
    D, B = 19, 160
    betas = s6.mixed(D)
    kaps = a6.kappas(D) if skew else np.ones(D, F)
    rng = np.random.default_rng(6)
    a = rng.uniform(0.3, 3.0, D).astype(F)
    a[::4] = 0.0
    v = np.zeros(D, F)
    for k in range(4):
        out, targ = batch(D, B, 20 + k)
        an, vn, _ = sm.step(a, v, sm.colsum(out, targ, betas, kaps if skew else None), B, betas, 0.05, 0.5, 1.0)
        for bv, kv, cols in a6.pairs(betas, kaps):
            ea, ev = sm.expect_step(a[cols], v[cols], out[:, cols], targ[:, cols], bv, kv, 0.05, 0.5, 1.0)
            ra, rv = b6.compare("alpha'", an[cols], ea), b6.compare("v'", vn[cols], ev)
            assert ra.ok and rv.ok, (k, bv, kv, ra.line(), rv.line())
        a, v = an, vn
    assert (a > 0).all()
