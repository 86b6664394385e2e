"""CPU: pkg.gv_fit (mlggd_gv_fit, csrc/gv_rule.h) -- the fit of the global variance equalisation factors.

Two pins.  (1) The rule restated in Python floats in the rule's own order (tests/gv64.fit_rule): both sides use IEEE
double + - * / and sqrt alone, so every double is compared as uint64 and every factor as uint32.  (2) Independently,
two-pass float64 variances of data the test draws (NumPy deviations, exact sums: tests/gv64.two_pass).  gv = r2 - mu^2
is formed from S1 and S2 with five roundings of magnitude <= r2 after the sums' own (the two divisions, the product,
the subtraction, and mu's error entering mu^2 twice), so each variance is within relative 8 * 2^-53 * (r2 / gv) of the
two-pass value -- the room above five is for the sums' roundings and the two-pass side's own --, and
eta = (float)sqrt(ref / est) within 2^-24 (the cast) plus
half the sum of the two variance bounds (the square root halves a relative error)."""
import numpy as np
import pytest

import gv64
from test_gpu_error_stats import FDIM, TOFF, make_chunk


def bits64(a):
    return np.asarray(a, np.float64).view(np.uint64)


def bits32(a):
    return np.asarray(a, np.float32).view(np.uint32)


def draw(n, seed):
    """outputs and targets as make_chunk draws its streams: y standard normal, t = 0.5 y + 0.5 noise"""
    feat, tstream, first, _, targ = make_chunk(n, seed)
    return np.ascontiguousarray(feat[first + TOFF]), targ


def assert_is_the_rule(pkg, n, sums):
    fit = pkg.gv_fit(n, sums)
    est, ref, eta, fitted, shared = gv64.fit_rule(n, sums)
    assert np.array_equal(bits64(fit.gv_est), bits64(est)) and np.array_equal(bits64(fit.gv_ref), bits64(ref))
    assert np.array_equal(bits32(fit.eta), bits32(eta)) and np.array_equal(fit.fitted, fitted)
    assert bits64(fit.gv_est_shared) == bits64(shared[0]) and bits64(fit.gv_ref_shared) == bits64(shared[1])
    assert bits32(fit.eta_shared) == bits32(shared[2]) and fit.fitted_shared == shared[3]
    return fit


@pytest.mark.parametrize("n", [2, 3, 33, 500])
def test_gv_fit_is_the_rule_bit_for_bit(pkg, n):
    y, t = draw(n, seed=40 + n)
    fit = assert_is_the_rule(pkg, n, gv64.exact_sums(y, t))
    assert fit.fitted.all() and fit.fitted_shared and fit.eta.dtype == np.float32 and fit.gv_est.dtype == np.float64
    # ... also on sums that are no exact statistics of anything
    rng = np.random.default_rng(n)
    s = rng.uniform(-50, 50, (4, 7))
    s[1], s[3] = np.abs(s[1]) * 40, np.abs(s[3]) * 40
    assert_is_the_rule(pkg, n, s)


@pytest.mark.parametrize("n", [8, 200, 5000])
def test_gv_fit_against_two_pass_variances(pkg, n):
    y, t = draw(n, seed=60 + n)
    model = gv64.fit_rule(n, gv64.exact_sums(y, t))
    assert model[3].all()                                    # the model alone fits every bin
    fit = pkg.gv_fit(n, gv64.exact_sums(y, t))
    assert fit.fitted.all()
    worst, bounds = 0.0, []
    for got, x in ((fit.gv_est, y), (fit.gv_ref, t)):
        var, r2 = gv64.two_pass(x)
        bound = 8 * gv64.U53 * (r2 / var)
        rel = np.abs(got - var) / var
        worst = max(worst, float((rel / bound).max()))
        assert (rel <= bound).all(), np.argwhere(rel > bound)[:5]
        bounds.append(bound)
    want = np.sqrt(gv64.two_pass(t)[0] / gv64.two_pass(y)[0])
    rel = np.abs(fit.eta.astype(np.float64) - want) / want
    bound = gv64.U24 + 0.5 * (bounds[0] + bounds[1])
    print("n %d: largest variance error / bound %.3g, largest eta error / bound %.3g" % (n, worst, (rel / bound).max()))
    assert (rel <= bound).all()


def test_bins_without_a_fit(pkg):
    n = 64
    y, t = draw(n, seed=70)
    # n = 1: no variance at all
    one = pkg.gv_fit(1, gv64.exact_sums(y[:1], t[:1]))
    assert not one.fitted.any() and (one.eta == 1).all() and one.eta_shared == 1 and not one.fitted_shared
    assert_is_the_rule(pkg, 1, gv64.exact_sums(y[:1], t[:1]))
    # a constant output column and a constant target column (values whose squares and sums are exact)
    yc, tc = y.copy(), t.copy()
    yc[:, 3] = 0.5
    tc[:, 5] = -2.0
    sums = gv64.exact_sums(yc, tc)
    fit = assert_is_the_rule(pkg, n, sums)
    assert not fit.fitted[3] and not fit.fitted[5] and fit.fitted.sum() == FDIM - 2
    assert fit.eta[3] == 1 and fit.eta[5] == 1 and fit.gv_est[3] == 0 and fit.gv_ref[5] == 0
    # ... and they are left out of the shared factor: it is the one of the other bins alone
    keep = np.ones(FDIM, bool)
    keep[[3, 5]] = False
    rest = pkg.gv_fit(n, np.ascontiguousarray(sums[:, keep]))
    assert rest.fitted.all() and fit.fitted_shared
    assert bits32(fit.eta_shared) == bits32(rest.eta_shared)
    assert bits64(fit.gv_est_shared) == bits64(rest.gv_est_shared)
    # every bin unfitted
    yc[:] = 0.25
    none = assert_is_the_rule(pkg, n, gv64.exact_sums(yc, t))
    assert not none.fitted.any() and none.eta_shared == 1 and not none.fitted_shared and (none.eta == 1).all()


def test_identical_columns_pool_to_the_bin_s_factor(pkg):
    n, D = 300, 9
    y, t = draw(n, seed=80)
    y, t = np.repeat(y[:, :1], D, axis=1), np.repeat(t[:, :1], D, axis=1)
    fit = pkg.gv_fit(n, gv64.exact_sums(y, t))
    assert fit.fitted.all() and fit.fitted_shared and len(set(fit.eta.tolist())) == 1
    # the pooled sums are D times a bin's, up to D - 1 additions each: the variances differ by the bound of the
    # two-pass test plus D 2^-53 r2 / gv for the additions, the factors by the casts and half the sum of those
    b = 0.0
    for x in (y, t):
        var, r2 = gv64.two_pass(x[:, :1])
        b += float((8 + D) * gv64.U53 * (r2 / var)[0]) * 2
    rel = abs(float(fit.eta_shared) - float(fit.eta[0])) / float(fit.eta[0])
    print("shared against per-bin: relative %.3g, bound %.3g" % (rel, 2 * gv64.U24 + 0.5 * b))
    assert rel <= 2 * gv64.U24 + 0.5 * b


def test_gv_fit_argument_errors(pkg):
    s = np.ones((4, 3))
    for n in (0, -5):
        with pytest.raises(pkg.MlggdError, match="error 1: n %d" % n):
            pkg.gv_fit(n, s)
    with pytest.raises(ValueError):
        pkg.gv_fit(4, np.ones((3, 3)))
    with pytest.raises(ValueError):
        pkg.gv_fit(4, np.ones(4))
    L = pkg.load()
    assert L.mlggd_gv_fit(3, 4, None, None, None, None, None, None, None, None, None) == 1
    assert "sums is NULL" in L.mlggd_last_error().decode()
    assert L.mlggd_gv_fit(0, 4, None, None, None, None, None, None, None, None, None) == 1
    assert "D 0 < 1" in L.mlggd_last_error().decode()
    # every output pointer is optional
    import ctypes as C
    assert L.mlggd_gv_fit(3, 4, s.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None, None, None, None, None) == 0
