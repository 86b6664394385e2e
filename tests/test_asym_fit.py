"""CPU, no device: pkg.asym_fit (mlggd_asym_fit, csrc/asym_rule.h), the closed-form fit of the asymmetric GGD error
model from the signed power sums P+ = sum_{e>0} e^beta and P- = sum_{e<0} (-e)^beta.

The closed form is checked twice: against the same expressions in float64 (tests/asym64.py) on sums built from known
P+ and P-, and -- since that only shows that two copies of a formula agree -- against a brute-force maximisation of
the likelihood itself over a fine kappa grid written here, on 200 000 float64 samples per bin drawn from the model.  The
comparison is with that maximiser, not with the true kappa, so its margin is the grid's step and no statistical
tolerance is involved."""
import ctypes

import numpy as np
import pytest

import asym64 as a6

BETAS = np.array([0.5, 0.8, 1.0, 1.5, 2.0], np.float32)


def sums_of(pp, pm):
    """[2 K][D] from [K][D] P+ and P-"""
    return np.concatenate([np.asarray(pp, np.float64), np.asarray(pm, np.float64)], axis=0)


def test_the_closed_form_on_known_sums(pkg):
    rng = np.random.default_rng(1)
    K, D, n = BETAS.size, 11, 5000
    pp, pm = rng.uniform(10, 4000, (K, D)), rng.uniform(10, 4000, (K, D))
    pm[:, 3] = pp[:, 3]                                    # P+ == P-: kappa is 1
    fit = pkg.asym_fit(n, sums_of(pp, pm), BETAS)
    assert fit.kappa.shape == fit.alpha.shape == fit.loglik.shape == (K, D) and fit.best.shape == (D,)
    for k, b in enumerate(BETAS.astype(np.float64)):
        kap, alpha, ll = a6.fit(pp[k], pm[k], b, n)
        assert np.allclose(fit.kappa[k], kap, rtol=1e-13, atol=0)
        assert np.allclose(fit.alpha[k], alpha, rtol=1e-13, atol=0)
        assert np.allclose(fit.loglik[k], ll, rtol=1e-12, atol=1e-9)
        assert np.allclose(fit.kappa[k], (pm[k] / pp[k]) ** (1.0 / (2.0 * (b + 1.0))), rtol=1e-13, atol=0)   # as the header states it
    assert np.allclose(fit.kappa[:, 3], 1.0, rtol=1e-15, atol=0)
    assert np.array_equal(fit.best, fit.loglik.argmax(axis=0))
    assert np.allclose(fit.loglik_shared, fit.loglik.sum(axis=1), rtol=1e-13, atol=0)
    assert fit.best_shared == int(fit.loglik_shared.argmax())
    # P+ and P- swapped: kappa goes to 1 / kappa, alpha and the likelihood stay
    mirror = pkg.asym_fit(n, sums_of(pm, pp), BETAS)
    assert np.allclose(mirror.kappa * fit.kappa, 1.0, rtol=1e-13, atol=0)
    assert np.allclose(mirror.alpha, fit.alpha, rtol=1e-13, atol=0) and np.array_equal(mirror.best, fit.best)


@pytest.mark.parametrize("beta,kappa", [(1.0, 1.0), (1.0, 1.6), (2.0, 0.7), (0.6, 1.3), (1.4, 0.5)])
def test_kappa_is_the_maximiser_of_the_likelihood(pkg, beta, kappa):
    """200 000 draws from the model; the likelihood (alpha profiled out, written from the density in asym64.loglik) is
    maximised over kappa on a grid of step 1e-4 in ln kappa around the fit: the closed form lies within one step of the
    grid's argmax, and no grid point has a higher likelihood than the fit's"""
    n = 200000
    rng = np.random.default_rng(int(1000 * beta + 10 * kappa))
    e = a6.sample(rng, n, beta, kappa, alpha=0.8)
    b32 = np.array([beta], np.float32)
    bb = float(b32[0])
    pp = (np.where(e > 0, e, 0.0) ** bb).sum()
    pm = (np.where(e < 0, -e, 0.0) ** bb).sum()
    fit = pkg.asym_fit(n, np.array([[pp], [pm]]), b32)
    got = float(fit.kappa[0, 0])
    step = 1e-4
    grid = np.exp(np.log(got) + step * np.arange(-3000, 3001))         # +-0.3 in ln kappa: far past the sampling error
    ll = a6.loglik(e, bb, grid)
    at = int(ll.argmax())
    assert 0 < at < grid.size - 1                                      # an interior maximum of the grid
    assert abs(np.log(grid[at]) - np.log(got)) <= step * (1 + 1e-9), (grid[at], got)
    assert fit.loglik[0, 0] >= ll.max() - 1e-12 * abs(ll.max())        # the fit is at least as likely as any grid point
    assert abs(fit.loglik[0, 0] - ll[3000]) <= 1e-12 * abs(ll[3000])   # ... and loglik is the likelihood at the fit


def test_bins_without_a_fit_and_ties(pkg):
    K, D, n = 3, 5, 100
    betas = np.array([1.0, 1.0, 2.0], np.float32)                      # shapes 0 and 1 tie everywhere
    pp = np.array([[4.0, 0.0, 3.0, 0.0, 2.0]] * K)
    pm = np.array([[1.0, 2.0, 0.0, 0.0, 2.0]] * K)
    fit = pkg.asym_fit(n, sums_of(pp, pm), betas)
    nofit = np.array([False, True, True, True, False])
    assert np.isnan(fit.kappa[:, nofit]).all() and np.isnan(fit.loglik[:, nofit]).all() and (fit.alpha[:, nofit] == 0).all()
    assert np.isfinite(fit.kappa[:, ~nofit]).all() and np.isfinite(fit.loglik[:, ~nofit]).all()
    assert fit.best.tolist() == [fit.best[0], -1, -1, -1, fit.best[4]] and fit.best[0] in (0, 2) and fit.best[4] in (0, 2)
    assert np.array_equal(fit.loglik[0], fit.loglik[1], equal_nan=True)           # the tie ...
    assert 1 not in fit.best.tolist()                                             # ... goes to the lower index
    assert np.allclose(fit.loglik_shared, fit.loglik[:, ~nofit].sum(axis=1))      # bins without a fit are left out
    assert fit.loglik_shared[0] == fit.loglik_shared[1] and fit.best_shared in (0, 2)
    none = pkg.asym_fit(n, sums_of(np.zeros((K, D)), pm), betas)                   # no bin has a fit
    assert (none.best == -1).all() and none.best_shared == -1 and not none.loglik_shared.any()


def test_argument_errors(pkg):
    L = pkg.load()
    s = np.ones((2, 4))
    one = np.ones(1, np.float32)
    with pytest.raises(ValueError):
        pkg.asym_fit(10, np.ones((3, 4)), one)                         # not [2 K][D]
    with pytest.raises(pkg.MlggdError, match="error 1: n 0"):
        pkg.asym_fit(0, s, one)
    for bad, msg in (([0.0], r"betas\[0\]"), ([1.0, float("nan")], r"betas\[1\]"), (np.ones(33, np.float32), "n_betas 33")):
        with pytest.raises(pkg.MlggdError, match="error 1: " + msg):
            pkg.asym_fit(10, np.ones((2 * len(bad), 4)), bad)
    dp = ctypes.POINTER(ctypes.c_double)
    fp = one.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    assert L.mlggd_asym_fit(4, 10, 1, fp, None, None, None, None, None, None, None) == 1 and b"NULL" in L.mlggd_last_error()
    assert L.mlggd_asym_fit(0, 10, 1, fp, s.ctypes.data_as(dp), None, None, None, None, None, None) == 1
    assert L.mlggd_asym_fit(4, 10, 1, fp, s.ctypes.data_as(dp), None, None, None, None, None, None) == 0   # every output optional
