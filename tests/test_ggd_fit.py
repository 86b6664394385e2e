"""CPU: mlggd_ggd_fit (pkg.ggd_fit), the host-only fit of the GGD error model, against the float64 restatement
tests/ggd64.py (math.lgamma): agreement on random sums and on sums of real GGD draws, recovery of a known shape and
scale, the kurtosis of Gaussian and Laplacian data, the no-fit rule, ties, the argument errors and additivity.

Both sides are double with a handful of operations in the same order, so every output agrees to 1e-12 relative."""
import ctypes as C

import numpy as np
import pytest

import ggd64

ERR_ARG = 1
RTOL = 1e-12
GRID = ggd64.grid()                                       # 0.5:0.1:2.5, 21 shapes
ALPHAS = np.linspace(0.3, 2.5, 5)


def assert_same(got, want):
    for name in ggd64.Fit._fields:
        g, w = np.asarray(getattr(got, name)), np.asarray(getattr(want, name))
        assert g.shape == w.shape, name
        if g.dtype.kind in "iu":
            assert np.array_equal(g, w), name
        else:
            assert np.array_equal(np.isnan(g), np.isnan(w)), name
            ok = ~np.isnan(w)
            assert (np.abs(g[ok] - w[ok]) <= RTOL * np.abs(w[ok])).all(), (name, g, w)


def test_the_grid_is_the_default_one():
    assert GRID.size == 21 and GRID[0] == np.float32(0.5) and GRID[-1] == np.float32(2.5)
    assert GRID[5] == np.float32(1.0) and GRID[15] == np.float32(2.0)


def test_random_sums_equal_the_model(pkg):
    rng = np.random.default_rng(11)
    D, n = 8, 5000
    # sums a data set could have: those of n draws of any law with these raw moments per bin
    s = np.empty((4 + GRID.size, D))
    s[0] = n * rng.uniform(-0.5, 0.5, D)
    s[1] = n * rng.uniform(0.5, 3.0, D)
    s[2] = n * rng.uniform(-2.0, 2.0, D)
    s[3] = n * rng.uniform(3.0, 30.0, D)
    s[4:] = n * rng.uniform(0.2, 4.0, (GRID.size, D))
    assert_same(pkg.ggd_fit(n, s, GRID), ggd64.fit(n, s, GRID))


@pytest.mark.parametrize("beta", [0.8, 1.0, 1.5, 2.0])
def test_sums_of_ggd_draws_equal_the_model_and_recover_shape_and_scale(pkg, beta):
    """n = 20,000 per bin, five bins with alpha from 0.3 to 2.5, grid 0.5:0.1:2.5: the shared argmax is the true beta,
    every per-bin argmax is within one grid step and the scale at the shared beta is within 3 % -- confirmed on the
    model first, then the library must return the model's fit."""
    n = 20000
    e = ggd64.draw(np.random.default_rng(2024), n, ALPHAS, beta)
    s = ggd64.sums(e, GRID)
    want = ggd64.fit(n, s, GRID)
    true_k = int(np.argmin(np.abs(GRID - beta)))
    for f in (want, pkg.ggd_fit(n, s, GRID)):
        assert f.best_shared == true_k
        assert (np.abs(np.asarray(f.best) - true_k) <= 1).all(), f.best
        assert (np.abs(f.alpha[f.best_shared] / ALPHAS - 1.0) <= 0.03).all(), f.alpha[f.best_shared]
        assert int(np.argmax(f.loglik_shared)) == f.best_shared
    assert_same(pkg.ggd_fit(n, s, GRID), want)


def test_kurtosis_of_gaussian_and_laplacian_data(pkg):
    n = 200000
    rng = np.random.default_rng(5)
    e = np.stack([rng.standard_normal(n) * 1.7 + 0.4, rng.laplace(-0.2, 0.9, n)], axis=1)
    s = ggd64.sums(e, [1.0, 2.0])
    for f in (ggd64.fit(n, s, [1.0, 2.0]), pkg.ggd_fit(n, s, [1.0, 2.0])):
        assert abs(f.kurt[0]) <= 0.1 and abs(f.kurt[1] - 3.0) <= 0.3, f.kurt
        assert abs(f.mean[0] - 0.4) < 0.02 and abs(f.var[0] - 1.7 ** 2) < 0.05
        assert list(f.best) == [1, 0]                     # Gaussian: beta 2, Laplacian: beta 1


def test_a_bin_without_errors_has_no_fit_and_is_left_out_of_the_shared_totals(pkg):
    n = 3000
    e = ggd64.draw(np.random.default_rng(3), n, [0.5, 1.0, 2.0], 1.0)
    e[:, 1] = 0.0
    betas = [0.7, 1.0, 1.6]
    s = ggd64.sums(e, betas)
    f = pkg.ggd_fit(n, s, betas)
    assert f.best[1] == -1 and (f.alpha[:, 1] == 0).all() and np.isnan(f.loglik[:, 1]).all() and np.isnan(f.kurt[1])
    assert f.mean[1] == 0 and f.var[1] == 0
    assert (f.best[[0, 2]] >= 0).all() and np.isfinite(f.loglik[:, [0, 2]]).all()
    assert np.array_equal(f.loglik_shared, f.loglik[:, 0] + f.loglik[:, 2])
    assert_same(f, ggd64.fit(n, s, betas))
    # no bin with a fit: no shared shape either
    z = pkg.ggd_fit(n, np.zeros((4 + 3, 2)), betas)
    assert z.best_shared == -1 and list(z.best) == [-1, -1] and (z.loglik_shared == 0).all()
    assert_same(z, ggd64.fit(n, np.zeros((4 + 3, 2)), betas))


def test_a_tie_goes_to_the_lower_index(pkg):
    n = 1000
    e = ggd64.draw(np.random.default_rng(4), n, [1.0, 0.6], 2.0)
    betas = [2.0, 1.2, 2.0]
    f = pkg.ggd_fit(n, ggd64.sums(e, betas), betas)
    assert np.array_equal(f.loglik[0], f.loglik[2]) and f.loglik_shared[0] == f.loglik_shared[2]
    assert list(f.best) == [0, 0] and f.best_shared == 0


def raw_fit(pkg, D, n, betas, sums, n_betas=None):
    b = np.asarray(betas, np.float32)
    s = np.asarray(sums, np.float64)
    rc = pkg.load().mlggd_ggd_fit(D, n, b.size if n_betas is None else n_betas, b.ctypes.data_as(C.POINTER(C.c_float)),
                                  s.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None, None, None, None, None)
    return rc, pkg.load().mlggd_last_error().decode()


def test_argument_errors(pkg):
    s = np.ones((4 + 33, 2))
    assert raw_fit(pkg, 2, 10, [1.0], s)[0] == 0            # every output is optional
    for n in (0, -5):
        rc, msg = raw_fit(pkg, 2, n, [1.0], s)
        assert rc == ERR_ARG and "n %d" % n in msg
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        rc, msg = raw_fit(pkg, 2, 10, [1.0, bad], s)
        assert rc == ERR_ARG and "betas[1]" in msg
    for k in (0, 33):
        rc, msg = raw_fit(pkg, 2, 10, np.ones(33), s, n_betas=k)
        assert rc == ERR_ARG and "n_betas %d" % k in msg
    assert raw_fit(pkg, 2, 10, np.ones(32), s)[0] == 0
    assert raw_fit(pkg, 0, 10, [1.0], s)[0] == ERR_ARG
    L = pkg.load()
    b = np.ones(1, np.float32)
    assert L.mlggd_ggd_fit(2, 10, 1, b.ctypes.data_as(C.POINTER(C.c_float)), None, *([None] * 8)) == ERR_ARG
    assert L.mlggd_ggd_fit(2, 10, 1, None, s.ctypes.data_as(C.POINTER(C.c_double)), *([None] * 8)) == ERR_ARG
    with pytest.raises(pkg.MlggdError, match="error 1: n 0"):
        pkg.ggd_fit(0, np.ones((5, 2)), [1.0])
    with pytest.raises(pkg.MlggdError, match="n_betas 33"):
        pkg.ggd_fit(5, np.ones((37, 2)), np.ones(33))
    with pytest.raises(ValueError):
        pkg.ggd_fit(5, np.ones((4, 2)), [1.0])


def test_the_fit_is_additive_over_chunks(pkg):
    rng = np.random.default_rng(6)
    a, b = ggd64.draw(rng, 1500, ALPHAS, 1.3), ggd64.draw(rng, 2500, ALPHAS, 1.3)
    whole = pkg.ggd_fit(4000, ggd64.sums(np.concatenate([a, b]), GRID), GRID)
    added = pkg.ggd_fit(4000, ggd64.sums(a, GRID) + ggd64.sums(b, GRID), GRID)
    assert_same(added, whole)
