"""The float64 model of global variance equalisation (csrc/gv_rule.h), restated for the tests: the fit in Python floats
in the rule's own order, the statistics by math.fsum with the bound of a double sum in any order, the two-pass
variances of NumPy, and the decoders' de-normalisation one fp32 operation at a time."""
import math

import numpy as np

U53 = 2.0 ** -53
U24 = 2.0 ** -24


def variance(s1, s2, n):
    """mu = S1 / n, r2 = S2 / n, gv = r2 - mu mu: Python floats are IEEE doubles, one rounding per operation"""
    mu = s1 / n
    r2 = s2 / n
    mm = mu * mu
    return r2 - mm


def fit_one(sy, syy, st, stt, n):
    est, ref = variance(sy, syy, n), variance(st, stt, n)
    fitted = est > 0.0 and ref > 0.0
    eta = np.float32(math.sqrt(ref / est)) if fitted else np.float32(1.0)
    return est, ref, eta, fitted


def fit_rule(n, sums):
    """(gv_est [D], gv_ref [D], eta [D] float32, fitted [D] bool, (gv_est, gv_ref, eta, fitted) shared)"""
    sums = np.asarray(sums, np.float64)
    D = sums.shape[1]
    est, ref, eta, fitted = np.zeros(D), np.zeros(D), np.ones(D, np.float32), np.zeros(D, bool)
    pool, bins = [0.0, 0.0, 0.0, 0.0], 0
    for d in range(D):
        est[d], ref[d], eta[d], fitted[d] = fit_one(*(float(sums[r, d]) for r in range(4)), float(n))
        if fitted[d]:
            for r in range(4):
                pool[r] = pool[r] + float(sums[r, d])
            bins += 1
    shared = fit_one(*pool, float(n) * float(bins)) if bins else (0.0, 0.0, np.float32(1.0), False)
    return est, ref, eta, fitted, shared


def terms(out, targ):
    """the four [n][D] float64 term arrays from the fp32 outputs and targets"""
    y = np.asarray(out, np.float32).astype(np.float64)
    t = np.asarray(targ, np.float32).astype(np.float64)
    return [y, y * y, t, t * t]


def exact_sums(out, targ):
    """[4][D] float64: every sum by math.fsum (one rounding)"""
    D = np.asarray(targ).shape[1]
    if np.asarray(out).shape[0] == 0:
        return np.zeros((4, D))
    return np.array([[math.fsum(t[:, d]) for d in range(D)] for t in terms(out, targ)], np.float64)


def pin(out, targ):
    """(want [4][D], bound [4][D]): a double sum of n terms in ANY order is within 2 n 2^-53 sum|term| of fsum's"""
    D = np.asarray(targ).shape[1]
    n = np.asarray(out).shape[0]
    if n == 0:
        return np.zeros((4, D)), np.zeros((4, D))
    tt = terms(out, targ)
    mag = np.array([[math.fsum(np.abs(t[:, d])) for d in range(D)] for t in tt], np.float64)
    return exact_sums(out, targ), 2.0 * n * U53 * mag


def two_pass(x):
    """population variance per column about the column's mean, and the mean square, in float64.  The deviations and
    their squares are NumPy float64; every sum is math.fsum's, so that the reference carries the roundings of its terms
    and one per sum -- NumPy's pairwise sums alone are off by several units of 2^-53 at a few thousand rows, more than
    the fit under test."""
    x = np.asarray(x, np.float64)
    n, D = x.shape
    mu = np.array([math.fsum(x[:, d]) for d in range(D)]) / n
    dev = x - mu
    var = np.array([math.fsum((dev * dev)[:, d]) for d in range(D)]) / n
    r2 = np.array([math.fsum((x * x)[:, d]) for d in range(D)]) / n
    return var, r2


def apply32(y, eta, inv, mean):
    """v = ((y * eta) / inv) + mean, three IEEE fp32 operations; eta None: (y / inv) + mean"""
    y = np.asarray(y, np.float32)
    s = y if eta is None else (y * np.asarray(eta, np.float32)).astype(np.float32)
    q = (s / np.asarray(inv, np.float32)).astype(np.float32)
    return (q + np.asarray(mean, np.float32)).astype(np.float32)


def draw_eta(D, seed):
    """factors in [0.5, 2] per bin"""
    return np.random.default_rng(seed).uniform(0.5, 2.0, D).astype(np.float32)


def write_gv_file(path, n, est, ref, eta, fitted, shared):
    """the trainer's file in its documented format: variances in %.17g, factors in %.9g, nan where there is no fit"""
    g = lambda v, ok: ("%.9g" % v) if ok else "nan"
    with open(path, "w") as f:
        f.write("# global variance equalisation of the CV set\n# n %d\n# D %d\n" % (n, len(eta)))
        f.write("# shared_eta %s\n# gv_ref_shared %.17g\n# gv_est_shared %.17g\n# d gv_ref gv_est eta\n"
                % (g(shared[2], shared[3]), shared[1], shared[0]))
        for d in range(len(eta)):
            f.write("%d %.17g %.17g %s\n" % (d, ref[d], est[d], g(eta[d], fitted[d])))
