"""float64 expectations for a per-bin shape vector (BPGpu.set_shapefactors), built on tests/bounds64.py as it is.

Column d of the ML-GGD loss chain depends on column d's errors and on beta_d alone (include/mlggd.h), so the existing
scalar bound applies per group of columns of equal beta: `bounds64.expect_loss` is called on the columns of one value
with that value, which is exactly the scalar case it was derived for (its B and n are the frame count, not the column
count).  Everything downstream of dE/dz (dX, dW, db, the updates) and the forward pass do not know the shape and keep
`bounds64.check_step`'s checks unchanged.  No new tolerance is introduced for the step.

The CV log-likelihood is the one bound that has to be restated, because two of its three terms now mix shapes:
`expect_cv_bins` below carries `bounds64.expect_cv`'s derivation over term by term."""
import math

import numpy as np

import bounds64 as b6

CYCLE = (0.6, 0.9, 1.0, 1.3, 2.0)   # the two self-cases of pow_or_self, 1.0 and 2.0, are in it on purpose


def mixed(D):
    """[D] float32 cycling through CYCLE"""
    return np.array([CYCLE[d % len(CYCLE)] for d in range(D)], np.float32)


def groups(betas):
    """(value, column mask) for every distinct shape"""
    betas = np.asarray(betas, np.float32)
    return [(float(v), betas == v) for v in np.unique(betas)]


def check_step_bins(s, betas, layers=None):
    """`bounds64.check_step` for a step trained with the vector `betas`: the loss and alpha reports are replaced by one
    pair per group of columns of equal beta (s.beta is not used), the rest is check_step's own."""
    L = len(s.W) + 1
    reps = [r for r in b6.check_step(s, layers) if not (r.name.startswith("loss ") or r.name == "alpha")]
    for v, cols in groups(betas):
        eg, ea = b6.expect_loss(s.out[:, cols], s.targ[:, cols], v, 1)
        reps.append(b6.compare("loss ML beta_d %g" % v, s.dedx[L - 1][:, cols], eg))
        reps.append(b6.compare("alpha beta_d %g" % v, s.alpha[cols], ea))
    return reps


def expect_cv_bins(out, targ, betas, alpha, gamma_fn):
    """`bounds64.expect_cv` with a shape per column.  sqerr and abserr do not know the shape and are expect_cv's.
    loglik = d1 - d2 - d3 with
      d1 = sum_d n ln(beta_d / (2 Gamma(fl(1/beta_d))))   (the engine adds the D fp32 logf values, times n, in double)
      d2 = n sum_u ln alpha_u                              (unchanged)
      d3 = sum (|t - o| / alpha_d)^beta_d                  (one fp32 sum over all N = n D terms, or double partials)
    Bounds, each the scalar one applied where the scalar argument applies:
      d1: per bin n (u + 4u |ln(.)|) as in expect_cv (the argument's division, logf within an ulp); the double sum over
          the bins adds nothing at this precision, and its rounding to fp32 (host order) is the u |d1| expect_cv
          already charges for "N as a float";
      d2: gamma_{D+3} n sum |ln alpha|, unchanged;
      d3: the sum's part gamma_N d3 is over all terms whatever their shape; the per-term part (2 beta + 2) u is
          charged per column with its own beta_d: sum_d (2 beta_d + 2) u d3_d;
      the two subtractions: 2u (|d1| + |d2| + |d3|), unchanged.
    The tight limit takes expect_cv's 4 sqrt(N) + 8 + 2 beta at the largest beta_d."""
    out, targ = b6._d(out), b6._d(targ)
    n, D = out.shape
    N = n * D
    res = b6.expect_cv(out, targ)
    e = out - targ
    bt = np.array([b6.f32(v) for v in betas], np.float64)
    a = b6._d(alpha)
    Lc = np.array([math.log(v / (2.0 * float(gamma_fn(float(np.float32(1.0 / v)))))) for v in bt])
    d1 = n * float(Lc.sum())
    la = np.log(a)
    d2 = n * float(la.sum())
    t3 = ((np.abs(e) / a) ** bt).sum(axis=0)          # d3 per column
    d3 = float(t3.sum())
    b1 = n * float((b6.U + 4.0 * b6.U * np.abs(Lc)).sum()) + b6.U * abs(d1)
    b2 = b6.gamma(D + 3) * n * float(np.abs(la).sum())
    b3 = b6.gamma(N) * d3 + float(((2.0 * bt + 2.0) * b6.U * t3).sum())
    b = b1 + b2 + b3 + 2.0 * b6.U * (abs(d1) + abs(d2) + abs(d3))
    den = b6.U * (abs(d1) + abs(d2) + d3)
    res["loglik"] = b6.Expect(np.float64(d1 - d2 - d3), np.float64(b), 0.0, np.float64(den),
                              4.0 * math.sqrt(N) + 8.0 + 2.0 * float(bt.max()))
    return res
