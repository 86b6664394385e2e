"""float64 model of the asymmetric GGD error model (BPGpu.set_asymmetry, csrc/asym_rule.h), built on tests/bounds64.py
and tests/shapes64.py as they are.

Per bin d with shape beta_d, scale alpha_d and skew kappa_d the error e = out - targ is charged through
    s(e) = kappa e (e > 0),  -e / kappa (e < 0),  0 (e == 0)
in the place of |e|: p = s^beta, alpha = (beta sum p / n)^(1/beta), g = sgn(e) s^(beta-1) beta / alpha^beta * ds/de / n
with ds/de = kappa for e > 0 and 1/kappa for e < 0.  Column d depends on column d's errors, beta_d and kappa_d alone, so
the loss bound applies per group of columns of equal (beta, kappa).

Bounds.  `expect_loss` below is bounds64.expect_loss with the two roundings the rule adds, each charged where
bounds64.loss_rel charges its like:
  s = fl(kappa e) or fl(-e / kappa)  : one more rounding of the power's argument, which already carries e's own u:
      p = s^beta           beta u more:      rel(p) = 2 beta u + pw
      P = s^(beta - 1)     |beta - 1| u more: rel(P) = 2 |beta - 1| u + pw
  g = fl(v kappa) or fl(-v / kappa)  : one more rounding of the gradient: rel(g) gains u.
Everything else (the column sum's gamma_B, / n, * beta, the 1/beta power and its exponent term, alpha^beta, the tight
statistic of the column sum) is loss_rel's and expect_loss's own.  No measured tolerance.

The CV log-likelihood carries shapes64.expect_cv_bins over term by term (`expect_cv`), with s(o - t) in d3 and the new
term dk = n sum_d ln((kappa_d + 1/kappa_d) / 2) taken off d1."""
import math

import numpy as np

import bounds64 as b6
import shapes64 as s6

KCYCLE = (0.5, 0.8, 1.0, 1.25, 2.0)
POW2 = (0.25, 0.5, 1.0, 2.0, 4.0)


def kappas(D, shift=1):
    """[D] float32 cycling through KCYCLE, one step ahead of shapes64.mixed's cycle: the pairs (beta, kappa) are
    (0.6, 0.8), (0.9, 1.0), (1.0, 1.25), (1.3, 2.0), (2.0, 0.5) -- kappa = 1 sits on a beta that takes pow_det"""
    return np.array([KCYCLE[(d + shift) % len(KCYCLE)] for d in range(D)], np.float32)


def pow2(D):
    """[D] float32 cycling through powers of two (the mirror identity)"""
    return np.array([POW2[d % len(POW2)] for d in range(D)], np.float32)


def pairs(betas, kaps):
    """(beta, kappa, column mask) for every distinct pair"""
    betas, kaps = np.asarray(betas, np.float32), np.asarray(kaps, np.float32)
    seen = sorted(set(zip(betas.tolist(), kaps.tolist())))
    return [(b, k, (betas == np.float32(b)) & (kaps == np.float32(k))) for b, k in seen]


def skewed(e, kappa):
    """s(e) in float64, kappa a scalar or one value per column"""
    e = b6._d(e)
    k = np.broadcast_to(b6._d(kappa), e.shape)
    return np.where(e > 0, k * e, np.where(e < 0, -e / k, 0.0))


def loss_rel(beta, B):
    """bounds64.loss_rel(beta, 1, B) with the rule's two roundings (module docstring)"""
    pw = 2.0 * b6.U
    rel_P = 2.0 * abs(beta - 1.0) * b6.U + pw
    rel_s = b6.gamma(B) + 2.0 * beta * b6.U + pw
    return (rel_s + 2.0 * b6.U) / beta + pw, rel_P + 4.0 * b6.U + pw + b6.U


def expect_loss(out, targ, beta, kappa, n=None):
    """(Expect for dE/dz, Expect for alpha) of columns that share one (beta, kappa), from the engine's own fp32 `out`"""
    out, targ = b6._d(out), b6._d(targ)
    B = out.shape[0]
    n = B if n is None else n
    beta, kappa = b6.f32(beta), b6.f32(kappa)
    e = out - targ
    s = skewed(e, kappa)
    with np.errstate(divide="ignore", invalid="ignore"):
        P = np.where(e == 0, 0.0, s ** (beta - 1.0))
    rel_alpha0, rel_g0 = loss_rel(beta, B)
    v2 = beta * (s ** beta).sum(axis=0) / n
    inv_beta32 = float(np.float32(1.0) / np.float32(beta))
    lnv = np.abs(np.log(np.where(v2 > 0, v2, 1.0)))
    rel_alpha = rel_alpha0 + lnv * abs(inv_beta32 - 1.0 / beta)
    alpha = v2 ** (1.0 / beta)
    dsde = np.where(e > 0, kappa, 1.0 / kappa)
    g = np.sign(e) * P * beta / alpha ** beta * dsde / n
    rel_g = rel_g0 + beta * rel_alpha
    ea = b6.Expect(alpha, rel_alpha * alpha, (rel_alpha - b6.gamma(B) / beta) * alpha, b6.U * alpha / beta,
                   4.0 * math.sqrt(B))
    eg = b6.Expect(g, rel_g * np.abs(g), (rel_g - b6.gamma(B)) * np.abs(g), b6.U * np.abs(g), 4.0 * math.sqrt(B))
    return eg, ea


def check_step(s, betas, kaps, layers=None):
    """`bounds64.check_step` for a step trained under the vectors `betas` and `kaps`: the loss and alpha reports are
    replaced by one pair per group of columns of equal (beta, kappa), the rest is check_step's own."""
    L = len(s.W) + 1
    reps = [r for r in b6.check_step(s, layers) if not (r.name.startswith("loss ") or r.name == "alpha")]
    for b, k, cols in pairs(betas, kaps):
        eg, ea = expect_loss(s.out[:, cols], s.targ[:, cols], b, k)
        reps.append(b6.compare("loss ML beta_d %g kappa_d %g" % (b, k), s.dedx[L - 1][:, cols], eg))
        reps.append(b6.compare("alpha beta_d %g kappa_d %g" % (b, k), s.alpha[cols], ea))
    return reps


def expect_cv(out, targ, betas, kaps, alpha, gamma_fn):
    """`shapes64.expect_cv_bins` under a skew per column.  sqerr and abserr know neither vector.
    loglik = (d1 - dk) - d2 - d3 with d1, d2 as in expect_cv_bins and
      dk = n sum_d ln((kappa_d + 1/kappa_d) / 2)   the engine adds the D fp32 logf values in double, times n; the
                                                   host-order scalar form rounds the product to fp32 once
      d3 = sum (s(o - t) / alpha_d)^beta_d
    Bounds, term by term:
      d1, d2: expect_cv_bins';
      dk: per bin the argument's two roundings (1/kappa, the sum; the halving is exact) move ln by at most 2u and logf
          is within an ulp, 4u |ln(.)| as expect_cv charges it: n sum_d (2u + 4u |ln(.)|), plus u |dk| for the
          rounding to fp32;
      d3: gamma_N d3 for the sum; per term three roundings of the power's argument (difference, s, division) instead of
          two: sum_d (3 beta_d + 2) u d3_d;
      three subtractions instead of two: 3u (|d1| + |dk| + |d2| + |d3|).
    The tight limit is expect_cv_bins' 4 sqrt(N) + 8 + 2 beta_max plus what the rule adds in units of u x magnitude:
    beta_max (s), 1 (the third subtraction), 1 (dk's rounding) and, since d3 >= N / beta_max at the ML scale while dk's
    per-bin part is 2u N whatever dk is, 2 beta_max: 4 sqrt(N) + 10 + 5 beta_max."""
    out, targ = b6._d(out), b6._d(targ)
    n, D = out.shape
    N = n * D
    res = b6.expect_cv(out, targ)
    e = out - targ
    bt = np.array([b6.f32(v) for v in betas], np.float64)
    kp = np.array([b6.f32(v) for v in kaps], np.float64)
    a = b6._d(alpha)
    Lc = np.array([math.log(v / (2.0 * float(gamma_fn(float(np.float32(1.0 / v)))))) for v in bt])
    Lk = np.log((kp + 1.0 / kp) / 2.0)
    d1 = n * float(Lc.sum())
    dk = n * float(Lk.sum())
    la = np.log(a)
    d2 = n * float(la.sum())
    t3 = ((skewed(e, kp) / a) ** bt).sum(axis=0)
    d3 = float(t3.sum())
    b1 = n * float((b6.U + 4.0 * b6.U * np.abs(Lc)).sum()) + b6.U * abs(d1)
    bk = n * float((2.0 * b6.U + 4.0 * b6.U * np.abs(Lk)).sum()) + b6.U * abs(dk)
    b2 = b6.gamma(D + 3) * n * float(np.abs(la).sum())
    b3 = b6.gamma(N) * d3 + float(((3.0 * bt + 2.0) * b6.U * t3).sum())
    b = b1 + bk + b2 + b3 + 3.0 * b6.U * (abs(d1) + abs(dk) + abs(d2) + abs(d3))
    den = b6.U * (abs(d1) + abs(dk) + abs(d2) + d3)
    res["loglik"] = b6.Expect(np.float64(d1 - dk - d2 - d3), np.float64(b), 0.0, np.float64(den),
                              4.0 * math.sqrt(N) + 10.0 + 5.0 * float(bt.max()))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# the fit
def fit(p_plus, p_minus, beta, n):
    """(kappa, alpha, loglik) of asym_rule.h in float64 for arrays of P+ and P-; NaN / 0 / NaN without a fit"""
    pp, pm = b6._d(p_plus), b6._d(p_minus)
    ok = (pp > 0) & (pm > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        kap = np.where(ok, (pm / np.where(ok, pp, 1.0)) ** (1.0 / (2.0 * (beta + 1.0))), np.nan)
        q = kap ** beta * pp + kap ** -beta * pm
        alpha = np.where(ok, (beta * q / n) ** (1.0 / beta), 0.0)
        ll = n * (math.log(beta) - np.log(kap + 1.0 / kap) - math.lgamma(1.0 / beta) - np.log(alpha) - 1.0 / beta)
    return kap, alpha, np.where(ok, ll, np.nan)


def loglik(e, beta, kappa):
    """the log-likelihood of the errors e [n] under (beta, kappa) with alpha at its ML value, for kappa an array [m]:
    n [ln beta - ln(kappa + 1/kappa) - lgamma(1/beta) - ln alpha - 1/beta], alpha^beta = (beta / n) sum s(e)^beta --
    written from the density, not from the closed form under test"""
    e = b6._d(e)
    k = b6._d(kappa)[:, None]
    n = e.size
    pp = (np.where(e > 0, e, 0.0) ** beta).sum()
    pm = (np.where(e < 0, -e, 0.0) ** beta).sum()
    q = (k[:, 0] ** beta) * pp + (k[:, 0] ** -beta) * pm
    ln_alpha = np.log(beta * q / n) / beta
    return n * (math.log(beta) - np.log(k[:, 0] + 1.0 / k[:, 0]) - math.lgamma(1.0 / beta) - ln_alpha - 1.0 / beta)


def sample(rng, n, beta, kappa, alpha=1.0):
    """n float64 draws from f(e) = beta / (alpha (kappa + 1/kappa) Gamma(1/beta)) exp(-(s(e)/alpha)^beta): the mass of
    e > 0 is (1/kappa) / (kappa + 1/kappa); on either side s/alpha is a GGD magnitude, Gamma(1/beta, 1)^(1/beta)"""
    up = rng.random(n) < (1.0 / kappa) / (kappa + 1.0 / kappa)
    s = alpha * rng.gamma(1.0 / beta, 1.0, n) ** (1.0 / beta)
    return np.where(up, s / kappa, -s * kappa)
