"""The learned GGD scale (BPGpu.set_scale_mode, csrc/scale_rule.h): the rule in float32 numpy, bit for bit, and a float64
statement with bounds, built on tests/bounds64.py and tests/asym64.py as they are.

float32 model.  `step` is scale_rule.h statement by statement in np.float32 (numpy rounds every operation once, nothing
is contracted), with pyoracle.exp_det / pyoracle.pow_det for the two functions and `colsum` for the column sum of
p = s(e)^beta in kernSumcol's order (one running fp32 sum per column, rows added in order): what the one-launch loss
and the MLGGD_LOSS_FUSE=0 pair on one device form.  The data-parallel paths sum in another order, so they equal this
model only where every sum is exact.

float64 statement (`expect_step`).  The state (alpha, v) going in and `out` are the engine's own fp32 values.  With
u = 2^-24, pw = 2u one pow_det call (bounds64.loss_rel), B the rows summed:
  v2 = beta sum s^beta / n   rel_v2 = gamma_B + 2 beta u + pw + 2u     asym64.loss_rel's rel_s and the / n, * beta
  q  = alpha^beta            rel pw                                    alpha and beta are exact inputs
  r  = v2 / q                rel_r = rel_v2 + pw + u
  gl = 1 - r                 E_gl = rel_r |r| + u |gl|
  keep = mu v                u |keep|
  push = eta gl              eta E_gl + u |push|
  v' = keep - push           E_v = the two above + u |v'|;  the clamp is monotone and 1-Lipschitz: E_v stays
  alpha' = alpha exp_det(v') exp_det is within an ulp (<= 2u relative, kernels.hip.h), its argument is off by E_v, the
                             product rounds once: rel = (e^E_v - 1) + 3u
A bin with alpha == 0 seeds: alpha' is asym64.expect_loss's alpha, the closed form under its own bound, and v' = 0
exactly.  No measured tolerance.

The stationary point (`stall`).  On a repeated minibatch with mu = 0 and x = ln alpha - ln alpha*, alpha* = v2^(1/beta),
one step is x' = x - eta g(x) + eps with g(x) = 1 - e^(-beta x) = 1 - beta S / alpha^beta.
  * the computed gl is off g by at most (pw + u) r + u |gl| <= 4u near r = 1 (q's pow, the division; 1 - r is exact for
    r in [1/2, 2]);
  * v' = fl(-eta gl) exactly (keep = +-0), and alpha does not move once exp_det(v') == 1.0f: its last statements are
    y = r + (negligible), y + 1, which rounds to 1 for -2^-25 <= v' <= 2^-24.  So alpha moves, in the right direction,
    while |g| > 2^-24 (1 + 2u) / eta + 4u;
  * a step that moves carries eps <= eps0 = (3 + 4 eta) u: exp_det within an ulp of 1 (<= 2u), the product alpha * ex
    (u), eta times the error of gl (4 eta u);
  * f(x) = x - eta g(x) has f'(x) = 1 - eta beta e^(-beta x) in (0, 1) around 0 for eta beta < 1, so |x| <= R is kept by
    a step when eta g(R) >= eps0.
  Both hold for every |g| above  delta = (2^-24 (1 + 2u) + eps0) / eta + 4u,  so the iteration enters |g| <= delta and
  stays: |ln alpha - ln alpha*| <= -ln(1 - delta) / beta.  `steps_to_stall` counts, in float64 with eps0 added against
  the motion at every step, how many steps a start needs to get there."""
import math

import numpy as np

import asym64 as a6
import bounds64 as b6
from oracle import pyoracle

F = np.float32
LRATE, MOMENTUM, VMAX = 0.05, 0.5, 1.0   # the defaults of mlggd_set_scale_mode


def pow_or_self(x, p):
    """kernels.hip.h pow_or_self on an fp32 array x with one exponent p"""
    x = np.asarray(x, F)
    p = F(p)
    if p == F(1.0):
        return x.copy()
    if p == F(0.0):
        return np.ones_like(x)
    return pyoracle.pow_det(x, p).reshape(x.shape)


def pow_cols(x, betas):
    """x [..., D] ** betas [D], one pow_or_self call per distinct exponent"""
    x = np.asarray(x, F)
    betas = np.asarray(betas, F)
    out = np.empty_like(x)
    for bv in np.unique(betas):
        cols = betas == bv
        out[..., cols] = pow_or_self(x[..., cols], bv)
    return out


def skewed(e, kappas):
    """asym_rule::skewed in fp32: kappa e (e > 0), (-e) / kappa (e < 0), 0"""
    e = np.asarray(e, F)
    k = np.broadcast_to(np.asarray(kappas, F), e.shape)
    with np.errstate(all="ignore"):
        return np.where(e > 0, k * e, np.where(e == 0, F(0.0), (-e) / k)).astype(F)


def colsum(out, targ, betas, kappas=None):
    """[D] fp32 column sums of p = s(out - targ)^beta in kernSumcol's order"""
    e = (np.asarray(out, F) - np.asarray(targ, F)).astype(F)
    mag = np.abs(e) if kappas is None else skewed(e, kappas)
    p = pow_cols(mag, betas)
    s = p[0].copy()
    for b in range(1, p.shape[0]):
        s = (s + p[b]).astype(F)
    return s


def beta_s32(s, nf, beta):
    """scale_rule::beta_s"""
    with np.errstate(all="ignore"):
        v1 = (np.asarray(s, F) / np.asarray(nf, F)).astype(F)
        return (v1 * np.asarray(beta, F)).astype(F)


def velocity32(v2, q, v, eta, mu, vmax):
    """scale_rule::velocity: a NaN passes both selects"""
    v2, q, v, eta, mu, vmax = (np.asarray(a, F) for a in (v2, q, v, eta, mu, vmax))
    with np.errstate(all="ignore"):
        r = (v2 / q).astype(F)
        gl = (F(1.0) - r).astype(F)
        keep = (mu * v).astype(F)
        push = (eta * gl).astype(F)
        vn = (keep - push).astype(F)
        vn = np.where(vn > vmax, vmax, vn).astype(F)
        return np.where(vn < -vmax, -vmax, vn).astype(F)


def advance32(alpha, ex):
    """scale_rule::advance"""
    with np.errstate(all="ignore"):
        return (np.asarray(alpha, F) * np.asarray(ex, F)).astype(F)


def step(alpha, v, s, nf, betas, eta=LRATE, mu=MOMENTUM, vmax=VMAX):
    """One step of scale_rule.h for D bins: (alpha', v', q), all [D] fp32.  q is the denominator of the step's gradient."""
    alpha, v, s, betas = (np.asarray(a, F) for a in (alpha, v, s, betas))
    with np.errstate(all="ignore"):
        v2 = beta_s32(s, nf, betas)
        an, vn, q = np.empty_like(alpha), np.empty_like(alpha), np.empty_like(alpha)
        for bv in np.unique(betas):
            c = betas == bv
            seed = alpha[c] == F(0.0)
            a_seed = pow_or_self(v2[c], F(1.0) / bv)
            q_seed = pow_or_self(a_seed, bv)
            q_run = pow_or_self(alpha[c], bv)
            vv = velocity32(v2[c], q_run, v[c], eta, mu, vmax)
            a_run = advance32(alpha[c], pyoracle.exp_det(vv).reshape(vv.shape))
            an[c] = np.where(seed, a_seed, a_run)
            vn[c] = np.where(seed, F(0.0), vv)
            q[c] = np.where(seed, q_seed, q_run)
    return an, vn, q


# ---------------------------------------------------------------------------------------------------------------------
# float64
def rel_v2(beta, B):
    pw = 2.0 * b6.U
    return b6.gamma(B) + 2.0 * beta * b6.U + pw + 2.0 * b6.U


def expect_step(alpha, v, out, targ, beta, kappa, eta, mu, vmax, n=None):
    """(Expect for alpha', Expect for v') of columns that share one (beta, kappa), module docstring"""
    out, targ = b6._d(out), b6._d(targ)
    alpha, v = b6._d(alpha), b6._d(v)
    B = out.shape[0]
    n = B if n is None else n
    beta, kappa, eta, mu, vmax = (b6.f32(x) for x in (beta, kappa, eta, mu, vmax))
    _, ea_seed = a6.expect_loss(out, targ, beta, kappa, n)
    seed = alpha == 0.0
    a_safe = np.where(seed, 1.0, alpha)
    pw = 2.0 * b6.U
    v2 = beta * (a6.skewed(out - targ, kappa) ** beta).sum(axis=0) / n
    r = v2 / a_safe ** beta
    rel_r = rel_v2(beta, B) + pw + b6.U
    gl = 1.0 - r
    E_gl = rel_r * np.abs(r) + b6.U * np.abs(gl)
    keep, push = mu * v, eta * gl
    raw = keep - push
    E_v = b6.U * np.abs(keep) + eta * E_gl + b6.U * np.abs(push) + b6.U * np.abs(raw)
    vn = np.clip(raw, -vmax, vmax)
    an = a_safe * np.exp(vn)
    rel_a = np.expm1(E_v) + 3.0 * b6.U
    ref_a = np.where(seed, ea_seed.ref, an)
    bound_a = np.where(seed, ea_seed.bound, rel_a * an)
    return b6.Expect(ref_a, bound_a), b6.Expect(np.where(seed, 0.0, vn), np.where(seed, 0.0, E_v))


def expect_grad_fixed(out, targ, beta, kappa, alpha, n=None):
    """dE/dz under a GIVEN scale vector (the frozen mode, and any learned step with q = alpha^beta of the alpha going
    in): asym64.expect_loss's gradient with alpha an exact input, so beta rel(alpha) drops out of its bound"""
    out, targ = b6._d(out), b6._d(targ)
    n = out.shape[0] if n is None else n
    beta, kappa = b6.f32(beta), b6.f32(kappa)
    e = out - targ
    s = a6.skewed(e, kappa)
    with np.errstate(divide="ignore", invalid="ignore"):
        P = np.where(e == 0, 0.0, s ** (beta - 1.0))
    dsde = np.where(e > 0, kappa, 1.0 / kappa)
    g = np.sign(e) * P * beta / b6._d(alpha) ** beta * dsde / n
    _, rel_g0 = a6.loss_rel(beta, out.shape[0])
    return b6.Expect(g, rel_g0 * np.abs(g), 0.0, b6.U * np.abs(g), rel_g0 / b6.U)


def eps0(eta):
    return (3.0 + 4.0 * eta) * b6.U


def stall_delta(eta):
    """|1 - beta S / alpha^beta| at which the fp32 iteration (mu = 0) has stalled, module docstring"""
    return (2.0 ** -24 * (1.0 + 2.0 * b6.U) + eps0(eta)) / eta + 4.0 * b6.U


def stall(eta, beta):
    """the bound on |ln alpha - ln alpha*| after the iteration has stalled"""
    return -math.log(1.0 - stall_delta(eta)) / beta


def steps_to_stall(x0, eta, beta, vmax, limit=10000):
    """steps of x' = x - clamp(eta (1 - e^(-beta x))) from x0 = ln(alpha0 / alpha*) until |x| <= stall(eta, beta), with
    eps0 added against the motion at every step"""
    x, R = float(x0), stall(eta, beta)
    for k in range(limit):
        if abs(x) <= R:
            return k
        vn = max(-vmax, min(vmax, -eta * (1.0 - math.exp(-beta * x))))
        x = x + vn
        x += math.copysign(eps0(eta), x)
    return limit
