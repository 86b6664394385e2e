"""Float64 references with per-element error bounds for every operation of a training step (CPU only).

Each `expect_*` function takes the fp32 INPUTS of one operation -- in the GPU tests the engine's own inputs, read back
through `debug_tensor` -- and returns an `Expect`: the float64 result, a hard per-element bound on the error of any
correct fp32 implementation, and the pieces of a second, tight statistic.  `compare` measures an fp32 result against
it.  Every kernel is thus checked in isolation: errors do not build up across layers (except in `expect_forward_chain`,
the one place where a bound is propagated on purpose), and the bounds stay tight.

Notation: u = 2^-24 (unit roundoff of fp32), gamma_n = n u / (1 - n u), TINY = 2^-149 (the smallest subnormal: the
absolute error of one rounding in the subnormal range is at most TINY / 2).

Hard bounds (first order; every bound is multiplied by (1 + 1e-6), which covers the second-order terms at the sizes
used here, where every sum of relative error coefficients stays below 1e-2):

* sum of n products, any order, one rounding per operation (an MFMA fp32 chain is fmaf, which only rounds less):
  |fl(sum) - sum| <= gamma_{n-1} sum |a||b|.  The forward adds the bias (+1) and the split-K slabs (+S).
* hidden forward + sigmoid: y = sigma(z), z = y_prev W + b.  E_z = gamma_{K+2} (sum |y||w| + |b|);
  |y - sigma(z)| <= sigma'(z) E_z + E_z^2 / 10 (|sigma''| < 0.0963) + 4 u y + 4 TINY.  4 u y is the sigmoid's own
  rounding: exp within 0.96 ulp (<= 1.92 u relative), 1 + e (u), 1 / (.) (u): 3.92 u < 4 u.  One more term:
  1 / (1 + exp(-z)) in fp32 is exactly 0 where exp(-z) overflows
  (z < -88.72283, the reference's kernSigmoid included), while sigma(z) there is a subnormal up to 2.9e-39; where
  z - E_z is below that threshold, y = 0 is allowed (the bound includes y itself).
* output layer: gamma_{K+S+2} (sum |y||w| + |b|).
* loss gradient dE/dz_L (`expect_loss`): a derived relative bound per element, see there.  e == 0 gives exactly 0.
* dX + Dsigmoid: dedx = (d W^T) * y (1 - y) with the engine's own y: y (1 - y) gamma_{N+2} sum |d||w| + 4 u |ref| +
  3 TINY (1 - y, y (1 - y), the product: three roundings, each may land in the subnormal range).
* dW + update: D' = mu D - lr (G / n + wc W), G = Y^T dEdX:
  lr gamma_B sum |y||d| / n + 6 u (|mu D| + lr |G| / n + lr wc |W|) + 2 TINY.
* bias update: d' = mu d - lr sum_b dEdX / n (no weight cost, BP_GPU.cu:435): the same with sum |d|.
* weight apply: W' = fl32(W + D') exactly (one IEEE add).
* CV sums: see `expect_cv`.

Data-parallel steps (one process per rank, or ranks emulated on one device): rows are independent up to the loss, so
the ranks' rows stacked in rank order -- world x B rows of x, y, out and dedx, each rank's read back where it produced
them -- form one step of n = world B rows, and `check_step` applies unchanged.  What the ranks do differently is only
the ORDER of the sums over frames, which the any-order bounds above already cover:
* dW / G on the all-reduce path: each rank's fp32 chain over its B frames, then world - 1 adds of the partial sums
  (Gpre + G, k_accum, or the collective's own order).  Along any path of that tree an element's product meets at most
  (B - 1) + (world - 1) <= n - 1 roundings, so |fl - exact| <= gamma_{n-1} sum |y||d| <= the gamma_B-of-n term of
  `expect_dw` / `expect_grad`.  The gather modes form the sum over all n frames in one chain: the same bound.
* a division by n taken per rank before the sum (G_r / n, then the adds) adds one rounding per term: gamma_n, which the
  bound of `expect_dw` (gamma_n for the GEMM, 6u of slack for the update) contains.
* the ML column sums met in rank order (k_colsum per rank, then k_accum, or the all-reduce): a sum of n non-negative
  terms in some order, gamma_{n-1} <= gamma_n of `loss_rel` -- evaluated at n = world B rows, which `expect_loss`
  does when it is given the stacked output.  The 1/n of the gradient and of alpha is the global n on every rank.
* the update (k_apply_update: fl(G / n), the same four operations as the fused epilogue) is the 6u slack of `expect_dw`.
So a data-parallel step needs no new bound; `expect_grad` adds the summed gradient G itself (before k_apply_update).

Dropout (training, one device): y = mask * sigma(z), no rescale, the same mask on the row-major and the transposed copy
of each layer; `expect_dropout_layer` expects exactly 0 where a unit was dropped and the sigmoid bound elsewhere.  The
mask is read off the engine's own y (y == 0 where the bound does not allow 0); `mask_stats` then holds it to binomial
limits (rate, per unit, per frame, overlap between masks), so that a mask read off wrongly -- or drawn wrongly -- shows.
CV under dropout (`cv_dropout_weights`): bunch j runs on fl32(W_j keep) with W_{j+1} = fl32(fl32(W_j keep) fl32(1/keep))
exactly (k_scale before and after each GEMM); the outputs go to `expect_forward_chain`, the weights compare exactly.

Tight statistic: err minus the non-GEMM part of the bound, divided by u times the GEMM's sum of |a||b| (scaled as the
element is), maximised over the tensor and asserted <= 4 sqrt(K + S).  A correct fp32 dot product of K terms sits at
a few units of this (the rounding errors of a chain do not all point one way); an order-preserving loss of precision
-- operands truncated to a 10-bit mantissa, a slab summed twice with small values -- moves it by orders of magnitude
while the hard bound, which is worst case, may still hold.
"""
import math
from dataclasses import dataclass, field

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149
EXP_OVF = 88.72283          # exp(-z) of the sigmoid is +inf in fp32 for -z above this (kernels.hip.h exp_det)
SECOND_ORDER = 1.0 + 1e-6


def gamma(n):
    n = float(n)
    return n * U / (1.0 - n * U)


def f32(v):
    """the fp32 value of a hyperparameter, as a float64 (the engine computes with fp32 lrate / momentum / ...)"""
    return float(np.float32(v))


def _d(a):
    return np.asarray(a, np.float64)


@dataclass
class Expect:
    ref: np.ndarray           # float64 result
    bound: np.ndarray         # hard per-element bound on |fp32 - ref|
    slack: np.ndarray = 0.0   # the part of `bound` that is not the GEMM's (subtracted before the tight ratio)
    den: np.ndarray = None    # u x the GEMM's sum |a||b| per element (None: no tight statistic)
    limit: float = math.inf   # the tight statistic's limit


@dataclass
class Report:
    name: str
    count: int                # elements over the hard bound
    size: int
    hard: float               # worst err / bound
    tight: float              # worst (err - slack) / den
    limit: float
    where: list = field(default_factory=list)   # first violating indices

    @property
    def ok(self):
        return self.count == 0 and self.tight <= self.limit

    def line(self):
        return "%-34s hard %8.4f  tight %8.2f / %-8.1f viol %d/%d%s" % (
            self.name, self.hard, self.tight, self.limit, self.count, self.size,
            (" at %s" % self.where) if self.where else "")

    def __str__(self):
        return self.line()


def compare(name, got, exp, show=5):
    """fp32 `got` against `exp`: count of elements over the hard bound, worst hard ratio, worst tight ratio and the
    first few violating (row, col) indices.  NaN / inf in `got` count as violations."""
    got = _d(got)
    ref = np.broadcast_to(_d(exp.ref), got.shape)
    bound = np.broadcast_to(_d(exp.bound) * SECOND_ORDER, got.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got - ref)
    err = np.where(np.isfinite(err), err, np.inf)
    bad = err > bound
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    tight = 0.0
    if exp.den is not None:
        den = np.broadcast_to(_d(exp.den), got.shape)
        excess = np.maximum(err - np.broadcast_to(_d(exp.slack), got.shape) * SECOND_ORDER, 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = np.where(den > 0, excess / np.where(den > 0, den, 1.0), np.where(excess > 0, np.inf, 0.0))
        tight = float(t.max()) if t.size else 0.0
    where = [tuple(int(i) for i in ix) for ix in np.argwhere(bad)[:show]]
    return Report(name, int(bad.sum()), int(got.size), float(ratio.max()) if ratio.size else 0.0, tight,
                  float(exp.limit), where)


# ---------------------------------------------------------------------------------------------------------------------
# values the tests feed in
def make_net(ls, seed, bias=0.5):
    """Glorot-uniform weights (synth.make_weights' rule) and NON-zero biases U(+-bias), so that a bias slip shows"""
    rng = np.random.default_rng(seed)
    W, b = [], []
    for k, n in zip(ls[:-1], ls[1:]):
        r = 2.0 * np.sqrt(6.0) / np.sqrt(k + n)
        W.append(rng.uniform(-r, r, (k, n)).astype(np.float32))
        b.append(rng.uniform(-bias, bias, n).astype(np.float32))
    return W, b


def make_data(ls, n, seed, sat_rows=0, W1=None, B=None):
    """n rows; the first `sat_rows` rows of every bunch of B scaled so that the first layer's pre-activations reach
    both saturations of sigma and its subnormal band; target column 0 of magnitude 1e3"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, ls[0])).astype(np.float32)
    for i in range(0, n, B or n):
        if sat_rows:
            s = 60.0 / float(np.std(x[i:i + sat_rows] @ W1))
            x[i:i + sat_rows] = (x[i:i + sat_rows] * np.float32(s)).astype(np.float32)
    t = rng.standard_normal((n, ls[-1])).astype(np.float32)
    t[:, 0] = (t[:, 0] * np.float32(1e3)).astype(np.float32)
    return x, t


# ---------------------------------------------------------------------------------------------------------------------
# forward
def _sigmoid64(z):
    """sigma(z) and sigma'(z) in float64 without overflow"""
    ez = np.exp(-np.abs(z))
    y = np.where(z >= 0, 1.0 / (1.0 + ez), ez / (1.0 + ez))
    return y, ez / (1.0 + ez) ** 2


def expect_linear(x, W, b, slabs=1):
    """output layer z = x W + b (split-K: `slabs` partial sums added in some order, then the bias)"""
    x, W, b = _d(x), _d(W), _d(b)
    K = W.shape[0]
    scale = np.abs(x) @ np.abs(W) + np.abs(b)
    return Expect(x @ W + b, gamma(K + slabs + 2) * scale, 0.0, U * scale, 4.0 * math.sqrt(K + slabs))


def _sigmoid_expect(z, Ez, scale_den, K):
    y, sp = _sigmoid64(z)
    ovf = (z - Ez) <= -EXP_OVF                      # exp(-z) may overflow: y = 0 is the fp32 formula's result
    # the tight statistic leaves out the worst-case second-order term E_z^2/10: |sigma''| <= sigma', so for the
    # actual error of z (a few u x scale) that term is negligible next to sigma' x (the GEMM's error)
    slack = 4.0 * U * y + 4.0 * TINY + np.where(ovf, y, 0.0)
    return Expect(y, sp * Ez + Ez * Ez / 10.0 + slack, slack, U * sp * scale_den, 4.0 * math.sqrt(K))


def expect_sigmoid_layer(x, W, b):
    """hidden layer y = sigma(x W + b) (k_fwd<SIGMOID>, k_fwd64): inputs exact (the engine's own fp32 inputs)"""
    x, W, b = _d(x), _d(W), _d(b)
    K = W.shape[0]
    scale = np.abs(x) @ np.abs(W) + np.abs(b)
    return _sigmoid_expect(x @ W + b, gamma(K + 2) * scale, scale, K)


def expect_forward_chain(x, Ws, bs, slabs=1, x_err=0.0):
    """out of a whole forward pass (forward(), CV): the layers chain, so each input's error bound is propagated:
    E_z = E_y |W| + gamma_{K+2} ((|y| + E_y) |W| + |b|),  E_y = sigma'(z) E_z + E_z^2/10 + 4 u y + 4 TINY (+ y where
    exp may overflow).  The tight statistic is measured against the first-order GEMM part of the final bound.
    x_err: a bound on the error of the fp32 input itself against the float64 `x` (scalar or per element; the input
    enters as E_y of layer 0), e.g. the roundings of the normalisation in front of the network (spec64.decode64)."""
    y = _d(x)
    Ey = np.zeros_like(y) + _d(x_err)
    L = len(Ws)
    for i, (W, b) in enumerate(zip(Ws, bs)):
        W, b = _d(W), _d(b)
        K = W.shape[0]
        aW = np.abs(W)
        prop = Ey @ aW
        last = i == L - 1
        scale = (np.abs(y) + Ey) @ aW + np.abs(b)
        z = y @ W + b
        Ez = prop + gamma(K + (slabs if last else 0) + 2) * scale
        if last:
            return Expect(z, Ez)   # a propagated bound: no tight statistic
        e = _sigmoid_expect(z, Ez, scale, K)
        y, Ey = e.ref, e.bound


# ---------------------------------------------------------------------------------------------------------------------
# loss
def loss_rel(beta, ml, B):
    """Relative error bounds (first order) of the loss chain.  pw = 2u is one pow_det call (<= 1 ulp,
    tests/test_gpu_loss_ulps.py; an ulp is at most 2u relative).  e = fl(o - t): u.
      p = |e|^beta               : beta u + pw
      s = sum_B p (p >= 0)       : gamma_B + beta u + pw
      v2 = (s / n) * beta        : + 2u
      alpha = v2^fl(1/beta)      : rel(v2) / beta + pw + |ln v2| |fl(1/beta) - 1/beta|  (the last term per column)
      q = alpha^beta             : beta rel(alpha) + pw
      P = |e|^(beta - 1)         : |beta - 1| u + pw        (beta - 1 is exact: Sterbenz)
      g = P * beta / q * fl(1/n) : rel(P) + rel(q) + 4u (ML);   beta * P * fl(1/n): rel(P) + 3u (MMSE)
    Returns (rel(alpha) without the exponent term, rel(g) without the beta rel(alpha) term)."""
    pw = 2.0 * U
    rel_P = abs(beta - 1.0) * U + pw
    if ml != 1:
        return None, rel_P + 3.0 * U
    rel_s = gamma(B) + beta * U + pw
    return (rel_s + 2.0 * U) / beta + pw, rel_P + 4.0 * U + pw


def expect_loss(out, targ, beta, ml, n=None):
    """dE/dz of the output layer (k_loss_norm, k_loss_ml, k_loss_err + k_colsum + k_loss_grad) from the engine's own
    fp32 `out`: the float64 value of tests/ref64.py's loss_grad (alpha from the column sums, 1/n) with the fp32
    shapefactor.  Returns (Expect for the gradient, Expect for alpha or None)."""
    out, targ = _d(out), _d(targ)
    B = out.shape[0]
    n = B if n is None else n
    beta = f32(beta)
    e = out - targ
    ae = np.abs(e)
    with np.errstate(divide="ignore", invalid="ignore"):
        P = np.where(e == 0, 0.0, ae ** (beta - 1.0))
    rel_alpha0, rel_g0 = loss_rel(beta, ml, B)
    if ml == 1:
        v2 = beta * (ae ** beta).sum(axis=0) / n
        inv_beta32 = float(np.float32(1.0) / np.float32(beta))
        lnv = np.abs(np.log(np.where(v2 > 0, v2, 1.0)))
        rel_alpha = rel_alpha0 + lnv * abs(inv_beta32 - 1.0 / beta)
        alpha = v2 ** (1.0 / beta)
        g = np.sign(e) * P * beta / alpha ** beta / n
        rel_g = rel_g0 + beta * rel_alpha
        # tight: the column sum's part (gamma_B in both) measured in units of u -- err(s) / (u s) <= 4 sqrt(B)
        ea = Expect(alpha, rel_alpha * alpha, (rel_alpha - gamma(B) / beta) * alpha, U * alpha / beta,
                    4.0 * math.sqrt(B))
        eg = Expect(g, rel_g * np.abs(g), (rel_g - gamma(B)) * np.abs(g), U * np.abs(g), 4.0 * math.sqrt(B))
        return eg, ea
    g = np.sign(e) * beta * P / n
    # elementwise only: the tight statistic is the error in units of u|g| against the same fixed count
    return Expect(g, rel_g0 * np.abs(g), 0.0, U * np.abs(g), rel_g0 / U), None


# ---------------------------------------------------------------------------------------------------------------------
# backward
def expect_dx(d_next, W_next, y):
    """dEdX_l = (dEdX_{l+1} W_{l+1}^T) * y_l (1 - y_l) (k_dx<4,4>, k_dx64), with the engine's own y_l"""
    d, W, y = _d(d_next), _d(W_next), _d(y)
    N = W.shape[1]
    sp = y * (1.0 - y)
    sc = np.abs(d) @ np.abs(W).T
    ref = (d @ W.T) * sp
    slack = 4.0 * U * np.abs(ref) + 3.0 * TINY
    return Expect(ref, sp * gamma(N + 2) * sc + slack, slack, U * sp * sc, 4.0 * math.sqrt(N))


def expect_dw(y_prev, d, W_old, dW_old, lr, mom, wc, n=None):
    """delta_w' = mom delta_w - lr (Y^T dEdX / n + wc W) (k_dwp fused; k_dwp<., false> + k_apply_update)"""
    y, d, W, D = _d(y_prev), _d(d), _d(W_old), _d(dW_old)
    B = y.shape[0]
    n = B if n is None else n
    lr, mom, wc = f32(lr), f32(mom), f32(wc)
    G = y.T @ d
    GS = np.abs(y).T @ np.abs(d)
    ref = mom * D - lr * (G / n + wc * W)
    slack = 6.0 * U * (np.abs(mom * D) + lr * np.abs(G) / n + lr * wc * np.abs(W)) + 2.0 * TINY
    return Expect(ref, lr * gamma(B) * GS / n + slack, slack, U * lr * GS / n, 4.0 * math.sqrt(B))


def expect_db(d, db_old, lr, mom, n=None):
    """delta_b' = mom delta_b - lr sum_frames dEdX / n (weight cost not applied to biases, BP_GPU.cu:435)"""
    d, D = _d(d), _d(db_old)
    B = d.shape[0]
    n = B if n is None else n
    lr, mom = f32(lr), f32(mom)
    g = d.sum(axis=0)
    gs = np.abs(d).sum(axis=0)
    ref = mom * D - lr * g / n
    slack = 6.0 * U * (np.abs(mom * D) + lr * np.abs(g) / n) + 2.0 * TINY
    return Expect(ref, lr * gamma(B) * gs / n + slack, slack, U * lr * gs / n, 4.0 * math.sqrt(B))


def apply_exact(W_old, delta_new):
    """W' = fl32(W + delta'): the one IEEE add of kernAccSum -- the engine's result must equal this bit for bit"""
    return (np.asarray(W_old, np.float32) + np.asarray(delta_new, np.float32)).astype(np.float32)


def compare_exact(name, got, want, show=5):
    got = np.asarray(got, np.float32)
    want = np.asarray(want, np.float32)
    bad = got.view(np.uint32) != want.view(np.uint32)
    where = [tuple(int(i) for i in ix) for ix in np.argwhere(bad)[:show]]
    return Report(name, int(bad.sum()), int(got.size), float(np.inf if bad.any() else 0.0), 0.0, 0.0, where)


# ---------------------------------------------------------------------------------------------------------------------
# CV
def expect_cv(out, targ, beta=None, alpha=None, gamma_fn=None):
    """The three CV numbers (CrossValid, CrossValiddB, CrossValid2; host order and k_cv_reduce) from the engine's own
    forward() output `out` [n][D] in float64.  Bounds (N = n D terms):
      sqerr  = sum (o - t)^2     : each term 3u (difference, square), the sum gamma_{N}: gamma_{N+3} sum
      abserr = sum |o - t| / D   : gamma_{N+2} sum / D
      loglik = d1 - d2 - d3 with d1 = N ln(beta / (2 Gamma(fl(1/beta)))) (Gamma: the engine's polynomial, gamma_fn),
               d2 = n sum_u ln alpha_u (alpha: the engine's scalefactor), d3 = sum (|t - o| / alpha)^beta:
               d1: N (u + 4u |ln(.)|) + u |d1| (logf <= 1 ulp, its argument one division, N as a float);
               d2: gamma_{D+3} n sum |ln alpha|;  d3: (gamma_N + (2 beta + 2) u) d3 (difference, division, one pow
               within 1 ulp of a perturbed argument);  the two subtractions: 2u (|d1| + |d2| + |d3|).
    Returns {name: Expect} with scalar entries."""
    out, targ = _d(out), _d(targ)
    n, D = out.shape
    N = n * D
    e = out - targ
    sq = float((e * e).sum())
    ab = float(np.abs(e).sum())
    res = {
        "sqerr": Expect(np.float64(sq), np.float64(gamma(N + 3) * sq), 0.0, np.float64(U * sq), 4.0 * math.sqrt(N)),
        "abserr": Expect(np.float64(ab / D), np.float64(gamma(N + 2) * ab / D), 0.0, np.float64(U * ab / D),
                         4.0 * math.sqrt(N)),
    }
    if alpha is not None:
        beta = f32(beta)
        a = _d(alpha)
        G = float(gamma_fn(float(np.float32(1.0 / beta))))
        Lc = math.log(beta / (2.0 * G))
        d1 = N * Lc
        la = np.log(a)
        d2 = n * float(la.sum())
        t3 = (np.abs(e) / a) ** beta
        d3 = float(t3.sum())
        b1 = N * (U + 4.0 * U * abs(Lc)) + U * abs(d1)
        b2 = gamma(D + 3) * n * float(np.abs(la).sum())
        b3 = (gamma(N) + (2.0 * beta + 2.0) * U) * d3
        b = b1 + b2 + b3 + 2.0 * U * (abs(d1) + abs(d2) + abs(d3))
        den = U * (abs(d1) + abs(d2) + d3)
        res["loglik"] = Expect(np.float64(d1 - d2 - d3), np.float64(b), 0.0, np.float64(den),
                               4.0 * math.sqrt(N) + 8.0 + 2.0 * beta)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# one training step, every operation against its own inputs
@dataclass
class Step:
    """What one training step took and produced.  Lists are indexed by layer - 1 (layer l = 1..L-1 of the engine);
    `y` and `dedx` are dicts by layer.  W, b, dW, db: before the step; *_new: after it."""
    x: np.ndarray
    targ: np.ndarray
    W: list
    b: list
    dW: list
    db: list
    y: dict
    out: np.ndarray
    dedx: dict
    dW_new: list
    db_new: list
    W_new: list
    b_new: list
    lr: float
    mom: float
    wc: float
    beta: float
    ml: int
    slabs: int = 1
    alpha: np.ndarray = None
    dropout: bool = False     # hidden layers masked (training with dropoutflag): `expect_dropout_layer`


def check_step(s, layers=None):
    """Reports for every operation of the step `s` (layers: the set of layers whose forward, dX, dW and updates are
    checked; the loss always is)."""
    L = len(s.W) + 1
    layers = set(range(1, L)) if layers is None else set(layers)
    yin = lambda l: s.x if l == 1 else s.y[l - 1]
    reps = []
    for l in sorted(layers):
        if l < L - 1 and s.dropout:
            reps.append(compare("fwd %d" % l, s.y[l], expect_dropout_layer(yin(l), s.W[l - 1], s.b[l - 1], s.y[l])[0]))
        elif l < L - 1:
            reps.append(compare("fwd %d" % l, s.y[l], expect_sigmoid_layer(yin(l), s.W[l - 1], s.b[l - 1])))
        else:
            reps.append(compare("out (S=%d)" % s.slabs, s.out, expect_linear(yin(l), s.W[l - 1], s.b[l - 1], s.slabs)))
    eg, ea = expect_loss(s.out, s.targ, s.beta, s.ml)
    reps.append(compare("loss %s beta %g" % ("ML" if s.ml == 1 else "MMSE", s.beta), s.dedx[L - 1], eg))
    if ea is not None and s.alpha is not None:
        reps.append(compare("alpha", s.alpha, ea))
    for l in sorted(layers):
        if l < L - 1:
            reps.append(compare("dx %d" % l, s.dedx[l], expect_dx(s.dedx[l + 1], s.W[l], s.y[l])))
        reps.append(compare("dw %d" % l, s.dW_new[l - 1],
                            expect_dw(yin(l), s.dedx[l], s.W[l - 1], s.dW[l - 1], s.lr, s.mom, s.wc)))
        reps.append(compare("db %d" % l, s.db_new[l - 1], expect_db(s.dedx[l], s.db[l - 1], s.lr, s.mom)))
        reps.append(compare_exact("apply W %d" % l, s.W_new[l - 1], apply_exact(s.W[l - 1], s.dW_new[l - 1])))
        reps.append(compare_exact("apply b %d" % l, s.b_new[l - 1], apply_exact(s.b[l - 1], s.db_new[l - 1])))
    return reps


# ---------------------------------------------------------------------------------------------------------------------
# data parallel
def expect_grad(y_prev, d):
    """G_l = Y^T dEdX over the whole minibatch, what the all-reduce path holds before k_apply_update (dEdX carries the
    1/n already): any order of the n products (per-rank chains, then the adds): gamma_n sum |y||d|; the products may
    underflow, n TINY / 2 more"""
    y, d = _d(y_prev), _d(d)
    n = y.shape[0]
    GS = np.abs(y).T @ np.abs(d)
    slack = n * TINY / 2.0
    return Expect(y.T @ d, gamma(n) * GS + slack, slack, U * GS, 4.0 * math.sqrt(n))


# ---------------------------------------------------------------------------------------------------------------------
# dropout
def expect_dropout_layer(x, W, b, y):
    """hidden layer under dropout: y = mask * sigma(x W + b), no rescale.  The mask is read off the engine's own `y`: a
    unit is dropped where y == 0 and the sigmoid bound does not allow 0.  Returns (Expect, dropped, known): exactly 0
    with a zero bound where dropped, the sigmoid bound elsewhere; `known` marks where the mask is determined (False
    where sigma may round to 0 anyway: there a dropped and a kept unit look alike).  Where the mask is unknown and
    y == 0, the unit may have been dropped: its error |0 - sigma(z)| is then no rounding error, so it joins the slack
    (the tight statistic measures the GEMM's rounding only); the hard bound already allows it (bound >= sigma(z))."""
    e = expect_sigmoid_layer(x, W, b)
    allow0 = e.ref - e.bound * SECOND_ORDER <= 0.0
    y0 = np.asarray(y) == 0
    drop = y0 & ~allow0
    z = lambda a: np.where(drop, 0.0, np.broadcast_to(a, drop.shape))
    slack = np.where(y0 & allow0, np.maximum(e.slack, e.ref), e.slack)
    return Expect(z(e.ref), z(e.bound), z(slack), z(e.den), e.limit), drop, ~allow0


def input_mask(x_raw, x_seen):
    """the input layer's mask from the raw rows and the rows the kernels consumed: every element is either untouched
    or exactly 0.  Returns (Report of elements that are neither, dropped, known)"""
    x_raw, x_seen = np.asarray(x_raw, np.float32), np.asarray(x_seen, np.float32)
    same = x_seen.view(np.uint32) == x_raw.view(np.uint32)
    drop = (x_seen == 0) & (x_raw != 0)
    bad = ~same & ~drop
    where = [tuple(int(i) for i in ix) for ix in np.argwhere(bad)[:5]]
    return Report("x = raw or 0", int(bad.sum()), int(bad.size), float(np.inf if bad.any() else 0.0), 0.0, 0.0,
                  where), drop, x_raw != 0


def _zreport(name, z, size):
    """a binomial statistic as a Report: hard = |z| / 6 (6 sigma), one violation when it exceeds 1"""
    h = abs(float(z)) / 6.0
    return Report(name, int(not h <= 1.0), size, h, 0.0, 0.0)


def _dispersion(c, n, p):
    """chi-square of counts c out of n (per unit or per frame) against Binomial(n, p), as a z-score: each standardised
    square has mean 1 and variance 2 + (1 - 6pq) / (npq)"""
    keep = n > 0
    c, n = c[keep].astype(np.float64), n[keep].astype(np.float64)
    q = 1.0 - p
    chi = ((c - n * p) ** 2 / (n * p * q)).sum()
    var = (2.0 + (1.0 - 6.0 * p * q) / (n * p * q)).sum()
    return (chi - keep.sum()) / math.sqrt(var)


def mask_stats(name, drop, known, p):
    """a dropout mask [frames][units] (True = dropped) against independent Bernoulli(p) draws, on the elements where
    it is known: the rate, the dispersion of the counts per unit and per frame (a hash of only the frame or only the
    unit makes them all-or-nothing)"""
    drop, known = np.asarray(drop, bool) & known, np.asarray(known, bool)
    n = int(known.sum())
    k = int(drop.sum())
    reps = [_zreport("%s rate %.4f" % (name, k / max(n, 1)), (k - n * p) / math.sqrt(n * p * (1.0 - p)), n)]
    reps.append(_zreport("%s per unit" % name, _dispersion(drop.sum(0), known.sum(0), p), n))
    reps.append(_zreport("%s per frame" % name, _dispersion(drop.sum(1), known.sum(1), p), n))
    return reps


def mask_overlap(name, d1, k1, d2, k2, p1, p2):
    """two masks that should be independent (consecutive steps, two layers, two seeds) on their common [frames][units]
    corner: the fraction dropped in both is p1 p2"""
    r, c = min(d1.shape[0], d2.shape[0]), min(d1.shape[1], d2.shape[1])
    known = k1[:r, :c] & k2[:r, :c]
    both = int((d1[:r, :c] & d2[:r, :c] & known).sum())
    n, pp = int(known.sum()), p1 * p2
    return _zreport("%s overlap %.4f" % (name, both / max(n, 1)), (both - n * pp) / math.sqrt(n * pp * (1.0 - pp)), n)


def cv_dropout_weights(W, keeps, bunches):
    """forward() under dropout scales W_l by keep_l before its GEMM and by fl32(1/keep_l) after it (k_scale; the
    reference's kernWeightMultiP, BP_GPU.cu:484-501).  Returns ([the weights bunch j's GEMMs read, j < bunches], the
    weights left behind), exactly in fp32"""
    F = np.float32
    cur = [np.asarray(w, F).copy() for w in W]
    used = []
    for _ in range(bunches):
        sc = [(w * F(k)).astype(F) for w, k in zip(cur, keeps)]
        used.append(sc)
        cur = [(s * (F(1) / F(k))).astype(F) for s, k in zip(sc, keeps)]
    return used, cur
