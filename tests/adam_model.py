"""The Adam rule of csrc/adam_rule.h restated in numpy: float32, one IEEE operation per line, the step size from running
products in double -- what pkg.adam_apply and the k_adam_apply launch must give bit for bit -- and the textbook form in
float64, the same real function, with a per-element bound on the distance between the two that is derived here from the
operation count (in the manner of bounds64.py; nothing in it is tuned).

    g  = G / nf + wc * w
    m' = b1 * m + c1 * g            c1 = float32(1 - float64(b1))
    v' = b2 * v + (c2 * g) * g      c2 likewise
    w' = w - a_t * (m' / (sqrt(v') + eps))
    a_t = float32(float64(lr) * sqrt(1 - p2_t) / (1 - p1_t)),  p_t = p_{t-1} * float64(b), p_0 = 1

Textbook (Kingma and Ba, algorithm 1): mhat = m' / (1 - b1^t), vhat = v' / (1 - b2^t), w' = w - lr mhat / (sqrt(vhat) +
epshat).  With epshat = eps / sqrt(1 - b2^t) that is lr sqrt(1 - b2^t) / (1 - b1^t) * m' / (sqrt(v') + eps): the rule above
in real numbers."""
import math

import numpy as np

F = np.float32
U = 2.0 ** -24                      # unit roundoff of float32
SPENT = 2.0 ** -60                  # adam_rule::kSpent: below it a product no longer reaches a_t


def complement(b):
    return F(1.0 - float(F(b)))


def products(b1, b2, steps):
    """(b1^steps, b2^steps) by repeated multiplication in double; the loop ends once both are spent, as adam_rule's does"""
    b1, b2 = float(F(b1)), float(F(b2))
    p1 = p2 = 1.0
    t = 0
    while t < steps and (p1 >= SPENT or p2 >= SPENT):
        p1 = p1 * b1
        p2 = p2 * b2
        t += 1
    return p1, p2


def stepsize(lr, b1, b2, steps):
    """a_t of update number `steps` >= 1"""
    p1, p2 = products(b1, b2, steps)
    num = math.sqrt(1.0 - p2)
    den = 1.0 - p1
    return F(float(F(lr)) * num / den)


def step32(w, m, v, G, nf, wc, lr, b1, b2, eps, steps_before):
    """one update of float32 arrays; returns new (w, m, v)"""
    w, m, v, G = (np.asarray(a, F) for a in (w, m, v, G))
    nf, wc, b1, b2, eps = F(nf), F(wc), F(b1), F(b2), F(eps)
    c1, c2 = complement(b1), complement(b2)
    a_t = stepsize(lr, b1, b2, steps_before + 1)
    t1 = G / nf
    t2 = wc * w
    g = t1 + t2
    keep_m = b1 * m
    push_m = c1 * g
    mn = keep_m + push_m
    keep_v = b2 * v
    cg = c2 * g
    push_v = cg * g
    vn = keep_v + push_v
    s = np.sqrt(vn)
    den = s + eps
    q = mn / den
    move = a_t * q
    wn = w - move
    for a in (wn, mn, vn):
        assert a.dtype == F
    return wn, mn, vn


def step64(w, m, v, G, nf, wc, lr, b1, b2, eps, steps_before):
    """the textbook form in float64 on the same (float32-valued) inputs; returns new (w, m, v)"""
    w, m, v, G = (np.asarray(a, np.float64) for a in (w, m, v, G))
    nf, wc, lr, b1, b2, eps = (float(F(x)) for x in (nf, wc, lr, b1, b2, eps))
    t = steps_before + 1
    g = G / nf + wc * w
    mn = b1 * m + (1.0 - b1) * g
    vn = b2 * v + (1.0 - b2) * g * g
    k1, k2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    mhat = mn / k1
    vhat = vn / k2
    wn = w - lr * mhat / (np.sqrt(vhat) + eps / math.sqrt(k2))
    return wn, mn, vn


def gamma(k):
    """(1 + d_1) ... (1 + d_k) - 1 <= gamma(k) for |d_i| <= U"""
    return k * U / (1.0 - k * U)


def bound(w, m, v, G, nf, wc, lr, b1, b2, eps, steps_before):
    """Per-element bounds (dw, dm, dv) on |step32 - step64| for the same inputs, from the rounding of every statement of
    step32.  Each float32 statement is exact times (1 + d), |d| <= U; c1 and c2 carry one rounding of their own; a
    float64 statement's error (2^-53) is covered by the DBL slack.  With A = |G / nf| + |wc w| >= |g|:
      g   : 3 roundings on the deepest chain (/, *, +)                       |dg| <= gamma(2) A    (each term meets 2)
      m'  : + c1's rounding, the product, the sum                            |dm| <= gamma(5) (b1 |m| + (1 - b1) A)
      v'  : g twice (2 x 2), c2's rounding, two products, the sum            |dv| <= gamma(8) (b2 v + (1 - b2) A^2)
      s   : |sqrt(x) - sqrt(y)| <= min(|x - y| / sqrt(y), sqrt(|x - y|)), then one rounding
      den : one sum;  q : one division;  move : a_t's relative error + one product;  w' : one difference
    a_t is float32(a double expression): relative error U plus the double expression's, which the running product makes
    at most (t + 16) 2^-52 over the t <= 2^20 multiplications that still matter (1 - p is then 1).  A bound that cannot
    be given (the denominator's error reaches the denominator) is +inf."""
    w, m, v, G = (np.asarray(a, np.float64) for a in (w, m, v, G))
    nf, wc, lr, b1, b2, eps = (float(F(x)) for x in (nf, wc, lr, b1, b2, eps))
    DBL = 64 * 2.0 ** -53
    t = steps_before + 1
    w64, m64, v64 = step64(w, m, v, G, nf, wc, lr, b1, b2, eps, steps_before)
    A = np.abs(G / nf) + np.abs(wc * w)
    dm = gamma(5) * (b1 * np.abs(m) + (1.0 - b1) * A) + DBL * np.abs(m64)
    dv = gamma(8) * (b2 * v + (1.0 - b2) * A * A) + DBL * v64
    s64 = np.sqrt(v64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ds = np.where(s64 > 0, np.minimum(dv / np.where(s64 > 0, s64, 1.0), np.sqrt(dv)), np.sqrt(dv))
    ds = ds + U * (s64 + ds)
    dden = ds + U * (s64 + eps + ds)
    den64 = s64 + eps
    den_lo = den64 - dden
    ok = den_lo > 0
    safe = np.where(ok, den_lo, 1.0)
    q64 = m64 / den64
    dq = dm / safe + np.abs(m64) * dden / (den64 * safe)
    dq = dq + U * (np.abs(q64) + dq)
    a_t = float(lr) * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)
    ea = U + (min(t, 2 ** 20) + 16) * 2.0 ** -52
    move64 = a_t * np.abs(q64)
    dmove = a_t * (1.0 + ea) * dq + (ea + U + ea * U) * (move64 + a_t * dq)
    dw = dmove + U * (np.abs(w) + move64 + dmove) + DBL * (np.abs(w) + move64)
    dw = np.where(ok, dw, np.inf)
    return dw, dm, dv


class AdamNet:
    """the state of a net under the rule: weights, biases, both moments of each, the step count"""

    def __init__(self, W, b, lr, wc, beta1=0.9, beta2=0.999, eps=1e-8):
        self.W = [np.array(a, F) for a in W]
        self.b = [np.array(a, F) for a in b]
        self.m_w = [np.zeros_like(a) for a in self.W]
        self.v_w = [np.zeros_like(a) for a in self.W]
        self.m_b = [np.zeros_like(a) for a in self.b]
        self.v_b = [np.zeros_like(a) for a in self.b]
        self.lr, self.wc, self.betas, self.eps = lr, wc, (beta1, beta2), eps
        self.steps = 0

    def apply(self, grad_w, grad_b, nf):
        """one update from the summed gradients of a minibatch of nf frames (the weightcost does not reach a bias)"""
        for i in range(len(self.W)):
            self.W[i], self.m_w[i], self.v_w[i] = step32(self.W[i], self.m_w[i], self.v_w[i], grad_w[i], nf, self.wc, self.lr,
                                                         *self.betas, self.eps, self.steps)
            self.b[i], self.m_b[i], self.v_b[i] = step32(self.b[i], self.m_b[i], self.v_b[i], grad_b[i], nf, 0.0, self.lr,
                                                         *self.betas, self.eps, self.steps)
        self.steps += 1


def oracle_gradients(pyoracle, ls, B, beta, ml, W, b, x, t, activation="sigmoid"):
    """(grad_w, grad_b) of one minibatch from an OracleNet built from (W, b), in whichever GEMM order pyoracle is set to:
    forward -> loss_colsum -> loss_grad -> backward.  The net's own rates play no part."""
    net = pyoracle.OracleNet(ls, B, 0.0, 0.0, 0.0, beta, ml, W, b, activation=activation)
    try:
        net.forward(x)
        cs = net.loss_colsum(t) if ml else np.zeros(ls[-1], F)
        net.loss_grad(t, B, cs)
        net.backward(x)
        L = len(ls)
        return [net.tensor("grad_w", l) for l in range(1, L)], [net.tensor("grad_b", l) for l in range(1, L)]
    finally:
        net.close()


def run(pyoracle, case, W, b, x, t, steps=None, model=None):
    """`steps` minibatches of case.B rows of (x, t) under the rule; returns the AdamNet"""
    model = model or AdamNet(W, b, case.lr, case.wc, case.beta1, case.beta2, case.eps)
    B = case.B
    for k in range(case.steps if steps is None else steps):
        rows = slice(k * B, (k + 1) * B)
        gw, gb = oracle_gradients(pyoracle, case.ls, B, case.beta, case.ml, model.W, model.b, x[rows], t[rows], case.activation)
        model.apply(gw, gb, B)
    return model
