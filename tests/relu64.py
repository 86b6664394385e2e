"""Float64 expectations with hard per-element bounds for rectified-linear hidden units (CPU only): the counterpart of
tests/bounds64.py's sigmoid entries, built on it (same notation: u = 2^-24, gamma_n = n u / (1 - n u)).

The engine's rules (csrc/kernels.hip.h relu4 / drelu): x = sum + bias in fp32, y = (x < 0) ? 0 : x; dE/dx = (y > 0) ?
dE/dy : 0.  Both are a comparison and a select: no rounding of their own.

* hidden forward: z = y_prev W + b, E_z = gamma_{K+2} (sum |y||w| + |b|) as for the sigmoid layer.  max(., 0) is exact
  and 1-Lipschitz, so |y - max(z, 0)| <= E_z; and where z + E_z < 0 the fp32 pre-activation is negative whatever the
  order of its sum, so y must be EXACTLY 0 there (bound 0).  Near z = 0 the fp32 and the float64 sign may differ: then
  one side is 0 and the other within E_z of it, which the bound allows.  The tight statistic of bounds64 (the error in
  units of u sum |y||w|, <= 4 sqrt(K)) applies unchanged: the whole bound is the GEMM's.
* dX: with the engine's own y (as `bounds64.expect_dx`), exactly 0 where y <= 0; elsewhere gamma_{N+2} sum |d||w|, with no
  extra rounding (the select passes the sum through).
* everything that is not an activation -- the output layer, the loss, dW, db, the weight add -- is bounds64's.

`check_step_relu` checks each kernel in isolation on the engine's own inputs, like `bounds64.check_step`.  `step64` is
a whole training step of a ReLU net in float64 (the loss gradient is bounds64.expect_loss's reference value): what the
exact-data test compares with bit for bit, and what the CPU tests use to show that a case is not degenerate."""
import math

import numpy as np

import bounds64 as b6
from bounds64 import Expect, U, _d, compare, compare_exact, gamma

# the per-kernel case of tests/test_gpu_relu.py (checked for degeneracy on the CPU in tests/test_relu_model.py)
CASE_LS = [45, 70, 33, 9]
CASE_SEED = 3
CASE_HP = (0.01, 0.9, 1e-5)
ZERO_FRACTION = (0.2, 0.8)


def expect_relu_layer(x, W, b):
    """hidden layer y = max(x W + b, 0) (k_fwd<FWD_RELU>, k_fwd64<FWD_RELU>): inputs exact (the engine's own)"""
    x, W, b = _d(x), _d(W), _d(b)
    K = W.shape[0]
    scale = np.abs(x) @ np.abs(W) + np.abs(b)
    z = x @ W + b
    Ez = gamma(K + 2) * scale
    off = z + Ez < 0                              # negative in fp32 whatever the order: exactly 0
    return Expect(np.maximum(z, 0.0), np.where(off, 0.0, Ez), 0.0, np.where(off, 0.0, U * scale), 4.0 * math.sqrt(K))


def expect_dx_relu(d_next, W_next, y):
    """dEdX_l = (dEdX_{l+1} W_{l+1}^T) where y_l > 0, exactly 0 elsewhere (k_dx<., ., ACT_RELU>, k_dx64<ACT_RELU>), with
    the engine's own y_l"""
    d, W, y = _d(d_next), _d(W_next), _d(y)
    N = W.shape[1]
    on = y > 0
    sc = np.abs(d) @ np.abs(W).T
    return Expect(np.where(on, d @ W.T, 0.0), np.where(on, gamma(N + 2) * sc, 0.0), 0.0, np.where(on, U * sc, 0.0),
                  4.0 * math.sqrt(N))


def expect_relu_dropout_layer(x, W, b, dropped):
    """hidden layer under dropout with the mask given ([frames][units], True = dropped): exactly 0 there, the plain ReLU
    bound on the masked inputs elsewhere"""
    e = expect_relu_layer(x, W, b)
    z = lambda a: np.where(dropped, 0.0, np.broadcast_to(a, dropped.shape))
    return Expect(z(e.ref), z(e.bound), 0.0, z(e.den), e.limit)


def check_step_relu(s, layers=None):
    """`bounds64.check_step` for a ReLU net: reports for every operation of the step `s` (a bounds64.Step)"""
    L = len(s.W) + 1
    layers = set(range(1, L)) if layers is None else set(layers)
    yin = lambda l: s.x if l == 1 else s.y[l - 1]
    reps = []
    for l in sorted(layers):
        if l < L - 1:
            reps.append(compare("relu fwd %d" % l, s.y[l], expect_relu_layer(yin(l), s.W[l - 1], s.b[l - 1])))
        else:
            reps.append(compare("out (S=%d)" % s.slabs, s.out, b6.expect_linear(yin(l), s.W[l - 1], s.b[l - 1], s.slabs)))
    eg, ea = b6.expect_loss(s.out, s.targ, s.beta, s.ml)
    reps.append(compare("loss %s beta %g" % ("ML" if s.ml == 1 else "MMSE", s.beta), s.dedx[L - 1], eg))
    if ea is not None and s.alpha is not None:
        reps.append(compare("alpha", s.alpha, ea))
    for l in sorted(layers):
        if l < L - 1:
            reps.append(compare("relu dx %d" % l, s.dedx[l], expect_dx_relu(s.dedx[l + 1], s.W[l], s.y[l])))
        reps.append(compare("dw %d" % l, s.dW_new[l - 1],
                            b6.expect_dw(yin(l), s.dedx[l], s.W[l - 1], s.dW[l - 1], s.lr, s.mom, s.wc)))
        reps.append(compare("db %d" % l, s.db_new[l - 1], b6.expect_db(s.dedx[l], s.db[l - 1], s.lr, s.mom)))
        reps.append(compare_exact("apply W %d" % l, s.W_new[l - 1], b6.apply_exact(s.W[l - 1], s.dW_new[l - 1])))
        reps.append(compare_exact("apply b %d" % l, s.b_new[l - 1], b6.apply_exact(s.b[l - 1], s.db_new[l - 1])))
    return reps


def zero_fractions(s):
    """the fraction of exact zeros in every hidden layer's y of a step"""
    return {l: float((np.asarray(y) == 0).mean()) for l, y in s.y.items()}


# ---------------------------------------------------------------------------------------------------------------------
# a whole step in float64
def forward64(x, W, b):
    """(hidden activations {layer: y}, out) of a ReLU net in float64"""
    y, a = {}, _d(x)
    for l, (w, bb) in enumerate(zip(W, b), 1):
        a = a @ _d(w) + _d(bb)
        if l < len(W):
            a = np.maximum(a, 0.0)
            y[l] = a
    return y, a


def step64(x, targ, W, b, dW, db, lr, mom, wc, beta, ml):
    """One training step of a ReLU net in float64 on float64 copies of the fp32 state; the hyperparameters take their
    fp32 values.  Returns a dict: y {l}, out, dedx {l}, dW_new, db_new, W_new, b_new (lists indexed by layer - 1)."""
    L = len(W) + 1
    n = np.asarray(x).shape[0]
    lr, mom, wc = b6.f32(lr), b6.f32(mom), b6.f32(wc)
    y, out = forward64(x, W, b)
    dedx = {L - 1: b6.expect_loss(out, targ, beta, ml)[0].ref}
    for l in range(L - 2, 0, -1):
        dedx[l] = np.where(y[l] > 0, dedx[l + 1] @ _d(W[l]).T, 0.0)
    yin = lambda l: _d(x) if l == 1 else y[l - 1]
    dWn = [mom * _d(dW[l - 1]) - lr * (yin(l).T @ dedx[l] / n + wc * _d(W[l - 1])) for l in range(1, L)]
    dbn = [mom * _d(db[l - 1]) - lr * dedx[l].sum(axis=0) / n for l in range(1, L)]
    return dict(y=y, out=out, dedx=dedx, dW_new=dWn, db_new=dbn, W_new=[_d(w) + d for w, d in zip(W, dWn)],
                b_new=[_d(v) + d for v, d in zip(b, dbn)])


# ---------------------------------------------------------------------------------------------------------------------
# fp32 restatements of the two rules in numpy (what tests/test_relu_model.py passes, and mutates)
def relu_layer_f32(x, W, b, mut=None):
    F = np.float32
    z = (np.asarray(x, F) @ np.asarray(W, F)).astype(F)
    if mut != "no bias":
        z = (z + np.asarray(b, F)).astype(F)
    if mut == "leaky":
        return np.where(z < 0, (F(0.01) * z).astype(F), z).astype(F)
    return np.where(z < 0, F(0), z).astype(F)


def dx_relu_f32(d_next, W_next, y, mut=None):
    F = np.float32
    dedy = (np.asarray(d_next, F) @ np.asarray(W_next, F).T).astype(F)
    y = np.asarray(y, F)
    if mut == "leaky":
        return np.where(y > 0, dedy, (F(0.01) * dedy).astype(F)).astype(F)
    on = (y >= 0) if mut == "mask y >= 0" else (y > 0)
    return np.where(on, dedy, F(0)).astype(F)


# ---------------------------------------------------------------------------------------------------------------------
# exactly representable data
def exact_case(seed=23):
    """A [587, 96, 577] net and 128 rows whose MMSE step is exact in fp32: inputs in {-1, 0, 1}, weights multiples of 1/8
    in [-1/4, 1/4], biases and targets multiples of 1/4, lrate 2^-1, momentum 2^-1, no weight cost.  Returns a dict."""
    ls, n = [587, 96, 577], 128
    rng = np.random.default_rng(seed)
    F = np.float32
    W = [(rng.integers(-2, 3, (k, m)) * 0.125).astype(F) for k, m in zip(ls[:-1], ls[1:])]
    b = [(rng.integers(-2, 3, m) * 0.25).astype(F) for m in ls[1:]]
    x = rng.integers(-1, 2, (n, ls[0])).astype(F)
    t = (rng.integers(-8, 9, (n, ls[-1])) * 0.25).astype(F)
    return dict(ls=ls, n=n, W=W, b=b, x=x, t=t, lr=0.5, mom=0.5, wc=0.0, beta=2.0, ml=0)


def exact_case_quanta(c):
    """[(name, worst sum |a||b| (or |value|) per element in units of the operation's quantum)] for every GEMM and update
    of the step of `exact_case`: all below 2^24 means every product, partial sum (in any order) and result of the step
    is an fp32 number, so the fp32 step equals the float64 one bit for bit"""
    W, b, x, t, n = c["W"], c["b"], c["x"], c["t"], c["n"]
    lr = c["lr"]
    m = step64(x, t, W, b, [np.zeros_like(w) for w in W], [np.zeros_like(v) for v in b], lr, c["mom"], c["wc"],
               c["beta"], c["ml"])
    A = lambda a: np.abs(_d(a))
    q_z1 = 1.0 / 8                      # x integer, W1 and b1 multiples of 1/8
    q_out = q_z1 / 8                    # y1 (q_z1) x W2 (1/8); b2 and t multiples of 1/4
    q_d2 = q_out * 2.0 / n              # dedx_2 = 2 e / n, n a power of two
    q_dy1 = q_d2 / 8                    # dedx_2 x W2
    rows = [("fwd 1", (A(x) @ A(W[0]) + A(b[0])).max() / q_z1),
            ("fwd 2", (A(m["y"][1]) @ A(W[1]) + A(b[1])).max() / q_out),
            ("loss", (A(m["out"]) + A(t)).max() / q_out),
            ("dx 1", (A(m["dedx"][2]) @ A(W[1]).T).max() / q_dy1),
            ("dw 2", (A(m["y"][1]).T @ A(m["dedx"][2])).max() / (q_z1 * q_d2)),
            ("dw 1", (A(x).T @ A(m["dedx"][1])).max() / q_dy1),
            ("db 2", A(m["dedx"][2]).sum(0).max() / q_d2),
            ("db 1", A(m["dedx"][1]).sum(0).max() / q_dy1),
            ("apply W 2", (A(W[1]) + A(m["dW_new"][1])).max() / (q_z1 * q_d2 * lr / n)),
            ("apply W 1", (A(W[0]) + A(m["dW_new"][0])).max() / (q_dy1 * lr / n)),
            ("apply b 2", (A(b[1]) + A(m["db_new"][1])).max() / (q_d2 * lr / n)),
            ("apply b 1", (A(b[0]) + A(m["db_new"][0])).max() / (q_dy1 * lr / n))]
    return rows, m
