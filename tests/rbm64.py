"""Float64 model of one CD-1 step of RBM pre-training (csrc/rbm_rule.h) with per-element bounds (CPU only).

The notation, the hard bounds and the tight statistic are those of tests/bounds64.py; every `expect_*` here takes the
fp32 INPUTS of one operation -- in the GPU tests the session's own tensors, read back through `Rbm.tensor` -- so each
kernel is checked in isolation and no tolerance is picked:

* h0p, h1p: `bounds64.expect_sigmoid_layer` on the engine's own v0 / v1 (the up-pass is the hidden forward's kernel).
* h0s: exactly (draws < h0p) for the engine's own h0p; `draws` restates the hash of rbm_rule.h in NumPy.
* v1 (`expect_recon`): the dX product without the derivative.  z = h0s W^T + c is a sum of N products and one bias add:
  E_z = gamma_{N+2} (sum |h||w| + |c|) (two roundings of slack, as in the forward).  Gaussian visibles: that is the
  bound.  Bernoulli: pushed through `bounds64._sigmoid_expect`.
* dW, db (`expect_dw`, `expect_db`): bounds64's own at depth 2 B on the stacked factors [v0; v1] and [-h0p; h1p] with
  n = B: the negation is exact, so g = sum_b (v1^T h1p - v0^T h0p) is one sum of 2 B products in some order.
* dc (`expect_dc`): each term fl(v1 - v0) is one rounding, the B terms are summed in some order: u + gamma_{B-1} <=
  gamma_B of sum |v1 - v0|, then the four operations of rbm_rule::update_bias: `bounds64.expect_db` on d = v1 - v0.
* W, b, c after the step: one IEEE add each (`bounds64.apply_exact`).
* the reconstruction error: sum (v0 - v1)^2 in float64 over fp32 values; its device order is fixed but not the
  model's, so it is compared within gamma64_{n} of the sum (`recon_sqerr`).
"""
import numpy as np

import bounds64 as b64

M32 = 0xFFFFFFFF


def _mix32(x):
    x = np.asarray(x, np.uint64)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & np.uint64(M32)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & np.uint64(M32)
    x ^= x >> np.uint64(16)
    return x


def draws(seed, step, B, N):
    """r [B][N] of rbm_rule::draw: hsh = mix32(mix32(seed ^ step * 0x9e3779b9) ^ idx), r = (hsh >> 8) 2^-24, idx = b N + j"""
    key = _mix32(np.uint64((int(seed) & M32) ^ ((int(step) * 0x9e3779b9) & M32)))
    idx = np.arange(B * N, dtype=np.uint64)
    hsh = _mix32(key ^ idx)
    return ((hsh >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(B, N)


def sample(r, h0p):
    return (np.asarray(r, np.float32) < np.asarray(h0p, np.float32)).astype(np.float32)


def expect_recon(h0s, W, c, visible):
    """v1 = h0s W^T + c (gaussian) or sigma of it (bernoulli), from the engine's own h0s, W [K][N] and c"""
    h, W, c = b64._d(h0s), b64._d(W), b64._d(c)
    N = W.shape[1]
    scale = np.abs(h) @ np.abs(W).T + np.abs(c)
    z = h @ W.T + c
    Ez = b64.gamma(N + 2) * scale
    if visible == "gaussian":
        return b64.Expect(z, Ez, 0.0, b64.U * scale, 4.0 * np.sqrt(N))
    return b64._sigmoid_expect(z, Ez, scale, N)


def stacked(v0, v1, h0p, h1p):
    """the two factors of the CD update at depth 2 B (float64; the negation is exact)"""
    return np.concatenate([b64._d(v0), b64._d(v1)]), np.concatenate([-b64._d(h0p), b64._d(h1p)])


def expect_dw(v0, v1, h0p, h1p, W_old, dW_old, lr, mom, wc):
    V, H = stacked(v0, v1, h0p, h1p)
    return b64.expect_dw(V, H, W_old, dW_old, lr, mom, wc, n=np.asarray(v0).shape[0])


def expect_db(h0p, h1p, db_old, lr, mom):
    H = np.concatenate([-b64._d(h0p), b64._d(h1p)])
    return b64.expect_db(H, db_old, lr, mom, n=np.asarray(h0p).shape[0])


def expect_dc(v0, v1, dc_old, lr, mom):
    return b64.expect_db(b64._d(v1) - b64._d(v0), dc_old, lr, mom)


def recon_sqerr(v0, v1):
    """(sum (v0 - v1)^2 in float64, a bound on any float64 summation order of it)"""
    d = b64._d(v0) - b64._d(v1)
    s = float((d * d).sum())
    n = d.size
    return s, (n + 2) * 2.0 ** -53 * s * 1.01


def sigmoid(z):
    return b64._sigmoid64(z)[0]


def cd1_step(v0, W, b, c, r, visible, lr, mom, wc, dW, db, dc, positive="h0p", negative_sign=1.0, use_c=True):
    """One whole CD-1 step in float64 (the chain, for the model tests and the learning range; the GPU tests check every
    operation against its own inputs instead).  positive / negative_sign / use_c plant the errors the tests must see.
    Returns a dict of every tensor and the updated W, b, c, dW, db, dc."""
    v0, W, b, c, dW, db, dc = (b64._d(a) for a in (v0, W, b, c, dW, db, dc))
    lr, mom, wc = b64.f32(lr), b64.f32(mom), b64.f32(wc)
    B = v0.shape[0]
    h0p = sigmoid(v0 @ W + b)
    h0s = (b64._d(r) < h0p).astype(np.float64)
    z = h0s @ W.T + (c if use_c else 0.0)
    v1 = z if visible == "gaussian" else sigmoid(z)
    h1p = sigmoid(v1 @ W + b)
    hpos = h0p if positive == "h0p" else h0s
    g = negative_sign * (v1.T @ h1p) - v0.T @ hpos
    dW2 = mom * dW - lr * (g / B + wc * W)
    db2 = mom * db - lr * (negative_sign * h1p - hpos).sum(0) / B
    dc2 = mom * dc - lr * (negative_sign * v1 - v0).sum(0) / B
    return dict(v0=v0, h0p=h0p, h0s=h0s, v1=v1, h1p=h1p, dW=dW2, db=db2, dc=dc2, W=W + dW2, b=b + db2, c=c + dc2,
                sqerr=float(((v0 - v1) ** 2).sum()))


def train64(data, W, b, B, visible, lr, mom, wc, seed, epochs):
    """float64 CD-1 over `epochs` passes of data [n][K] in bunches of B, the session's step counter running on: the mean
    reconstruction error per frame of every epoch"""
    W, b = b64._d(W).copy(), b64._d(b).copy()
    K, N = W.shape
    c, dW, db, dc = np.zeros(K), np.zeros((K, N)), np.zeros(N), np.zeros(K)
    step, out = 0, []
    for _ in range(epochs):
        tot, frames = 0.0, 0
        for i in range(0, data.shape[0] - B + 1, B):
            s = cd1_step(data[i:i + B], W, b, c, draws(seed, step, B, N), visible, lr, mom, wc, dW, db, dc)
            W, b, c, dW, db, dc = s["W"], s["b"], s["c"], s["dW"], s["db"], s["dc"]
            tot += s["sqerr"]
            frames += B
            step += 1
        out.append(tot / frames)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the case the GPU test runs (tests/test_gpu_rbm.py) and the model test shows to be non-degenerate
LS = [45, 70, 33, 9]
RATES = dict(lrate=0.05, momentum=0.5, weightcost=0.002)


def make_case(B, seed=11, ls=LS, bunches=3):
    """(Ws, bs, x [bunches B][ls[0]]): Glorot weights, non-zero biases, unit-variance input rows"""
    Ws, bs = b64.make_net(ls, seed)
    x = np.random.default_rng(seed + 1).standard_normal((bunches * B, ls[0])).astype(np.float32)
    return Ws, bs, x


def layer_input(x, Ws, bs, layer):
    """v0 of an RBM on `layer` in float64 arithmetic, rounded to fp32 (the model test's stand-in for the engine's own)"""
    y = b64._d(x)
    for l in range(1, layer):
        y = sigmoid(y @ b64._d(Ws[l - 1]) + b64._d(bs[l - 1]))
    return y.astype(np.float32)


def learn_case(B=16, bunches=64, K=24, N=12, rank=3, seed=5):
    """a small structured set: low-rank rows plus noise, z-normalised per column; and a net [K, N, 4] to pre-train"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B * bunches, rank)) @ rng.standard_normal((rank, K)) + 0.3 * rng.standard_normal((B * bunches, K))
    x = ((x - x.mean(0)) / x.std(0)).astype(np.float32)
    Ws, bs = b64.make_net([K, N, 4], seed + 1, bias=0.1)
    Ws[0] = (Ws[0] * np.float32(0.1)).astype(np.float32)
    return x, Ws, bs
