"""CPU: the float64 checker of tests/bounds64.py is itself checked.

1. No false alarms: several correct fp32 implementations of a training step -- numpy's float32 matmul, a sequential
   k-loop, a split-K sum in another order, and the CPU oracle (its documented order) at the shipped shape -- pass
   every hard bound and every tight statistic.
2. Mutation kill list: each planted slip of an fp32 result, of the kind a kernel makes (a dropped K-chunk or K-slab,
   swapped columns in a ragged edge tile, a neighbour's bias, the last frame left out, 1/n over the wrong count,
   weight decay or momentum misapplied, an off-by-one column sum, stale rows of a ragged bunch, Dsigmoid wrong, a
   double rounding in the weight apply), is flagged by the hard bound; operands truncated to a 10-bit mantissa
   (tf32-like) by the tight statistic.  This is the evidence that tests/test_gpu_vs_float64.py would fail if a kernel
   were subtly wrong.
"""
import math

import numpy as np
import pytest

import bounds64 as b6

F = np.float32


# ---------------------------------------------------------------------------------------------------------------------
# fp32 implementations of the GEMMs
def mm_np32(a, b):
    return np.matmul(np.asarray(a, F), np.asarray(b, F)).astype(F)


def mm_seq(a, b):
    """one rounding per multiply and per add, k in order (the k-ordered chain of a dot product)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    acc = np.zeros((a.shape[0], b.shape[1]), F)
    for k in range(a.shape[1]):
        acc = (acc + (a[:, k:k + 1] * b[k:k + 1, :]).astype(F)).astype(F)
    return acc


def mm_split(S):
    """split-K: S contiguous partial sums (each by numpy's float32 matmul), added last slab first"""
    def mm(a, b):
        a, b = np.asarray(a, F), np.asarray(b, F)
        cuts = np.linspace(0, a.shape[1], S + 1).astype(int)
        parts = [mm_np32(a[:, lo:hi], b[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])]
        acc = parts[-1]
        for p in parts[-2::-1]:
            acc = (acc + p).astype(F)
        return acc
    return mm


def tf32(a):
    return (np.asarray(a, F).view(np.uint32) & np.uint32(0xFFFFE000)).view(F)


def sigmoid32(z):
    with np.errstate(over="ignore"):
        return (F(1) / (F(1) + np.exp(-z))).astype(F)


# ---------------------------------------------------------------------------------------------------------------------
# one fp32 training step (the engine's formulas), with optional planted mutations
def fp32_step(x, t, W, b, dW, db, hp, beta, ml, mm=mm_np32, slabs=1, mut=None):
    lr, mom, wc = (F(v) for v in hp)
    beta = F(beta)
    L = len(W) + 1
    x = np.asarray(x, F)
    B = x.shape[0]
    n = B
    y = {0: x}
    for l in range(1, L - 1):
        xin = tf32(y[l - 1]) if (mut == "tf32" and l == 1) else y[l - 1]
        Wl = tf32(W[l - 1]) if (mut == "tf32" and l == 1) else W[l - 1]
        z = mm(xin, Wl)
        bias = b[l - 1].copy()
        if mut == "neighbour_bias" and l == 1:
            bias[5] = b[l - 1][6]
        z = (z + bias).astype(F)
        if mut == "drop_k_chunk" and l == 1:      # one 32-wide chunk of K missing from the output tile (rows, cols) 0..31
            z[:32, :32] = (z[:32, :32] - mm_np32(y[0][:32, 64:96], W[0][64:96, :32])).astype(F)
        if mut == "swap_cols_ragged_tile" and l == 1:
            N = z.shape[1]
            assert N % 32 >= 2
            z[:, [N - 2, N - 1]] = z[:, [N - 1, N - 2]]
        y[l] = sigmoid32(z)
    Wo, bo = W[L - 2], b[L - 2]
    K = Wo.shape[0]
    cuts = np.linspace(0, K, slabs + 1).astype(int)
    used = slabs - 1 if mut == "drop_last_slab" else slabs
    out = np.zeros((B, Wo.shape[1]), F)
    for s in range(used):
        out = (out + mm(y[L - 2][:, cuts[s]:cuts[s + 1]], Wo[cuts[s]:cuts[s + 1]])).astype(F)
    out = out if mut == "no_bias" else (out + bo).astype(F)
    # loss (kernerror .. kernVecMulNum)
    e = (out - np.asarray(t, F)).astype(F)
    ae = np.abs(e)
    inv_n = F(1) / F(n)
    alpha = None
    with np.errstate(divide="ignore"):
        P = np.where(e == 0, F(0), ae ** (beta - F(1))).astype(F)
    if ml == 1:
        p = (ae ** beta).astype(F)
        s = (p[:-1] if mut == "colsum_off_by_one" else p).sum(axis=0, dtype=F)
        v2 = ((s / F(n)).astype(F) * beta).astype(F)
        alpha = (v2 ** (F(1) / beta)).astype(F)
        q = (alpha ** beta).astype(F)
        g = ((np.sign(e) * P * beta).astype(F) / q).astype(F)
    else:
        g = (beta * np.sign(e) * P).astype(F)
    d = {L - 1: (g * inv_n).astype(F)}
    for l in range(L - 2, 0, -1):
        dy = mm(d[l + 1], W[l].T)
        sp = y[l] if mut == "dsigmoid_y" else (y[l] * (F(1) - y[l])).astype(F)
        d[l] = (dy * sp).astype(F)
    dW_new, db_new, W_new, b_new = [], [], [], []
    nf = F(n - 1) if mut == "wrong_n" else F(n)
    wcu = F(0) if mut == "no_weight_decay" else wc
    for l in range(1, L):
        yl, dl = y[l - 1], d[l]
        if mut == "dw_drop_last_frame":
            yl, dl = yl[:-1], dl[:-1]
        G = mm(yl.T, dl)
        base = W[l - 1] if mut == "momentum_on_W" else dW[l - 1]
        D = (mom * base - lr * ((G / nf).astype(F) + (wcu * W[l - 1]).astype(F))).astype(F)
        gb = dl.sum(axis=0, dtype=F)
        Db = (mom * db[l - 1] - lr * (gb / nf).astype(F)).astype(F)
        if mut == "apply_twice":
            h = (D * F(0.5)).astype(F)
            Wn = ((W[l - 1] + h).astype(F) + h).astype(F)
        else:
            Wn = (W[l - 1] + D).astype(F)
        dW_new.append(D)
        db_new.append(Db)
        W_new.append(Wn)
        b_new.append((b[l - 1] + Db).astype(F))
    st = b6.Step(x, t, list(W), list(b), list(dW), list(db), {l: y[l] for l in range(1, L - 1)}, out, d,
                 dW_new, db_new, W_new, b_new, float(lr), float(mom), float(wc), float(beta), ml, slabs, alpha)
    return st


def two_steps(ls, B, hp, beta, ml, seed=1, mm=mm_np32, slabs=1, mut=None, sat_rows=8):
    """step 1 correct (so that delta is non-zero), step 2 with the mutation; returns step 2"""
    W, b = b6.make_net(ls, seed)
    dW = [np.zeros_like(w) for w in W]
    db = [np.zeros_like(v) for v in b]
    x, t = b6.make_data(ls, 2 * B, seed + 1, sat_rows, W[0], B)
    s1 = fp32_step(x[:B], t[:B], W, b, dW, db, hp, beta, ml, mm, slabs)
    return fp32_step(x[B:], t[B:], s1.W_new, s1.b_new, s1.dW_new, s1.db_new, hp, beta, ml, mm, slabs, mut)


def assert_clean(reps):
    bad = [r.line() for r in reps if not r.ok]
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# 1. no false alarms
@pytest.mark.parametrize("impl", ["np32", "seq", "split5"])
@pytest.mark.parametrize("ml,beta,hp", [(1, 1.2, (0.1, 0.9, 1e-5)), (1, 0.9, (0.3, 0.5, 1e-2)),
                                        (0, 2.0, (0.05, 0.0, 0.0)), (1, 1.0, (0.1, 0.9, 1e-5))])
def test_fp32_implementations_pass_every_bound(impl, ml, beta, hp):
    mm = {"np32": mm_np32, "seq": mm_seq, "split5": mm_split(5)}[impl]
    ls, B = ([131, 97, 33, 1, 57], 40) if impl == "seq" else ([531, 97, 33, 1, 257], 200)
    s = two_steps(ls, B, hp, beta, ml, seed=3, mm=mm, slabs=5 if impl == "split5" else 1)
    assert_clean(b6.check_step(s))


def test_saturation_reaches_zero_one_and_the_subnormal_band():
    """the value construction the GPU tests use does produce y == 0, y == 1 and subnormal y, and the bounds hold there"""
    ls, B = [1799, 2048, 257], 128
    s = two_steps(ls, B, (0.1, 0.9, 1e-5), 1.0, 1, seed=5)
    y = s.y[1]
    assert (y == 0).sum() > 0 and (y == 1).sum() > 0 and ((y > 0) & (y < 2.0 ** -126)).sum() > 0
    assert_clean(b6.check_step(s))


def test_exact_zero_error_gives_an_exact_zero_gradient():
    out, t = np.array([[1.5, 2.0], [0.25, 3.0]], F), np.array([[1.5, 1.0], [1.0, 1.0]], F)
    e0 = b6.expect_loss(out, t, 0.9, 1)[0]
    assert e0.ref[0, 0] == 0 and e0.bound[0, 0] == 0
    good = e0.ref.astype(F)
    assert b6.compare("e0", good, e0).ok
    good[0, 0] = 1e-30
    assert not b6.compare("e0", good, e0).ok


@pytest.mark.parametrize("ls,B", [([1799, 2048, 2048, 2048, 257], 128), ([531, 97, 33, 1, 257], 200)])
def test_the_cpu_oracle_passes_every_bound(pyoracle, ls, B):
    """the oracle (documented order, glibc's powf) at the shipped shape and at a ragged one, two steps"""
    hp, beta, ml = (0.1, 0.9, 1e-5), 1.0, 1
    W, b = b6.make_net(ls, 7)
    x, t = b6.make_data(ls, 2 * B, 8, 8, W[0], B)
    o = pyoracle.OracleNet(ls, B, *hp, beta, ml, W, b)
    assert o.train(x[:B], t[:B]) == 1
    Wp, bp = o.get_weights()
    dWp = [o.tensor("delta_w", l) for l in range(1, len(ls))]
    dbp = [o.tensor("delta_b", l) for l in range(1, len(ls))]
    assert o.train(x[B:], t[B:]) == 1
    Wn, bn = o.get_weights()
    L = len(ls)
    s = b6.Step(x[B:], t[B:], Wp, bp, dWp, dbp, {l: o.tensor("y", l, rows=B) for l in range(1, L - 1)},
                o.tensor("out", rows=B), {l: o.tensor("dedx", l, rows=B) for l in range(1, L)},
                [o.tensor("delta_w", l) for l in range(1, L)], [o.tensor("delta_b", l) for l in range(1, L)], Wn, bn,
                *hp, beta, ml, 1, o.tensor("scalefactor"))
    o.close()
    assert_clean(b6.check_step(s))


def test_cv_bounds_hold_for_the_host_order():
    rng = np.random.default_rng(4)
    n, D, beta = 300, 257, F(1.2)
    out = rng.standard_normal((n, D)).astype(F)
    t = rng.standard_normal((n, D)).astype(F)
    alpha = rng.uniform(0.5, 1.5, D).astype(F)
    e = (out - t).astype(F)
    sq, ab, d3 = F(0), F(0), F(0)
    for v in e.ravel():                        # host order: fp32 scalars, frame-major
        sq = F(sq + F(v * v))
        ab = F(ab + abs(v))
    for i in range(n):
        d3 = F(d3 + ((np.abs(-e[i]) / alpha).astype(F) ** beta).astype(F).sum(dtype=F))
    d1 = F(n * D) * F(np.log(F(beta / F(2 * F(math.gamma(float(F(1.0 / beta))))))))
    d2 = F(np.log(alpha).astype(F).sum(dtype=F)) * F(n)
    ll = F(F(d1 - d2) - d3)
    ex = b6.expect_cv(out, t, beta, alpha, math.gamma)
    for name, got in (("sqerr", sq), ("abserr", F(ab / F(D))), ("loglik", ll)):
        r = b6.compare(name, np.array(got), ex[name])
        assert r.ok, r.line()
    r = b6.compare("sqerr", np.array(sq * F(1 + 1e-3)), ex["sqerr"])     # a dropped frame's worth
    assert not r.ok


# ---------------------------------------------------------------------------------------------------------------------
# 2. mutation kill list: (mutation, report that must flag it, hard or tight)
SHAPE, BUNCH, HP_WC = [300, 250, 97, 33], 96, (0.3, 0.5, 1e-2)
KILLS = [
    ("drop_k_chunk", "fwd 1", "hard"),
    ("drop_last_slab", "out (S=4)", "hard"),
    ("swap_cols_ragged_tile", "fwd 1", "hard"),
    ("neighbour_bias", "fwd 1", "hard"),
    ("no_bias", "out (S=4)", "hard"),
    ("dw_drop_last_frame", "dw 1", "hard"),
    ("dw_drop_last_frame", "db 3", "hard"),
    ("wrong_n", "dw 2", "hard"),
    ("wrong_n", "db 2", "hard"),
    ("no_weight_decay", "dw 1", "hard"),
    ("momentum_on_W", "dw 1", "hard"),
    ("colsum_off_by_one", "alpha", "hard"),
    ("colsum_off_by_one", "loss ML beta 1.2", "hard"),
    ("dsigmoid_y", "dx 2", "hard"),
    ("apply_twice", "apply W 1", "hard"),
    ("tf32", "fwd 1", "tight"),
]


@pytest.mark.parametrize("mut,report,kind", KILLS)
def test_mutation_is_killed(mut, report, kind):
    s = two_steps(SHAPE, BUNCH, HP_WC, 1.2, 1, seed=11, slabs=4, mut=mut)
    reps = {r.name: r for r in b6.check_step(s)}
    r = reps[report]
    print("%-22s -> %s" % (mut, r.line()))
    if kind == "hard":
        assert r.count > 0, r.line()
    else:
        assert r.tight > r.limit, r.line()


def test_tf32_truncation_is_caught_by_the_tight_statistic_alone():
    """at the shipped first layer (K = 1799) operands truncated to a 10-bit mantissa stay inside the worst-case hard
    bound -- only the tight statistic sees them"""
    ls = [1799, 2048, 257]
    W, b = b6.make_net(ls, 13)
    x, _ = b6.make_data(ls, 128, 14)
    ex = b6.expect_sigmoid_layer(x, W[0], b[0])
    good = b6.compare("fwd", sigmoid32((mm_np32(x, W[0]) + b[0]).astype(F)), ex)
    bad = b6.compare("fwd tf32", sigmoid32((mm_np32(tf32(x), tf32(W[0])) + b[0]).astype(F)), ex)
    print(good.line())
    print(bad.line())
    assert good.ok
    assert bad.count == 0 and bad.tight > bad.limit, bad.line()


def test_unmutated_kill_list_shape_is_clean():
    """the same construction without a mutation passes: each kill above is the mutation's doing"""
    assert_clean(b6.check_step(two_steps(SHAPE, BUNCH, HP_WC, 1.2, 1, seed=11, slabs=4)))


def fp32_forward(x, W, b, B, mut=None):
    """forward() in bunches of B with a ragged last bunch; mutations: its rows left zero, or stale (the previous
    bunch's rows)"""
    outs = []
    for i in range(0, x.shape[0], B):
        y = np.asarray(x[i:i + B], F)
        for l in range(len(W) - 1):
            y = sigmoid32((mm_np32(y, W[l]) + b[l]).astype(F))
        outs.append((mm_np32(y, W[-1]) + b[-1]).astype(F))
    out = np.vstack(outs)
    last = (x.shape[0] - 1) // B * B
    if mut == "ragged_zero":
        out[last:] = 0
    elif mut == "ragged_stale":
        k = x.shape[0] - last
        out[last:] = out[last - B:last - B + k]
    return out


@pytest.mark.parametrize("mut", [None, "ragged_zero", "ragged_stale"])
def test_forward_chain_bound_and_ragged_rows(mut):
    ls, B = [531, 1024, 257], 64
    W, b = b6.make_net(ls, 21)
    x, _ = b6.make_data(ls, 2 * B + 44, 22)
    out = fp32_forward(x, W, b, B, mut)
    r = b6.compare("forward chain", out, b6.expect_forward_chain(x, W, b))
    print(mut, r.line())
    if mut is None:
        assert r.ok, r.line()
    else:
        assert r.count > 0 and all(i >= 2 * B for i, _ in r.where), r.line()



def test_forward_chain_bound_with_an_input_error():
    """x_err: an fp32 forward from inputs scaled up by 5 to 10 % (a correlated input error) stays within the bound propagated from that
    input error, and leaves it when the error is not declared; the default (and x_err = 0) gives the bits of the loop as it was
    before x_err (a frozen copy)"""
    ls, B = [531, 1024, 96, 257], 64
    W, b = b6.make_net(ls, 23)
    x, _ = b6.make_data(ls, 2 * B + 5, 24)
    x64 = x.astype(np.float64)
    rel = 0.1
    r = np.random.default_rng(25).uniform(0.5, 1.0, x.shape)
    xp = (x64 * (1.0 + rel * r)).astype(F)                       # within rel |x| (1 + u) of x64
    out = fp32_forward(xp, W, b, B)
    ex = b6.expect_forward_chain(x64, W, b, x_err=rel * (1.0 + 2 * b6.U) * np.abs(x64))
    rep = b6.compare("forward chain, x_err", out, ex)
    print(rep.line())
    assert rep.ok, rep.line()
    plain = b6.compare("forward chain, no x_err", out, b6.expect_forward_chain(x64, W, b))
    print(plain.line())
    assert plain.count > 0
    for slabs in (1, 4):
        frozen = frozen_forward_chain(x, W, b, slabs)
        for e in (b6.expect_forward_chain(x, W, b, slabs=slabs), b6.expect_forward_chain(x, W, b, slabs, x_err=0.0)):
            assert np.array_equal(e.bound, frozen.bound) and np.array_equal(e.ref, frozen.ref)


def frozen_forward_chain(x, Ws, bs, slabs=1):
    """bounds64.expect_forward_chain as it was before x_err, frozen: the default must give these bits"""
    y = b6._d(x)
    Ey = np.zeros_like(y)
    L = len(Ws)
    for i, (Wl, bl) in enumerate(zip(Ws, bs)):
        Wl, bl = b6._d(Wl), b6._d(bl)
        K = Wl.shape[0]
        aW = np.abs(Wl)
        prop = Ey @ aW
        last = i == L - 1
        scale = (np.abs(y) + Ey) @ aW + np.abs(bl)
        z = y @ Wl + bl
        Ez = prop + b6.gamma(K + (slabs if last else 0) + 2) * scale
        if last:
            return b6.Expect(z, Ez)
        e = b6._sigmoid_expect(z, Ez, scale, K)
        y, Ey = e.ref, e.bound

# ---------------------------------------------------------------------------------------------------------------------
# 3. data-parallel steps: a rank-split fp32 implementation (per-rank chains, statistics and partial sums met in rank
# order), checked as ONE step of the ranks' rows stacked in rank order -- the form tests/test_gpu_dp_vs_float64.py uses
def fp32_dp_step(x, t, W, b, dW, db, hp, beta, ml, world, mut=None):
    lr, mom, wc = (F(v) for v in hp)
    beta = F(beta)
    L = len(W) + 1
    n = x.shape[0]
    B = n // world
    rows = [slice(r * B, (r + 1) * B) for r in range(world)]
    ys, outs, es = [], [], []
    for sl in rows:
        y = {0: np.asarray(x[sl], F)}
        for l in range(1, L - 1):
            y[l] = sigmoid32((mm_np32(y[l - 1], W[l - 1]) + b[l - 1]).astype(F))
        out = (mm_np32(y[L - 2], W[L - 2]) + b[L - 2]).astype(F)
        ys.append(y)
        outs.append(out)
        es.append((out - np.asarray(t[sl], F)).astype(F))
    inv_n = F(1) / F(n)
    alpha = None
    if ml == 1:                                     # k_colsum per rank, k_accum in rank order
        parts = [(np.abs(e) ** beta).astype(F).sum(axis=0, dtype=F) for e in es]
        s = parts[-1] if mut == "ml_last_rank" else parts[0]
        for p in ([] if mut == "ml_last_rank" else parts[1:]):
            s = (s + p).astype(F)
        alpha = (((s / F(n)).astype(F) * beta).astype(F) ** (F(1) / beta)).astype(F)
        q = (alpha ** beta).astype(F)
    ds = []
    for y, e in zip(ys, es):
        with np.errstate(divide="ignore"):
            P = np.where(e == 0, F(0), np.abs(e) ** (beta - F(1))).astype(F)
        g = ((np.sign(e) * P * beta).astype(F) / q).astype(F) if ml == 1 else (beta * np.sign(e) * P).astype(F)
        d = {L - 1: (g * inv_n).astype(F)}
        for l in range(L - 2, 0, -1):
            d[l] = (mm_np32(d[l + 1], W[l].T) * (y[l] * (F(1) - y[l])).astype(F)).astype(F)
        ds.append(d)
    nf = F(B) if mut == "local_n" else F(n)
    dW_new, db_new, W_new, b_new = [], [], [], []
    for l in range(1, L):
        fy = [y[l - 1].copy() for y in ys]
        fd = [d[l].copy() for d in ds]
        if mut == "seam":                           # rank r's first frame replaced by rank r-1's last in the factors
            for r in range(world - 1, 0, -1):
                fy[r][0], fd[r][0] = fy[r - 1][-1], fd[r - 1][-1]
        G = [mm_np32(a.T, c) for a, c in zip(fy, fd)]
        order = list(range(world))
        if mut == "rank_twice":
            order.append(0)
        elif mut == "rank_missing":
            order.remove(1)
        Gs = G[order[0]]
        for r in order[1:]:
            Gs = (Gs + G[r]).astype(F)
        gb = [c.sum(axis=0, dtype=F) for c in fd]
        gbs = gb[-1] if mut == "bias_last_rank" else gb[0]
        for v in ([] if mut == "bias_last_rank" else gb[1:]):
            gbs = (gbs + v).astype(F)
        upd = lambda Wo, Do: ((mom * Do - lr * ((Gs / nf).astype(F) + (wc * Wo).astype(F))).astype(F))
        D = upd(W[l - 1], dW[l - 1])
        Wn = (W[l - 1] + D).astype(F)
        if l == 1 and mut in ("tile_row_stale", "tile_row_twice"):   # the 64-row shard tile row 1 of layer 1
            tr = slice(64, 128)
            if mut == "tile_row_stale":
                D[tr], Wn[tr] = dW[0][tr], W[0][tr]
            else:
                D2 = upd(Wn, D)
                D[tr], Wn[tr] = D2[tr], (Wn + D2).astype(F)[tr]
        dW_new.append(D)
        W_new.append(Wn)
        Db = (mom * db[l - 1] - lr * (gbs / nf).astype(F)).astype(F)
        db_new.append(Db)
        b_new.append((b[l - 1] + Db).astype(F))
    stack = lambda k: np.vstack([y[k] for y in ys])
    st = b6.Step(np.asarray(x, F), np.asarray(t, F), list(W), list(b), list(dW), list(db),
                 {l: stack(l) for l in range(1, L - 1)}, np.vstack(outs),
                 {l: np.vstack([d[l] for d in ds]) for l in range(1, L)}, dW_new, db_new, W_new, b_new,
                 float(lr), float(mom), float(wc), float(beta), ml, 1, alpha)
    st.grad = [(np.vstack([y[l - 1] for y in ys]), Gs) for l in [L - 1]]   # layer L-1's factors and summed G
    return st


def dp_two_steps(ls, B, world, hp, beta, ml, seed=1, mut=None):
    W, b = b6.make_net(ls, seed)
    n = world * B
    x, t = b6.make_data(ls, 2 * n, seed + 1, 8, W[0], B)
    s1 = fp32_dp_step(x[:n], t[:n], W, b, [np.zeros_like(w) for w in W], [np.zeros_like(v) for v in b], hp, beta,
                      ml, world)
    return fp32_dp_step(x[n:], t[n:], s1.W_new, s1.b_new, s1.dW_new, s1.db_new, hp, beta, ml, world, mut)


@pytest.mark.parametrize("world,B", [(2, 50), (3, 50), (8, 20)])
@pytest.mark.parametrize("ml,beta,hp", [(1, 1.2, (0.3, 0.5, 1e-2)), (1, 0.9, (0.1, 0.9, 1e-5)), (0, 2.0, (0.1, 0.9, 1e-5))])
def test_rank_split_implementation_passes_every_bound(world, B, ml, beta, hp):
    s = dp_two_steps([300, 250, 97, 33], B, world, hp, beta, ml, seed=5 + world)
    reps = b6.check_step(s)
    y, G = s.grad[0]
    reps.append(b6.compare("grad %d" % (len(s.W)), G, b6.expect_grad(y, s.dedx[len(s.W)])))
    print("rank split world %d B %d: worst hard %.4f tight %.2f" % (
        world, B, max(r.hard for r in reps), max(r.tight / r.limit for r in reps if r.limit > 0)))
    assert_clean(reps)


DP_KILLS = [
    ("local_n", "dw 1"), ("local_n", "db 2"),
    ("ml_last_rank", "alpha"), ("ml_last_rank", "loss ML beta 1.2"),
    ("rank_twice", "dw 1"), ("rank_missing", "dw 2"),
    ("seam", "dw 1"),
    ("tile_row_stale", "apply W 1"), ("tile_row_stale", "dw 1"), ("tile_row_twice", "dw 1"),
    ("bias_last_rank", "db 1"),
]


@pytest.mark.parametrize("mut,report", DP_KILLS)
def test_data_parallel_slip_is_killed(mut, report):
    s = dp_two_steps([300, 250, 97, 33], 50, 3, (0.3, 0.5, 1e-2), 1.2, 1, seed=8, mut=mut)
    r = {r.name: r for r in b6.check_step(s)}[report]
    print("%-16s -> %s" % (mut, r.line()))
    assert r.count > 0, r.line()


# ---------------------------------------------------------------------------------------------------------------------
# 4. dropout: the training step with masks, CV's weight round trips, the mask statistics
def fp32_dropout_step(x, t, W, b, dW, db, hp, beta, p_in, p_hid, rng, mut=None):
    """one training step under dropout (MMSE, beta as given): a mask per layer, the row-major copy (reported, dW's
    operand) and the transposed copy (the next forward's and dX's operand).  Returns (Step, {layer: mask})."""
    lr, mom, wc = (F(v) for v in hp)
    beta = F(beta)
    L = len(W) + 1
    n = x.shape[0]

    def draw(shape, p):
        if mut == "unit_hash":
            return np.broadcast_to(rng.random(shape[1]) < p, shape).copy()
        return rng.random(shape) < p

    masks = {0: draw(x.shape, p_in)}
    xr = np.where(masks[0], F(0), x).astype(F)            # row-major input (in_bunch)
    yt = {0: xr}
    if mut == "input_row_missing":
        xr = np.asarray(x, F)
    yr = {0: xr}
    for l in range(1, L - 1):
        z = (mm_np32(yt[l - 1], W[l - 1]) + b[l - 1]).astype(F)
        s = sigmoid32(z)
        masks[l] = draw(s.shape, p_hid)
        yt[l] = np.where(masks[l], F(0), s).astype(F)
        if mut == "inverted":
            yt[l] = (yt[l] * (F(1) / F(1 - p_hid))).astype(F)
        yr[l] = s if (mut == "mask_T_only" and l == 1) else yt[l]
    out = (mm_np32(yt[L - 2], W[L - 2]) + b[L - 2]).astype(F)
    e = (out - np.asarray(t, F)).astype(F)
    P = (np.abs(e) ** (beta - F(1))).astype(F)
    d = {L - 1: ((beta * np.sign(e) * P).astype(F) * (F(1) / F(n))).astype(F)}
    for l in range(L - 2, 0, -1):
        d[l] = (mm_np32(d[l + 1], W[l].T) * (yt[l] * (F(1) - yt[l])).astype(F)).astype(F)
    dW_new, db_new, W_new, b_new = [], [], [], []
    for l in range(1, L):
        D = (mom * dW[l - 1] - lr * ((mm_np32(yr[l - 1].T, d[l]) / F(n)).astype(F) + (wc * W[l - 1]).astype(F))).astype(F)
        Db = (mom * db[l - 1] - lr * (d[l].sum(axis=0, dtype=F) / F(n)).astype(F)).astype(F)
        dW_new.append(D)
        db_new.append(Db)
        W_new.append((W[l - 1] + D).astype(F))
        b_new.append((b[l - 1] + Db).astype(F))
    st = b6.Step(yr[0], np.asarray(t, F), list(W), list(b), list(dW), list(db), {l: yr[l] for l in range(1, L - 1)},
                 out, d, dW_new, db_new, W_new, b_new, float(lr), float(mom), float(wc), float(beta), 0, 1, None,
                 dropout=True)
    return st, masks


def dropout_checks(st, x_raw, p_in, p_hid):
    """what the GPU test asserts of one dropout step: every operation, the input rows raw-or-0, the mask statistics"""
    L = len(st.W) + 1
    reps = b6.check_step(st)
    rep, drop0, known0 = b6.input_mask(x_raw, st.x)
    reps.append(rep)
    reps += b6.mask_stats("mask 0", drop0, known0, p_in)
    masks = {0: (drop0, known0)}
    for l in range(1, L - 1):
        _, dr, kn = b6.expect_dropout_layer(st.x if l == 1 else st.y[l - 1], st.W[l - 1], st.b[l - 1], st.y[l])
        masks[l] = (dr, kn)
        reps += b6.mask_stats("mask %d" % l, dr, kn, p_hid)
    if L > 3:
        reps.append(b6.mask_overlap("masks 1 x 2", *masks[1], *masks[2], p_hid, p_hid))
    return reps, masks


DROP_LS, DROP_P = [300, 250, 97, 33], (0.2, 0.3)


def dropout_run(mut=None, seed=31):
    rng = np.random.default_rng(seed)
    W, b = b6.make_net(DROP_LS, seed)
    x, t = b6.make_data(DROP_LS, 2 * 96, seed + 1, 8, W[0], 96)    # saturating rows: y == 0 without a mask too
    s1, _ = fp32_dropout_step(x[:96], t[:96], W, b, [np.zeros_like(w) for w in W], [np.zeros_like(v) for v in b],
                              (0.3, 0.5, 1e-2), 2.0, *DROP_P, rng)
    s2, _ = fp32_dropout_step(x[96:], t[96:], s1.W_new, s1.b_new, s1.dW_new, s1.db_new, (0.3, 0.5, 1e-2), 2.0, *DROP_P,
                              rng, mut)
    r1, m1 = dropout_checks(s1, x[:96], *DROP_P)
    r2, m2 = dropout_checks(s2, x[96:], *DROP_P)
    r2.append(b6.mask_overlap("mask 1 steps 1 x 2", *m1[1], *m2[1], DROP_P[1], DROP_P[1]))
    return r1, r2


def test_dropout_step_passes_every_bound_and_statistic():
    r1, r2 = dropout_run()
    for r in r1 + r2:
        print(r.line())
    assert_clean(r1 + r2)


DROP_KILLS = [("inverted", "fwd 1"), ("mask_T_only", "fwd 2"), ("input_row_missing", "fwd 1"),
              ("input_row_missing", "mask 0 rate"), ("unit_hash", "mask 1 per unit")]


@pytest.mark.parametrize("mut,report", DROP_KILLS)
def test_dropout_slip_is_killed(mut, report):
    _, r2 = dropout_run(mut)
    hit = [r for r in r2 if r.name.startswith(report)]
    assert hit, [r.name for r in r2]
    print("%-18s -> %s" % (mut, hit[0].line()))
    assert hit[0].count > 0, hit[0].line()


def test_mask_statistics_see_a_repeated_or_reseeded_mask():
    """masks of two steps (or two seeds) that coincide fail the overlap test; independent ones pass it"""
    rng = np.random.default_rng(3)
    a, b = rng.random((128, 200)) < 0.25, rng.random((128, 200)) < 0.25
    k = np.ones_like(a)
    assert b6.mask_overlap("indep", a, k, b, k, 0.25, 0.25).ok
    assert not b6.mask_overlap("same", a, k, a, k, 0.25, 0.25).ok


@pytest.mark.parametrize("mut", [None, "div_keep"])
def test_cv_dropout_weight_round_trips(mut):
    """forward() under dropout leaves fl32(fl32(W keep) fl32(1/keep)) per bunch; dividing by keep instead rounds
    differently and the exact compare sees it"""
    ls, B, keeps = [300, 250, 33], 64, (F(1) - F(0.2), F(1) - F(0.3))
    W, b = b6.make_net(ls, 41)
    x, _ = b6.make_data(ls, 3 * B + 17, 42)
    used, left = b6.cv_dropout_weights(W, keeps, 4)
    cur, outs = [w.copy() for w in W], []
    for j in range(4):
        sc = [(w * k).astype(F) for w, k in zip(cur, keeps)]
        y = x[j * B:(j + 1) * B]
        y = sigmoid32((mm_np32(y, sc[0]) + b[0]).astype(F))
        outs.append((mm_np32(y, sc[1]) + b[1]).astype(F))
        cur = [((s / k) if mut == "div_keep" else (s * (F(1) / k))).astype(F) for s, k in zip(sc, keeps)]
    reps = [b6.compare_exact("W %d after CV" % (l + 1), cur[l], left[l]) for l in range(2)]
    for j in range(4):
        reps.append(b6.compare("bunch %d" % j, outs[j], b6.expect_forward_chain(x[j * B:(j + 1) * B], used[j], b)))
    for r in reps:
        print(mut, r.line())
    if mut is None:
        assert_clean(reps)
    else:
        assert any(r.count > 0 for r in reps[:2])
