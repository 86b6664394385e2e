"""GPU: CD-1 pre-training of a hidden layer (csrc/rbm_rule.h, csrc/rbm.hip.h, mlggd_rbm_*) against tests/rbm64.py.

Every kernel of a step is checked in isolation on the session's own inputs, read back through Rbm.tensor: the bounds are
those of tests/rbm64.py (derived, bounds64's notation).  Shapes [45, 70, 33, 9]: edge tiles in K and N, a one-row strip,
70 > 64; B = 24 (a partial frame tile, and 2 B = 48 leaves pad rows inside the stacked factors) and B = 128.  MLGGD_TILE64=2
at [96, 128, 128, 40], B = 64: the forward launches below the RBM's layer take the 64 x 64 kernels, the RBM's own three
products ignore the knob (include/mlggd.h) -- the case shows that both hold."""
import ctypes as C

import numpy as np
import pytest

import bounds64 as b64
import rbm64

pytestmark = pytest.mark.gpu

KNOBS = ("MLGGD_TILE64", "MLGGD_DW_TILE", "MLGGD_DW_PERSIST", "MLGGD_TILE_MAP", "MLGGD_STAGE_AHEAD", "MLGGD_LOSS_FUSE")
HP = (0.1, 0.9, 1e-5)         # the engine's fine-tuning rates: pre-training must not read them
R = rbm64.RATES
VIS = {1: "gaussian", 2: "bernoulli"}


def new_engine(pkg, monkeypatch, ls, B, W, b, env=None, **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return pkg.BPGpu(1, 0, ls, B, *HP, W, b, 1.2, 1, **kw)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def session_state(eng, rbm, layer):
    W, b = eng.returnWeights()
    return dict(W=W[layer - 1], b=b[layer - 1], c=rbm.visible_bias(), dW=rbm.tensor("delta_w"), db=rbm.tensor("delta_b"),
                dc=rbm.tensor("delta_c"))


def check_steps(pkg, monkeypatch, ls, B, layer, env=None, steps=3, seed=7):
    Ws, bs, x = rbm64.make_case(B, ls=ls, bunches=steps)
    visible = VIS[layer]
    eng = new_engine(pkg, monkeypatch, ls, B, Ws, bs, env)
    lines, samples = [], []
    try:
        with eng.rbm(layer, visible, seed=seed, **R) as rbm:
            K, N = ls[layer - 1], ls[layer]
            for t in range(steps):
                pre = session_state(eng, rbm, layer)
                xb = x[t * B:(t + 1) * B]
                n, sq = rbm.train(np.concatenate([xb, x[:B // 2]]))          # a trailing partial bunch is skipped
                assert n == 1
                T = {k: rbm.tensor(k) for k in ("v0", "h0p", "h0s", "v1", "h1p")}
                post = session_state(eng, rbm, layer)
                if layer == 1:
                    assert same_bits(T["v0"], xb)
                else:       # l = 2 takes its v0 from the engine's forward pass, bit for bit
                    assert same_bits(T["v0"], eng.debug_tensor("y", layer - 1))
                    eng.forward(xb)
                    assert same_bits(T["v0"], eng.debug_tensor("y", layer - 1))
                    if layer == 2:
                        lines.append(b64.compare("v0 = fwd 1", T["v0"], b64.expect_sigmoid_layer(xb, Ws[0], bs[0])))
                reps = [
                    b64.compare("h0p", T["h0p"], b64.expect_sigmoid_layer(T["v0"], pre["W"], pre["b"])),
                    b64.compare("v1 " + visible, T["v1"], rbm64.expect_recon(T["h0s"], pre["W"], pre["c"], visible)),
                    b64.compare("h1p", T["h1p"], b64.expect_sigmoid_layer(T["v1"], pre["W"], pre["b"])),
                    b64.compare("delta_w", post["dW"], rbm64.expect_dw(T["v0"], T["v1"], T["h0p"], T["h1p"], pre["W"], pre["dW"],
                                                                       R["lrate"], R["momentum"], R["weightcost"])),
                    b64.compare("delta_b", post["db"], rbm64.expect_db(T["h0p"], T["h1p"], pre["db"], R["lrate"], R["momentum"])),
                    b64.compare("delta_c", post["dc"], rbm64.expect_dc(T["v0"], T["v1"], pre["dc"], R["lrate"], R["momentum"])),
                    b64.compare_exact("W", post["W"], b64.apply_exact(pre["W"], post["dW"])),
                    b64.compare_exact("b", post["b"], b64.apply_exact(pre["b"], post["db"])),
                    b64.compare_exact("c", post["c"], b64.apply_exact(pre["c"], post["dc"])),
                    b64.compare_exact("h0s = (draws < h0p)", T["h0s"], rbm64.sample(pkg.rbm_draws(seed, t, B, N), T["h0p"])),
                ]
                lines += reps
                want, tol = rbm64.recon_sqerr(T["v0"], T["v1"])
                assert abs(sq - want) <= tol, (sq, want, tol)
                assert 0.2 <= T["h0s"].mean() <= 0.8 and np.abs(T["v1"] - T["v0"]).max() > 0.05
                assert (post["dW"] != 0).mean() > 0.99 and (post["dW"] != pre["dW"]).mean() > 0.99
                samples.append(T["h0s"])
                # the other layers were not touched
                Wn, bn = eng.returnWeights()
                for l in range(1, len(ls)):
                    if l != layer:
                        assert same_bits(Wn[l - 1], Ws[l - 1]) and same_bits(bn[l - 1], bs[l - 1])
            if steps > 1:
                assert np.abs(session_state(eng, rbm, layer)["c"]).min() > 0
                # same probabilities, another step: other samples -- the draws depend on `step`
                p = rbm.tensor("h0p")
                assert (rbm64.sample(pkg.rbm_draws(seed, 0, B, N), p) != rbm64.sample(pkg.rbm_draws(seed, 1, B, N), p)).any()
                assert any((a != b).any() for a, b in zip(samples, samples[1:]))
    finally:
        eng.close()
    print()
    for r in lines:
        print("  [%s l=%d B=%d] %s" % (ls, layer, B, r.line()))
    bad = [r.line() for r in lines if not r.ok]
    assert not bad, "\n".join(bad)


# ---- 1 and 3. every tensor of three consecutive steps, per layer; l = 2 takes its v0 from forward
@pytest.mark.parametrize("B", [24, 128])
@pytest.mark.parametrize("layer", [1, 2])
def test_every_tensor_of_three_steps(pkg, monkeypatch, layer, B):
    check_steps(pkg, monkeypatch, rbm64.LS, B, layer)


@pytest.mark.parametrize("layer", [1, 2])
def test_tile64_is_honoured_below_the_layer_and_ignored_by_the_rbm(pkg, monkeypatch, layer):
    ls, B = [96, 128, 128, 40], 64
    check_steps(pkg, monkeypatch, ls, B, layer, env={"MLGGD_TILE64": "2"})
    Ws, bs, _ = rbm64.make_case(B, ls=ls)
    eng = new_engine(pkg, monkeypatch, ls, B, Ws, bs, {"MLGGD_TILE64": "2"})
    try:
        assert eng.gemm_plan()[0][0] == 1          # the engine's own forward of layer 1 does take the 64 x 64 kernel
    finally:
        eng.close()


# ---- 2. one step on exactly representable data
def test_one_step_on_exactly_representable_data_equals_float64(pkg, monkeypatch):
    """[45, 70, 9], B = 32, gaussian: v0 in {-1, 0, 1}, W multiples of 1/8, b of 1/4, c = 0, lrate and momentum powers of two.
    Every product and partial sum of z0 = v0 W + b, of v1 = h0s W^T + c and of z1 = v1 W + b is then an fp32 number in any
    order (sum |a||b| in units of the quantum 1/64 stays far below 2^24, asserted), so: v1 equals the float64 value bit
    for bit; h0p and h1p equal the device's own packed sigmoid (debug_math "sigmoid4", the forward epilogue's form) of the float64 z0 and z1 bit for bit -- the GEMMs
    in front of them added nothing; delta_c = -lr sum (v1 - v0) / 32 and c equal float64 bit for bit.  delta_w and delta_b
    sum sigmoid values, 24-bit mantissas whose partial sums round: they are held to their bounds in the tests above."""
    ls, B = [45, 70, 9], 32
    rng = np.random.default_rng(3)
    W1 = (rng.integers(-8, 9, (45, 70)) / 8.0).astype(np.float32)
    b1 = (rng.integers(-4, 5, 70) / 4.0).astype(np.float32)
    Ws, bs = b64.make_net(ls, 1)
    Ws[0], bs[0] = W1, b1
    x = rng.integers(-1, 2, (B, 45)).astype(np.float32)
    lr, mom = 0.25, 0.5
    eng = new_engine(pkg, monkeypatch, ls, B, Ws, bs)
    try:
        with eng.rbm(1, "gaussian", lrate=lr, momentum=mom, weightcost=0.0, seed=3) as rbm:
            assert rbm.train(x)[0] == 1
            T = {k: rbm.tensor(k) for k in ("v0", "h0p", "h0s", "v1", "h1p", "delta_c", "vbias")}
            z0 = x.astype(np.float64) @ W1 + b1
            v1 = T["h0s"].astype(np.float64) @ W1.T.astype(np.float64)
            z1 = v1 @ W1 + b1
            assert (np.abs(x) @ np.abs(W1) + np.abs(b1)).max() * 64 < 2 ** 24
            assert (np.abs(v1) @ np.abs(W1).astype(np.float64) + np.abs(b1)).max() * 64 < 2 ** 24
            for z in (z0, z1):
                assert np.array_equal(z.astype(np.float32).astype(np.float64), z)
            assert same_bits(T["v0"], x)
            assert same_bits(T["h0p"], eng.debug_math("sigmoid4", z0.astype(np.float32).ravel()).reshape(z0.shape))
            assert same_bits(T["h0s"], rbm64.sample(pkg.rbm_draws(3, 0, B, 70), T["h0p"]))
            assert np.array_equal(T["v1"].astype(np.float64), v1) and 0.2 < T["h0s"].mean() < 0.8
            assert same_bits(T["h1p"], eng.debug_math("sigmoid4", z1.astype(np.float32).ravel()).reshape(z1.shape))
            dc = -lr * (v1 - x).sum(0) / B
            assert np.array_equal(dc.astype(np.float32).astype(np.float64), dc) and (dc != 0).mean() > 0.9
            assert np.array_equal(T["delta_c"].astype(np.float64), dc) and np.array_equal(T["vbias"].astype(np.float64), dc)
    finally:
        eng.close()


# ---- 4. determinism and neutrality
def test_determinism_and_neutrality(pkg, monkeypatch):
    ls, B, layer, ctx = [45, 70, 33, 9], 24, 2, 5
    Ws, bs, _ = rbm64.make_case(B)
    rng = np.random.default_rng(9)
    feat = rng.standard_normal((3 * B + ctx + 6, ls[0] // ctx)).astype(np.float32)
    first = rng.permutation(feat.shape[0] - ctx + 1)[:3 * B + 7].astype(np.int32)      # 3 bunches and a partial one
    rows = np.stack([feat[f:f + ctx].ravel() for f in first])
    xt, tt = b64.make_data(ls, 2 * B, 4)

    def session(seed, frames, fine_tune_first=True):
        eng = new_engine(pkg, monkeypatch, ls, B, Ws, bs)
        try:
            if fine_tune_first:
                assert eng.train(xt, tt) == 2                 # the fine-tuning momentum is non-zero from here on
            mom = [eng.debug_tensor("delta_w", l) for l in (1, 2, 3)]
            stats = eng.buffer_stats()
            sq = []
            with eng.rbm(layer, "bernoulli", seed=seed, **R) as rbm:
                assert eng.buffer_stats()[1] > stats[1]
                for _ in range(2):
                    n, s = rbm.train_frames(feat, first, ctx) if frames else rbm.train(rows)
                    assert n == 3
                    sq.append(s)
                    out = eng.forward(rows[:5])                # every other entry works between two calls
                    assert np.isfinite(out).all() and np.isfinite(eng.cv_all(xt, tt)[0])
                c = rbm.visible_bias()
            # stats: the chunk buffers of the calls above may have grown; the session's own bytes are back
            after = eng.buffer_stats()
            for l in (1, 2, 3):
                assert same_bits(eng.debug_tensor("delta_w", l), mom[l - 1])
            W, b = eng.returnWeights()
            assert eng.train(xt, tt) == 2
            return W, b, c, sq, eng.returnWeights(), (stats, after)
        finally:
            eng.close()

    a, b_, fr, other = session(7, False), session(7, False), session(7, True), session(8, False)
    for l in range(3):
        assert same_bits(a[0][l], b_[0][l]) and same_bits(a[1][l], b_[1][l])
        assert same_bits(a[0][l], fr[0][l]) and same_bits(a[1][l], fr[1][l])        # train_frames = train on expanded rows
    assert same_bits(a[2], b_[2]) and a[3] == b_[3] and same_bits(a[2], fr[2]) and a[3] == fr[3]
    assert not same_bits(a[0][layer - 1], other[0][layer - 1]) and not same_bits(a[2], other[2]) and a[3] != other[3]
    # a train step after pre-training = the same step on a fresh engine given the pre-trained weights (and, here, the
    # same fine-tuning history: the fresh engine takes the history's two steps first, then the weights)
    eng = new_engine(pkg, monkeypatch, ls, B, Ws, bs)
    try:
        assert eng.train(xt, tt) == 2
        eng.set_weights(a[0], a[1])
        assert eng.train(xt, tt) == 2
        W, b = eng.returnWeights()
    finally:
        eng.close()
    for l in range(3):
        assert same_bits(W[l], a[4][0][l]) and same_bits(b[l], a[4][1][l])


def test_buffer_bytes_return_after_close(pkg, monkeypatch):
    ls, B = rbm64.LS, 24
    Ws, bs, x = rbm64.make_case(B)
    eng = new_engine(pkg, monkeypatch, ls, B, Ws, bs)
    try:
        eng.forward(x)                                   # the chunk buffers exist at their final size
        before = eng.buffer_stats()
        rbm = eng.rbm(1, "gaussian", **R)
        opened = eng.buffer_stats()
        assert opened[1] > before[1] + 4 * 2 * 45 * 70
        assert rbm.train(x)[0] == 3
        assert eng.buffer_stats()[1] >= opened[1]
        rbm.close()
        assert eng.buffer_stats()[1] == before[1]
        rbm.close()                                      # closing twice is harmless
        with eng.rbm(2, "bernoulli", **R) as again:       # ... and the engine takes another session
            assert again.train(x)[0] == 3
        assert eng.buffer_stats()[1] == before[1]
    finally:
        eng.close()


# ---- 5. it learns
def test_it_learns_within_the_models_range(pkg, monkeypatch):
    x, Ws, bs = rbm64.learn_case()
    B, epochs, rates = 16, 4, (0.02, 0.5, 0.0002)
    model = [rbm64.train64(x, Ws[0], bs[0], B, "gaussian", *rates, seed, epochs) for seed in range(1, 9)]
    lo, hi = min(m[-1] for m in model), max(m[-1] for m in model)
    print("\n  float64 model, mean reconstruction error per frame, epochs 1..%d:" % epochs)
    for seed, m in enumerate(model, 1):
        print("    seed %d: %s" % (seed, " ".join("%.5f" % v for v in m)))
    print("    last epoch over 8 seeds: [%.5f, %.5f]; widened by 10 %%: [%.5f, %.5f]" % (lo, hi, 0.9 * lo, 1.1 * hi))
    eng = new_engine(pkg, monkeypatch, [24, 12, 4], B, Ws, bs)
    try:
        with eng.rbm(1, "gaussian", lrate=rates[0], momentum=rates[1], weightcost=rates[2], seed=1) as rbm:
            got = []
            for _ in range(epochs):
                n, sq = rbm.train(x)
                assert n == 64
                got.append(sq / (n * B))
    finally:
        eng.close()
    print("    device, seed 1: %s" % " ".join("%.5f" % v for v in got))
    assert got[-1] < got[0]
    assert 0.9 * lo <= got[-1] <= 1.1 * hi, (got, lo, hi)


# ---- 6. refusals
def test_refusals(pkg, monkeypatch):
    ls, B = rbm64.LS, 24
    Ws, bs, x = rbm64.make_case(B)
    lib = pkg.load()
    relu = new_engine(pkg, monkeypatch, ls, B, Ws, bs, activation="relu")
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_rbm_open: pre-training of a rectified-linear engine is not built"):
        relu.rbm(1)
    relu.close()
    nls = [36, 16, 9]
    nW, nb = b64.make_net(nls, 2)
    nat = new_engine(pkg, monkeypatch, nls, B, nW, nb, nat_frames=2)
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_rbm_open: pre-training of an engine with nat_frames = 2 is not built"):
        nat.rbm(1)
    nat.close()
    fake = new_engine(pkg, monkeypatch, ls, B, Ws, bs)
    fake.fake_world(2, allreduce=True)
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_rbm_open runs on a single-device engine"):
        fake.rbm(1)
    fake.close()
    joined = new_engine(pkg, monkeypatch, ls, B, Ws, bs)
    joined.comm_init(pkg.comm_unique_id(), 1, 0)
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_rbm_open runs on a single-device engine"):
        joined.rbm(1)
    joined.close()
    eng = new_engine(pkg, monkeypatch, ls, B, Ws, bs)
    try:
        for layer in (0, 3, -1, 9):
            with pytest.raises(pkg.MlggdError, match=r"error 1: mlggd_rbm_open: layer %d is not a hidden layer 1\.\.2" % layer):
                eng.rbm(layer)
        with pytest.raises(pkg.MlggdError, match=r"error 1: mlggd_rbm_open: visible 2 is neither"):
            eng.rbm(1, visible=2)
        with pytest.raises(ValueError):
            eng.rbm(1, visible="binomial")
        assert lib.mlggd_rbm_open(eng._h, 1, 0, 0.1, 0.5, 0.0, 1, None) == 1
        rbm = eng.rbm(1, "gaussian", **R)
        with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_rbm_open: this engine already has an open RBM session"):
            eng.rbm(2, "bernoulli")
        assert lib.mlggd_destroy(eng._h) == 4 and "RBM session" in lib.mlggd_last_error().decode()
        with pytest.raises(pkg.MlggdError, match=r"error 1: unknown RBM tensor name"):
            C_name = b"nothing"
            out = np.empty(4, np.float32)
            pkg._check(lib.mlggd_rbm_debug_tensor(rbm._h, C_name, out.ctypes.data_as(C.POINTER(C.c_float)), 4))
        with pytest.raises(ValueError):
            rbm.train(x[:, :10])
        # the engine and the session keep working afterwards
        assert rbm.train(x)[0] == 3 and np.isfinite(eng.forward(x[:5])).all()
        rbm.close()
        xt, tt = b64.make_data(ls, B, 4)
        assert eng.train(xt, tt) == 1
    finally:
        eng.close()
