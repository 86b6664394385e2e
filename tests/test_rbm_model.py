"""CPU: the float64 model of CD-1 pre-training (tests/rbm64.py) and the host statement of its draws.

pkg.rbm_draws (the library's host-only entry over csrc/rbm_rule.h) equals the Python restatement of the hash; the case
tests/test_gpu_rbm.py runs is not degenerate in the model; and the errors worth planting -- samples instead of
probabilities in the positive statistics, the negative phase's sign, the visible bias left out of the down-pass -- move the
model's outputs beyond the bounds the GPU test applies, so that test can see them."""
import numpy as np
import pytest

import bounds64 as b64
import rbm64

F = np.float32


def test_rbm_draws_is_the_python_restatement(pkg):
    for seed, step, B, N in ((0, 0, 1, 1), (1, 0, 24, 70), (1, 1, 24, 70), (2, 0, 24, 70), (77, 2, 128, 33),
                             (0xFFFFFFFF, 0xFFFFFFFF, 3, 9), (5, 123456, 7, 5)):
        got, want = pkg.rbm_draws(seed, step, B, N), rbm64.draws(seed, step, B, N)
        assert got.dtype == np.float32 and got.shape == (B, N)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (seed, step)
    assert pkg.rbm_draws(1, 0, 0, 5).shape == (0, 5)
    with pytest.raises(pkg.MlggdError, match="mlggd_rbm_draws"):
        pkg.rbm_draws(1, 0, 70000, 70000)


def model_steps(layer, visible, B, steps=3, seed=7):
    """the model's chain over the GPU case: a list of (inputs of the step, its outputs)"""
    Ws, bs, x = rbm64.make_case(B)
    W, b = Ws[layer - 1].astype(np.float64), bs[layer - 1].astype(np.float64)
    K, N = W.shape
    c, dW, db, dc = np.zeros(K), np.zeros((K, N)), np.zeros(N), np.zeros(K)
    out = []
    for t in range(steps):
        v0 = rbm64.layer_input(x[t * B:(t + 1) * B], Ws, bs, layer)
        r = rbm64.draws(seed, t, B, N)
        s = rbm64.cd1_step(v0, W, b, c, r, visible, dW=dW, db=db, dc=dc, lr=rbm64.RATES["lrate"],
                           mom=rbm64.RATES["momentum"], wc=rbm64.RATES["weightcost"])
        out.append((dict(v0=v0, W=W, b=b, c=c, dW=dW, db=db, dc=dc, r=r), s))
        W, b, c, dW, db, dc = s["W"], s["b"], s["c"], s["dW"], s["db"], s["dc"]
    return out


@pytest.mark.parametrize("layer,visible", [(1, "gaussian"), (2, "bernoulli")])
@pytest.mark.parametrize("B", [24, 128])
def test_the_gpu_case_is_not_degenerate_in_the_model(layer, visible, B):
    steps = model_steps(layer, visible, B)
    samples = []
    for inp, s in steps:
        ones = s["h0s"].mean()
        assert 0.2 <= ones <= 0.8, ones
        assert np.abs(s["v1"] - s["v0"]).max() > 0.05 and np.abs(s["v1"] - s["v0"]).mean() > 0.01
        K, N = s["dW"].shape
        for k0 in range(0, K, 32):           # every 32 x 32 tile of the update has moved
            for n0 in range(0, N, 32):
                assert (s["dW"][k0:k0 + 32, n0:n0 + 32] != 0).all()
        assert (s["db"] != 0).all() and (s["dc"] != 0).all()
        samples.append(s["h0s"])
    assert np.abs(steps[1][0]["c"]).min() > 0         # from the second step on the down-pass adds a non-zero c
    assert (samples[0] != samples[1]).any() and (samples[1] != samples[2]).any()
    # the draws alone already differ between steps: same probabilities, other samples
    h0p = steps[0][1]["h0p"]
    assert (rbm64.sample(rbm64.draws(7, 0, *h0p.shape), h0p) != rbm64.sample(rbm64.draws(7, 1, *h0p.shape), h0p)).mean() > 0.1


@pytest.mark.parametrize("layer,visible", [(1, "gaussian"), (2, "bernoulli")])
def test_planted_errors_leave_the_bounds(layer, visible):
    B = 24
    inp, good = model_steps(layer, visible, B)[1]          # the second step: c, dW, db, dc are non-zero
    lr, mom, wc = (rbm64.RATES[k] for k in ("lrate", "momentum", "weightcost"))
    f = lambda a: np.asarray(a, F)
    run = lambda **kw: rbm64.cd1_step(inp["v0"], inp["W"], inp["b"], inp["c"], inp["r"], visible, lr, mom, wc, inp["dW"],
                                      inp["db"], inp["dc"], **kw)
    W32, b32, c32 = f(inp["W"]), f(inp["b"]), f(inp["c"])

    def reports(s):
        """what tests/test_gpu_rbm.py measures, on a model run rounded to fp32 where the engine holds fp32"""
        v0, h0p, h0s, v1, h1p = (f(s[k]) for k in ("v0", "h0p", "h0s", "v1", "h1p"))
        return {
            "v1": b64.compare("v1", v1, rbm64.expect_recon(h0s, W32, c32, visible)),
            "dW": b64.compare("dW", f(s["dW"]), rbm64.expect_dw(v0, v1, h0p, h1p, W32, f(inp["dW"]), lr, mom, wc)),
            "db": b64.compare("db", f(s["db"]), rbm64.expect_db(h0p, h1p, f(inp["db"]), lr, mom)),
            "dc": b64.compare("dc", f(s["dc"]), rbm64.expect_dc(v0, v1, f(inp["dc"]), lr, mom)),
        }

    # the correct step passes its own checks (the fp32 rounding of the model's inputs is inside the bounds' slack only
    # where the inputs are the engine's own; here W, b, c are rounded first and the chain redone on them)
    inp = dict(inp, W=W32.astype(np.float64), b=b32.astype(np.float64), c=c32.astype(np.float64),
               dW=f(inp["dW"]).astype(np.float64), db=f(inp["db"]).astype(np.float64), dc=f(inp["dc"]).astype(np.float64))
    ok = reports(run())
    assert all(r.ok for r in ok.values()), [str(r) for r in ok.values()]
    bad = reports(run(positive="h0s"))
    assert not bad["dW"].ok and bad["dW"].hard > 100 and not bad["db"].ok, [str(r) for r in bad.values()]
    bad = reports(run(negative_sign=-1.0))
    assert not bad["dW"].ok and bad["dW"].hard > 100 and not bad["db"].ok and not bad["dc"].ok, [str(r) for r in bad.values()]
    bad = reports(run(use_c=False))
    assert not bad["v1"].ok and bad["v1"].hard > 100, [str(r) for r in bad.values()]


def test_the_learning_case_learns_in_the_model():
    x, Ws, bs = rbm64.learn_case()
    errs = [rbm64.train64(x, Ws[0], bs[0], 16, "gaussian", 0.02, 0.5, 0.0002, seed, 4) for seed in range(1, 9)]
    for e in errs:
        assert e[-1] < 0.8 * e[0], e
    last = [e[-1] for e in errs]
    assert max(last) < 1.2 * min(last), last      # the seeds agree: a range is a usable yardstick
