"""CPU: the float64 model of rectified-linear hidden units (tests/relu64.py) and the switch's host-side plumbing.

The bounds pass an fp32 numpy restatement of the engine's two rules on random nets and refuse three slips -- a leaky
rectifier with slope 0.01, a backward mask taken from y >= 0 instead of y > 0, a forward pass that forgets the bias.
The case the GPU test runs is shown not to be degenerate (both signs of z in every hidden layer, for three steps), and
the exact-data case is shown to be exact.  Without a device: mlggd_create refuses an unknown activation, each of the
three executables refuses one before it opens anything, and the Python keyword maps strings and integers."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import bounds64 as b6
import hostlib
import relu64 as r6

NETS = [([45, 70, 33, 9], 24), ([45, 70, 33, 9], 128), ([531, 97, 33, 1, 40], 33), ([96, 128, 128, 40], 64)]


def fp32_step(ls, n, seed, mut=None):
    """hidden activations and dX of an fp32 numpy ReLU net, each from the fp32 inputs it was computed from"""
    W, b = b6.make_net(ls, seed)
    x, t = b6.make_data(ls, n, seed + 1)
    L = len(ls)
    y = {0: x}
    for l in range(1, L - 1):
        y[l] = r6.relu_layer_f32(y[l - 1], W[l - 1], b[l - 1], mut)
    out = (y[L - 2] @ W[L - 2] + b[L - 2]).astype(np.float32)
    d = {L - 1: b6.expect_loss(out, t, 2.0, 0)[0].ref.astype(np.float32)}
    for l in range(L - 2, 0, -1):
        d[l] = r6.dx_relu_f32(d[l + 1], W[l], y[l], mut)
    return W, b, y, d


def reports(ls, n, seed, mut=None):
    W, b, y, d = fp32_step(ls, n, seed, mut)
    L = len(ls)
    fwd = [b6.compare("fwd %d" % l, y[l], r6.expect_relu_layer(y[l - 1], W[l - 1], b[l - 1])) for l in range(1, L - 1)]
    dx = [b6.compare("dx %d" % l, d[l], r6.expect_dx_relu(d[l + 1], W[l], y[l])) for l in range(1, L - 1)]
    return fwd, dx


@pytest.mark.parametrize("ls,n", NETS)
def test_the_fp32_rules_pass_the_bounds(ls, n):
    fwd, dx = reports(ls, n, seed=n)
    bad = [r.line() for r in fwd + dx if not r.ok]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("ls,n", NETS[:2])
def test_planted_slips_fail_the_bounds(ls, n):
    fwd, dx = reports(ls, n, seed=n, mut="leaky")
    assert not fwd[0].ok and not dx[-1].ok                    # a leak shows in both directions
    fwd, dx = reports(ls, n, seed=n, mut="no bias")
    assert not fwd[0].ok
    fwd, dx = reports(ls, n, seed=n, mut="mask y >= 0")
    assert all(r.ok for r in fwd) and not dx[-1].ok           # the forward is untouched; the gradient leaks through y == 0


def test_exactly_zero_is_demanded_where_the_sum_is_negative_in_any_order():
    """a result of 1e-30 where z is far below zero passes |y - max(z, 0)| <= E_z but not the exact-zero region"""
    ls, n = NETS[0]
    W, b, y, _ = fp32_step(ls, n, seed=5)
    e = r6.expect_relu_layer(y[0], W[0], b[0])
    assert (e.bound == 0).any() and (e.ref[e.bound == 0] == 0).all()
    got = y[1].copy()
    got[e.bound == 0] = np.float32(1e-30)
    assert not b6.compare("fwd 1", got, e).ok and b6.compare("fwd 1", y[1], e).ok


@pytest.mark.parametrize("ml,beta", [(0, 2.0), (0, 1.0), (1, 0.9)])
@pytest.mark.parametrize("n", [24, 128])
def test_the_gpu_case_is_not_degenerate(ml, beta, n):
    """the seed, net and data of tests/test_gpu_relu.py's per-kernel case in float64: for three steps between 20 % and
    80 % of every hidden layer's units are off, so both arms of both rules are exercised"""
    ls = r6.CASE_LS
    W, b = b6.make_net(ls, r6.CASE_SEED)
    x, t = b6.make_data(ls, 3 * n, r6.CASE_SEED + 1)
    lr, mom, wc = r6.CASE_HP
    dW, db = [np.zeros_like(w) for w in W], [np.zeros_like(v) for v in b]
    lo, hi = r6.ZERO_FRACTION
    for k in range(3):
        m = r6.step64(x[k * n:(k + 1) * n], t[k * n:(k + 1) * n], W, b, dW, db, lr, mom, wc, beta, ml)
        for l, y in m["y"].items():
            assert lo <= (y == 0).mean() <= hi, (k, l, (y == 0).mean())
        W, b, dW, db = m["W_new"], m["b_new"], m["dW_new"], m["db_new"]


def test_the_exact_case_is_exact():
    """every GEMM and update of the exact-data step stays below 2^24 quanta per element, every float64 value of the step
    is an fp32 number, and the hidden layer has units on and off"""
    c = r6.exact_case()
    rows, m = r6.exact_case_quanta(c)
    for name, worst in rows:
        assert worst < 2.0 ** 24, (name, worst)
    for v in [m["out"], m["y"][1], m["dedx"][1], m["dedx"][2]] + m["dW_new"] + m["db_new"] + m["W_new"] + m["b_new"]:
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    assert 0.2 <= (m["y"][1] == 0).mean() <= 0.8 and np.abs(m["dW_new"][0]).max() > 0


# ---------------------------------------------------------------------------------------------------------------------
# plumbing that needs no device
def test_create_rejects_an_unknown_activation_before_touching_a_device(pkg):
    L = pkg.load()
    fp = ctypes.POINTER(ctypes.c_float)
    arr = (fp * pkg.MAXLAYER)()  # never dereferenced: the checks come first

    def create(act):
        cfg = pkg._Config()
        cfg.struct_size = ctypes.sizeof(pkg._Config)
        cfg.numlayers = 3
        for i, v in enumerate([100, 50, 10]):
            cfg.layersizes[i] = v
        cfg.bunchsize = 8
        cfg.activation = act
        h = ctypes.c_void_p()
        rc = L.mlggd_create(ctypes.byref(cfg), arr, arr, ctypes.byref(h))
        return rc, L.mlggd_last_error().decode(), h

    for act in (2, -1):
        rc, msg, h = create(act)
        assert rc == 1 and "activation" in msg and not h, (act, rc, msg)
    assert "mlggd_get_activation" in pkg.EXPORTS
    assert pkg._Config.activation.offset == 4 * (4 + 10 + 1 + 4 + 2 + 2 + 1)      # the first of the reserved words


@pytest.mark.parametrize("tool,argv", [
    ("BPtrain_Sigmoid", ["layersizes=10,5,3", "activation=bogus"]),
    ("BPtrain_ReLU", ["activation=bogus"]),
    ("enhance_wav", ["wts=a.wts", "norm_file=a.norm", "in=a.wav", "out=b.wav", "activation=bogus"]),
    ("enhance_lps", ["wts=a.wts", "norm_file=a.norm", "in=a.lps", "out=b.htk", "activation=bogus"])])
def test_a_tool_refuses_an_unknown_activation(pkg, tool, argv, tmp_path):
    pkg.build()
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    r = subprocess.run([os.path.join(hostlib.HOST, tool)] + argv, capture_output=True, text=True, timeout=60,
                       cwd=tmp_path)
    assert r.returncode != 0 and "activation=bogus" in r.stderr, r.stderr
    assert not os.listdir(tmp_path)                                       # nothing was opened for writing


def test_the_python_keyword(pkg):
    assert [pkg.activation_code(a) for a in ("sigmoid", "relu", 0, 1, np.int32(1))] == [0, 1, 0, 1, 1]
    for bad in ("bogus", "ReLU", 2, -1, 1.0, None, True):
        with pytest.raises(ValueError, match="activation"):
            pkg.activation_code(bad)
    W, b = b6.make_net([15, 8, 5], 1)
    with pytest.raises(ValueError, match="activation"):                   # before the library or a device is touched
        pkg.BPGpu(1, 0, [15, 8, 5], 8, 0.1, 0.9, 0.0, W, b, 2.0, 0, activation="bogus")
