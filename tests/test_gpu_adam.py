"""GPU: the Adam optimizer (BPGpu.set_optimizer, csrc/adam_rule.h, k_adam_apply) BIT FOR BIT.

What a step must leave: the gradient of the oracle's MFMA-order twin in the engine's own plan -- an OracleNet built from
the current weights, forward -> loss_colsum -> loss_grad -> backward, its grad_w / grad_b -- put through the numpy
restatement of the rule (tests/adam_model.py).  Weights, biases, both moments of each and the step count are compared
after every step; there is no tolerance in this file.  The cases live in tests/adam_cases.py, and tests/test_adam_model.py
shows on the CPU that none is degenerate."""
import contextlib

import numpy as np
import pytest

import adam_cases as ac
import adam_model as am
from test_gpu_shapefactors import KNOBS

pytestmark = pytest.mark.gpu
MOMENTUM = 0.9          # of the SGD rule: ignored in the mode, used by the tests that go back to SGD


def engine(pkg, monkeypatch, c, W, b, adam=True, **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    eng = pkg.BPGpu(1, 0, c.ls, c.B, c.lr, MOMENTUM, c.wc, W, b, c.beta, c.ml, activation=c.activation, **kw)
    if adam:
        eng.set_optimizer("adam", beta1=c.beta1, beta2=c.beta2, eps=c.eps)
    return eng


@contextlib.contextmanager
def twin_order(pyoracle, eng):
    """the oracle in the engine's own plan; the documented order is restored whatever happens"""
    pyoracle.set_gemm_order("hip", eng.out_slabs(), plan=eng.gemm_plan())
    try:
        yield
    finally:
        pyoracle.set_gemm_order("ref")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(name, got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(bits(got) != bits(want))
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: engine %r, model %r" % (name, len(bad), got.size, i, got[i], want[i]))


def snapshot(eng):
    """(weights, biases, m_w, v_w, m_b, v_b, steps) as the engine holds them"""
    we, be = eng.returnWeights()
    st = eng.optimizer_state()
    return we, be, st.m_w, st.v_w, st.m_b, st.v_b, st.steps


def same_as_model(eng, model, what=""):
    we, be, m_w, v_w, m_b, v_b, steps = snapshot(eng)
    assert steps == model.steps == eng.optimizer().steps, what
    for l in range(len(we)):
        for name, got, want in (("W", we, model.W), ("b", be, model.b), ("m_w", m_w, model.m_w), ("v_w", v_w, model.v_w),
                                ("m_b", m_b, model.m_b), ("v_b", v_b, model.v_b)):
            same("%s%s %d" % (what, name, l + 1), got[l], want[l])


def same_snapshots(a, b, what=""):
    assert a[6] == b[6], what
    for name, x, y in zip(("W", "b", "m_w", "v_w", "m_b", "v_b"), a[:6], b[:6]):
        for l, (p, q) in enumerate(zip(x, y)):
            same("%s%s %d" % (what, name, l + 1), p, q)


def pads_are_zero(eng, L):
    for l in range(1, L):
        assert not eng.debug_tensor("adam_pads", l).any(), "layer %d: pad entries of W, m_w, v_w, bias, m_b, v_b that are not zero: %s" % (
            l, eng.debug_tensor("adam_pads", l))


def step_by_step(pkg, pyoracle, monkeypatch, c, every_step=True):
    W, b = ac.net(c)
    x, t = ac.data(c)
    eng = engine(pkg, monkeypatch, c, W, b)
    try:
        assert eng.optimizer() == ("adam", np.float32(c.beta1), np.float32(c.beta2), np.float32(c.eps), 0)
        model = am.AdamNet(W, b, c.lr, c.wc, c.beta1, c.beta2, c.eps)
        with twin_order(pyoracle, eng):
            for k in range(c.steps):
                rows = slice(k * c.B, (k + 1) * c.B)
                assert eng.train(x[rows], t[rows]) == 1
                am.run(pyoracle, c, None, None, x[rows], t[rows], steps=1, model=model)
                if k == 0:  # the gradient itself first, so that a failure names the side it is on
                    gw, gb = am.oracle_gradients(pyoracle, c.ls, c.B, c.beta, c.ml, W, b, x[rows], t[rows], c.activation)
                    for l in range(1, len(c.ls)):
                        same("grad_w %d" % l, eng.debug_tensor("grad_w", l), gw[l - 1])
                        same("grad_b %d" % l, eng.debug_tensor("grad_b", l), gb[l - 1])
                if every_step or k == c.steps - 1:
                    same_as_model(eng, model, "step %d: " % (k + 1))
        pads_are_zero(eng, len(c.ls))
        assert all(not np.array_equal(a, w0) for a, w0 in zip(model.W, W))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1. bit for bit over whole runs
@pytest.mark.parametrize("c", ac.RUNS, ids=lambda c: c.id)
def test_a_whole_run_equals_the_twins_gradient_under_the_numpy_rule(pkg, pyoracle, monkeypatch, c):
    step_by_step(pkg, pyoracle, monkeypatch, c)


# 2. shapes at which the launch can go wrong
@pytest.mark.parametrize("c", ac.SHAPES, ids=lambda c: c.id)
def test_shapes_at_which_the_launch_can_go_wrong(pkg, pyoracle, monkeypatch, c):
    """pads in both directions; the unfused k_dwp as the gradient's source; a layer of more padded floats than one pass
    of the capped grid covers; 9 weight layers = 18 jobs.  The pads of W, bias and every moment stay zero."""
    if c.id == "two-trips":
        kp, np_ = -(-c.ls[0] // 32) * 32, -(-c.ls[1] // 32) * 32
        assert kp * np_ > ac.ONE_PASS_FLOATS
    step_by_step(pkg, pyoracle, monkeypatch, c, every_step=c.id != "two-trips")


# 3. the state
def test_a_restored_state_continues_as_if_uninterrupted(pkg, monkeypatch):
    c = ac.STATE
    W, b = ac.net(c)
    x, t = ac.data(c)
    B = c.B
    whole = engine(pkg, monkeypatch, c, W, b)
    first = engine(pkg, monkeypatch, c, W, b)
    try:
        for k in range(6):
            assert whole.train(x[k * B:(k + 1) * B], t[k * B:(k + 1) * B]) == 1
        for k in range(3):
            assert first.train(x[k * B:(k + 1) * B], t[k * B:(k + 1) * B]) == 1
        we, be, m_w, v_w, m_b, v_b, steps = snapshot(first)
        assert steps == 3
    finally:
        first.close()
    second = engine(pkg, monkeypatch, c, we, be)
    try:
        second.set_optimizer_state(m_w, v_w, m_b, v_b, steps)
        assert second.optimizer().steps == 3
        same_snapshots(snapshot(second), (we, be, m_w, v_w, m_b, v_b, 3), "restored: ")
        for k in range(3, 6):
            assert second.train(x[k * B:(k + 1) * B], t[k * B:(k + 1) * B]) == 1
        same_snapshots(snapshot(second), snapshot(whole), "3 + 3 against 6: ")
        # entering the mode again zeroes m, v and the step count; the weights stay
        ws = second.returnWeights()
        second.set_optimizer("adam", beta1=c.beta1, beta2=c.beta2, eps=c.eps)
        st = second.optimizer_state()
        assert st.steps == 0 and second.optimizer().steps == 0
        assert not any(a.any() for group in st[:4] for a in group)
        same_snapshots(ws + ([], [], [], [], 0), second.returnWeights() + ([], [], [], [], 0))
    finally:
        second.close()
        whole.close()


def test_a_chunk_of_several_bunches_equals_the_loop_of_single_steps(pkg, monkeypatch):
    """train_frames on a frame stream, 5 bunches and a partial one: the loop's bits, and steps counts the bunches"""
    c = ac.case("frames", [3 * 19, 70, 19], 32, 5, 42, ac.GGD)
    W, b = ac.net(c)
    rng = np.random.default_rng(c.seed)
    n = 5 * c.B + 7
    feat = rng.standard_normal((n + 2, 19)).astype(np.float32)
    targ = rng.standard_normal((n + 2, 19)).astype(np.float32)
    first = np.arange(n, dtype=np.int32)
    a = engine(pkg, monkeypatch, c, W, b)
    e = engine(pkg, monkeypatch, c, W, b)
    try:
        assert a.train_frames(feat, targ, first, targ_offset=1, fea_context=3) == 5
        assert a.optimizer().steps == 5
        for k in range(5):
            rows = first[k * c.B:(k + 1) * c.B]
            x = np.stack([feat[f:f + 3].ravel() for f in rows])
            assert e.train(x, targ[rows + 1]) == 1
        same_snapshots(snapshot(a), snapshot(e))
    finally:
        a.close()
        e.close()


# 4. SGD is untouched
def sgd_state(eng, L):
    we, be = eng.returnWeights()
    return we, be, [eng.debug_tensor("delta_w", l) for l in range(1, L)], [eng.debug_tensor("delta_b", l) for l in range(1, L)], [], [], 0


def test_sgd_is_untouched(pkg, monkeypatch):
    c = ac.case("sgd", [41, 70, 19], 32, 4, 51, ac.GGD)
    L = len(c.ls)
    W, b = ac.net(c)
    x, t = ac.data(c, 8)
    B = c.B
    plain = engine(pkg, monkeypatch, c, W, b, adam=False)
    chosen = engine(pkg, monkeypatch, c, W, b, adam=False)
    other = engine(pkg, monkeypatch, c, W, b)                  # an Adam engine that trains in the same process
    try:
        chosen.set_optimizer("sgd")
        assert chosen.optimizer().name == "sgd" == plain.optimizer().name
        assert plain.train(x[:2 * B], t[:2 * B]) == 2
        assert other.train(x[:2 * B], t[:2 * B]) == 2
        assert chosen.train(x[:2 * B], t[:2 * B]) == 2
        ref = sgd_state(plain, L)
        same_snapshots(sgd_state(chosen, L), ref, "set_optimizer('sgd') on a fresh engine: ")
        alone = engine(pkg, monkeypatch, c, W, b, adam=False)
        try:
            assert alone.train(x[:2 * B], t[:2 * B]) == 2
            same_snapshots(sgd_state(alone, L), ref, "beside an Adam engine: ")
        finally:
            alone.close()
        # Adam steps leave the momentum buffers as they were: the next SGD step against an engine that took no Adam steps,
        # was given the same weights and has the same deltas (read directly, and shown by the next step's bits)
        deltas = ref[2], ref[3]
        chosen.set_optimizer("adam")
        assert chosen.train(x[2 * B:4 * B], t[2 * B:4 * B]) == 2 and chosen.optimizer().steps == 2
        chosen.set_optimizer("sgd")
        assert chosen.optimizer().name == "sgd"
        for l in range(1, L):
            same("delta_w %d after Adam steps" % l, chosen.debug_tensor("delta_w", l), deltas[0][l - 1])
            same("delta_b %d after Adam steps" % l, chosen.debug_tensor("delta_b", l), deltas[1][l - 1])
        we, be = chosen.returnWeights()
        assert any(not np.array_equal(p, q) for p, q in zip(we, ref[0]))
        plain.set_weights(we, be)                                # same weights, the deltas of its own two SGD steps
        assert chosen.train(x[4 * B:5 * B], t[4 * B:5 * B]) == 1 and plain.train(x[4 * B:5 * B], t[4 * B:5 * B]) == 1
        same_snapshots(sgd_state(chosen, L), sgd_state(plain, L), "the SGD step after Adam steps: ")
    finally:
        plain.close()
        chosen.close()
        other.close()


# 5. composition: finite, and two runs give the same bits
def twice(run):
    a, b = run(), run()
    same_snapshots(a, b, "second run: ")
    for group in a[:6]:
        for arr in group:
            assert np.isfinite(arr).all()
    assert a[6] > 0 and any(arr.any() for arr in a[3])
    return a


def test_with_dropout(pkg, monkeypatch):
    c = ac.case("dropout", [41, 70, 33, 19], 32, 4, 61, ac.GGD)
    W, b = ac.net(c)
    x, t = ac.data(c)

    def run():
        eng = engine(pkg, monkeypatch, c, W, b, dropoutflag=1, visible_omit=0.2, hid_omit=0.5)
        try:
            assert eng.train(x, t) == c.steps
            return snapshot(eng)
        finally:
            eng.close()
    twice(run)


def test_with_a_learned_scale(pkg, monkeypatch):
    c = ac.case("scale", [41, 70, 19], 32, 4, 62, ac.GGD)
    W, b = ac.net(c)
    x, t = ac.data(c)

    def run():
        eng = engine(pkg, monkeypatch, c, W, b)
        try:
            eng.set_scale_mode("learned")
            assert eng.train(x, t) == c.steps and eng.scale_mode().steps == c.steps
            a, v = eng.scale_state()
            assert np.isfinite(a).all() and (a > 0).all()
            return snapshot(eng)
        finally:
            eng.close()
    twice(run)


def test_a_mask_engine_through_train_waves(pkg, synth):
    from test_gpu_mask import B as MASK_B
    from test_gpu_mask import CTX, Train
    t = Train(pkg, synth, 8)

    def run():
        eng = t.engine(1, 1.0, cap=t.n + 1)
        try:
            eng.set_optimizer("adam")
            eng.set_noise(t.noise)
            assert eng.train_waves(t.cleans, t.snr, t.start, t.mean, t.inv, t.first, t.toff, noise_seg=t.seg, fea_context=CTX,
                                   fs_khz=t.fs) == t.n // MASK_B
            assert eng.optimizer().steps == t.n // MASK_B
            return snapshot(eng)
        finally:
            eng.close()
    twice(run)


# 6. refusals
def test_refusals_leave_the_optimizer_as_it_was(pkg, monkeypatch):
    c = ac.case("refusals", [41, 70, 19], 32, 1, 71, ac.GGD)
    W, b = ac.net(c)
    L = pkg.load()
    ARG, STATE = 1, 4                                            # MLGGD_ERR_ARG, MLGGD_ERR_STATE (include/mlggd.h)
    eng = engine(pkg, monkeypatch, c, W, b, adam=False)
    try:
        before = eng.optimizer()
        nan, inf = float("nan"), float("inf")
        for kind, b1, b2, eps in ((2, 0.9, 0.999, 1e-8), (-1, 0.9, 0.999, 1e-8), (1, 1.0, 0.999, 1e-8), (1, -0.1, 0.999, 1e-8),
                                  (1, 0.9, 1.0, 1e-8), (1, 0.9, nan, 1e-8), (1, 0.9, 0.999, 0.0), (1, 0.9, 0.999, -1e-8),
                                  (1, 0.9, 0.999, inf), (1, 0.9, 0.999, nan), (0, 1.5, 0.999, 1e-8)):
            assert L.mlggd_set_optimizer(eng._h, kind, b1, b2, eps) == ARG, (kind, b1, b2, eps)
            assert eng.optimizer() == before
        with pytest.raises(ValueError):
            eng.set_optimizer("adamw")
        # state calls outside the mode
        shapes = [(c.ls[l], c.ls[l + 1]) for l in range(len(c.ls) - 1)]
        zw = [np.zeros(s, np.float32) for s in shapes]
        zb = [np.zeros(s[1], np.float32) for s in shapes]
        with pytest.raises(pkg.MlggdError, match="not Adam"):
            eng.optimizer_state()
        with pytest.raises(pkg.MlggdError, match="not Adam"):
            eng.set_optimizer_state(zw, zw, zb, zb, 0)
        assert L.mlggd_get_optimizer_state(eng._h, *[pkg._ptr_array(a) for a in (zw, zw, zb, zb)]) == STATE
        assert eng.optimizer() == before
        # in the mode: negative steps, a negative second moment, a moment that is not finite
        eng.set_optimizer("adam", beta1=0.8, beta2=0.9, eps=1e-6)
        mode = eng.optimizer()
        assert mode == ("adam", np.float32(0.8), np.float32(0.9), np.float32(1e-6), 0)
        assert L.mlggd_set_optimizer_state(eng._h, *[pkg._ptr_array(a) for a in (zw, zw, zb, zb)], -1) == ARG
        neg = [a.copy() for a in zw]
        neg[1][3, 2] = -1.0
        with pytest.raises(pkg.MlggdError, match="layer 2"):
            eng.set_optimizer_state(zw, neg, zb, zb, 1)
        bad = [a.copy() for a in zb]
        bad[0][5] = nan
        with pytest.raises(pkg.MlggdError, match="layer 1"):
            eng.set_optimizer_state(zw, zw, bad, zb, 1)
        assert L.mlggd_set_optimizer(eng._h, 1, 0.9, 0.999, 0.0) == ARG
        assert eng.optimizer() == mode
        # a communicator or an emulated world on an engine in the mode
        with pytest.raises(pkg.MlggdError, match="Adam"):
            eng.fake_world(2, allreduce=True)
        assert L.mlggd_debug_fake_world(eng._h, 2, 2) == STATE
        assert L.mlggd_comm_init(eng._h, bytes(pkg.UNIQUE_ID_BYTES), 1, 0) == STATE
        assert eng.optimizer() == mode
    finally:
        eng.close()
    # the mode on an engine that has joined an emulated world
    eng = engine(pkg, monkeypatch, c, W, b, adam=False)
    try:
        eng.fake_world(2, allreduce=True)
        before = eng.optimizer()
        assert L.mlggd_set_optimizer(eng._h, 1, 0.9, 0.999, 1e-8) == STATE
        with pytest.raises(pkg.MlggdError, match="single-device"):
            eng.set_optimizer("adam")
        assert eng.optimizer() == before == ("sgd", np.float32(0.9), np.float32(0.999), np.float32(1e-8), 0)
        eng.set_optimizer("sgd")                                 # SGD is what it runs
    finally:
        eng.close()
