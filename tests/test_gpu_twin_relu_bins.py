"""GPU: rectified-linear hidden units and a shape factor per output bin against the oracle's MFMA-order twin, BIT FOR BIT.

The twin (pyoracle.set_gemm_order("hip", ...)) restates the HIP kernels' summation order, exponential and power on the
CPU; since it knows both features -- OracleNet(activation="relu"), OracleNet.set_shapefactors -- whole training runs of
ReLU nets and of nets trained under a mixed shape vector must leave exactly its bits, as sigmoid nets with a scalar
shape do (tests/test_gpu_mfma_order.py).  A ReLU step has no exponential at all, so what is compared is GEMM order,
indexing, the two selects and IEEE arithmetic; under a mixed vector a thread that read its neighbour's beta would differ
here, where a comparison of the engine with itself shares the slip and a float64 bound may hide it.

Every comparison is of bits: there is no tolerance in this file.  Ordinary random data: Glorot weights, biases U(+-0.5),
standard-normal inputs and targets (tests/twin_cases.py).  Every ReLU case asserts on the engine's own y that between
20 % and 80 % of each hidden layer are exactly 0 in the last step, and that the weights moved;
tests/test_oracle_relu_bins.py shows the same on the CPU, where the seeds were picked."""
import contextlib

import numpy as np
import pytest

import shapes64 as s6
import twin_cases as tc
from test_gpu_dp_vs_float64 import MODES, set_world, stacked
from test_gpu_shapefactors import HP as BIN_HP
from test_gpu_shapefactors import KNOBS, SINGLE, WORLDS
from test_gpu_shapefactors import engine as bin_engine
from test_gpu_shapefactors import frames as bin_frames
from test_gpu_shapefactors import ls_of, rows_per_step
from test_gpu_shapefactors import net as bin_net

pytestmark = pytest.mark.gpu


def engine(pkg, monkeypatch, ls, B, ml, beta, W, b, env=None, activation="relu", seed=1, **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    eng = pkg.BPGpu(seed, 0, ls, B, *tc.HP, W, b, beta, ml, activation=activation, **kw)
    assert eng.activation == activation
    return eng


@contextlib.contextmanager
def twin_of(pyoracle, eng, *args, world=1, allreduce=False, **kw):
    """an OracleNet under the twin in the engine's own plan; the documented order is restored whatever happens"""
    pyoracle.set_gemm_order("hip", eng.out_slabs(), plan=eng.gemm_plan(), dp_world=world, dp_allreduce=allreduce)
    try:
        twin = pyoracle.OracleNet(*args, **kw)
        try:
            yield twin
        finally:
            twin.close()
    finally:
        pyoracle.set_gemm_order("ref")


def same(name, got, want):
    got = np.ascontiguousarray(got, np.float32)
    want = np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        i = tuple(bad[0])
        raise AssertionError("%s: %d of %d elements differ, first at %s: engine %r, twin %r"
                             % (name, len(bad), got.size, i, got[i], want[i]))


def same_state(eng, twin, L, ml):
    """delta_w, delta_b, W, b of every layer and the scalefactor"""
    we, be = eng.returnWeights()
    wt, bt = twin.get_weights()
    for l in range(1, L):
        same("delta_w %d" % l, eng.debug_tensor("delta_w", l), twin.tensor("delta_w", l))
        same("delta_b %d" % l, eng.debug_tensor("delta_b", l), twin.tensor("delta_b", l))
        same("W %d" % l, we[l - 1], wt[l - 1])
        same("b %d" % l, be[l - 1], bt[l - 1])
    if ml:
        same("scalefactor", eng.scalefactor(), twin.tensor("scalefactor"))
    return we


def same_step(eng, twin, L, B):
    """the last step's y of every hidden layer, out and every dedx -- in the order in which a step computes them, so that
    the first failure names the first tensor that diverged"""
    for l in range(1, L - 1):
        same("y %d" % l, eng.debug_tensor("y", l), twin.tensor("y", l, rows=B))
    same("out", eng.debug_tensor("out"), twin.tensor("out", rows=B))
    for l in range(L - 1, 0, -1):
        same("dedx %d" % l, eng.debug_tensor("dedx", l), twin.tensor("dedx", l, rows=B))


def same_cv(eng, twin, ls, n, seed, ml):
    """cv_all's three numbers on n frames (a whole bunch and a partial one), sums formed in the reference's host order"""
    cx, ct = tc.data(ls, n, seed + 1)
    eng.set_cv_device_reduce(False)
    sq, ab, ll = eng.cv_all(cx, ct)
    assert sq == twin.cv_sqerr(cx, ct), "sqerr"
    assert ab == twin.cv_abserr(cx, ct), "abserr"
    if ml:
        assert ll == twin.cv_loglik(cx, ct), "loglik"


def trained_and_alive(eng, we, W0, L):
    assert all(not np.array_equal(a, b) for a, b in zip(we, W0))            # every layer's weights moved
    fr = tc.zero_fractions(eng, L, None)
    print("zero fractions of y:", fr)
    tc.assert_not_degenerate(fr)


def whole_run(pkg, pyoracle, monkeypatch, ls, B, steps, seed, ml, beta, env=None, s_out=None, plan_check=None):
    L = len(ls)
    W, b = tc.net(ls, seed)
    x, t = tc.data(ls, steps * B, seed)
    eng = engine(pkg, monkeypatch, ls, B, ml, beta, W, b, env)
    try:
        if s_out is not None:
            assert eng.out_slabs() == s_out
        if plan_check is not None:
            plan_check(eng.gemm_plan())
        with twin_of(pyoracle, eng, ls, B, *tc.HP, beta, ml, W, b, activation="relu") as twin:
            assert eng.train(x, t) == steps and twin.train(x, t) == steps
            same_step(eng, twin, L, B)
            we = same_state(eng, twin, L, ml)
            trained_and_alive(eng, we, W, L)
            same_cv(eng, twin, ls, B + 7, seed, ml)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# a. whole ReLU runs
@pytest.mark.parametrize("ml,beta", tc.LOSSES)
@pytest.mark.parametrize("ls,B,steps,seed", tc.RUNS, ids=lambda v: str(v).replace(" ", "") if isinstance(v, list) else None)
def test_a_whole_relu_run_equals_the_twin(pkg, pyoracle, monkeypatch, ls, B, steps, seed, ml, beta):
    """[45, 70, 33, 9] at B = 24 and 128 (edge tiles in every layer, a one-row strip, a partial frame tile), 6 steps, and
    [1210, 1060, 70, 262, 40] at B = 96 (a wave's K range of several chunks plus a partial one, a single partial chunk, an
    empty one), 3 steps, under every loss: y of every hidden layer, out, every dedx, delta_w, delta_b, W, b, the
    scalefactor and cv_all's three numbers on B + 7 frames"""
    whole_run(pkg, pyoracle, monkeypatch, ls, B, steps, seed, ml, beta)


@pytest.mark.parametrize("ls,B,steps,seed,ml,beta", tc.SINGLE_RUNS, ids=["real_widths", "dwp4", "dwp8", "dx_both_forms"])
def test_relu_runs_at_the_real_widths_and_behind_the_wide_dw_kernels(pkg, pyoracle, monkeypatch, ls, B, steps, seed, ml, beta):
    """2827-2048^3-257 at B = 128, 8 ML-GGD steps with beta = 1: only there does the persistent k_dwp walk many tiles per
    workgroup after ReLU-sparse activations.  [300, 96, 40] at B = 256 and 512: k_dwp<4> / k_dwp<8> behind a ReLU layer.
    [40, 531, 64, 19] at B = 512: the dX launch over the 531 units has 17 x 16 = 272 workgroups, more than 256, and takes
    its operands through staging registers; the one over the 64 units has 2 x 16 and takes them by LDS-DMA -- both
    forms of k_dx<.., ACT_RELU> in one run (544 is no multiple of 64 and 2 x 8 tiles of 64 x 64 are fewer than the CUs, so
    the plan must say 4 waves for both; 8 units of 64 frames, so k_dwp<8> forms the gradients)."""
    check = None
    if ls == tc.DX_BOTH_LS:
        assert tc.dx_workgroups(ls, B) == {2: 17 * 16, 3: 2 * 16} and 2 * 16 <= 256 < 17 * 16 and B % 64 == 0 and B // 64 == 8

        def check(got):
            assert got[1][1] == 4 and got[2][1] == 4, got

    whole_run(pkg, pyoracle, monkeypatch, ls, B, steps, seed, ml, beta, plan_check=check)


# ---------------------------------------------------------------------------------------------------------------------
# b. the 64 x 64 kernels
@pytest.mark.parametrize("ls,B,steps,seed,plan", tc.TILE64, ids=["96-128-128-40", "64-192-128-257"])
def test_relu_through_the_64x64_tile_kernels_equals_the_twin(pkg, pyoracle, monkeypatch, ls, B, steps, seed, plan):
    """MLGGD_TILE64=2: k_fwd64<FWD_RELU> for every hidden forward, k_dx64<ACT_RELU> for every dX launch -- the plan must
    say so -- one chain per output element in the twin (waves = 1)"""
    L = len(ls)

    def check(got):
        assert all(got[l - 1][0] == 1 for l in range(1, L - 1)), got       # hidden forwards
        assert all(got[l - 1][1] == 1 for l in range(2, L)), got           # dX launches (layer 1 has none)

    whole_run(pkg, pyoracle, monkeypatch, ls, B, steps, seed, *tc.TILE64_LOSS, env={"MLGGD_TILE64": "2"}, plan_check=check)


# ---------------------------------------------------------------------------------------------------------------------
# c. the output layer's slabs behind a ReLU layer
@pytest.mark.parametrize("s_out", [None, "1", "3"])
def test_output_slabs_behind_a_relu_layer_equal_the_twin(pkg, pyoracle, monkeypatch, s_out):
    ls, B, steps, seed, ml, beta = tc.S_OUT_CASE
    whole_run(pkg, pyoracle, monkeypatch, ls, B, steps, seed, ml, beta, env={"MLGGD_S_OUT": s_out} if s_out else None,
              s_out=int(s_out) if s_out else None)


# ---------------------------------------------------------------------------------------------------------------------
# d. ReLU with dropout
@pytest.mark.parametrize("ml,beta", tc.DROP_LOSSES)
def test_relu_dropout_runs_equal_the_twin(pkg, pyoracle, monkeypatch, ml, beta):
    """[771, 256, 192, 257], B = 128, 6 steps, visible_omit 0.2, hid_omit 0.5, seed 77: the same masks on both sides (the
    oracle restates the engine's counter hash), a dropped unit's y is 0 and y > 0 then gives it no gradient.  Weights, y
    and dedx after training; the CV forward of 300 rows bunch by bunch (weights scaled by the keep-probability around
    each GEMM); the weights after that scale / unscale round trip."""
    ls, B, steps, seed = tc.DROP_CASE
    L = len(ls)
    W, b = tc.net(ls, seed)
    x, t = tc.data(ls, steps * B, seed)
    eng = engine(pkg, monkeypatch, ls, B, ml, beta, W, b, seed=tc.DROP_SEED, **tc.DROP_KW)
    try:
        with twin_of(pyoracle, eng, ls, B, *tc.HP, beta, ml, W, b, activation="relu", random_seed=tc.DROP_SEED,
                     **tc.DROP_KW) as twin:
            assert eng.train(x, t) == steps and twin.train(x, t) == steps
            same_step(eng, twin, L, B)
            we = same_state(eng, twin, L, ml)
            trained_and_alive(eng, we, W, L)
            for l in range(1, L - 1):                                     # more zeros than the rectifier alone leaves
                y, d = eng.debug_tensor("y", l), eng.debug_tensor("dedx", l)
                assert (y == 0).mean() > 0.5 and (d[y == 0] == 0).all()
            out = eng.forward(x[:300])
            want = np.concatenate([twin.cv_forward(x[i:min(i + B, 300)]) for i in range(0, 300, B)])
            same("CV forward of 300 rows", out, want)
            after = eng.returnWeights()[0]
            for l, (p, q) in enumerate(zip(after, twin.get_weights()[0]), 1):
                same("W %d after the scale / unscale round trip" % l, p, q)
            assert any(not np.array_equal(p, q) for p, q in zip(after, we))   # ... which is not the identity
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# e. emulated worlds
@pytest.mark.parametrize("world", tc.WORLD_SIZES)
@pytest.mark.parametrize("mode", list(MODES))
def test_relu_in_an_emulated_world_equals_the_data_parallel_twin(pkg, pyoracle, monkeypatch, mode, world):
    """fake_world(w) x 32 rows under each exchange, ML-GGD beta 0.9, 3 steps, against the twin's data-parallel form at
    bunchsize w x 32: the ranks' ML statistics (and, gradient all-reduce, their weight / bias gradients) met in rank
    order.  The ranks' y, out and dedx of the last step, stacked in rank order, are the twin's rows."""
    ls, B, steps, seed, ml, beta = tc.WORLD_CASE
    L, n = len(ls), world * B
    W, b = tc.net(ls, seed)
    x, t = tc.data(ls, steps * n, seed)
    eng = engine(pkg, monkeypatch, ls, B, ml, beta, W, b)
    try:
        set_world(eng, mode, world)
        assert eng.dp_mode() == MODES[mode]
        eng.keep_ranks()
        with twin_of(pyoracle, eng, ls, n, *tc.HP, beta, ml, W, b, activation="relu", world=world,
                     allreduce=mode == "allreduce") as twin:
            assert eng.train(x, t) == steps and twin.train(x, t) == steps
            ys = {l: stacked(eng, "y", l, world) for l in range(1, L - 1)}
            for l in range(1, L - 1):
                same("y %d" % l, ys[l], twin.tensor("y", l, rows=n))
            same("out", stacked(eng, "out", 0, world), twin.tensor("out", rows=n))
            for l in range(L - 1, 0, -1):
                same("dedx %d" % l, stacked(eng, "dedx", l, world), twin.tensor("dedx", l, rows=n))
            we = same_state(eng, twin, L, ml)
            assert all(not np.array_equal(p, q) for p, q in zip(we, W))
            tc.assert_not_degenerate({l: float((y == 0).mean()) for l, y in ys.items()})
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# f. a mixed shape vector, sigmoid net
def bins_run(pkg, pyoracle, monkeypatch, mode, D, B, betas, steps=4):
    """tests/test_gpu_shapefactors.py's net, frames and engine (its own shapefactor is 1.7: the vector must be what
    counts) under `betas`, beside the twin with the same vector -- for the emulated worlds in its data-parallel form at
    bunchsize 2 B"""
    ls, L = ls_of(D), 3
    world = 2 if mode in ("gather", "allreduce") else 1
    n = rows_per_step(mode, B)
    W, b = bin_net(D)
    x, t = bin_frames(D, steps * n, seed=5)
    cx, ct = bin_frames(D, B + 7, seed=4)
    eng = bin_engine(pkg, monkeypatch, mode, D, B, 1.7)
    try:
        eng.set_shapefactors(betas)
        with twin_of(pyoracle, eng, ls, n, *BIN_HP, 1.7, 1, W, b, shapefactors=betas, world=world,
                     allreduce=mode == "allreduce") as twin:
            assert eng.train(x, t) == steps and twin.train(x, t) == steps
            we = same_state(eng, twin, L, 1)
            assert all(not np.array_equal(p, q) for p, q in zip(we, W))
            eng.set_cv_device_reduce(False)                               # the reference's host order: the twin's
            sq, ab, ll = eng.cv_all(cx, ct)
            assert sq == twin.cv_sqerr(cx, ct), "sqerr"
            assert ab == twin.cv_abserr(cx, ct), "abserr"
            assert ll == twin.cv_loglik(cx, ct), "loglik"
            twin.set_shapefactors(None)
            assert ll != twin.cv_loglik(cx, ct)                           # the vector is what the number was formed with
    finally:
        eng.close()


@pytest.mark.parametrize("mode,D,B", SINGLE + WORLDS)
def test_a_mixed_shape_vector_equals_the_twin(pkg, pyoracle, monkeypatch, mode, D, B):
    """40-64-D, D = 19 / 257, B = 32 / 160 (partly filled unit groups, the fused kernel's second partial pass), fused,
    unfused (MLGGD_LOSS_FUSE=0) and the two emulated worlds, shapes64.mixed(D): 4 steps leave every bit of the twin's W,
    b, delta_w, delta_b and scalefactor, and cv_all on B + 7 frames its three numbers"""
    bins_run(pkg, pyoracle, monkeypatch, mode, D, B, s6.mixed(D))


@pytest.mark.parametrize("mode,B", [("fused", 160), ("unfused", 160), ("gather", 32), ("allreduce", 160)])
def test_a_vector_of_257_different_shapes_equals_the_twin(pkg, pyoracle, monkeypatch, mode, B):
    """betas drawn from U(0.5, 2.2), no two equal: the shape of a neighbouring bin, read by mistake, cannot coincide"""
    bins_run(pkg, pyoracle, monkeypatch, mode, 257, B, tc.distinct_betas(257))


# ---------------------------------------------------------------------------------------------------------------------
# g. both features and dropout together
def test_relu_with_a_mixed_vector_and_dropout_equals_the_twin(pkg, pyoracle, monkeypatch):
    ls, B, steps, seed = tc.ALL_CASE
    L, betas = len(ls), s6.mixed(ls[-1])
    W, b = tc.net(ls, seed)
    x, t = tc.data(ls, steps * B, seed)
    eng = engine(pkg, monkeypatch, ls, B, 1, 1.7, W, b, seed=tc.DROP_SEED, **tc.ALL_DROP_KW)
    try:
        eng.set_shapefactors(betas)
        with twin_of(pyoracle, eng, ls, B, *tc.HP, 1.7, 1, W, b, activation="relu", shapefactors=betas,
                     random_seed=tc.DROP_SEED, **tc.ALL_DROP_KW) as twin:
            assert eng.train(x, t) == steps and twin.train(x, t) == steps
            same_step(eng, twin, L, B)
            we = same_state(eng, twin, L, 1)
            trained_and_alive(eng, we, W, L)
    finally:
        eng.close()
