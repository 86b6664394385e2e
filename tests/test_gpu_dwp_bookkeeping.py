"""GPU: the tile bookkeeping of the persistent dW + update kernel (csrc/kernels.hip.h dwp_body) at the smallest shapes
at which it can go wrong, against the oracle's MFMA-order twin, BIT FOR BIT (0 differing elements, no tolerance).

What the bookkeeping is: which rows of a 64 x 64 tile exist is decided by the tile record's buffer descriptor (szW ends
with the tile's last real row, csrc/engine.hip dwp_table) and no longer by a per-lane test; which columns exist is a
per-lane test formed once per tile; the four 16-byte pieces of a lane are one add apart; the LDS-DMA operand loads carry
their row in the scalar offset; the bias pointers of a record stay in the fetched vector until the rare bias update
wants them.  The contract these must keep: pad rows and pad columns of W / delta are never
written -- a store that leaked into one shows up as a wrong sum in the NEXT layer's forward, which is what the last
test looks at -- and whatever is cached per tile follows the record when one launch walks layers of different widths.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HP = (0.1, 0.9, 1e-5)                      # lrate, momentum, weightcost
RAGGED = [75, 96, 160, 33]                 # four different ldA / Np in one k_dwp launch; every layer has an edge tile


def differing(name, a, b):
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    n = int((a.view(np.int32) != b.view(np.int32)).sum())
    print("%s: %d of %d elements differ" % (name, n, a.size))
    return n


def random_net(ls, seed):
    rng = np.random.default_rng(seed)
    ws = [rng.normal(0, 0.05, (ls[l], ls[l + 1])).astype(np.float32) for l in range(len(ls) - 1)]
    bs = [rng.normal(0, 0.1, ls[l + 1]).astype(np.float32) for l in range(len(ls) - 1)]
    return ws, bs


def random_frames(n, ls, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 1, (n, ls[0])).astype(np.float32), rng.normal(0, 1, (n, ls[-1])).astype(np.float32)


@pytest.mark.parametrize("K,D,B", [
    (65, 33, 64),       # a second tile row with one real row; one column tile 33 wide; one unit per tile
    (127, 257, 128),    # 257 -> a last column tile with a single real column (the headline's edge, small)
    (203, 100, 100),    # B not a power of two: the division form of G / n; frames 100..127 padded
    (64, 64, 256),      # no edge at all; four units per tile
    (300, 40, 512),     # eight units per tile
    (96, 64, 1024),     # sixteen units: more than k_dwp takes on one device -- k_dw<1> over sixteen 64-frame chunks (the
                        # sixteen-unit dwp_body runs over gathered factors only: tests/test_gpu_dw_choices.py)
])
def test_one_layer_nets_equal_the_twin_bitwise(pkg, pyoracle, K, D, B):
    """Two MMSE steps (the second with momentum and weight decay at work): dEdX, delta_w, delta_b, then W and b."""
    ws, bs = random_net([K, D], K + D + B)
    x, t = random_frames(2 * B, [K, D], K + D + B + 1)
    eng = pkg.BPGpu(1, 0, [K, D], B, *HP, ws, bs, 2.0, 0)
    try:
        pyoracle.set_gemm_order("hip", eng.out_slabs(), plan=eng.gemm_plan())
        twin = pyoracle.OracleNet([K, D], B, *HP, 2.0, 0, ws, bs)
        bad = 0
        for step in (0, 1):
            rows = slice(step * B, (step + 1) * B)
            assert eng.train(x[rows], t[rows]) == 1 and twin.train(x[rows], t[rows]) == 1
            tag = "(%d, %d, %d) step %d " % (K, D, B, step)
            bad += differing(tag + "dedx", eng.debug_tensor("dedx", 1), twin.tensor("dedx", 1, rows=B))
            bad += differing(tag + "delta_w", eng.debug_tensor("delta_w", 1), twin.tensor("delta_w", 1))
            bad += differing(tag + "delta_b", eng.debug_tensor("delta_b", 1), twin.tensor("delta_b", 1))
            (we,), (be,) = eng.returnWeights()
            (wt,), (bt,) = twin.get_weights()
            bad += differing(tag + "W", we, wt) + differing(tag + "b", be, bt)
        assert not np.array_equal(we, ws[0])                      # the net was trained
        twin.close()
    finally:
        pyoracle.set_gemm_order("ref")
        eng.close()
    assert bad == 0


def ragged_run(pkg, pyoracle, hp, steps=3, fresh=0):
    """`steps` MMSE steps of the ragged net on the engine and on the twin -> differing elements over all weights, biases
    and delta_w (and, with `fresh` > 0, over the forward of that many new frames)."""
    ls, B = RAGGED, 128
    ws, bs = random_net(ls, 7)
    x, t = random_frames(steps * B, ls, 8)
    eng = pkg.BPGpu(1, 0, ls, B, *hp, ws, bs, 2.0, 0)
    try:
        pyoracle.set_gemm_order("hip", eng.out_slabs(), plan=eng.gemm_plan())
        twin = pyoracle.OracleNet(ls, B, *hp, 2.0, 0, ws, bs)
        assert eng.train(x, t) == steps and twin.train(x, t) == steps
        we, be = eng.returnWeights()
        wt, bt = twin.get_weights()
        bad = 0
        for l in range(len(we)):
            bad += differing("W_%d" % (l + 1), we[l], wt[l]) + differing("b_%d" % (l + 1), be[l], bt[l])
            bad += differing("delta_w_%d" % (l + 1), eng.debug_tensor("delta_w", l + 1), twin.tensor("delta_w", l + 1))
        assert all(not np.array_equal(a, b) for a, b in zip(we, ws))          # every layer was trained
        if fresh:
            xf, _ = random_frames(fresh, ls, 9)
            want = np.concatenate([twin.cv_forward(xf[i:i + B]) for i in range(0, fresh, B)])
            bad += differing("forward of %d fresh frames" % fresh, eng.forward(xf), want)
        twin.close()
    finally:
        pyoracle.set_gemm_order("ref")
        eng.close()
    return bad


def test_one_launch_over_four_ragged_layers_equals_the_twin_bitwise(pkg, pyoracle):
    """[75, 96, 160, 33], B = 128, three steps: one k_dwp launch walks three layers' tiles with different ldA / Np, so
    whatever is cached per tile or per layer has to follow the record."""
    assert ragged_run(pkg, pyoracle, HP) == 0


@pytest.mark.parametrize("hp", [(0.1, 0.9, 0.0), (0.1, 0.0, 1e-5)], ids=["weightcost0", "momentum0"])
def test_constants_that_fold_change_no_bit(pkg, pyoracle, hp):
    """The same net (no dropout) with weightcost = 0, and with momentum = 0: an update whose constants fold to nothing
    on the CPU is still the same IEEE expression on the GPU."""
    assert ragged_run(pkg, pyoracle, hp) == 0


def test_a_new_learning_rate_reuses_the_plans_and_equals_a_fresh_engine(pkg):
    """531-97-33-1-257 at B = 64, momentum 0 (so the weights are the whole state): two minibatches, set_lrate, two more.
    Hyper-parameters are no part of a launch plan (csrc/engine.hip dwp_table), so the second call builds none; and they
    reach the kernel with every launch, so its result is that of a fresh engine created with the new rate on the weights
    the first call left, bit for bit."""
    ls, B = [531, 97, 33, 1, 257], 64
    ws, bs = random_net(ls, 21)
    x, t = random_frames(4 * B, ls, 22)
    eng = pkg.BPGpu(1, 0, ls, B, 0.1, 0.0, 1e-5, ws, bs, 2.0, 0)
    try:
        assert eng.train(x[:2 * B], t[:2 * B]) == 2
        w1, b1 = eng.returnWeights()
        plans = eng.plan_count()
        assert plans >= 1
        eng.set_lrate(0.025)
        assert eng.train(x[2 * B:], t[2 * B:]) == 2
        assert eng.plan_count() == plans
        wa, ba = eng.returnWeights()
    finally:
        eng.close()
    fresh = pkg.BPGpu(1, 0, ls, B, 0.025, 0.0, 1e-5, w1, b1, 2.0, 0)
    try:
        assert fresh.train(x[2 * B:], t[2 * B:]) == 2
        wf, bf = fresh.returnWeights()
    finally:
        fresh.close()
    bad = 0
    for l in range(len(wa)):
        bad += differing("W_%d" % (l + 1), wa[l], wf[l]) + differing("b_%d" % (l + 1), ba[l], bf[l])
        assert not np.array_equal(wa[l], w1[l])                   # the second call trained the layer
    assert bad == 0


def test_the_next_forward_sees_no_leaked_store(pkg, pyoracle):
    """After the three steps, the forward of a fresh batch (a whole minibatch and a ragged rest) equals the twin's: a
    store that had leaked into a pad row or pad column of W would be summed by the next layer's GEMM."""
    assert ragged_run(pkg, pyoracle, HP, fresh=128 + 37) == 0


def relmax(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def test_the_unfused_form_under_a_gradient_allreduce(pkg, pyoracle):
    """k_dwp with FUSED = false (the gradient goes to G, the update is a launch of its own): the ragged net as two
    emulated ranks with the gradient all-reduce, compared the way tests/test_gpu_configs.py
    (test_config4_eight_ranks_at_the_real_shape, arm "allreduce") compares that arm: the documented-order oracle with
    bunchsize world x B at that test's tolerances, and every bit of the twin in its data-parallel form."""
    ls, B, world, steps = RAGGED, 128, 2, 3
    ws, bs = random_net(ls, 17)
    x, t = random_frames(steps * world * B, ls, 18)
    eng = pkg.BPGpu(1, 0, ls, B, *HP, ws, bs, 1.2, 1)
    eng.fake_world(world, allreduce=True)
    ora = pyoracle.OracleNet(ls, world * B, *HP, 1.2, 1, ws, bs)
    try:
        assert eng.train(x, t) == steps and ora.train(x, t) == steps
        we, be = eng.returnWeights()
        wo, bo = ora.get_weights()
        for l in range(len(we)):
            assert relmax(we[l], wo[l]) < 2e-5, l
            assert relmax(be[l], bo[l]) < 2e-5, l
            assert relmax(eng.debug_tensor("delta_w", l + 1), ora.tensor("delta_w", l + 1)) < 5e-4, l
            assert relmax(eng.debug_tensor("delta_b", l + 1), ora.tensor("delta_b", l + 1)) < 5e-4, l
        assert relmax(eng.scalefactor(), ora.tensor("scalefactor")) < 1e-5
        pyoracle.set_gemm_order("hip", eng.out_slabs(), plan=eng.gemm_plan(), dp_world=world, dp_allreduce=True)
        twin = pyoracle.OracleNet(ls, world * B, *HP, 1.2, 1, ws, bs)
        assert twin.train(x, t) == steps
        wt, bt = twin.get_weights()
        bad = 0
        for l in range(len(we)):
            bad += differing("W_%d" % (l + 1), we[l], wt[l]) + differing("b_%d" % (l + 1), be[l], bt[l])
        bad += differing("scalefactor", eng.scalefactor(), twin.tensor("scalefactor"))
        twin.close()
    finally:
        pyoracle.set_gemm_order("ref")
        ora.close()
        eng.close()
    assert bad == 0
