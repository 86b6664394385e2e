"""GPU: every kernel path of a training step, the forward pass and the CV sums against float64, element by element.

Each step reads back the engine's own fp32 inputs of every operation (weights, biases and momentum before the step,
activations and gradients after it) and holds every output to the hard per-element bound and the tight statistic of
tests/bounds64.py -- independent of the oracle and of its MFMA-order twin, which restate the kernels' arithmetic and so
cannot see a mistake in it.  tests/test_bounds64.py shows on the CPU that these checks pass correct fp32
implementations and kill a list of planted slips.  Each case asserts the launch plan it is meant to exercise
(gemm_plan, out_slabs, dp_mode), so that a change of plan cannot quietly turn it into a duplicate.  A table of the
worst hard ratio and the worst tight ratio per case and kernel is printed at the end (-s)."""
import numpy as np
import pytest

import bounds64 as b6

pytestmark = pytest.mark.gpu

SHIPPED = (0.1, 0.9, 1e-5)
NO_MOM = (0.05, 0.0, 0.0)
DECAY = (0.3, 0.5, 1e-2)      # lr wc W of the order of the gradient term
KNOBS = ("MLGGD_TILE64", "MLGGD_S_OUT", "MLGGD_LOSS_FUSE", "MLGGD_DW_MERGE", "MLGGD_STAGE_AHEAD", "MLGGD_CV_DEVICE",
         "MLGGD_DW_TILE", "MLGGD_DW_PERSIST", "MLGGD_DWP_PER_CU", "MLGGD_TILE_MAP")
TABLE = {}


def record(case, reps):
    for r in reps:
        key = (case, r.name)
        h, t, lim = TABLE.get(key, (0.0, 0.0, r.limit))
        TABLE[key] = (max(h, r.hard), max(t, r.tight), r.limit)


@pytest.fixture(scope="module", autouse=True)
def print_table():
    yield
    print("\n%-44s %-22s %10s %10s %8s" % ("case", "kernel", "hard", "tight", "limit"))
    for (case, name), (h, t, lim) in TABLE.items():
        print("%-44s %-22s %10.4f %10.2f %8.1f" % (case, name, h, t, lim))


def fail_lines(reps):
    return [r.line() for r in reps if not r.ok]


def new_engine(pkg, monkeypatch, ls, B, hp, beta, ml, W, b, env=None):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return pkg.BPGpu(1, 0, ls, B, *hp, W, b, beta, ml)


def state(eng, L):
    W, b = eng.returnWeights()
    return W, b, [eng.debug_tensor("delta_w", l) for l in range(1, L)], [eng.debug_tensor("delta_b", l) for l in range(1, L)]


def read_step(eng, x, t, pre, lr, hp, beta, ml, L):
    W, b, dW, db = pre
    Wn, bn, dWn, dbn = state(eng, L)
    return b6.Step(x, t, W, b, dW, db, {l: eng.debug_tensor("y", l) for l in range(1, L - 1)}, eng.debug_tensor("out"),
                   {l: eng.debug_tensor("dedx", l) for l in range(1, L)}, dWn, dbn, Wn, bn, lr, hp[1], hp[2], beta, ml,
                   eng.out_slabs(), eng.scalefactor() if ml == 1 else None)


def data(ls, B, steps, seed, W, b):
    """inputs with saturating rows; targets: column 0 of magnitude 1e3, column 1 within 1e-6 of the initial output"""
    x, t = b6.make_data(ls, steps * B, seed, min(8, B), W[0], B)
    y = x.astype(np.float64)
    for l in range(len(W)):
        y = y @ W[l] + b[l]
        if l < len(W) - 1:
            y = b6._sigmoid64(y)[0]
    rng = np.random.default_rng(seed + 1)
    t[:, 1] = (y[:, 1] + 1e-6 * rng.standard_normal(y.shape[0])).astype(np.float32)
    return x, t


def run_case(pkg, monkeypatch, case, ls, B, hp, beta, ml, env=None, layers=None, steps=2, lrate2=None, seed=1,
             plan=None, slabs=None, fake_allreduce=False, x=None, t=None, W=None, b=None, dw_kinds=None):
    """dw_kinds: the dW kernel of every layer's launch, as test_gpu_dw_choices.dw_kernel names it from the stamp rows
    (taken by one further step per layer after the checked ones)"""
    L = len(ls)
    if W is None:
        W, b = b6.make_net(ls, seed)
    if x is None:
        x, t = data(ls, B, steps, seed + 1, W, b)
    eng = new_engine(pkg, monkeypatch, ls, B, hp, beta, ml, W, b, env)
    if fake_allreduce:
        eng.fake_world(1, allreduce=True)
        assert eng.dp_mode() == 1                      # k_dwp<., false> + k_apply_update + k_bias_apply
    got_plan, got_slabs = eng.gemm_plan(), eng.out_slabs()
    if plan is not None:
        for l, want in plan.items():
            assert got_plan[l - 1] == want, (case, l, got_plan)
    if slabs is not None:
        assert got_slabs == slabs, (case, got_slabs)
    case = "%s plan%s S%d" % (case, "".join("%d%d" % p for p in got_plan), got_slabs)
    lr = hp[0]
    bad, steps_done = [], []
    try:
        for k in range(steps):
            if lrate2 is not None and k == 1:
                eng.set_lrate(lrate2)
                lr = lrate2
            pre = state(eng, L)
            xb, tb = x[k * B:(k + 1) * B], t[k * B:(k + 1) * B]
            assert eng.train(xb, tb) == 1
            s = read_step(eng, xb, tb, pre, lr, hp, beta, ml, L)
            reps = b6.check_step(s, layers)
            record(case, reps)
            bad += ["step %d %s" % (k + 1, ln) for ln in fail_lines(reps)]
            steps_done.append(s)
        if dw_kinds is not None:
            from test_gpu_dw_choices import dw_kernel, tiles
            got = [dw_kernel(eng, l, lambda: eng.train(x[:B], t[:B])) for l in range(1, L)]
            assert [k for _, k in got] == dw_kinds, (case, [(len(rows), k) for rows, k in got])
            assert [len(rows) for rows, _ in got] == [tiles(ls, l, 128 if k == "k_dw2" else 64)
                                                      for l, k in zip(range(1, L), dw_kinds)]
    finally:
        eng.close()
    assert not bad, case + "\n" + "\n".join(bad)
    return steps_done


# ---------------------------------------------------------------------------------------------------------------------
# training steps
def test_shipped_net(pkg, monkeypatch):
    """1799-2048^3-257, B = 128, ML-GGD beta = 1 (what finetune.pl runs): 32-tile forward and dX, automatic split-K of
    the output layer, k_loss_ml; the saturating rows reach y == 0, y == 1 and subnormal y in the first layer"""
    ls = [1799, 2048, 2048, 2048, 257]
    steps = run_case(pkg, monkeypatch, "shipped", ls, 128, SHIPPED, 1.0, 1, plan={1: (4, 4), 2: (4, 4), 3: (4, 4)})
    for s in steps:
        y = s.y[1]
        assert (y == 0).any() and (y == 1).any() and ((y > 0) & (y < 2.0 ** -126)).any()
        assert (s.dedx[1][(y > 0) & (y < 2.0 ** -126)] != 0).any()     # subnormal activations survive into dX


def test_shipped_net_with_set_lrate(pkg, monkeypatch):
    run_case(pkg, monkeypatch, "shipped set_lrate(0.025)", [1799, 2048, 2048, 257], 128, SHIPPED, 1.0, 1,
             lrate2=0.025, seed=3)


def test_config5_net(pkg, monkeypatch):
    """2827-4096^6-257, B = 512, ML beta = 1.2: the 64-tile forward and dX, k_dwp at 512 frames; layers 1, 2, the last
    hidden one and the output checked in full (the middle layers repeat layer 2)"""
    ls = [2827] + [4096] * 6 + [257]
    run_case(pkg, monkeypatch, "config-5", ls, 512, SHIPPED, 1.2, 1, layers={1, 2, 6, 7},
             plan={1: (1, 4), 2: (1, 1), 6: (1, 1)}, seed=5)


def test_global_bunch_1024(pkg, monkeypatch):
    """2827-2048^3-257, B = 1024, MMSE, weight decay of the gradient's order.  On one device 1024 frames are sixteen
    64-frame units, which dwp_usable() does not admit (1, 2, 4, 8): every layer runs k_dw<1> over sixteen chunks, one
    workgroup per 64 x 64 tile.  (k_dwp<16> runs only over gathered factors: tests/test_gpu_dw_choices.py.)"""
    run_case(pkg, monkeypatch, "B1024 MMSE", [2827, 2048, 2048, 2048, 257], 1024, DECAY, 2.0, 0, seed=7,
             dw_kinds=["k_dw1"] * 4)


RAGGED = [(1, NO_MOM, 2.0, 0, None), (7, SHIPPED, 1.2, 1, None), (33, DECAY, 1.2, 1, None),
          (96, SHIPPED, 0.9, 1, 0.025), (200, DECAY, 1.0, 1, None), (500, NO_MOM, 1.2, 1, None)]


@pytest.mark.parametrize("B,hp,beta,ml,lrate2", RAGGED)
def test_ragged_shapes(pkg, monkeypatch, B, hp, beta, ml, lrate2):
    """531-97-33-1-257: no dimension a multiple of 32 or 64, a one-unit hidden layer, ragged bunches"""
    run_case(pkg, monkeypatch, "ragged B%d" % B, [531, 97, 33, 1, 257], B, hp, beta, ml, lrate2=lrate2, seed=B)


RAGGED_LS = [531, 97, 33, 1, 257]
RAGGED_KINDS_128 = ["k_dw2", "k_dw2", "k_dw", "k_dw2"]      # 33 -> 1 is one workgroup at either tile size


@pytest.mark.parametrize("B,hp,beta,ml,lrate2", [r for r in RAGGED if r[0] in (7, 96, 200)])
def test_ragged_shapes_with_128_tiles(pkg, monkeypatch, B, hp, beta, ml, lrate2):
    """MLGGD_DW_TILE=2: k_dw<2> (128 x 128 tiles, 128-frame chunks staged in two passes of 64 rows) on the ragged net --
    Bp = 32: one short chunk; 96: one chunk, the second pass masked from row 96; 224: 128 + 96"""
    run_case(pkg, monkeypatch, "ragged B%d DW_TILE=2" % B, RAGGED_LS, B, hp, beta, ml, lrate2=lrate2, seed=B,
             env={"MLGGD_DW_TILE": "2"}, dw_kinds=RAGGED_KINDS_128)


def test_ragged_shapes_with_128_tiles_unfused(pkg, monkeypatch):
    """k_dw<2, false> + k_apply_update + k_bias_apply (the unfused launch carries no stamps: the fused cases above and
    tests/test_gpu_dw_choices.py assert that this configuration selects k_dw<2>)"""
    B, hp, beta, ml, lrate2 = RAGGED[3]
    assert B == 96
    run_case(pkg, monkeypatch, "ragged B96 DW_TILE=2 unfused", RAGGED_LS, B, hp, beta, ml, lrate2=lrate2, seed=B,
             env={"MLGGD_DW_TILE": "2"}, fake_allreduce=True)


def test_128_tiles_where_k_dwp_would_run(pkg, monkeypatch):
    """MLGGD_DW_PERSIST=0 with MLGGD_DW_TILE=2 at B = 128: k_dw<2> over exactly one full chunk"""
    run_case(pkg, monkeypatch, "DW_PERSIST=0 DW_TILE=2", [531, 300, 130, 257], 128, DECAY, 1.2, 1, seed=13,
             env={"MLGGD_DW_PERSIST": "0", "MLGGD_DW_TILE": "2"}, dw_kinds=["k_dw2"] * 3)


def test_forced_tile64(pkg, monkeypatch):
    run_case(pkg, monkeypatch, "TILE64=2", [192, 128, 64, 257], 64, DECAY, 1.2, 1, env={"MLGGD_TILE64": "2"},
             plan={1: (1, 4), 2: (1, 1)}, seed=9)


@pytest.mark.parametrize("s_out", [1, 3, 32])
def test_forced_output_slabs(pkg, monkeypatch, s_out):
    run_case(pkg, monkeypatch, "S_OUT=%d" % s_out, [300, 200, 257], 96, SHIPPED, 1.2, 1,
             env={"MLGGD_S_OUT": str(s_out)}, slabs=s_out, seed=11)


@pytest.mark.parametrize("env", [{"MLGGD_LOSS_FUSE": "0"}, {"MLGGD_DW_MERGE": "0"}],
                         ids=["loss_pair", "dw_per_layer"])
def test_forced_loss_and_dw_variants(pkg, monkeypatch, env):
    """k_loss_err + k_colsum + k_loss_grad instead of k_loss_ml; one k_dwp launch per layer instead of one for all"""
    run_case(pkg, monkeypatch, ",".join("%s=%s" % kv for kv in env.items()), [531, 300, 130, 257], 128, DECAY, 1.2, 1,
             env=env, seed=13)


def test_apply_update_path(pkg, monkeypatch):
    """the unfused dW (gradient only) + k_apply_update + k_bias_apply of the all-reduce path, on a one-rank emulated
    world (its exchange is the identity)"""
    run_case(pkg, monkeypatch, "k_apply_update", [531, 300, 130, 257], 128, DECAY, 1.2, 1, fake_allreduce=True, seed=15)


@pytest.mark.parametrize("ml,beta", [(1, 0.9), (1, 1.0), (1, 1.2), (1, 2.0), (0, 1.0), (0, 2.0)])
def test_loss_configurations(pkg, monkeypatch, ml, beta):
    run_case(pkg, monkeypatch, "beta %g ML%d" % (beta, ml), [300, 130, 257], 128, SHIPPED, beta, ml, seed=17)


@pytest.mark.parametrize("stage_ahead", ["1", "0"])
def test_steps_of_one_chunk(pkg, monkeypatch, stage_ahead):
    """two steps in ONE train() call: the second bunch's input is staged during the first step's loss kernel (unless
    MLGGD_STAGE_AHEAD=0).  The second step's pre-step state comes from an engine that trained the first bunch only."""
    ls, B, hp, beta = [531, 300, 130, 257], 128, SHIPPED, 1.2
    L = len(ls)
    W, b = b6.make_net(ls, 19)
    x, t = data(ls, B, 2, 20, W, b)
    env = {"MLGGD_STAGE_AHEAD": stage_ahead}
    first = new_engine(pkg, monkeypatch, ls, B, hp, beta, 1, W, b, env)
    assert first.train(x[:B], t[:B]) == 1
    pre = state(first, L)
    first.close()
    eng = new_engine(pkg, monkeypatch, ls, B, hp, beta, 1, W, b, env)
    assert eng.train(x, t) == 2
    s = read_step(eng, x[B:], t[B:], pre, hp[0], hp, beta, 1, L)
    eng.close()
    reps = b6.check_step(s)
    record("one chunk, STAGE_AHEAD=%s" % stage_ahead, reps)
    assert not fail_lines(reps), "\n".join(fail_lines(reps))


def test_exact_zero_errors_with_beta_below_one(pkg, monkeypatch):
    """ML beta = 0.9: |e|^(beta-1) diverges at 0, so e == 0 must give exactly 0 (kernfunc2's middle branch).  An
    exactly representable output layer (as in test_gpu_loss_ulps.py) lets targets hit the output exactly."""
    K, D, B = 96, 257, 128
    rng = np.random.default_rng(7)
    W = (rng.integers(-4, 5, (K, D)) * 0.125).astype(np.float32)
    b = (rng.integers(-8, 9, D) * 0.25).astype(np.float32)
    x = rng.integers(-3, 4, (2 * B, K)).astype(np.float32)
    t = rng.normal(0, 1.5, (2 * B, D)).astype(np.float32)
    exact = (x[:B].astype(np.float64) @ W + b).astype(np.float32)
    t[:B][::5, ::7] = exact[::5, ::7]
    s = run_case(pkg, monkeypatch, "beta 0.9 e==0", [K, D], B, DECAY, 0.9, 1, x=x, t=t, W=[W], b=[b])[0]
    hit = s.out[::5, ::7] == t[:B][::5, ::7]
    assert hit.all() and (s.dedx[1][::5, ::7] == 0).all()


def test_frame_stream(pkg, monkeypatch):
    """train_frames with fea_context 11 and a target offset: rows expanded on the device; the first layer (and the
    rest of the step) against float64 of the host-expanded rows"""
    dim, ctx, B, toff = 257, 11, 128, 5
    ls, hp, beta = [dim * ctx, 512, 257], SHIPPED, 1.2
    L = len(ls)
    rng = np.random.default_rng(23)
    nfr = 600
    feat = rng.standard_normal((nfr, dim), dtype=np.float32)
    targ = (0.5 * feat + 0.5 * rng.standard_normal((nfr, dim), dtype=np.float32)).astype(np.float32)
    first = rng.permutation(nfr - ctx + 1)[:2 * B].astype(np.int32)
    W, b = b6.make_net(ls, 24)
    eng = new_engine(pkg, monkeypatch, ls, B, hp, beta, 1, W, b)
    bad = []
    try:
        for k in range(2):
            fk = first[k * B:(k + 1) * B]
            x = np.ascontiguousarray(feat[fk[:, None] + np.arange(ctx)[None, :]].reshape(B, ctx * dim))
            t = np.ascontiguousarray(targ[fk + toff])
            pre = state(eng, L)
            assert eng.train_frames(feat, targ, fk, ctx, toff) == 1
            reps = b6.check_step(read_step(eng, x, t, pre, hp[0], hp, beta, 1, L))
            record("frame stream ctx 11", reps)
            bad += fail_lines(reps)
    finally:
        eng.close()
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# forward() and CV
@pytest.mark.parametrize("tile64", [None, "2"])
@pytest.mark.parametrize("B", [64, 128, 256, 512])
def test_forward_row_by_row(pkg, monkeypatch, B, tile64):
    """forward() (the CV / enhance_lps path, trailing partial bunch included) on 1, B-1, B+1 and 2B+44 frames: every
    output row against a float64 forward with the bound propagated through the layers; the last bunch's hidden layer
    and output also against their own inputs (debug_tensor holds that bunch)"""
    ls = [531, 1024, 257]
    W, b = b6.make_net(ls, 31)
    eng = new_engine(pkg, monkeypatch, ls, B, SHIPPED, 1.2, 1, W, b, {"MLGGD_TILE64": tile64} if tile64 else None)
    case = "forward B%d plan%s S%d" % (B, "".join("%d%d" % p for p in eng.gemm_plan()), eng.out_slabs())
    if tile64:
        assert eng.gemm_plan()[0][0] == 1
    bad = []
    try:
        for n in (1, B - 1, B + 1, 2 * B + 44):
            x, _ = b6.make_data(ls, n, 32 + n, min(8, n), W[0], B)
            out = eng.forward(x)
            reps = [b6.compare("forward chain n=%d" % n, out, b6.expect_forward_chain(x, W, b, eng.out_slabs()))]
            last = (n - 1) // B * B
            fb = n - last
            y1 = eng.debug_tensor("y", 1)[:fb]
            reps.append(b6.compare("fwd 1 last bunch", y1, b6.expect_sigmoid_layer(x[last:], W[0], b[0])))
            reps.append(b6.compare("out last bunch", out[last:], b6.expect_linear(y1, W[1], b[1], eng.out_slabs())))
            record(case, reps)
            bad += fail_lines(reps)
    finally:
        eng.close()
    assert not bad, case + "\n" + "\n".join(bad)


@pytest.mark.parametrize("device_reduce", [False, True])
def test_cv_sums(pkg, monkeypatch, device_reduce):
    """cv_all (host order, and k_cv_reduce) against float64 sums of the engine's own forward() output"""
    ls, B = [531, 300, 257], 128
    W, b = b6.make_net(ls, 41)
    x, t = data(ls, B, 2, 42, W, b)
    eng = new_engine(pkg, monkeypatch, ls, B, SHIPPED, 1.2, 1, W, b)
    try:
        assert eng.train(x, t) == 2
        eng.set_cv_device_reduce(device_reduce)
        cx, ct = b6.make_data(ls, 2 * B + 44, 43)
        sq, ab, ll = eng.cv_all(cx, ct)
        ex = b6.expect_cv(eng.forward(cx), ct, 1.2, eng.scalefactor(), pkg.gamma)
    finally:
        eng.close()
    reps = [b6.compare(k, np.array(v), ex[k]) for k, v in (("sqerr", sq), ("abserr", ab), ("loglik", ll))]
    record("cv_all %s" % ("k_cv_reduce" if device_reduce else "host order"), reps)
    assert not fail_lines(reps), "\n".join(fail_lines(reps))
