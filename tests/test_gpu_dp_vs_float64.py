"""GPU: the data-parallel step (emulated worlds and a 1-rank RCCL communicator, all four exchanges) and dropout against
float64, element by element, for every rank and every step.

The per-rank read-back (mlggd_debug_keep_ranks / mlggd_debug_rank_tensor) returns what each emulated rank computed --
its input rows, activations, gradients and output -- copied where it produced them, not from the gathered buffers.  The
ranks' rows stacked in rank order are one step of world x B rows, which tests/bounds64.py checks unchanged (its module
docstring shows why the any-order bounds cover the per-rank chains and the sums met in rank order); a wrong gathered
slot, a frame dropped or counted twice at a rank seam, a statistic of one rank only then shows up in dW, db, alpha or
the loss.  Dropout: the input rows the kernels consumed and every hidden layer hold exactly 0 or the plain sigmoid,
the masks pass binomial limits, CV's weight round trips are exact.  tests/test_bounds64.py shows on the CPU that a
rank-split implementation passes these checks and that the slips they are meant for fail them.  The worst hard and
tight ratio per case and kernel is printed at the end (-s)."""
import numpy as np
import pytest

import bounds64 as b6
from test_gpu_vs_float64 import DECAY, KNOBS, SHIPPED, data, fail_lines, new_engine, state

pytestmark = pytest.mark.gpu

MODES = {"gather": 2, "shard": 3, "allreduce": 1, "shard_a2a": 4}
TABLE = {}


def record(case, reps):
    for r in reps:
        key = (case, r.name)
        h, t, lim = TABLE.get(key, (0.0, 0.0, r.limit))
        TABLE[key] = (max(h, r.hard), max(t, r.tight), r.limit)


@pytest.fixture(scope="module", autouse=True)
def print_table():
    yield
    print("\n%-52s %-26s %10s %10s %8s" % ("case", "kernel", "hard", "tight", "limit"))
    for (case, name), (h, t, lim) in TABLE.items():
        print("%-52s %-26s %10.4f %10.2f %8.1f" % (case, name, h, t, lim))


def set_world(eng, mode, world):
    eng.fake_world(world, sharded=mode == "shard", allreduce=mode == "allreduce", a2a=mode == "shard_a2a")


def stacked(eng, name, layer, world):
    return np.vstack([eng.rank_tensor(name, layer, r) for r in range(world)])


def read_dp_step(eng, x, t, pre, hp, beta, ml, L, world, layers):
    """the step of all ranks, stacked in rank order; the input rows the kernels consumed must be the caller's rows"""
    W, b, dW, db = pre
    Wn, bn, dWn, dbn = state(eng, L)
    xs = stacked(eng, "x", 0, world)
    assert np.array_equal(xs.view(np.uint32), np.asarray(x, np.float32).view(np.uint32))
    need = set(layers) | {l - 1 for l in layers} | {l + 1 for l in layers}
    y = {l: stacked(eng, "y", l, world) for l in range(1, L - 1) if l in need}
    d = {l: stacked(eng, "dedx", l, world) for l in range(1, L) if l in need or l == L - 1}
    return b6.Step(xs, t, W, b, dW, db, y, stacked(eng, "out", 0, world), d, dWn, dbn, Wn, bn, hp[0], hp[1], hp[2],
                   beta, ml, eng.out_slabs(), eng.scalefactor() if ml == 1 else None)


def check_dp(eng, s, layers, grad):
    reps = b6.check_step(s, layers)
    if grad:   # all-reduce path: the summed gradient before k_apply_update
        yin = lambda l: s.x if l == 1 else s.y[l - 1]
        reps += [b6.compare("grad %d" % l, eng.debug_tensor("grad_w", l), b6.expect_grad(yin(l), s.dedx[l]))
                 for l in sorted(layers)]
    return reps


def dp_run(pkg, monkeypatch, case, mode, world, B, ls, hp, beta, ml, seed, env=None, layers=None, steps=2,
           comm=False, x=None, t=None, W=None, b=None):
    """`steps` global steps of world x B rows on an emulated world (or a 1-rank communicator, comm=True), every step
    of every rank checked; returns the stacked steps"""
    L = len(ls)
    layers = set(range(1, L)) if layers is None else set(layers)
    if W is None:
        W, b = b6.make_net(ls, seed)
    if x is None:
        x, t = data(ls, B, steps * world, seed + 1, W, b)
    n = world * B
    env = dict(env or {})
    if comm:
        env["MLGGD_DP_MODE"] = mode
    eng = new_engine(pkg, monkeypatch, ls, B, hp, beta, ml, W, b, env)
    bad, done = [], []
    try:
        if comm:
            eng.comm_init(pkg.comm_unique_id(), 1, 0)
        else:
            set_world(eng, mode, world)
        assert eng.dp_mode() == MODES[mode]
        eng.keep_ranks()
        case = "%s %s w%d B%d S%d" % (case, mode, world, B, eng.out_slabs())
        for k in range(steps):
            pre = state(eng, L)
            xb, tb = x[k * n:(k + 1) * n], t[k * n:(k + 1) * n]
            assert eng.train(xb, tb) == 1
            s = read_dp_step(eng, xb, tb, pre, hp, beta, ml, L, world, layers)
            reps = check_dp(eng, s, layers, mode == "allreduce")
            record(case, reps)
            bad += ["step %d %s" % (k + 1, ln) for ln in fail_lines(reps)]
            done.append(s)
    finally:
        eng.close()
    assert not bad, case + "\n" + "\n".join(bad)
    return done


# ---------------------------------------------------------------------------------------------------------------------
# emulated worlds
NET = [200, 160, 96, 40]      # 8 ranks: uneven and empty 64-row shard blocks
LOSSES = [(0, 2.0, DECAY), (1, 1.2, SHIPPED), (1, 0.9, DECAY)]


# the factor exchange needs B % 32 == 0: the ragged world 3 x 50 is the all-reduce path's only
WORLDS = [(m, w, B) for m in MODES for w, B in [(2, 64), (4, 32), (4, 128), (8, 128)]] + [("allreduce", 3, 50)]


@pytest.mark.parametrize("ml,beta,hp", LOSSES, ids=["MMSE2", "ML1.2", "ML0.9"])
@pytest.mark.parametrize("mode,world,B", WORLDS)
def test_emulated_world(pkg, monkeypatch, mode, world, B, ml, beta, hp):
    dp_run(pkg, monkeypatch, "emulated", mode, world, B, NET, hp, beta, ml, seed=world * 1000 + B)


@pytest.mark.parametrize("mode", list(MODES))
def test_emulated_world_exact_zero_errors_with_beta_below_one(pkg, monkeypatch, mode):
    """ML beta = 0.9 on 4 x 32 frames with an exactly representable output layer: targets hit the output exactly in
    every rank's rows, where the gradient must be exactly 0 (and the statistic summed across ranks stays finite)"""
    K, D, world, B = 96, 257, 4, 32
    rng = np.random.default_rng(71)
    W = (rng.integers(-4, 5, (K, D)) * 0.125).astype(np.float32)
    b = (rng.integers(-8, 9, D) * 0.25).astype(np.float32)
    x = rng.integers(-3, 4, (2 * world * B, K)).astype(np.float32)
    t = rng.normal(0, 1.5, (2 * world * B, D)).astype(np.float32)
    exact = (x.astype(np.float64) @ W + b).astype(np.float32)
    t[:world * B][::5, ::7] = exact[:world * B][::5, ::7]
    s = dp_run(pkg, monkeypatch, "e==0", mode, world, B, [K, D], DECAY, 0.9, 1, 0, x=x, t=t, W=[W], b=[b])[0]
    hit = s.out[::5, ::7] == t[:world * B][::5, ::7]
    assert hit.all() and (s.dedx[1][::5, ::7] == 0).all()


@pytest.mark.parametrize("mode", list(MODES))
def test_config4_eight_ranks_at_the_real_shape(pkg, monkeypatch, mode):
    """2827-2048^3-257 on 8 x 128 frames, ML beta = 1.2: layer 1 splits 45 tile rows of 64 into 8 uneven blocks"""
    dp_run(pkg, monkeypatch, "config-4", mode, 8, 128, [2827, 2048, 2048, 2048, 257], SHIPPED, 1.2, 1, seed=4)


def test_config5_allreduce_on_eight_ranks(pkg, monkeypatch):
    """2827-4096^6-257 on 8 emulated ranks, all-reduce, G checked; 8 x 64 frames (the global 512 of the single-device
    config-5 case; 8 x 512 takes too long in float64), layers 1, 2, the last hidden one and the output"""
    ls = [2827] + [4096] * 6 + [257]
    dp_run(pkg, monkeypatch, "config-5", "allreduce", 8, 64, ls, SHIPPED, 1.2, 1, seed=5, layers={1, 2, 6, 7})


@pytest.mark.parametrize("ml,beta", [(0, 2.0), (1, 1.2)])
@pytest.mark.parametrize("mode", list(MODES))
def test_one_rank_communicator(pkg, monkeypatch, mode, ml, beta):
    """mlggd_comm_init(world 1): the real exchange path through RCCL, at the shape of
    test_gpu_e2e.py::test_exchange_path_on_one_rank_communicator"""
    dp_run(pkg, monkeypatch, "rccl-1", mode, 1, 64, [257 * 3, 256, 160, 257], SHIPPED, beta, ml, seed=6, comm=True)


@pytest.mark.parametrize("ml,beta", [(0, 2.0), (1, 1.2)])
def test_fine_grained_factor_exchange(pkg, monkeypatch, ml, beta):
    dp_run(pkg, monkeypatch, "DP_FINE=1", "gather", 4, 32, NET, DECAY, beta, ml, seed=81, env={"MLGGD_DP_FINE": "1"})


@pytest.mark.parametrize("mode", list(MODES))
def test_frame_stream_chunk_on_the_exchange_path(pkg, monkeypatch, mode):
    """a frame-stream chunk of two bunches through a 1-rank communicator (rows gathered on the device, the second
    bunch staged ahead); the second step's pre-step state comes from an engine that trained the first bunch only"""
    dim, ctx, B, toff = 40, 5, 64, 2
    ls, hp, beta = [dim * ctx, 128, 96, dim], SHIPPED, 1.2
    L = len(ls)
    rng = np.random.default_rng(91)
    nfr = 400
    feat = rng.standard_normal((nfr, dim), dtype=np.float32)
    targ = (0.5 * feat + 0.5 * rng.standard_normal((nfr, dim), dtype=np.float32)).astype(np.float32)
    first = rng.permutation(nfr - ctx + 1)[:2 * B].astype(np.int32)
    W, b = b6.make_net(ls, 92)
    engs = []
    try:
        for nb in (1, 2):
            eng = new_engine(pkg, monkeypatch, ls, B, hp, beta, 1, W, b, {"MLGGD_DP_MODE": mode})
            engs.append(eng)
            eng.comm_init(pkg.comm_unique_id(), 1, 0)
            assert eng.dp_mode() == MODES[mode]
            assert eng.train_frames(feat, targ, first[:nb * B], ctx, toff) == nb
        pre = state(engs[0], L)
        fk = first[B:]
        x = np.ascontiguousarray(feat[fk[:, None] + np.arange(ctx)[None, :]].reshape(B, ctx * dim))
        s = read_dp_step(engs[1], x, np.ascontiguousarray(targ[fk + toff]), pre, hp, beta, 1, L, 1, set(range(1, L)))
        reps = check_dp(engs[1], s, set(range(1, L)), mode == "allreduce")
    finally:
        for e in engs:
            e.close()
    record("frame stream rccl-1 %s" % mode, reps)
    assert not fail_lines(reps), "\n".join(fail_lines(reps))


@pytest.mark.parametrize("mode,world", [("gather", 4), ("shard", 8), ("allreduce", 3), ("shard_a2a", 8),
                                        ("single", 1), ("dropout", 1)])
def test_keeping_ranks_changes_no_bit(pkg, monkeypatch, mode, world):
    """the read-back hook on and off: W, b, delta_w, delta_b and the scale factor after two steps are the same bits"""
    ls, B = NET, 50 if mode == "allreduce" else 32
    W, b = b6.make_net(ls, 101)
    x, t = data(ls, B, 2 * world, 102, W, b)
    out = []
    for keep in (True, False):
        eng = drop_engine(pkg, monkeypatch, 7, ls, B, SHIPPED, 1.2, 1, W, b, drop=mode == "dropout")
        try:
            if mode in MODES:
                set_world(eng, mode, world)
            if keep:
                eng.keep_ranks()
            for k in range(2):
                n = world * B
                assert eng.train(x[k * n:(k + 1) * n], t[k * n:(k + 1) * n]) == 1
            out.append(state(eng, len(ls)) + (eng.scalefactor(),))
        finally:
            eng.close()
    a, c = out
    for ta, tc in zip(a[:4], c[:4]):
        for u, v in zip(ta, tc):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), mode
    assert np.array_equal(a[4].view(np.uint32), c[4].view(np.uint32)), mode


# ---------------------------------------------------------------------------------------------------------------------
# dropout, one device
P_IN, P_HID = 0.1, 0.2


def drop_engine(pkg, monkeypatch, seed, ls, B, hp, beta, ml, W, b, env=None, drop=True):
    """an engine with dropoutflag (visible_omit P_IN, hid_omit P_HID) and the launch-plan knobs of `env` only"""
    for k in KNOBS + ("MLGGD_DP_FINE", "MLGGD_DP_MODE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return pkg.BPGpu(seed, 0, ls, B, *hp, W, b, beta, ml, *((1, P_IN, P_HID) if drop else (0, 0.0, 0.0)))


def dropout_checks(eng, x_raw, t, pre, hp, beta, ml, L, p_in=P_IN, p_hid=P_HID):
    """every operation of the last step with the masked input rows and activations; the input rows raw-or-0; the mask
    statistics of every layer and the overlap of the first two layers' masks.  Returns (reports, masks)."""
    W, b, dW, db = pre
    Wn, bn, dWn, dbn = state(eng, L)
    xs = eng.rank_tensor("x", 0, 0)
    s = b6.Step(xs, t, W, b, dW, db, {l: eng.rank_tensor("y", l, 0) for l in range(1, L - 1)},
                eng.rank_tensor("out", 0, 0), {l: eng.rank_tensor("dedx", l, 0) for l in range(1, L)}, dWn, dbn, Wn,
                bn, hp[0], hp[1], hp[2], beta, ml, eng.out_slabs(), eng.scalefactor() if ml == 1 else None,
                dropout=True)
    reps = b6.check_step(s)
    rep, d0, k0 = b6.input_mask(x_raw, xs)
    reps.append(rep)
    reps += b6.mask_stats("mask 0", d0, k0, p_in)
    masks = {0: (d0, k0)}
    for l in range(1, L - 1):
        _, dr, kn = b6.expect_dropout_layer(s.x if l == 1 else s.y[l - 1], W[l - 1], b[l - 1], s.y[l])
        masks[l] = (dr, kn)
        reps += b6.mask_stats("mask %d" % l, dr, kn, p_hid)
    if L > 3:
        reps.append(b6.mask_overlap("masks 1 x 2", *masks[1], *masks[2], p_hid, p_hid))
    return reps, masks


def dropout_run(pkg, monkeypatch, case, ls, B, hp, beta, ml, seed, env=None, steps=2):
    L = len(ls)
    W, b = b6.make_net(ls, seed)
    x, t = data(ls, B, steps, seed + 1, W, b)
    eng = drop_engine(pkg, monkeypatch, seed, ls, B, hp, beta, ml, W, b, env)
    bad, prev = [], None
    case = "dropout %s B%d plan%s S%d" % (case, B, "".join("%d%d" % p for p in eng.gemm_plan()), eng.out_slabs())
    try:
        assert eng.dp_mode() == 0
        for k in range(steps):
            pre = state(eng, L)
            xb, tb = x[k * B:(k + 1) * B], t[k * B:(k + 1) * B]
            assert eng.train(xb, tb) == 1
            reps, masks = dropout_checks(eng, xb, tb, pre, hp, beta, ml, L)
            if prev is not None:
                reps += [b6.mask_overlap("mask %d steps %d x %d" % (l, k, k + 1), *prev[l], *masks[l],
                                         P_IN if l == 0 else P_HID, P_IN if l == 0 else P_HID) for l in masks]
            prev = masks
            record(case, reps)
            bad += ["step %d %s" % (k + 1, ln) for ln in fail_lines(reps)]
    finally:
        eng.close()
    assert not bad, case + "\n" + "\n".join(bad)
    return prev


@pytest.mark.parametrize("case,ls,B,env", [
    ("shipped", [1799, 2048, 2048, 2048, 257], 128, None),
    ("ragged", [531, 300, 130, 257], 50, None),
    ("ragged", [531, 300, 130, 257], 200, None),
    ("TILE64=2", [192, 128, 64, 257], 64, {"MLGGD_TILE64": "2"}),
    ("LOSS_FUSE=0", [531, 300, 130, 257], 128, {"MLGGD_LOSS_FUSE": "0"}),
])
def test_dropout_training(pkg, monkeypatch, case, ls, B, env):
    dropout_run(pkg, monkeypatch, case, ls, B, SHIPPED, 1.2, 1, seed=B + len(ls), env=env)


def test_dropout_mask_differs_with_the_seed(pkg, monkeypatch):
    ls, B = [531, 300, 130, 257], 128
    m = []
    for seed in (3, 4):
        W, b = b6.make_net(ls, 5)
        x, t = data(ls, B, 1, 6, W, b)
        eng = drop_engine(pkg, monkeypatch, seed, ls, B, SHIPPED, 2.0, 0, W, b)
        try:
            pre = state(eng, len(ls))
            assert eng.train(x, t) == 1
            reps, masks = dropout_checks(eng, x, t, pre, SHIPPED, 2.0, 0, len(ls))
        finally:
            eng.close()
        assert not fail_lines(reps), "\n".join(fail_lines(reps))
        m.append(masks)
    reps = [b6.mask_overlap("mask %d seeds 3 x 4" % l, *m[0][l], *m[1][l], P_IN if l == 0 else P_HID,
                            P_IN if l == 0 else P_HID) for l in m[0]]
    record("dropout seeds", reps)
    assert not fail_lines(reps), "\n".join(fail_lines(reps))


@pytest.mark.parametrize("stage_ahead", ["1", "0"])
def test_dropout_steps_of_one_chunk(pkg, monkeypatch, stage_ahead):
    """two steps in ONE train() call (the second bunch staged during the first step's loss unless STAGE_AHEAD=0):
    the second step's masks are drawn on the staged rows"""
    ls, B, hp, beta = [531, 300, 130, 257], 128, SHIPPED, 1.2
    L = len(ls)
    W, b = b6.make_net(ls, 19)
    x, t = data(ls, B, 2, 20, W, b)
    engs = []
    try:
        for nb in (1, 2):
            eng = drop_engine(pkg, monkeypatch, 9, ls, B, hp, beta, 1, W, b, {"MLGGD_STAGE_AHEAD": stage_ahead})
            engs.append(eng)
            assert eng.train(x[:nb * B], t[:nb * B]) == nb
        reps, _ = dropout_checks(engs[1], x[B:], t[B:], state(engs[0], L), hp, beta, 1, L)
    finally:
        for e in engs:
            e.close()
    record("dropout one chunk, STAGE_AHEAD=%s" % stage_ahead, reps)
    assert not fail_lines(reps), "\n".join(fail_lines(reps))


def test_dropout_frame_stream(pkg, monkeypatch):
    """train_frames with fea_context 11: the rows gathered on the device are what the input mask applies to"""
    dim, ctx, B, toff = 257, 11, 128, 5
    ls, hp, beta = [dim * ctx, 512, 257], SHIPPED, 1.2
    L = len(ls)
    rng = np.random.default_rng(23)
    nfr = 600
    feat = rng.standard_normal((nfr, dim), dtype=np.float32)
    targ = (0.5 * feat + 0.5 * rng.standard_normal((nfr, dim), dtype=np.float32)).astype(np.float32)
    first = rng.permutation(nfr - ctx + 1)[:2 * B].astype(np.int32)
    W, b = b6.make_net(ls, 24)
    eng = drop_engine(pkg, monkeypatch, 11, ls, B, hp, beta, 1, W, b)
    bad = []
    try:
        for k in range(2):
            fk = first[k * B:(k + 1) * B]
            x = np.ascontiguousarray(feat[fk[:, None] + np.arange(ctx)[None, :]].reshape(B, ctx * dim))
            pre = state(eng, L)
            assert eng.train_frames(feat, targ, fk, ctx, toff) == 1
            reps, _ = dropout_checks(eng, x, np.ascontiguousarray(targ[fk + toff]), pre, hp, beta, 1, L)
            record("dropout frame stream ctx 11", reps)
            bad += fail_lines(reps)
    finally:
        eng.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("B", [64, 128])
def test_dropout_cv_forward(pkg, monkeypatch, B):
    """forward() with dropoutflag over 3 bunches and a ragged tail: bunch j runs on fl32(W_j keep), W_{j+1} =
    fl32(fl32(W_j keep) fl32(1/keep)); the outputs against float64 of those weights, the weights left behind exactly"""
    ls = [531, 1024, 300, 257]
    W, b = b6.make_net(ls, 111)
    eng = drop_engine(pkg, monkeypatch, 1, ls, B, SHIPPED, 1.2, 1, W, b)
    slabs = eng.out_slabs()
    n = 3 * B + 37
    nb = (n + B - 1) // B
    x, _ = b6.make_data(ls, n, 112, 8, W[0], B)
    keeps = [np.float32(1) - np.float32(P_IN)] + [np.float32(1) - np.float32(P_HID)] * (len(ls) - 2)
    try:
        out = eng.forward(x)
        Wl, bl = eng.returnWeights()
    finally:
        eng.close()
    used, left = b6.cv_dropout_weights(W, keeps, nb)
    reps = [b6.compare_exact("W %d after %d bunches" % (l + 1, nb), Wl[l], left[l]) for l in range(len(W))]
    reps += [b6.compare_exact("b %d unchanged" % (l + 1), bl[l], b[l]) for l in range(len(b))]
    for j in range(nb):
        sl = slice(j * B, min((j + 1) * B, n))
        reps.append(b6.compare("bunch %d" % j, out[sl], b6.expect_forward_chain(x[sl], used[j], b, slabs)))
    record("dropout CV forward B%d" % B, reps)
    assert not fail_lines(reps), "\n".join(fail_lines(reps))
