"""GPU: the instruments every performance figure comes from (kernel-class profiling, phase stamps, kernel_work,
last_train_ms) and the state setters (set_weights, set_scalefactor).

A. Instruments change no bit: three steps in ONE train() call (the staged-ahead bunch included) on an engine with an
   instrument switched on leave W, b, delta_w, delta_b of every layer, the scale factor and the last step's output in
   the bits of an engine that ran the same data without it -- on every launch path of one device (each case asserts its
   path) and on the exchange path in all four modes (1-rank communicator and an emulated world of 4), where a profiled
   launch takes the event slots the armed stop event would have ridden on.  One case per mode is also held to float64.
B. Instruments report what happened: launch counts worked out from the plan, the structural bound launches x mean <=
   the ev_t0 / ev_t1 bracket, kernel_work against DESIGN.md's figures restated here, stamps per workgroup.
C. set_weights / set_scalefactor: exact round trips, momentum untouched, the next step against float64 and against a
   fresh engine bit for bit, ordering after steps still in flight, on one device and on the exchange path."""
import numpy as np
import pytest

import bounds64 as b6
from test_gpu_dp_vs_float64 import MODES, check_dp, read_dp_step, set_world
from test_gpu_vs_float64 import DECAY, KNOBS, SHIPPED, data, fail_lines, read_step, state

pytestmark = pytest.mark.gpu

DP_KNOBS = ("MLGGD_DP_MODE", "MLGGD_DP_FINE", "MLGGD_DP_STOPEV", "MLGGD_DP_MAINLINE", "MLGGD_DP_AR_SHARD",
            "MLGGD_DP_STAT_COMM", "MLGGD_DW_PERSIST", "MLGGD_FAKE_ONLY_RANK")
CLASSES = ("transpose", "fwd", "loss", "dx", "dw", "update")
NET, RAGGED, NET64 = [531, 300, 130, 257], [531, 97, 33, 1, 257], [192, 128, 64, 257]
NO_MOM = (0.05, 0.0, 1e-2)      # momentum 0: the step forgets the old delta, weight decay still reads every W
STEPS = 3
BIG = 64                        # event pairs: more than any run here launches
STAMP_ROWS = 8192               # rows of the engine's stamp buffer (mlggd_debug_stamp_select)


def P32(layers):
    return {l: (4, 4) for l in range(1, layers + 1)}


# name: (layersizes, B, env, gemm_plan {layer: (fwd waves, dx waves)}: 4 = the 32 x 32-tile kernels, 1 = the 64 x 64-tile
# ones, dw launches per step)
SHAPES = {
    "merged":       (NET, 128, {}, P32(3), 1),                      # one persistent k_dwp, k_loss_ml
    "dw_per_layer": (NET, 128, {"MLGGD_DW_MERGE": "0"}, P32(3), 3),
    "loss_pair":    (NET, 128, {"MLGGD_LOSS_FUSE": "0"}, P32(3), 1),   # k_loss_err + k_colsum + k_loss_grad
    "tile64":       (NET64, 64, {"MLGGD_TILE64": "2"}, {1: (1, 4), 2: (1, 1)}, 1),   # k_fwd64 / k_dx64
    "ragged":       (RAGGED, 96, {}, P32(4), 4),                    # Bp = 96: the per-layer k_dw fallback
}


def ceil32(n):
    return (n + 31) // 32 * 32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def engine(pkg, monkeypatch, ls, B, hp, beta, ml, W, b, env=None):
    for k in KNOBS + DP_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    return pkg.BPGpu(1, 0, ls, B, *hp, W, b, beta, ml)


def snapshot(eng):
    """every tensor group A compares: W, b, delta_w, delta_b per layer, the scale factor, the last step's output"""
    W, b, dW, db = state(eng, eng.numlayers)
    names = ["%s %d" % (n, l + 1) for n in ("W", "b", "delta_w", "delta_b") for l in range(eng.numlayers - 1)]
    return dict(zip(names, W + b + dW + db), scalefactor=eng.scalefactor(), out=eng.debug_tensor("out"))


def differing(got, want):
    return ["%s: %d of %d elements differ" % (k, int((bits(got[k]) != bits(want[k])).sum()), want[k].size)
            for k in want if not np.array_equal(bits(got[k]), bits(want[k]))]


def assert_path(eng, plan, dw_launches):
    got = eng.gemm_plan()
    for l, want in (plan or {}).items():
        assert got[l - 1] == want, (l, got)
    assert eng.dw_launches_per_step() == dw_launches
    assert eng.out_slabs() >= 1


class Subject:
    """one engine shape, its data and the un-instrumented results (computed once per train() split)"""

    def __init__(self, pkg, monkeypatch, name, hp=SHIPPED, beta=1.2, ml=1):
        self.pkg, self.mp, self.name = pkg, monkeypatch, name
        self.ls, self.B, self.env, self.plan, self.dw = SHAPES[name]
        self.hp, self.beta, self.ml = hp, beta, ml
        self.W, self.b = b6.make_net(self.ls, 7)
        self.x, self.t = data(self.ls, self.B, STEPS, 8, self.W, self.b)
        self.base = {}

    def new(self):
        eng = engine(self.pkg, self.mp, self.ls, self.B, self.hp, self.beta, self.ml, self.W, self.b, self.env)
        assert_path(eng, self.plan, self.dw)
        assert eng.dp_mode() == 0
        return eng

    def run(self, before=None, between=None, split=None):
        """`before(eng)` switches an instrument on; one train() call of STEPS steps, or -- split = k -- k steps and the
        rest in a second call with `between(eng)` in the middle"""
        eng = self.new()
        try:
            if before:
                before(eng)
            B = self.B
            if split is None:
                assert eng.train(self.x, self.t) == STEPS
            else:
                assert eng.train(self.x[:split * B], self.t[:split * B]) == split
                if between:
                    between(eng)
                assert eng.train(self.x[split * B:], self.t[split * B:]) == STEPS - split
            return snapshot(eng)
        finally:
            eng.close()

    def baseline(self, split=None):
        if split not in self.base:
            self.base[split] = self.run(split=split)
        return self.base[split]


def small_pool(cls, layer, dw):
    """fewer event pairs than the run launches, so the pool runs dry inside a step where a step has several launches"""
    if layer:
        return 2
    return {"fwd": 4, "dx": 3, "dw": 4 if dw > 1 else 2}.get(cls, 2)


# ---------------------------------------------------------------------------------------------------------------------
# A. instruments change no bit: one device
@pytest.mark.parametrize("shape", list(SHAPES))
def test_profiling_changes_no_bit(pkg, monkeypatch, shape):
    """every class x (all layers | layer 2) x stride (1 | 3) x event pool (BIG | smaller than the run's launches)"""
    sub = Subject(pkg, monkeypatch, shape)
    want = sub.baseline()
    bad = []
    for cls in CLASSES:
        for layer in (0, 2):
            for stride in (1, 3):
                for pool in (BIG, small_pool(cls, layer, sub.dw)):
                    got = sub.run(lambda e: e.profile_select(cls, layer, pool, stride))
                    bad += ["%s layer %d stride %d pool %d: %s" % (cls, layer, stride, pool, d)
                            for d in differing(got, want)]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_profile_overhead_between_steps_changes_no_bit(pkg, monkeypatch, shape):
    """the calibration launches of profile_overhead() between two train() calls of a profiled run"""
    sub = Subject(pkg, monkeypatch, shape)
    want = sub.baseline(split=1)
    got = sub.run(lambda e: e.profile_select("dw", 0, BIG, 1), lambda e: e.profile_overhead(), split=1)
    assert not differing(got, want), "\n".join(differing(got, want))
    assert not differing(sub.baseline(), want), "one train() call of 3 steps against 1 + 2 steps"


@pytest.mark.parametrize("shape", list(SHAPES))
def test_stamps_change_no_bit(pkg, monkeypatch, shape):
    """stamp_select(fwd | dx | dw, every layer) and ("dw", -1), the k_dwp_phases twin where the plan has one"""
    sub = Subject(pkg, monkeypatch, shape)
    want = sub.baseline()
    L = len(sub.ls)
    bad = []
    for cls, layer in [(c, l) for c in ("fwd", "dx", "dw") for l in range(1, L)] + [("dw", -1)]:
        got = sub.run(lambda e: e.stamp_select(cls, layer))
        bad += ["stamp %s %d: %s" % (cls, layer, d) for d in differing(got, want)]
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# A. instruments change no bit: the exchange path
def dp_engine(pkg, monkeypatch, mode, world, hp, W, b, env=None, ls=NET, beta=1.2, ml=1):
    """world 1: a one-rank communicator with B = 128; world 4: an emulated world of 4 x 32 frames"""
    env = dict(env or {})
    if world == 1:
        env["MLGGD_DP_MODE"] = mode
    eng = engine(pkg, monkeypatch, ls, 128 // world, hp, beta, ml, W, b, env)
    try:
        if world == 1:
            eng.comm_init(pkg.comm_unique_id(), 1, 0)
        else:
            set_world(eng, mode, world)
        assert eng.dp_mode() == MODES[mode]
    except Exception:
        eng.close()
        raise
    return eng


def dp_subject_run(pkg, monkeypatch, mode, world, W, b, x, t, env=None, before=None):
    eng = dp_engine(pkg, monkeypatch, mode, world, SHIPPED, W, b, env)
    try:
        if before:
            before(eng)
        assert eng.train(x, t) == STEPS
        return snapshot(eng)
    finally:
        eng.close()


@pytest.mark.parametrize("world", [1, 4], ids=["rccl-1", "emulated-4"])
@pytest.mark.parametrize("mode", list(MODES))
def test_profiling_changes_no_bit_on_the_exchange_path(pkg, monkeypatch, mode, world):
    """MLGGD_DP_STOPEV at its default: a profiled fwd / dx / dw launch owns the event slots the armed stop event would
    have ridden on, so the exchange records its event itself; dw again with every collective on the communication
    stream (MLGGD_DP_MAINLINE=0)"""
    W, b = b6.make_net(NET, 7)
    x, t = data(NET, 128, STEPS, 8, W, b)
    bad = []
    for env in (None, {"MLGGD_DP_MAINLINE": "0"}):
        want = dp_subject_run(pkg, monkeypatch, mode, world, W, b, x, t, env)
        for cls in ("fwd", "dx", "dw") if env is None else ("dw",):
            for layer in (0, 2) if env is None else (0,):
                got = dp_subject_run(pkg, monkeypatch, mode, world, W, b, x, t, env,
                                     lambda e: e.profile_select(cls, layer, BIG, 1))
                bad += ["%s layer %d %s: %s" % (cls, layer, env or "", d) for d in differing(got, want)]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mode", list(MODES))
def test_profiled_exchange_steps_against_float64(pkg, monkeypatch, mode):
    """two engines wrong in the same way would agree with each other: emulated world of 4 x 32 frames with dx, then
    dw, profiled (stop events displaced), every rank's step checked element by element"""
    world, B, L = 4, 32, len(NET)
    W, b = b6.make_net(NET, 17)
    x, t = data(NET, B, 2 * world, 18, W, b)
    bad = []
    for cls in ("dx", "dw"):
        eng = dp_engine(pkg, monkeypatch, mode, world, SHIPPED, W, b)
        try:
            eng.keep_ranks()
            eng.profile_select(cls, 0, BIG, 1)
            for k in range(2):
                pre = state(eng, L)
                n = world * B
                xb, tb = x[k * n:(k + 1) * n], t[k * n:(k + 1) * n]
                assert eng.train(xb, tb) == 1
                s = read_dp_step(eng, xb, tb, pre, SHIPPED, 1.2, 1, L, world, set(range(1, L)))
                bad += ["%s step %d %s" % (cls, k + 1, ln)
                        for ln in fail_lines(check_dp(eng, s, set(range(1, L)), mode == "allreduce"))]
            assert eng.profile_read()[1] > 0
        finally:
            eng.close()
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# B. instruments report what happened
def expected_launches(cls, layer, L, dw):
    """launches of (class, layer) in ONE step of a single-device engine, from the plan"""
    if cls == "fwd":
        return L - 1 if layer == 0 else 1
    if cls == "dx":
        return L - 2 if layer == 0 else 0 if layer == 1 else 1
    assert cls == "dw" and layer == 0
    return dw


@pytest.mark.parametrize("shape", list(SHAPES))
def test_launch_counts_and_timing_bound(pkg, monkeypatch, shape):
    sub = Subject(pkg, monkeypatch, shape)
    L, B, s = len(sub.ls), sub.B, STEPS
    eng = sub.new()
    bad = []
    try:
        with pytest.raises(pkg.MlggdError, match="mlggd error 4"):
            eng.last_train_ms()                                    # MLGGD_ERR_STATE before any train_resident
        with pytest.raises(pkg.MlggdError, match="mlggd error 1"):
            eng.profile_select("nonsense")                         # MLGGD_ERR_ARG
        eng.load_chunk(sub.x, sub.t)
        counter = 0                                                # the engine's step counter: steps run so far

        def run(cls, layer, pool, stride):
            nonlocal counter
            eng.profile_select(cls, layer, pool, stride)
            assert eng.train_resident(0, s * B) == s
            timed = sum(1 for c in range(counter, counter + s) if c % stride == 0)
            counter += s
            us, n = eng.profile_read()
            ms, steps = eng.last_train_ms()
            assert steps == s and ms > 0
            tag = "%s layer %d pool %d stride %d" % (cls, layer, pool, stride)
            print("%-40s launches %3d mean %9.3f us, train_resident %9.3f us" % (tag, n, us, 1000 * ms))
            if n > 0 and not us > 0:
                bad.append("%s: mean %g us over %d launches" % (tag, us, n))
            # the profiled intervals are disjoint and lie inside the ev_t0 / ev_t1 bracket of the same in-order stream
            if not n * us <= 1000.0 * ms * (1 + 1e-3):
                bad.append("%s: %d launches x %g us > %g us of train_resident" % (tag, n, us, 1000 * ms))
            if eng.profile_read() != (0.0, 0):
                bad.append("%s: a second profile_read still reports launches" % tag)
            return n, timed

        for cls, layers in (("fwd", range(L)), ("dx", range(L)), ("dw", [0])):
            for layer in layers:
                per_step = expected_launches(cls, layer, L, sub.dw)
                for stride in (1, 3):
                    for pool in (BIG, small_pool(cls, layer, sub.dw), 1):
                        n, timed = run(cls, layer, pool, stride)
                        if n != min(per_step * timed, pool):
                            bad.append("%s layer %d stride %d pool %d: %d launches, the plan gives min(%d x %d, %d)"
                                       % (cls, layer, stride, pool, n, per_step, timed, pool))
        per_layer = [run("dw", l, BIG, 1)[0] for l in range(1, L)]
        if sum(per_layer) != s * sub.dw:
            bad.append("dw per layer %s does not sum to %d" % (per_layer, s * sub.dw))
        for cls in ("transpose", "loss", "update"):               # bracketed classes: the bound only
            run(cls, 0, BIG, 1)
        eng.profile_select(None)
        assert eng.train_resident(0, s * B) == s
        if eng.profile_read() != (0.0, 0):
            bad.append("launches recorded after profile_select(None)")
    finally:
        eng.close()
    assert not bad, "\n".join(bad)


def work(ls, B, world, dp_mode):
    """DESIGN.md's algorithmic work per launch, restated: fwd 2BKN FLOP, 4(KN + BK + 2BN) bytes; dx 2BKN FLOP,
    4(KN + BN + 3BK) bytes, none for layer 1; dw + update 2BKN FLOP, 16 bytes per weight and the operands once,
    4(4KN + BK + BN) -- over the world x B gathered frames in the gather mode (dp_mode 2), over 1 / world of the weight
    rows in the sharded modes (3, 4); the all-reduce mode (1) forms the gradient of the rank's own B frames (DESIGN.md
    states its FLOPs only)"""
    out = {}
    for l in range(1, len(ls)):
        K, N = float(ls[l - 1]), float(ls[l])
        out["fwd", l] = (2 * B * K * N, 4 * (K * N + B * K + 2 * B * N))
        out["dx", l] = (2 * B * K * N, 4 * (K * N + B * N + 3 * B * K)) if l > 1 else (0.0, 0.0)
        G = B * world
        if dp_mode == 2:
            out["dw", l] = (2 * G * K * N, 4 * (4 * K * N + G * K + G * N))
        elif dp_mode in (3, 4):
            out["dw", l] = (2 * G * K * N / world, 4 * (4 * K * N / world + G * K / world + G * N))
        else:
            out["dw", l] = (2 * B * K * N, 4 * (4 * K * N + B * K + B * N) if dp_mode == 0 else None)
    return out


@pytest.mark.parametrize("mode,world,ls,B", [(None, 1, RAGGED, 96), (None, 1, NET, 128), ("allreduce", 4, NET, 32),
                                             ("gather", 4, NET, 32), ("shard", 4, NET, 32), ("shard_a2a", 4, NET, 32)])
def test_kernel_work(pkg, monkeypatch, mode, world, ls, B):
    W, b = b6.make_net(ls, 3)
    eng = engine(pkg, monkeypatch, ls, B, SHIPPED, 1.2, 1, W, b)
    bad = []
    try:
        if mode:
            set_world(eng, mode, world)
        assert eng.dp_mode() == (MODES[mode] if mode else 0)
        want = work(ls, B, world, eng.dp_mode())
        L = len(ls)
        for cls in ("fwd", "dx", "dw"):
            tot_f = tot_b = 0.0
            for l in range(1, L):
                f, by = eng.kernel_work(cls, l)
                wf, wb = want[cls, l]
                tot_f, tot_b = tot_f + f, tot_b + by
                if not np.isclose(f, wf, rtol=1e-12, atol=0) or (wb is not None and not np.isclose(by, wb, rtol=1e-12, atol=0)):
                    bad.append("%s layer %d: kernel_work (%.17g, %.17g), DESIGN.md gives (%.17g, %s)" % (cls, l, f, by, wf, wb))
            f0, b0 = eng.kernel_work(cls, 0)
            if not np.isclose(f0, tot_f, rtol=1e-12) or not np.isclose(b0, tot_b, rtol=1e-12):
                bad.append("%s layer 0 (%g, %g) is not the sum over layers (%g, %g)" % (cls, f0, b0, tot_f, tot_b))
            for l in (L, L + 5, -3):
                if eng.kernel_work(cls, l) != (0.0, 0.0):
                    bad.append("%s layer %d out of range: %s" % (cls, l, eng.kernel_work(cls, l)))
        if eng.kernel_work("dx", 1) != (0.0, 0.0):
            bad.append("dx of layer 1: %s" % (eng.kernel_work("dx", 1),))
    finally:
        eng.close()
    assert not bad, "\n".join(bad)


def stamp_plan(gemm, ls, B, dw):
    """(class, layer) -> (rows stamp_read returns, kernel) for one step of a single-device engine.  The output layer's
    forward GEMM, k_fwd64 / k_dx64 and layers without a launch of their own carry no stamps: 0 rows."""
    L, Bp = len(ls), ceil32(B)
    tiles = {l: -(-ceil32(ls[l - 1]) // 64) * -(-ceil32(ls[l]) // 64) for l in range(1, L)}
    plan = {}
    for l in range(1, L):
        fw, xw = gemm[l - 1]
        plan["fwd", l] = (0, None) if l == L - 1 or fw != 4 else (ceil32(ls[l]) // 32 * (Bp // 32), "fwd")
        plan["dx", l] = (0, None) if l == 1 or xw != 4 else (ceil32(ls[l - 1]) // 32 * (Bp // 32), "dx")
        if Bp % 64:
            plan["dw", l] = (tiles[l], "k_dw")
        elif dw == 1:
            plan["dw", l] = (min(512, sum(tiles.values())), "dwp", sum(tiles.values())) if l == 1 else (0, None)
        else:
            plan["dw", l] = (min(512, tiles[l]), "dwp", tiles[l])
    return plan


def check_stamps(tag, rows, kernel, total=None):
    """slots the stamp() call sites of csrc/kernels.hip.h write are non-zero; successive phases do not go backwards"""
    bad = []
    written, chains = {"fwd": (range(8), [(0, 4, 1, 2, 3, 6), (5, 7)]), "dx": (range(4), [(0, 1, 2, 3)]),
                       "k_dw": (range(6), [(0, 1, 2, 3, 4, 5)]), "dwp": (range(5), [(0, 2), (1, 3)])}[kernel]
    for slot in written:
        if (rows[:, slot] == 0).any():
            bad.append("%s: slot %d is 0 in %d of %d workgroups" % (tag, slot, int((rows[:, slot] == 0).sum()), len(rows)))
    for chain in chains:
        for a, c in zip(chain[:-1], chain[1:]):
            if (rows[:, c] < rows[:, a]).any():
                bad.append("%s: slot %d < slot %d in %d workgroups" % (tag, c, a, int((rows[:, c] < rows[:, a]).sum())))
    if kernel == "dwp" and int(rows[:, 4].sum()) != total:       # slot 4: tiles the workgroup walked
        bad.append("%s: the workgroups walked %d tiles of %d" % (tag, int(rows[:, 4].sum()), total))
    return bad


@pytest.mark.parametrize("shape", ["merged", "dw_per_layer", "ragged", "tile64"])
def test_stamps_report_the_selected_launch(pkg, monkeypatch, shape):
    sub = Subject(pkg, monkeypatch, shape)
    L, B = len(sub.ls), sub.B
    eng = sub.new()
    plan = stamp_plan(eng.gemm_plan(), sub.ls, B, sub.dw)
    bad = []
    try:
        k = 0

        def step():
            nonlocal k
            sl = slice((k % STEPS) * B, (k % STEPS + 1) * B)
            k += 1
            assert eng.train(sub.x[sl], sub.t[sl]) == 1

        for (cls, l), want in plan.items():
            tag = "%s stamp %s %d" % (shape, cls, l)
            eng.stamp_select(cls, l)
            step()
            rows = eng.stamp_read()
            if len(rows) != want[0]:
                bad.append("%s: %d rows, the launch has %d workgroups" % (tag, len(rows), want[0]))
                continue
            if want[0]:
                bad += check_stamps(tag, rows, *want[1:])
                step()                                             # one-shot: the next step leaves buffer and rows alone
                again = eng.stamp_read()
                if again.shape != rows.shape or not np.array_equal(again, rows):
                    bad.append("%s: a following step changed the stamps" % tag)
        if shape == "merged":                                      # the phase twin: rows grid .. 2 grid - 1 hold its sums
            eng.stamp_select("dw", -1)
            step()
            rows = eng.stamp_read()
            grid = plan["dw", 1][0]
            if len(rows) != 2 * grid:
                bad.append("dw -1: %d rows, 2 x %d expected" % (len(rows), grid))
            else:
                bad += check_stamps("dw -1", rows[:grid], "dwp", plan["dw", 1][2])
                ph = rows[grid:]
                for slot in (0, 1, 2, 4):
                    if (ph[:, slot] <= 0).any():
                        bad.append("dw -1: phase sum %d not positive in %d workgroups" % (slot, int((ph[:, slot] <= 0).sum())))
                if (ph[:, 3] != 0).any() or (ph[:, 5:] != 0).any():
                    bad.append("dw -1: unused phase slots written")
    finally:
        eng.close()
    assert not bad, "\n".join(bad)


def test_stamp_grid_larger_than_the_buffer(pkg, monkeypatch):
    """32-8224-257 at B = 1024: the first layer's forward grid is 257 x 32 = 8224 workgroups > 8192 rows"""
    ls, B = [32, 8224, 257], 1024
    assert ceil32(ls[1]) // 32 * (B // 32) > STAMP_ROWS
    W, b = b6.make_net(ls, 5)
    x, t = b6.make_data(ls, 2 * B, 6)
    out = []
    for stamped in (False, True):
        eng = engine(pkg, monkeypatch, ls, B, SHIPPED, 1.2, 1, W, b)
        try:
            assert eng.gemm_plan()[0][0] == 4                      # the 32 x 32-tile kernel, which takes stamps
            if stamped:
                eng.stamp_select("fwd", 1)
            assert eng.train(x, t) == 2
            if stamped:
                assert len(eng.stamp_read()) == 0
            out.append(snapshot(eng))
        finally:
            eng.close()
    assert not differing(out[1], out[0]), "\n".join(differing(out[1], out[0]))


# ---------------------------------------------------------------------------------------------------------------------
# C. state setters
def other_net(ls, seed):
    """a second set of weights and biases with every bit different from make_net(ls, 7)"""
    return b6.make_net(ls, seed, bias=0.25)


SETTER_CASES = [(RAGGED, 96, 1.2, 1), (NET, 128, 2.0, 0)]


@pytest.mark.parametrize("ls,B,beta,ml", SETTER_CASES, ids=["ragged-ML", "net-MMSE"])
def test_set_weights_round_trip_momentum_and_next_step(pkg, monkeypatch, ls, B, beta, ml):
    L = len(ls)
    W0, b0 = b6.make_net(ls, 7)
    W1, b1 = other_net(ls, 70)
    x, t = data(ls, B, 2, 8, W0, b0)
    hp = (DECAY[0], 0.9, DECAY[2])                                 # momentum 0.9 and DECAY's weight decay
    eng = engine(pkg, monkeypatch, ls, B, hp, beta, ml, W0, b0)
    try:
        assert eng.train(x[:B], t[:B]) == 1                        # momentum buffers no longer zero
        _, _, dW, db = state(eng, L)
        assert all(np.abs(d).max() > 0 for d in dW + db)
        eng.set_weights(W1, b1)
        Wg, bg, dWg, dbg = state(eng, L)
        for l in range(L - 1):
            assert np.array_equal(bits(Wg[l]), bits(W1[l])) and np.array_equal(bits(bg[l]), bits(b1[l])), l + 1
            assert np.array_equal(bits(dWg[l]), bits(dW[l])) and np.array_equal(bits(dbg[l]), bits(db[l])), l + 1
        # a NULL layer pointer: MLGGD_ERR_ARG, and no layer has been written (the last layer is the NULL one)
        import ctypes as C
        fp = C.POINTER(C.c_float)
        wp, bp = (fp * L)(), (fp * L)()
        for l in range(1, L - 1):
            wp[l] = W0[l - 1].ctypes.data_as(fp)
            bp[l] = b0[l - 1].ctypes.data_as(fp)
        assert pkg.load().mlggd_set_weights(eng._h, wp, bp) == 1
        Wg, bg = eng.returnWeights()
        for l in range(L - 1):
            assert np.array_equal(bits(Wg[l]), bits(W1[l])) and np.array_equal(bits(bg[l]), bits(b1[l])), l + 1
        # the next step from (W1, b1, the old momentum), momentum 0.9 and weight decay: against float64
        assert eng.train(x[B:], t[B:]) == 1
        reps = b6.check_step(read_step(eng, x[B:], t[B:], (W1, b1, dW, db), hp[0], hp, beta, ml, L))
    finally:
        eng.close()
    assert not fail_lines(reps), "\n".join(fail_lines(reps))


def after_set_weights(eng, x, t, n, W1, b1):
    """one step on W0, set_weights(W1, b1), one step"""
    assert eng.train(x[:n], t[:n]) == 1
    eng.set_weights(W1, b1)
    assert eng.train(x[n:2 * n], t[n:2 * n]) == 1
    return snapshot(eng)


@pytest.mark.parametrize("ls,B,beta,ml", SETTER_CASES, ids=["ragged-ML", "net-MMSE"])
def test_set_weights_equals_a_fresh_engine(pkg, monkeypatch, ls, B, beta, ml):
    """momentum 0: the step after set_weights(W1, b1) is the first step of an engine created with (W1, b1)"""
    W0, b0 = b6.make_net(ls, 7)
    W1, b1 = other_net(ls, 70)
    x, t = data(ls, B, 2, 8, W0, b0)
    eng = engine(pkg, monkeypatch, ls, B, NO_MOM, beta, ml, W0, b0)
    try:
        got = after_set_weights(eng, x, t, B, W1, b1)
    finally:
        eng.close()
    eng = engine(pkg, monkeypatch, ls, B, NO_MOM, beta, ml, W1, b1)
    try:
        assert eng.train(x[B:], t[B:]) == 1
        want = snapshot(eng)
    finally:
        eng.close()
    assert not differing(got, want), "\n".join(differing(got, want))


@pytest.mark.parametrize("ls,B,beta,ml", SETTER_CASES, ids=["ragged-ML", "net-MMSE"])
def test_set_weights_orders_itself_after_enqueued_steps(pkg, monkeypatch, ls, B, beta, ml):
    """train_frames(wait=False) of 6 steps, then set_weights at once: the same bits as with a sync() in between"""
    ctx, toff, nsteps = 3, 1, 6
    dim = ls[0] // ctx
    W0, b0 = b6.make_net(ls, 7)
    W1, b1 = other_net(ls, 70)
    rng = np.random.default_rng(9)
    nfr = nsteps * B + ctx
    feat = rng.standard_normal((nfr, dim), dtype=np.float32)
    targ = rng.standard_normal((nfr, ls[-1]), dtype=np.float32)
    first = rng.permutation(nfr - ctx + 1)[:nsteps * B].astype(np.int32)
    out = []
    for sync in (True, False):
        eng = engine(pkg, monkeypatch, ls, B, SHIPPED, beta, ml, W0, b0)
        try:
            assert eng.train_frames(feat, targ, first, ctx, toff, wait=False) == nsteps
            if sync:
                eng.sync()
            eng.set_weights(W1, b1)
            Wg, bg = eng.returnWeights()
            for l in range(len(ls) - 1):
                assert np.array_equal(bits(Wg[l]), bits(W1[l])) and np.array_equal(bits(bg[l]), bits(b1[l])), l + 1
            assert eng.train_frames(feat, targ, first[:B], ctx, toff) == 1
            out.append(snapshot(eng))
        finally:
            eng.close()
    assert not differing(out[1], out[0]), "\n".join(differing(out[1], out[0]))


@pytest.mark.parametrize("world", [1, 4], ids=["rccl-1", "emulated-4"])
@pytest.mark.parametrize("mode", list(MODES))
def test_set_weights_on_the_exchange_path(pkg, monkeypatch, mode, world):
    """momentum 0, 531-300-130-257 on 128 global frames: after the sharded exchanges' weight all-gathers, set_weights
    + one step equals the first step of a fresh engine on (W1, b1)"""
    W0, b0 = b6.make_net(NET, 7)
    W1, b1 = other_net(NET, 70)
    x, t = data(NET, 128, 2, 8, W0, b0)
    eng = dp_engine(pkg, monkeypatch, mode, world, NO_MOM, W0, b0)
    try:
        got = after_set_weights(eng, x, t, 128, W1, b1)
    finally:
        eng.close()
    eng = dp_engine(pkg, monkeypatch, mode, world, NO_MOM, W1, b1)
    try:
        assert eng.train(x[128:], t[128:]) == 1
        want = snapshot(eng)
    finally:
        eng.close()
    assert not differing(got, want), "\n".join(differing(got, want))


@pytest.mark.parametrize("mode", ["shard", "shard_a2a"])
def test_step_after_set_weights_on_sharded_updates_against_float64(pkg, monkeypatch, mode):
    world, B, L = 4, 32, len(NET)
    W0, b0 = b6.make_net(NET, 7)
    W1, b1 = other_net(NET, 70)
    x, t = data(NET, B, 2 * world, 8, W0, b0)
    n = world * B
    eng = dp_engine(pkg, monkeypatch, mode, world, DECAY, W0, b0)
    try:
        eng.keep_ranks()
        assert eng.train(x[:n], t[:n]) == 1
        _, _, dW, db = state(eng, L)
        eng.set_weights(W1, b1)
        assert eng.train(x[n:], t[n:]) == 1
        s = read_dp_step(eng, x[n:], t[n:], (W1, b1, dW, db), DECAY, 1.2, 1, L, world, set(range(1, L)))
        reps = check_dp(eng, s, set(range(1, L)), False)
    finally:
        eng.close()
    assert not fail_lines(reps), "\n".join(fail_lines(reps))


@pytest.mark.parametrize("device_reduce", [False, True])
def test_set_scalefactor(pkg, monkeypatch, device_reduce):
    """round trip in every bit; cv_all of an engine that has never trained uses the alpha it was given; a training step
    then replaces it with the minibatch's own (check_step verifies that value).

    CV targets: the device sums (per-tile partials in double) take make_data's targets, whose column 0 has magnitude
    1e3.  The host-order sums are ONE fp32 chain over all n D terms in frame-major order (the reference's loop), and
    expect_cv's tight limit 4 sqrt(N) presumes rounding errors that do not all point one way.  That holds only while a
    term is above half an ulp of the running sum: column 0's 300 terms of 1e6 raise the sum to 3e8 (ulp 32), every one
    of the 77,000 terms of order 1 is then absorbed whole, and a plain numpy fp32 chain over these very values sits at
    4367 against the limit of 1111 (hard ratio 0.056) -- the stagnation include/mlggd.h describes for the host-order
    sums, not an error of the engine.  So in host order the targets are plain N(0, 1): every term stays above 100 ulps
    of a running sum that ends near 2e5, and the same numpy chain sits at 177."""
    ls, B, beta = [531, 300, 257], 128, 1.2
    L = len(ls)
    W, b = b6.make_net(ls, 41)
    x, t = data(ls, B, 1, 42, W, b)
    alpha = np.random.default_rng(43).uniform(0.05, 3.0, ls[-1]).astype(np.float32)
    eng = engine(pkg, monkeypatch, ls, B, SHIPPED, beta, 1, W, b)
    try:
        eng.set_scalefactor(alpha)
        assert np.array_equal(bits(eng.scalefactor()), bits(alpha))
        eng.set_cv_device_reduce(device_reduce)
        cx, ct = b6.make_data(ls, 2 * B + 44, 44)
        if not device_reduce:
            ct = np.random.default_rng(45).standard_normal(ct.shape).astype(np.float32)
        sq, ab, ll = eng.cv_all(cx, ct)
        assert np.array_equal(bits(eng.scalefactor()), bits(alpha))
        ex = b6.expect_cv(eng.forward(cx), ct, beta, alpha, pkg.gamma)
        reps = [b6.compare(k, np.array(v), ex[k]) for k, v in (("sqerr", sq), ("abserr", ab), ("loglik", ll))]
        pre = state(eng, L)
        assert eng.train(x, t) == 1
        assert not np.array_equal(bits(eng.scalefactor()), bits(alpha))
        reps += b6.check_step(read_step(eng, x, t, pre, SHIPPED[0], SHIPPED, beta, 1, L))
    finally:
        eng.close()
    assert not fail_lines(reps), "\n".join(fail_lines(reps))
