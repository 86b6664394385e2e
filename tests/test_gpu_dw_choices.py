"""GPU: every dW kernel and every workgroup-to-tile map that a knob or a bunch size selects, against the oracle's
MFMA-order twin and against the default engine, BIT FOR BIT (0 differing elements, no tolerance).

The twin states dW as one chain per weight over the frames in order.  k_dw<1> (64 x 64 tiles, one launch per layer),
k_dw<2> (128 x 128 tiles, MLGGD_DW_TILE=2 or the automatic choice at >= 192 such tiles) and k_dwp<H> (persistent, Bp = 64 H
frames, H in 1, 2, 4, 8 on one device and up to 16 over gathered factors) are three tilings of that one chain, so whichever
of them a bunch size or a knob selects must leave the same bits -- as must every placement of the forward / dX tiles on
the workgroups (MLGGD_TILE_MAP) and every grid of the persistent kernel (MLGGD_DWP_PER_CU).

Which kernel ran is asserted, not assumed: the stamp instrument returns one row per workgroup of the selected launch, and
the row count is the launch's grid (dw_kernel below).  Every test first asserts, on the host, that the counts it relies on
differ at its shapes."""
import types

import numpy as np
import pytest

from test_gpu_dwp_bookkeeping import differing, random_frames, random_net
from test_gpu_vs_float64 import KNOBS

pytestmark = pytest.mark.gpu

HP = (0.1, 0.9, 1e-5)                      # lrate, momentum, weightcost
DP_KNOBS = ("MLGGD_DP_MODE", "MLGGD_DP_FINE", "MLGGD_DP_STOPEV", "MLGGD_DP_MAINLINE", "MLGGD_DP_AR_SHARD",
            "MLGGD_DP_STAT_COMM", "MLGGD_FAKE_ONLY_RANK")
R = [531, 97, 33, 1, 257]                  # no dimension a multiple of 32, 64 or 128; a one-unit layer; 257 -> Np = 288: the
#                                            last 128-tile is 32 columns wide; 531 -> Kp = 544: 32 rows in the last 128-tile row
M = [531, 300, 130, 257]
LOSSES = [(0, 2.0), (1, 1.2)]              # MMSE, ML-GGD beta = 1.2
TILES = (None, "2")                        # MLGGD_DW_TILE unset (k_dw<1>) and "2" (k_dw<2>)
_DATA, _TWIN = {}, {}


def ceil32(n):
    return (n + 31) // 32 * 32


def tiles(ls, l, width):
    """workgroups of layer l's dW launch at `width` x `width` tiles (csrc/engine.hip launch_dw, dwp_args)"""
    return -(-ceil32(ls[l - 1]) // width) * -(-ceil32(ls[l]) // width)


def total64(ls):
    return sum(tiles(ls, l, 64) for l in range(1, len(ls)))


def dw_kernel(eng, l, step, per_cu=2):
    """Which kernel runs layer l's dW: stamp_select("dw", l), one training step (`step()`), stamp_read() ->
    (rows, kind).  The row count is the grid of the stamped launch:
      "k_dw1"  ceil(Kp/64) ceil(Np/64) rows, slot 5 written (k_dw stamps its last store; k_dwp has no slot 5);
      "k_dw2"  ceil(Kp/128) ceil(Np/128) rows, slot 5 written;
      "k_dw"   a k_dw launch of a layer so small that both tilings have the same grid (33 -> 1: one workgroup);
      "dwp"    min(256 per_cu, total) rows, slot 5 untouched, and slot 4 -- tiles the workgroup walked -- sums to the
               total: the layer's own 64 x 64 tiles, or all layers' where the engine merges them into one launch (that
               launch carries layer 1's stamps; the other layers then have no launch and return no rows);
      None     anything else.
    The unfused k_dw<T, false> launch is passed no stamp buffer, so it returns no rows; the tests of the unfused form
    assert the kind on the same engine configuration in its fused form -- the same `big` expression of launch_dw_layer
    picks T for both."""
    ls = eng.layersizes
    eng.stamp_select("dw", l)
    step()
    rows = eng.stamp_read()
    n1, n2 = tiles(ls, l, 64), tiles(ls, l, 128)
    total = total64(ls) if eng.dw_launches_per_step() == 1 else n1
    kind = None
    if len(rows) and (rows[:, 5] != 0).all():
        if len(rows) in (n1, n2):
            kind = "k_dw" if n1 == n2 else "k_dw1" if len(rows) == n1 else "k_dw2"
    elif len(rows) == min(256 * per_cu, total) and (rows[:, 5] == 0).all() and int(rows[:, 4].sum()) == total:
        kind = "dwp"
    return rows, kind


def k_dw_kinds(ls, tile):
    """what dw_kernel must say per layer when k_dw<1> (tile None) or k_dw<2> (tile "2") runs every layer"""
    return ["k_dw" if tiles(ls, l, 64) == tiles(ls, l, 128) else "k_dw2" if tile == "2" else "k_dw1"
            for l in range(1, len(ls))]


def run_data(ls, n, ml):
    key = (tuple(ls), n, ml)
    if key not in _DATA:
        ws, bs = random_net(ls, sum(ls) + ml)
        x, t = random_frames(n, ls, sum(ls) + n + ml)
        for a in ws + bs + [x, t]:
            a.setflags(write=False)
        _DATA[key] = (ws, bs, x, t)
    return _DATA[key]


def twin_state(pyoracle, ls, n, steps, ml, beta, world, allreduce, slabs, plan, acts, fresh):
    """the twin's side of a run, computed once per (net, bunch, loss, world, launch plan) and never written to"""
    key = (tuple(ls), n, steps, ml, beta, world, allreduce, slabs, tuple(plan), acts, fresh)
    if key not in _TWIN:
        ws, bs, x, t = run_data(ls, steps * n + fresh, ml)
        # allreduce at world 1: fake_world(1, allreduce=True), a world of one rank -- its statistic is k_colsum's
        pyoracle.set_gemm_order("hip", slabs, plan=plan, dp_world=world, dp_allreduce=allreduce,
                                dp_one_rank=allreduce and world == 1)
        try:
            twin = pyoracle.OracleNet(ls, n, *HP, beta, ml, ws, bs)
            assert twin.train(x[:steps * n], t[:steps * n]) == steps
            wt, bt = twin.get_weights()
            s = {}
            for l in range(1, len(ls)):
                s["W_%d" % l], s["b_%d" % l] = wt[l - 1], bt[l - 1]
                s["delta_w_%d" % l], s["delta_b_%d" % l] = twin.tensor("delta_w", l), twin.tensor("delta_b", l)
                if acts:
                    s["dedx_%d" % l] = twin.tensor("dedx", l, rows=n)
                    if l < len(ls) - 1:
                        s["y_%d" % l] = twin.tensor("y", l, rows=n)
            if acts:
                s["out"] = twin.tensor("out", rows=n)
            if ml == 1:
                s["scalefactor"] = twin.tensor("scalefactor")
            if fresh:
                xf = x[steps * n:]
                s["forward"] = np.concatenate([twin.cv_forward(xf[i:i + n]) for i in range(0, fresh, n)])
            twin.close()
        finally:
            pyoracle.set_gemm_order("ref")
        _TWIN[key] = s
    return _TWIN[key]


def count_differing(tag, got, want):
    assert set(got) == set(want), (tag, sorted(got), sorted(want))
    return sum(differing("%s %s" % (tag, k), got[k], want[k]) for k in want)


@pytest.fixture
def twin_run(pkg, pyoracle, monkeypatch):
    def run(ls, B, steps, env, ml, beta, world=1, allreduce=False, kinds=(), per_cu=2, acts=False, fresh=0):
        """`steps` >= 2 training steps (the second reads the W / delta the first one's epilogue wrote, with momentum and
        weight decay at work) on an engine built under `env` alone -- every knob is deleted first -- and on the twin in
        the engine's own launch plan.  world > 1 or allreduce: an emulated world (factor gather, or the gradient
        all-reduce and the unfused dW) against the twin's data-parallel form.  -> .bad: differing elements over W, b,
        delta_w, delta_b of every layer and the ML scale factor (acts: also y, dedx, out of the last step; fresh: also
        forward() of that many new rows); .state: the engine's tensors; .kinds: dw_kernel of the layers in `kinds`, taken
        on this engine by further steps after the comparison; .launches, .dp_mode, .plan, .slabs."""
        assert steps >= 2
        for k in KNOBS + DP_KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        L, n = len(ls), world * B
        ws, bs, x, t = run_data(ls, steps * n + fresh, ml)
        tag = "%s B %d %s" % (ls, B, " ".join("%s=%s" % (k[6:], v) for k, v in env.items()))
        eng = pkg.BPGpu(1, 0, ls, B, *HP, ws, bs, beta, ml)
        try:
            if world > 1 or allreduce:
                eng.fake_world(world, allreduce=allreduce)
            r = types.SimpleNamespace(launches=eng.dw_launches_per_step(), dp_mode=eng.dp_mode(), plan=eng.gemm_plan(),
                                      slabs=eng.out_slabs())
            assert eng.train(x[:steps * n], t[:steps * n]) == steps
            we, be = eng.returnWeights()
            s = {}
            for l in range(1, L):
                s["W_%d" % l], s["b_%d" % l] = we[l - 1], be[l - 1]
                s["delta_w_%d" % l], s["delta_b_%d" % l] = eng.debug_tensor("delta_w", l), eng.debug_tensor("delta_b", l)
                if acts:
                    s["dedx_%d" % l] = eng.debug_tensor("dedx", l)
                    if l < L - 1:
                        s["y_%d" % l] = eng.debug_tensor("y", l)
            if acts:
                s["out"] = eng.debug_tensor("out")
            if ml == 1:
                s["scalefactor"] = eng.scalefactor()
            if fresh:
                s["forward"] = eng.forward(x[steps * n:])
            assert all(not np.array_equal(s["W_%d" % l], ws[l - 1]) for l in range(1, L))     # every layer was trained
            r.state = s
            r.kinds = [dw_kernel(eng, l, lambda: eng.train(x[:n], t[:n]), per_cu) for l in kinds]
        finally:
            eng.close()
        want = twin_state(pyoracle, ls, n, steps, ml, beta, world, allreduce, r.slabs, r.plan, acts, fresh)
        r.bad = count_differing(tag + " vs twin:", s, want)
        return r
    return run


def tile_env(tile, **more):
    env = {"MLGGD_DW_TILE": tile} if tile else {}
    env.update(more)
    return env


def assert_k_dw_counts_differ(ls, least=None):
    """host side: the grids of k_dw<1>, k_dw<2> and the merged k_dwp differ on at least `least` layers (all by default)"""
    pairs = [(tiles(ls, l, 64), tiles(ls, l, 128)) for l in range(1, len(ls))]
    told_apart = sum(1 for a, b in pairs if a != b)
    assert told_apart >= (len(pairs) if least is None else least), pairs
    assert all(min(512, total64(ls)) not in p for p in pairs), (pairs, total64(ls))


# ---------------------------------------------------------------------------------------------------------------------
# 1. k_dw<1> and k_dw<2> where Bp is no bunch size of k_dwp
@pytest.mark.parametrize("B", [7, 96, 150, 192])
@pytest.mark.parametrize("ls", [R, M], ids=["R", "M"])
def test_k_dw_both_tiles_equal_the_twin_bitwise(twin_run, ls, B):
    """Bp = 32: one short chunk (T = 2: the first staging pass masked from row 32); 96: T = 1 runs 64 + 32, T = 2 one chunk
    whose second staging pass is masked from row 96; 160: 64 + 64 + 32 and 128 + 32; 192: Bp / 64 = 3, a multiple of 64
    k_dwp still refuses, 128 + 64.  Two steps of each loss; the kind of every layer's launch; k_dw<2>'s bits are also
    k_dw<1>'s."""
    L = len(ls)
    assert_k_dw_counts_differ(ls, least=3)             # R's 33 -> 1 layer is one workgroup either way
    assert ceil32(B) // 64 not in (1, 2, 4, 8) or ceil32(B) % 64
    bad = 0
    for ml, beta in LOSSES:
        runs = {}
        for tile in TILES:
            r = runs[tile] = twin_run(ls, B, 2, tile_env(tile), ml, beta, kinds=range(1, L))
            assert [k for _, k in r.kinds] == k_dw_kinds(ls, tile), (tile, [(len(rows), k) for rows, k in r.kinds])
            assert r.launches == L - 1 and r.dp_mode == 0
            bad += r.bad
        bad += count_differing("DW_TILE=2 vs unset:", runs["2"].state, runs[None].state)
    assert bad == 0


# ---------------------------------------------------------------------------------------------------------------------
# 2. MLGGD_DW_PERSIST=0: k_dw where k_dwp would run
@pytest.mark.parametrize("B", [64, 128])
def test_dw_persist_0_equals_the_twin_and_k_dwp_bitwise(twin_run, B):
    assert_k_dw_counts_differ(M)
    bad = 0
    for ml, beta in LOSSES:
        base = twin_run(M, B, 2, {}, ml, beta, kinds=[1])
        assert base.launches == 1 and base.kinds[0][1] == "dwp", len(base.kinds[0][0])
        bad += base.bad
        for tile in TILES:
            r = twin_run(M, B, 2, tile_env(tile, MLGGD_DW_PERSIST="0"), ml, beta, kinds=range(1, len(M)))
            assert [k for _, k in r.kinds] == k_dw_kinds(M, tile), (tile, [(len(rows), k) for rows, k in r.kinds])
            assert r.launches == 3
            bad += r.bad + count_differing("DW_PERSIST=0 DW_TILE=%s vs k_dwp:" % tile, r.state, base.state)
    assert bad == 0


# ---------------------------------------------------------------------------------------------------------------------
# 3. B = 1024 on one device: dwp_usable() stops at eight units, so k_dw walks 16 (T = 1) or 8 (T = 2) chunks
@pytest.mark.parametrize("tile", TILES, ids=["tile1", "tile2"])
def test_1024_frames_on_one_device_run_k_dw(twin_run, tile):
    ls = [300, 130, 40]
    assert_k_dw_counts_differ(ls)
    bad = 0
    for ml, beta in LOSSES:
        r = twin_run(ls, 1024, 2, tile_env(tile), ml, beta, kinds=[1, 2])
        assert [k for _, k in r.kinds] == k_dw_kinds(ls, tile), [(len(rows), k) for rows, k in r.kinds]
        assert r.launches == 2 and r.dp_mode == 0
        bad += r.bad
    assert bad == 0


# ---------------------------------------------------------------------------------------------------------------------
# 4. MLGGD_DW_TILE=0: the automatic choice on both sides of its threshold of 192 tiles of 128 x 128
@pytest.mark.parametrize("K,want", [(1536, ["k_dw2", "k_dw1"]), (1408, ["k_dw1", "k_dw1"])])
def test_dw_tile_auto_on_both_sides_of_the_threshold(twin_run, K, want):
    ls = [K, 2048, 257]
    assert_k_dw_counts_differ(ls)
    assert [tiles(ls, l, 128) >= 192 for l in (1, 2)] == [k == "k_dw2" for k in want]
    assert tiles(ls, 1, 128) == (192 if K == 1536 else 176) and tiles(ls, 2, 128) == 48
    r = twin_run(ls, 32, 2, {"MLGGD_DW_TILE": "0"}, 0, 2.0, kinds=[1, 2])
    assert [k for _, k in r.kinds] == want, [(len(rows), k) for rows, k in r.kinds]
    assert r.bad == 0


# ---------------------------------------------------------------------------------------------------------------------
# 5. the unfused form: k_dw<T, false> + k_apply_update + k_bias_apply under the gradient all-reduce
@pytest.mark.parametrize("world", [1, 2])
def test_unfused_k_dw_under_a_gradient_allreduce(twin_run, world):
    """R at B = 96 as one and as two emulated ranks with the gradient all-reduce, against the twin in its data-parallel
    form (as test_the_unfused_form_under_a_gradient_allreduce does for k_dwp).  The unfused launch carries no stamps, so
    the kind is asserted on the fused engine of the same configuration (dw_kernel's docstring)."""
    assert_k_dw_counts_differ(R, least=3)
    bad = 0
    for tile in TILES:
        fused = twin_run(R, 96, 2, tile_env(tile), 1, 1.2, kinds=range(1, len(R)))
        assert [k for _, k in fused.kinds] == k_dw_kinds(R, tile), (tile, [(len(rows), k) for rows, k in fused.kinds])
        for ml, beta in LOSSES:
            r = twin_run(R, 96, 2, tile_env(tile), ml, beta, world=world, allreduce=True, kinds=[1])
            assert r.dp_mode == 1 and r.launches == len(R) - 1
            assert len(r.kinds[0][0]) == 0                         # FUSED = false: no stamp buffer
            bad += r.bad
    assert bad == 0


# ---------------------------------------------------------------------------------------------------------------------
# 6. k_dwp<16> where it really runs: the factor-gather exchange at 1024 global frames
@pytest.mark.parametrize("world,B", [(8, 128), (2, 512)])
@pytest.mark.parametrize("ls", [[96, 64], R], ids=["96-64", "R"])
def test_k_dwp_16_over_1024_gathered_frames(twin_run, ls, world, B):
    """launch_dwp's switch takes world x Bp / 64 = 16 units, which only launch_dwp_t<16> serves (any other count fails
    with "no dW kernel for ... units per tile"); the stamps of that one merged launch give its grid and tile total.  On
    96-64 that grid is k_dw<1>'s too (two workgroups): there the kind rests on slots 4 and 5 (dw_kernel)."""
    assert world * B == 1024 and world * B // 64 == 16
    assert total64(ls) < 512 and total64(ls) != tiles(ls, 1, 128)
    bad = 0
    for ml, beta in LOSSES:
        r = twin_run(ls, B, 2, {}, ml, beta, world=world, kinds=[1])
        rows, kind = r.kinds[0]
        assert r.dp_mode == 2 and r.launches == 1
        assert kind == "dwp" and len(rows) == total64(ls), (len(rows), kind)
        bad += r.bad
    assert bad == 0


# ---------------------------------------------------------------------------------------------------------------------
# 7. MLGGD_DWP_PER_CU: the grid of the persistent kernel
WIDE = [1100, 1024, 257]                   # 18 x 16 + 16 x 5 = 368 tiles over two layers: more than one grid of 256


@pytest.mark.parametrize("ls", [WIDE, M], ids=["368-tiles", "75-tiles"])
def test_dwp_per_cu_grids_equal_the_twin_bitwise(twin_run, ls):
    """per_cu = 1 on 368 tiles: 256 workgroups, 112 of which walk two tiles and cross from layer 2's job into layer 1's;
    "3": one tile per workgroup; "0" falls back to 2 (dwp_grid).  Three ML steps."""
    total = total64(ls)
    assert (total > 256 and len(ls) >= 3) if ls is WIDE else total < 256
    assert total == (368 if ls is WIDE else 75)
    base = twin_run(ls, 128, 3, {}, 1, 1.2, kinds=[1])
    assert base.kinds[0][1] == "dwp" and len(base.kinds[0][0]) == min(512, total) and base.launches == 1
    bad = base.bad
    for knob, n in (("1", 1), ("3", 3), ("0", 2)):
        r = twin_run(ls, 128, 3, {"MLGGD_DWP_PER_CU": knob}, 1, 1.2, kinds=[1], per_cu=n)
        rows, kind = r.kinds[0]
        assert kind == "dwp" and len(rows) == min(256 * n, total), (knob, len(rows), kind)
        assert int(rows[:, 4].sum()) == total
        if knob == "1" and ls is WIDE:
            assert rows[:, 4].max() >= 2 and len(rows) == 256
        bad += r.bad + count_differing("DWP_PER_CU=%s vs default:" % knob, r.state, base.state)
    assert bad == 0


# ---------------------------------------------------------------------------------------------------------------------
# 8. MLGGD_TILE_MAP: the workgroup -> tile map of k_fwd, k_dx, k_fwd64, k_dx64 and the split-K output layer
MAPPED = [531, 256, 512, 300, 256]         # unit tiles of 32: 8, 16, 10, 8 (output); of 64: 4, 8, 5


@pytest.mark.parametrize("B,tile64", [(96, None), (128, None), (128, "2")], ids=["B96", "B128", "B128-tile64"])
def test_tile_maps_equal_the_twin_bitwise(twin_run, B, tile64):
    """tile_of_block takes its XCD branch where the unit-tile count is a multiple of 8: 256 and 512 units for the 32-tile
    kernels, 512 for the 64-tile ones, the 256-wide output layer in three split-K slabs; 300 units (10 and 5 tiles) take
    the plain branch.  B = 96: divmod_by's division form (three bunch tiles), 128: its shift form.  Three ML steps on
    different rows -- a tile left unwritten keeps the previous step's values -- then y, dedx, out of the last step, all
    weights and the forward of B + 37 fresh rows."""
    t32 = [ceil32(u) // 32 for u in MAPPED[1:]]
    assert [n % 8 == 0 for n in t32] == [True, True, False, True]
    assert [ceil32(u) // 64 % 8 == 0 for u in MAPPED[1:4]] == [False, True, False] and ceil32(MAPPED[3]) % 64 == 0
    env = {"MLGGD_S_OUT": "3"}
    if tile64:
        env["MLGGD_TILE64"] = tile64
    base = twin_run(MAPPED, B, 3, env, 1, 1.2, acts=True, fresh=B + 37)
    assert base.slabs == 3
    assert base.plan == ([(1, 4), (1, 1), (1, 1), (4, 1)] if tile64 else [(4, 4)] * 4), base.plan
    bad = base.bad
    for m in ("1", "2"):
        r = twin_run(MAPPED, B, 3, dict(env, MLGGD_TILE_MAP=m), 1, 1.2, acts=True, fresh=B + 37)
        assert r.plan == base.plan and r.slabs == 3
        bad += r.bad + count_differing("TILE_MAP=%s vs unset:" % m, r.state, base.state)
    assert bad == 0
