"""The cases of tests/test_gpu_twin_relu_bins.py (GPU: the engine against the oracle's MFMA-order twin, bit for bit, with
rectified-linear hidden units and with a shape factor per output bin), kept apart from it so that
tests/test_oracle_relu_bins.py can show on the CPU, with the twin alone, that every ReLU case is not degenerate: between
20 % and 80 % of each hidden layer's y exactly 0 in the last step (relu64.ZERO_FRACTION), finite values, weights that
moved.  The seeds are picked there.

Data: Glorot weights with biases U(+-0.5) (bounds64.make_net), standard-normal inputs and targets."""
import numpy as np

import bounds64 as b6
import relu64 as r6
import shapes64 as s6

HP = r6.CASE_HP                         # lrate 0.01, momentum 0.9, weightcost 1e-5
LOSSES = [(0, 2.0), (0, 1.0), (1, 1.0), (1, 1.2), (1, 0.9)]
REAL_LS = [2827, 2048, 2048, 2048, 257]
VAR_LS = [1210, 1060, 70, 262, 40]      # a wave's K range of several chunks plus a partial one, a single partial chunk,
                                        # an empty one
DX_BOTH_LS = [40, 531, 64, 19]          # at B = 512 one dX launch in each form of k_dx (dx_workgroups below)
DROP_LS = [257 * 3, 256, 192, 257]      # the shape of test_dropout_runs_equal_the_twin_bit_for_bit
DROP_KW = dict(dropoutflag=1, visible_omit=0.2, hid_omit=0.5)
DROP_SEED = 77

# a. whole ReLU runs: (layersizes, B, steps, seed) x LOSSES ...
RUNS = [(r6.CASE_LS, 24, 6, 3), (r6.CASE_LS, 128, 6, 3), (VAR_LS, 96, 3, 31)]
# ... and single cases (layersizes, B, steps, seed, ml, beta): the real widths; k_dwp<4> / <8> behind a ReLU layer; both
# forms of k_dx in one run
SINGLE_RUNS = [(REAL_LS, 128, 8, 51, 1, 1.0), ([300, 96, 40], 256, 3, 52, 1, 1.2), ([300, 96, 40], 512, 3, 52, 1, 1.2),
               (DX_BOTH_LS, 512, 3, 53, 1, 1.2)]
# b. the 64 x 64 kernels (MLGGD_TILE64=2): (layersizes, B, steps, seed, the plan the CPU check runs: hidden forwards
# and dX launches in the 64 x 64 form, which the GPU test requires of the engine's own plan)
TILE64 = [([96, 128, 128, 40], 64, 3, 41, [(1, 4), (1, 1), (4, 1)]),
          ([64, 192, 128, 257], 128, 3, 43, [(1, 4), (1, 1), (4, 1)])]
TILE64_LOSS = (1, 1.2)
# c. MLGGD_S_OUT behind a ReLU layer
S_OUT_CASE = ([99, 64, 257], 128, 3, 61, 1, 1.2)
# d. ReLU with dropout
DROP_CASE = (DROP_LS, 128, 6, 71)
DROP_LOSSES = [(0, 2.0), (1, 1.0)]
# e. emulated worlds, ReLU: CASE_LS, 32 rows per rank, ML-GGD beta 0.9
WORLD_CASE = (r6.CASE_LS, 32, 3, 3, 1, 0.9)
WORLD_SIZES = (2, 4)
# g. ReLU + a mixed shape vector + dropout
ALL_CASE = (r6.CASE_LS, 128, 4, 3)
ALL_DROP_KW = dict(dropoutflag=1, visible_omit=0.2, hid_omit=0.3)


def net(ls, seed):
    return b6.make_net(ls, seed)


def data(ls, n, seed):
    """n rows of standard-normal inputs and targets; never written to"""
    rng = np.random.default_rng(seed + 1000)
    x = rng.standard_normal((n, ls[0])).astype(np.float32)
    t = rng.standard_normal((n, ls[-1])).astype(np.float32)
    x.setflags(write=False)
    t.setflags(write=False)
    return x, t


def dx_workgroups(ls, B):
    """{l: workgroups of the 32 x 32-tile dX launch of layer l, l = 2 .. L - 1}: unit tiles of layer l - 1 x frame tiles.
    Up to 256 of them k_dx takes its operands by LDS-DMA, above that through staging registers (engine.hip dx_dma)."""
    return {l: -(-ls[l - 1] // 32) * -(-B // 32) for l in range(2, len(ls))}


def distinct_betas(D, seed=5):
    """[D] float32 drawn from U(0.5, 2.2) with no two equal: a read of a neighbouring bin's beta cannot coincide"""
    v = np.random.default_rng(seed).uniform(0.5, 2.2, D).astype(np.float32)
    assert len(np.unique(v)) == D
    return v


def relu_cases():
    """every ReLU case of the GPU file as (id, layersizes, rows per step, steps, seed, ml, beta, OracleNet keywords,
    plan or None, dp_world): what the CPU check walks"""
    out = []
    for ls, B, steps, seed in RUNS:
        for ml, beta in LOSSES:
            out.append(("run %s B%d ml%d beta%g" % (ls, B, ml, beta), ls, B, steps, seed, ml, beta, {}, None, 1))
    for ls, B, steps, seed, ml, beta in SINGLE_RUNS:
        out.append(("run %s B%d" % (ls, B), ls, B, steps, seed, ml, beta, {}, None, 1))
    for ls, B, steps, seed, plan in TILE64:
        out.append(("tile64 %s" % ls, ls, B, steps, seed) + TILE64_LOSS + ({}, plan, 1))
    ls, B, steps, seed, ml, beta = S_OUT_CASE
    out.append(("s_out", ls, B, steps, seed, ml, beta, {}, None, 1))
    ls, B, steps, seed = DROP_CASE
    for ml, beta in DROP_LOSSES:
        out.append(("dropout ml%d" % ml, ls, B, steps, seed, ml, beta, dict(DROP_KW, random_seed=DROP_SEED), None, 1))
    ls, B, steps, seed, ml, beta = WORLD_CASE
    for w in WORLD_SIZES:
        out.append(("world %d" % w, ls, w * B, steps, seed, ml, beta, {}, None, w))
    ls, B, steps, seed = ALL_CASE
    out.append(("relu + bins + dropout", ls, B, steps, seed, 1, 1.7,
                dict(ALL_DROP_KW, random_seed=DROP_SEED, shapefactors=s6.mixed(ls[-1])), None, 1))
    return out


def zero_fractions(net, L, rows):
    """the fraction of exact zeros in every hidden layer's y of the last step (an OracleNet or a BPGpu)"""
    get = (lambda l: net.tensor("y", l, rows=rows)) if hasattr(net, "tensor") else (lambda l: net.debug_tensor("y", l))
    return {l: float((get(l) == 0).mean()) for l in range(1, L - 1)}


def assert_not_degenerate(fracs):
    lo, hi = r6.ZERO_FRACTION
    for l, f in fracs.items():
        assert lo <= f <= hi, "layer %d: %.3f of y are zero" % (l, f)
