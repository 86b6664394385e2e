"""The cases of tests/test_gpu_adam.py (GPU: whole Adam runs against the oracle's MFMA-order twin plus the numpy rule, bit
for bit), kept apart from it so that tests/test_adam_model.py can show on the CPU, with the model alone, that no case is
degenerate: after its steps every layer's W, m and v differ from their start in more than half their elements and all
of it is finite.

Data: Glorot weights with biases U(+-0.5) (bounds64.make_net), standard-normal inputs and targets (twin_cases.data)."""
import collections

import bounds64 as b6
import twin_cases as tc

Case = collections.namedtuple("Case", "id ls B steps seed ml beta activation wc lr beta1 beta2 eps")
RATE = dict(lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8)          # lr: large enough that six steps move every weight visibly
MMSE, GGD = (0, 2.0), (1, 1.2)


def case(id, ls, B, steps, seed, loss, activation="sigmoid", wc=1e-5, **kw):
    return Case(id, ls, B, steps, seed, loss[0], loss[1], activation, wc, **dict(RATE, **kw))


# 1. bit for bit over whole runs: both nets, both bunch sizes (B = 32 and 160: the per-layer k_dw launches; neither is a
# multiple of 64), both losses; one ReLU case, one without weightcost, one with other betas and a large eps
RUNS = [case("%s-B%d-%s" % ("x".join(map(str, ls)), B, "ggd" if loss[0] else "mmse"), ls, B, 6, 11 + i, loss)
        for i, (ls, B, loss) in enumerate((ls, B, loss) for ls in ([40, 64, 19], [40, 64, 257]) for B in (32, 160)
                                          for loss in (MMSE, GGD))]
RUNS += [case("relu", [40, 64, 64, 19], 32, 6, 21, GGD, activation="relu"),
         case("no-weightcost", [40, 64, 19], 32, 6, 22, MMSE, wc=0.0),
         case("other-betas", [40, 64, 19], 32, 6, 23, GGD, beta1=0.5, beta2=0.75, eps=1e-3)]
# 2. shapes at which the launch can go wrong
#    - K and N off every multiple of 32 and of 4: pads in both directions
#    - B = 128: Bp is a multiple of 64, the gradient comes from the unfused instance of the persistent k_dwp
#    - a layer of 1024 x 2112 = 2,162,688 padded floats: more than the 2048 x 256 float4 = 2,097,152 floats one pass of
#      k_adam_apply's capped grid covers, so the grid-stride loop takes a second trip
#    - 9 weight layers (MLGGD_MAXLAYER = 10): 18 jobs, the job table's far end
BIG_LS = [1024, 2112, 19]
SHAPES = [case("odd", [41, 70, 19], 32, 3, 31, GGD),
          case("dwp", [41, 70, 19], 128, 3, 32, GGD),
          case("two-trips", BIG_LS, 32, 2, 33, MMSE),
          case("nine-layers", [24, 40, 33, 40, 36, 40, 34, 40, 38, 19], 32, 3, 34, MMSE)]
ONE_PASS_FLOATS = 2048 * 256 * 4
# 3. the state: 3 + 3 steps against 6
STATE = case("state", [41, 70, 19], 32, 6, 41, GGD)
ALL = RUNS + SHAPES + [STATE]


def net(c):
    return b6.make_net(c.ls, c.seed)


def data(c, steps=None):
    return tc.data(c.ls, (c.steps if steps is None else steps) * c.B, c.seed)
