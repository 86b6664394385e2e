"""Cost of a shape factor per output bin (BPGpu.set_shapefactors) at 2827-2048^3-257, B = 128, MLflag 1: the loss
class (mlggd_profile_select("loss"): k_loss_ml / k_loss_ml_bins bracketed by two events) and the whole step
(last_train_ms over a resident chunk of 128 minibatches) in three configurations of ONE engine,
  * scalar  -- no vector set, shapefactor 1.0 (what the reference ships): k_loss_ml, no libm call in the chain;
  * uniform -- a vector of 1.0 in every bin: k_loss_ml_bins on the same arithmetic, the cost of reading beta per bin;
  * mixed   -- the grid 0.5:0.1:2.5 cycled over the 257 bins: pow_det in 19 of every 21 columns.
Writes profiles/shapefactors_bench.json and prints it as one JSON line.

    python tools/shapefactors_bench.py [--reps 15] [--gpu 0] [--out FILE] [--scalar-only] [--pkg-root DIR]

The arms alternate inside every repetition (weights reset at the start of each window, so every window trains the same
steps), every arm is warmed up first, and the MEDIAN over the repetitions is reported with the fastest and slowest
beside it.  The loss figure includes the event bracket (profile_overhead, reported).  --scalar-only runs the first arm
alone and uses no entry point of this feature, so the same file also times a build from before it (--pkg-root: the
directory that holds that build's package) -- run both a few times in one session, alternating, and compare the scalar
arm of this build with the spread of the older one.  No figure is promised; the file records what the run gave.  Needs
a GPU: there is no CPU path."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "speech-enhancement-based-on-a-maximum-likelihood-criterion_amd"
B, NB = 128, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shapefactors_bench.json"))
    ap.add_argument("--scalar-only", action="store_true")
    ap.add_argument("--pkg-root", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg_root))
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    ls = synth.baseline_layersizes()
    assert ls == [2827, 2048, 2048, 2048, 257], ls
    D = ls[-1]
    ws, bs = synth.make_weights(ls)
    inp, targ = synth.make_frames(NB * B, 257, 11)
    grid = np.array([np.float32(0.5 + 0.1 * i) for i in range(21)], np.float32)
    arms = {"scalar": None}
    if not a.scalar_only:
        arms["uniform"] = np.full(D, 1.0, np.float32)
        arms["mixed"] = grid[np.arange(D) % grid.size]
    eng = pkg.BPGpu(1, a.gpu, ls, B, 0.001, 0.9, 1e-5, ws, bs, 1.0, 1)
    eng.load_chunk(inp, targ)

    def window(name, profile):
        if not a.scalar_only:
            eng.set_shapefactors(arms[name])
        eng.set_weights(ws, bs)
        if profile:
            eng.profile_select("loss", 0, 4096)
        assert eng.train_resident(0, NB * B) == NB
        eng.sync()
        if profile:
            us, n = eng.profile_read()
            eng.profile_select(None)
            assert n == NB, n
            return us
        ms, steps = eng.last_train_ms()
        assert steps == NB, steps
        return 1e3 * ms / steps

    for name in arms:                                      # warm-up: code objects, LDS attributes, the beta array
        for _ in range(3):
            window(name, False)
        window(name, True)
    loss = {k: [] for k in arms}
    step = {k: [] for k in arms}
    for _ in range(a.reps):
        for name in arms:
            step[name].append(window(name, False))
            loss[name].append(window(name, True))
    overhead = eng.profile_overhead()
    finite = bool(np.isfinite(eng.returnWeights()[0][0]).all())
    eng.close()
    assert finite
    stat = lambda v: {"median": round(float(np.median(v)), 2), "min": round(float(min(v)), 2), "max": round(float(max(v)), 2)}
    res = {"workload": "ML-GGD training step, 2827-2048^3-257, B 128, %d resident minibatches per window" % NB,
           "command": "python tools/shapefactors_bench.py" + (" --scalar-only" if a.scalar_only else ""),
           "reps": a.reps, "unit": "microseconds per step", "profile_bracket_us": round(float(overhead), 2),
           "loss_class_us": {k: stat(v) for k, v in loss.items()}, "step_us": {k: stat(v) for k, v in step.items()}}
    if not a.scalar_only:
        for k in ("uniform", "mixed"):
            res["loss_%s_over_scalar" % k] = round(res["loss_class_us"][k]["median"] / res["loss_class_us"]["scalar"]["median"], 3)
            res["step_%s_over_scalar" % k] = round(res["step_us"][k]["median"] / res["step_us"]["scalar"]["median"], 4)
    line = json.dumps(res)
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
