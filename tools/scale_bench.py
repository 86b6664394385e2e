"""Cost of the learned scale (BPGpu.set_scale_mode) at 2827-2048^3-257, B = 128, MLflag 1, beta = 1: the loss class
(mlggd_profile_select("loss"): k_loss_ml / k_loss_ml_learn bracketed by two events) and the whole resident step
(last_train_ms over a resident chunk of 128 minibatches) in two configurations of ONE engine,
  * alternating -- the default (what the reference ships): k_loss_ml, alpha re-solved from every minibatch;
  * learned     -- k_loss_ml_learn at the default rates: the 8 threads per workgroup that run the serial column sum
                   also read (alpha, v), apply the rule (a dozen fp32 operations and one exp_det) and write the other copy.
Writes profiles/scale_bench.json and prints it as one JSON line.

    python tools/scale_bench.py [--reps 7] [--gpu 0] [--out FILE] [--parent-root DIR] [--bench-steps 400]

The arms alternate inside every repetition (weights and the scale's state reset at the start of each window, so every
window trains the same steps), every arm is warmed up first, and the MEDIAN over the repetitions is reported with the
fastest and slowest beside it.  The loss figure includes the event bracket (profile_overhead, reported).

--parent-root DIR names a built checkout of the parent commit: `bench.py --gpus 1` (a plain engine: it never switches
the mode on) is then run in DIR and here, alternating, parent first, --bench-rounds times each, every run a fresh
process, and the headline of every run goes into the json ("bench_headline") with each build's median and range.
Without it the json holds the command to run and says that the figure is unmeasured.  No figure is promised; the file
records what the run gave.  Needs a GPU: there is no CPU path."""
import argparse
import importlib
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "speech-enhancement-based-on-a-maximum-likelihood-criterion_amd"
B, NB = 128, 128
ARMS = ("alternating", "learned")


def bench_headline(root, steps, warmup):
    """the JSON result line of one `bench.py --gpus 1` run in `root`, a fresh process"""
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    res = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=900)
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    if res.returncode != 0 or not lines:
        return {"error": "exit %d" % res.returncode, "stderr_tail": res.stderr[-400:]}
    out = json.loads(lines[-1])
    return {k: out[k] for k in ("value", "ms_per_step", "unit", "metric") if k in out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_bench.json"))
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--bench-steps", type=int, default=400)
    ap.add_argument("--bench-warmup", type=int, default=40)
    ap.add_argument("--bench-rounds", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    ls = synth.baseline_layersizes()
    assert ls == [2827, 2048, 2048, 2048, 257], ls
    D = ls[-1]
    ws, bs = synth.make_weights(ls)
    inp, targ = synth.make_frames(NB * B, 257, 11)
    eng = pkg.BPGpu(1, a.gpu, ls, B, 0.001, 0.9, 1e-5, ws, bs, 1.0, 1)
    eng.load_chunk(inp, targ)

    def window(name, profile):
        eng.set_scale_mode("alternating")
        eng.set_weights(ws, bs)
        if name == "learned":
            eng.set_scalefactor(np.zeros(D, np.float32))   # entering the mode takes alpha from here: every bin seeds
            eng.set_scale_mode("learned")
        if profile:
            eng.profile_select("loss", 0, 4096)
        assert eng.train_resident(0, NB * B) == NB
        eng.sync()
        if name == "learned":
            assert eng.scale_mode().steps == NB
        if profile:
            us, n = eng.profile_read()
            eng.profile_select(None)
            assert n == NB, n
            return us
        ms, steps = eng.last_train_ms()
        assert steps == NB, steps
        return 1e3 * ms / steps

    for name in ARMS:                                      # warm-up: code objects, LDS attributes, the state's buffer
        for _ in range(3):
            window(name, False)
        window(name, True)
    loss = {k: [] for k in ARMS}
    step = {k: [] for k in ARMS}
    for _ in range(a.reps):
        for name in ARMS:
            step[name].append(window(name, False))
            loss[name].append(window(name, True))
    overhead = eng.profile_overhead()
    alpha, vel = eng.scale_state()
    finite = bool(np.isfinite(eng.returnWeights()[0][0]).all() and np.isfinite(alpha).all() and (alpha > 0).all() and vel.any())
    eng.close()
    assert finite
    stat = lambda v: {"median": round(float(np.median(v)), 2), "min": round(float(min(v)), 2), "max": round(float(max(v)), 2)}
    res = {"workload": "ML-GGD training step, 2827-2048^3-257, B 128, beta 1, %d resident minibatches per window" % NB,
           "command": "python tools/scale_bench.py", "reps": a.reps, "unit": "microseconds per step",
           "profile_bracket_us": round(float(overhead), 2),
           "loss_class_us": {k: stat(v) for k, v in loss.items()}, "step_us": {k: stat(v) for k, v in step.items()}}
    res["loss_learned_over_alternating"] = round(res["loss_class_us"]["learned"]["median"] / res["loss_class_us"]["alternating"]["median"], 3)
    res["step_learned_over_alternating"] = round(res["step_us"]["learned"]["median"] / res["step_us"]["alternating"]["median"], 4)
    bench_cmd = "python bench.py --gpus 1 --steps %d --warmup %d" % (a.bench_steps, a.bench_warmup)
    if a.parent_root:
        runs = []
        for r in range(a.bench_rounds):                    # one session, alternating, parent first
            for which, root in (("parent", os.path.abspath(a.parent_root)), ("this", ROOT)):
                runs.append({"build": which, "round": r, "result": bench_headline(root, a.bench_steps, a.bench_warmup)})
        res["bench_headline"] = {"command": bench_cmd, "runs": runs}
        for which in ("parent", "this"):
            vals = [r["result"]["value"] for r in runs if r["build"] == which and "value" in r["result"]]
            if vals:
                res["bench_headline"][which] = {"median": float(np.median(vals)), "min": min(vals), "max": max(vals), "runs": len(vals)}
    else:
        res["bench_headline"] = {"command": bench_cmd, "runs": None,
                                 "note": "unmeasured: run with --parent-root DIR, a built checkout of the parent commit"}
    line = json.dumps(res)
    if a.out != "-":
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
