"""Cost of the Adam optimizer (BPGpu.set_optimizer) at 2827-2048^3-257, B = 128, MLflag 1, beta = 1: the whole resident
step (last_train_ms over a resident chunk of 128 minibatches), the "update" kernel class (mlggd_profile_select("update"):
the k_adam_apply launch bracketed by two events; an SGD step has no launch of that class on one device, its update is
k_dwp's epilogue) and the "dw" class, in two configurations of ONE engine,
  * sgd  -- the default (what the reference ships): one fused k_dwp launch forms all gradients and applies the rule;
  * adam -- one unfused k_dwp launch per layer writes G_l / gb_l, then ONE k_adam_apply launch reads G, W, m, v and
            writes W, m, v of every layer: seven arrays of 58.8 MB at this shape.
Writes profiles/adam_bench.json and prints it as one JSON line.

    python tools/adam_bench.py [--reps 7] [--gpu 0] [--out FILE] [--parent-root DIR] [--bench-steps 400]

The arms alternate inside every repetition (weights reset and the mode entered anew at the start of each window, so every
window trains the same steps), every arm is warmed up first, and the MEDIAN over the repetitions is reported with the
fastest and slowest beside it.  The update figure includes the event bracket (profile_overhead, reported); the launch's
rate is its bytes over (that figure minus the bracket), to be read beside the bare-traffic figures of
profiles/r01_update_stream_microbench.txt.  The expectation written into the json is an expectation, not a threshold.

--parent-root DIR names a built checkout of the parent commit: `bench.py --gpus 1` (a plain engine: it never enters the
mode) is then run in DIR and here, alternating, parent first, --bench-rounds times each, every run a fresh process, and
the headline of every run goes into the json ("bench_headline") with each build's median and range.  Without it the json
holds the command to run and says that the figure is unmeasured.  Needs a GPU: there is no CPU path."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from scale_bench import bench_headline  # noqa: E402  (one definition of "a bench.py run")

PKG = "speech-enhancement-based-on-a-maximum-likelihood-criterion_amd"
B, NB = 128, 128
ARMS = ("sgd", "adam")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_bench.json"))
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
    ws, bs = synth.make_weights(ls)
    inp, targ = synth.make_frames(NB * B, 257, 11)
    eng = pkg.BPGpu(1, a.gpu, ls, B, 0.001, 0.9, 1e-5, ws, bs, 1.0, 1)
    eng.load_chunk(inp, targ)
    pad = lambda n: -(-n // 32) * 32
    floats = sum(pad(ls[l]) * pad(ls[l + 1]) + pad(ls[l + 1]) for l in range(len(ls) - 1))   # what one array of a job set holds
    apply_bytes = 7 * 4 * floats

    def window(name, profile):
        eng.set_optimizer("sgd")
        eng.set_weights(ws, bs)
        if name == "adam":
            eng.set_optimizer("adam")                      # zero moments, step 0
        if profile:
            eng.profile_select(profile, 0, 4096)
        assert eng.train_resident(0, NB * B) == NB
        eng.sync()
        if name == "adam":
            assert eng.optimizer().steps == NB
        if profile:
            us, n = eng.profile_read()
            eng.profile_select(None)
            return us, n
        ms, steps = eng.last_train_ms()
        assert steps == NB, steps
        return 1e3 * ms / steps

    for name in ARMS:                                      # warm-up: code objects, LDS attributes, the mode's buffers
        for _ in range(3):
            window(name, False)
        window(name, "dw")
    step = {k: [] for k in ARMS}
    dw = {k: [] for k in ARMS}
    dw_launches = {}
    update = []
    for _ in range(a.reps):
        for name in ARMS:
            step[name].append(window(name, False))
            us, n = window(name, "dw")
            dw[name].append(us * n / NB)                   # microseconds of the class per step
            dw_launches[name] = n / NB
        us, n = window("adam", "update")
        assert n == NB, n
        update.append(us)
    us, n = window("sgd", "update")
    assert n == 0, n                                       # an SGD step on one device has no launch of the class
    overhead = eng.profile_overhead()
    window("adam", False)
    st = eng.optimizer_state()
    finite = bool(all(np.isfinite(w).all() for w in eng.returnWeights()[0]) and all(np.isfinite(v).all() and v.any() for v in st.v_w))
    eng.close()
    assert finite
    stat = lambda v: {"median": round(float(np.median(v)), 2), "min": round(float(min(v)), 2), "max": round(float(max(v)), 2)}
    res = {"workload": "ML-GGD training step, 2827-2048^3-257, B 128, beta 1, %d resident minibatches per window" % NB,
           "command": "python tools/adam_bench.py", "reps": a.reps, "unit": "microseconds per step",
           "profile_bracket_us": round(float(overhead), 2),
           "step_us": {k: stat(v) for k, v in step.items()},
           "dw_class_us_per_step": {k: stat(v) for k, v in dw.items()}, "dw_launches_per_step": dw_launches,
           "update_class_us": {"sgd": "no launch of the class on one device: the update is k_dwp's epilogue", "adam": stat(update)}}
    med = res["update_class_us"]["adam"]["median"]
    bare = max(med - float(overhead), 1e-3)
    res["adam_apply"] = {"arrays": 7, "bytes": apply_bytes, "MB_per_array": round(4 * floats / 1e6, 2),
                         "us_without_bracket": round(bare, 2), "TB_per_s": round(apply_bytes / bare / 1e6, 3),
                         "beside": "profiles/r01_update_stream_microbench.txt (bare update traffic)",
                         "expectation": "about 65 us at the 6.3 TB/s a float4 copy reaches; an expectation, not a threshold"}
    res["step_adam_over_sgd"] = round(res["step_us"]["adam"]["median"] / res["step_us"]["sgd"]["median"], 3)
    res["expectation_step_ratio"] = "near 1.5 (a 127 us SGD step plus about 65 us); an expectation, not a threshold"
    res["not_measured"] = ["other shapes and bunch sizes", "beta != 1 and the beta-norm losses (the update does not see the loss)",
                           "any effect on speech: no default of the optimizer has been evaluated on speech"]
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
