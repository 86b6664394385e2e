"""The device-resident training step at 2827-2048^3-257, B = 128, MMSE, for activation=sigmoid and activation=relu:
does the rectifier's epilogue -- a comparison and a select where the sigmoid has an exponential and a division -- cost
anything, and did adding the switch cost the sigmoid path anything?

    python tools/relu_bench.py [--steps 400] [--warmup 40] [--ramp 512] [--reps 7] [--gpu 0] [--out FILE]
                               [--bench-parent FILE] [--bench-this FILE]

Each activation runs in a process of its own (a fresh child of this one): engine, resident chunk of 64 bunches, an
untimed clock ramp and warm-up as bench.py's headline has them, then --reps (>= 5) timed windows of --steps steps, each
a host clock around train_resident calls that end in a stream synchronise.  Reported per activation: the median step
time and the fastest and slowest window; `spread_ms` is the larger of the two activations' (slowest - fastest).

Condition on the new path: relu median <= sigmoid median + spread.  Condition on the old path: the sigmoid step of this
commit is not slower than the parent commit's by more than the spread -- that needs the parent's code, so it is measured
with `python bench.py --gpus 1` on both commits, same machine, same session; --bench-parent / --bench-this name files
holding the two JSON result lines, whose headlines (ms_per_step, value) are recorded beside the step times.  Writes
profiles/relu_bench.json and prints it as one JSON line.  No figure is promised; the file records what the run gave.
Needs a GPU: there is no CPU path."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "speech-enhancement-based-on-a-maximum-likelihood-criterion_amd"
B = 128


def child(a):
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    ls = synth.baseline_layersizes(hidden=2048, nhid=3)
    ws, bs = synth.make_weights(ls)
    nb = 64
    inp, targ = synth.make_frames(nb * B, 257, 11, seed=synth.DEFAULT_SEED + 1)
    # a small step size: 1,000 steps leave both nets finite; the kernels' work does not depend on it
    eng = pkg.BPGpu(synth.DEFAULT_SEED, a.gpu, ls, B, 0.001, 0.9, 1e-5, ws, bs, 2.0, 0, activation=a.child)
    assert eng.activation == a.child
    eng.load_chunk(inp, targ)

    def run_steps(k):
        done = 0
        while done < k:
            m = min(k - done, nb)
            assert eng.train_resident(0, m * B) == m
            done += m

    run_steps(a.ramp)
    eng.sync()
    run_steps(a.warmup)
    eng.sync()
    wins = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        run_steps(a.steps)
        eng.sync()
        wins.append((time.perf_counter() - t0) / a.steps * 1e3)
    eng.close()
    print(json.dumps({"activation": a.child, "window_ms_per_step": wins}))


def headline(path):
    if not path:
        return None
    for line in reversed(open(path).read().splitlines()):
        if line.startswith("{"):
            r = json.loads(line)
            return {k: r[k] for k in ("value", "ms_per_step", "unit", "metric") if k in r}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--ramp", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relu_bench.json"))
    ap.add_argument("--bench-parent", default=None, help="file with the JSON line of `python bench.py` on the parent commit")
    ap.add_argument("--bench-this", default=None, help="file with the JSON line of `python bench.py` on this commit")
    ap.add_argument("--child", choices=["sigmoid", "relu"], default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    if a.child:
        return child(a)
    res = {"workload": "device-resident step, 2827-2048^3-257, B 128, MMSE", "steps_per_window": a.steps, "reps": a.reps,
           "command": "python tools/relu_bench.py"}
    arms = {}
    for act in ("sigmoid", "relu"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", act, "--steps", str(a.steps), "--warmup",
                            str(a.warmup), "--ramp", str(a.ramp), "--reps", str(a.reps), "--gpu", str(a.gpu)],
                           capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            return 1
        w = sorted(json.loads(r.stdout.strip().splitlines()[-1])["window_ms_per_step"])
        med = w[len(w) // 2] if len(w) % 2 else 0.5 * (w[len(w) // 2 - 1] + w[len(w) // 2])
        arms[act] = {"step_ms_median": round(med, 5), "step_ms_min": round(w[0], 5), "step_ms_max": round(w[-1], 5)}
    res.update(arms)
    spread = max(v["step_ms_max"] - v["step_ms_min"] for v in arms.values())
    res["spread_ms"] = round(spread, 5)
    res["relu_not_slower_than_sigmoid_plus_spread"] = arms["relu"]["step_ms_median"] <= arms["sigmoid"]["step_ms_median"] + spread
    hp, ht = headline(a.bench_parent), headline(a.bench_this)
    res["bench_py_headline_parent_commit"] = hp
    res["bench_py_headline_this_commit"] = ht
    if hp and ht and "ms_per_step" in hp and "ms_per_step" in ht:
        res["sigmoid_not_slower_than_parent_plus_spread"] = ht["ms_per_step"] <= hp["ms_per_step"] + spread
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
