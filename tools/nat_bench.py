"""What the separate staging launch of a noise-aware (NAT) engine costs: the device-resident 128-frame training step at
3084-2048^3-257 (context 11 plus the noise row, csrc/nat_rule.h), MMSE,
  (nat)      on a NAT engine through load_frames_nat: every step stages its minibatch with its own k_transpose_in_nat
             launch in front of the forward pass;
  (expanded) on an engine of the same layer sizes fed rows [window | noise row] expanded on the host: the next
             minibatch is staged inside the loss kernel's launch, as on every engine before.
Both train the same rows (the weights after one pass are compared bit for bit before anything is timed).

    python tools/nat_bench.py [--steps 400] [--warmup 40] [--ramp 512] [--reps 7] [--gpu 0] [--out FILE]
                              [--bench-parent FILE ...] [--bench-this FILE ...]

One process, two engines, each with its resident chunk of 64 bunches; after an untimed clock ramp and warm-up as
bench.py's headline has them, --reps (>= 5) pairs of timed windows of --steps steps ALTERNATE between the two arms, each
window a host clock around train_resident calls that end in a stream synchronise.  Reported per arm: the median step
time and the fastest and slowest window; `spread_ms` is the larger of the two arms' (slowest - fastest) and
`staging_launch_cost_ms` the difference of the medians.  It is recorded, not gated.

bench.py's headline concerns an engine without NAT: --bench-parent / --bench-this name files that each hold the JSON
line of one `python bench.py --gpus 1` run on the parent commit's build and on this one, taken alternately in the same
session; their headlines are recorded in the order given.  Writes profiles/nat_bench.json and prints it as one JSON
line.  No figure is promised; the file records what the run gave.  Needs a GPU: there is no CPU path."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "speech-enhancement-based-on-a-maximum-likelihood-criterion_amd"
B, D, CTX, T, NB = 128, 257, 11, 6, 64


def headline(path):
    for line in reversed(open(path).read().splitlines()):
        if line.startswith("{"):
            r = json.loads(line)
            return {k: r[k] for k in ("value", "ms_per_step", "unit", "metric") if k in r}
    return None


def stats(w):
    w = sorted(w)
    med = w[len(w) // 2] if len(w) % 2 else 0.5 * (w[len(w) // 2 - 1] + w[len(w) // 2])
    return {"step_ms_median": round(med, 5), "step_ms_min": round(w[0], 5), "step_ms_max": round(w[-1], 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--ramp", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nat_bench.json"))
    ap.add_argument("--bench-parent", nargs="*", default=[], help="files with the JSON line of `python bench.py` on the parent commit")
    ap.add_argument("--bench-this", nargs="*", default=[], help="files with the JSON line of `python bench.py` on this commit")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("--reps must be at least 5")
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    ls = [(CTX + 1) * D, 2048, 2048, 2048, D]
    ws, bs = synth.make_weights(ls)
    rng = np.random.default_rng(synth.DEFAULT_SEED + 1)
    # 64 utterances of B + CTX - 1 frames: B windows each, so the chunk holds 64 bunches
    F = B + CTX - 1
    feat = rng.standard_normal((NB * F, D), dtype=np.float32)
    targ = rng.standard_normal((NB * F, D), dtype=np.float32)
    frame_off = (np.arange(NB + 1) * F).astype(np.int32)
    table = np.concatenate([frame_off[u] + np.arange(B, dtype=np.int32) for u in range(NB)])
    first = table[rng.permutation(table.size)].astype(np.int32)
    nat = pkg.nat_estimate(feat, frame_off, T)
    nat_row = pkg.nat_rows(frame_off, first)
    toff = CTX // 2
    idx = first[:, None] + np.arange(CTX)[None, :]
    rows = np.concatenate([feat[idx].reshape(first.size, CTX * D), nat[nat_row]], axis=1)
    trows = np.ascontiguousarray(targ[first + toff])

    def engine(nat_frames):
        # a small step size: thousands of steps leave the net finite; the kernels' work does not depend on it
        return pkg.BPGpu(synth.DEFAULT_SEED, a.gpu, ls, B, 0.001, 0.9, 1e-5, ws, bs, 2.0, 0, nat_frames=nat_frames)

    def load(eng, arm):
        if arm == "nat":
            eng.load_frames_nat(feat, targ, first, CTX, toff, nat, nat_row)
        else:
            eng.load_chunk(rows, trows)

    # the arms train the same thing: every bit of every weight after one pass on fresh engines
    states = []
    for arm in ("nat", "expanded"):
        eng = engine(T if arm == "nat" else 0)
        load(eng, arm)
        assert eng.train_resident(0, NB * B) == NB
        eng.sync()
        states.append(eng.returnWeights())
        eng.close()
    equal = all(x.tobytes() == y.tobytes() for x, y in zip(states[0][0] + states[0][1], states[1][0] + states[1][1]))
    assert equal, "the NAT frames path and the expanded rows left different weights"

    engs = {"nat": engine(T), "expanded": engine(0)}
    for arm, eng in engs.items():
        load(eng, arm)

    def run_steps(eng, k):
        done = 0
        while done < k:
            m = min(k - done, NB)
            assert eng.train_resident(0, m * B) == m
            done += m

    for eng in engs.values():
        run_steps(eng, a.ramp)
        eng.sync()
        run_steps(eng, a.warmup)
        eng.sync()
    wins = {k: [] for k in engs}
    for _ in range(a.reps):
        for arm, eng in engs.items():
            t0 = time.perf_counter()
            run_steps(eng, a.steps)
            eng.sync()
            wins[arm].append((time.perf_counter() - t0) / a.steps * 1e3)
    for eng in engs.values():
        eng.close()
    res = {"workload": "device-resident step, 3084-2048^3-257 (context 11 + noise row), B 128, MMSE",
           "steps_per_window": a.steps, "reps": a.reps, "command": "python tools/nat_bench.py",
           "weights_equal_nat_expanded": bool(equal),
           "nat_frames_path": stats(wins["nat"]), "expanded_rows": stats(wins["expanded"])}
    res["spread_ms"] = round(max(v["step_ms_max"] - v["step_ms_min"] for v in (res["nat_frames_path"], res["expanded_rows"])), 5)
    res["staging_launch_cost_ms"] = round(res["nat_frames_path"]["step_ms_median"] - res["expanded_rows"]["step_ms_median"], 5)
    res["bench_command"] = "python bench.py --gpus 1 --steps 400 --warmup 40"
    res["bench_py_headline_parent_commit"] = [headline(p) for p in a.bench_parent]
    res["bench_py_headline_this_commit"] = [headline(p) for p in a.bench_this]
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
