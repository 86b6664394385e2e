"""Cost of a steady-state live push (BPGpu.live, mlggd_live_push) at the shipped shape 1799-2048^3-257, 16 kHz,
context 7: for n_sessions in {1, 64, 1024} every session receives one hop (256 samples) per push.  Writes
profiles/live_bench.json and prints it as one JSON line.

    python tools/live_bench.py [--sessions 1,64,1024] [--pushes 300] [--gpu 0] [--out FILE]

Per group size, after warm-up pushes that fill every carry and grow every buffer:
* push_median_ms / push_worst_ms: wall time of one push (it ends in a stream synchronise) over --pushes pushes, each
  of which decodes one frame per session; realtime_share = the median / the 16 ms a hop lasts: what share of real time
  a server that pushes every hop spends.
* offline_ms: one BPGpu.enhance_waves call over the same number of frames (n_sessions utterances of --pushes frames),
  best of 3 after a warm-up, in the same process -- the offline pass doing the same arithmetic without carried state --
  and offline_ms_per_push = offline_ms / pushes; ratio = push_median_ms / offline_ms_per_push.
No threshold is promised; the file records what the run gave.  Needs a GPU: there is no CPU path."""
import argparse
import importlib
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "speech-enhancement-based-on-a-maximum-likelihood-criterion_amd"
L, S = 512, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", default="1,64,1024")
    ap.add_argument("--pushes", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_bench.json"))
    a = ap.parse_args()
    pkg = importlib.import_module(PKG)
    import spec64
    import torch
    rng = np.random.default_rng(0)
    ls = [7 * 257, 2048, 2048, 2048, 257]
    ws = [(rng.normal(0, 1.0, (ls[i], ls[i + 1])) / np.sqrt(ls[i])).astype(np.float32) for i in range(4)]
    bs = [rng.normal(0, 0.1, ls[i + 1]).astype(np.float32) for i in range(4)]
    mean = rng.normal(10, 2, 257).astype(np.float32)
    inv = (1.0 / rng.uniform(2, 4, 257)).astype(np.float32)
    total = a.warmup + a.pushes
    pool = spec64.synth_speech(total * S + L + 16000 * 30, 16, seed=1)
    res = {"workload": "live push of one hop per session, 1799-2048^3-257 16 kHz context 7", "pushes": a.pushes,
           "warmup_pushes": a.warmup, "hop_ms": 16.0, "bunchsize": 512,
           "command": "python tools/live_bench.py " + " ".join(sys.argv[1:]),
           "box": {"gpu": torch.cuda.get_device_name(a.gpu), "host": platform.machine(), "torch": torch.__version__},
           "groups": []}
    eng = pkg.BPGpu(1, a.gpu, ls, 512, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    for n in [int(x) for x in a.sessions.split(",")]:
        starts = rng.integers(0, 16000 * 30, n)
        live = eng.live(mean, inv, n)
        first = [np.ascontiguousarray(pool[s:s + L - S]) for s in starts]   # so that every later hop completes a frame
        live.push(first)
        times = []
        emitted = 0
        for i in range(total):
            blocks = [pool[s + L - S + i * S:s + L + i * S] for s in starts]
            t0 = time.perf_counter()
            out = live.push(blocks)
            dt = time.perf_counter() - t0
            if i >= a.warmup:
                times.append(dt)
                emitted += sum(o.size for o in out)
        live.close()
        assert emitted == a.pushes * n * S                                  # each timed push emitted one hop per session
        waves = [np.ascontiguousarray(pool[s:s + a.pushes * S + L - S]) for s in starts]
        eng.enhance_waves(waves, mean, inv)
        off = []
        for _ in range(3):
            t0 = time.perf_counter()
            eng.enhance_waves(waves, mean, inv)
            off.append(time.perf_counter() - t0)
        med, worst, offline = float(np.median(times)), float(np.max(times)), min(off)
        res["groups"].append({"n_sessions": n, "frames_per_push": n, "push_median_ms": round(med * 1e3, 4),
                              "push_worst_ms": round(worst * 1e3, 4), "realtime_share": round(med * 1e3 / 16.0, 5),
                              "offline_frames": n * a.pushes, "offline_ms": round(offline * 1e3, 3),
                              "offline_ms_per_push": round(offline * 1e3 / a.pushes, 4),
                              "ratio": round(med * a.pushes / offline, 3)})
    eng.close()
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
