"""Cost of STOI in a scored decoding pass at the shipped shape 1799-2048^3-257, 16 kHz: BPGpu.enhance_waves with cleans=
and stoi=True (mlggd_enhance_waves_scored_stoi) against the same call with stoi=False (mlggd_enhance_waves_scored), in
one process, on the synthetic list of tools/score_waves_bench.py.  Writes profiles/stoi_bench.json and prints it as one
JSON line.

    python tools/stoi_bench.py [--utterances 200] [--seconds 3] [--reps 3] [--gpu 0] [--out FILE]

Both forms end in a stream synchronise; each is warmed up once, then they alternate inside every repetition, best of
--reps.  stoi_share = (with - without) / with: the part of the scored pass that STOI takes (five kernels and 2 n words
back; the clean wave is already on the device).  No figure is promised; the file records what the run gave.  Needs a
GPU: there is no CPU path."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PKG = "speech-enhancement-based-on-a-maximum-likelihood-criterion_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=3.0, help="mean utterance length")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stoi_bench.json"))
    a = ap.parse_args()
    pkg = importlib.import_module(PKG)
    import spec64
    from score_waves_bench import best_of
    rng = np.random.default_rng(0)                   # the list of score_waves_bench.py: the same draws in the same order
    ls = [7 * 257, 2048, 2048, 2048, 257]
    ws = [(rng.normal(0, 1.0, (ls[i], ls[i + 1])) / np.sqrt(ls[i])).astype(np.float32) for i in range(4)]
    bs = [rng.normal(0, 0.1, ls[i + 1]).astype(np.float32) for i in range(4)]
    mean = rng.normal(10, 2, 257).astype(np.float32)
    inv = (1.0 / rng.uniform(2, 4, 257)).astype(np.float32)
    lengths = rng.integers(int(a.seconds * 16000 * 2 / 3), int(a.seconds * 16000 * 4 / 3) + 1, a.utterances)
    pool = spec64.synth_speech(int(lengths.max()) + 16000 * 60, 16, seed=1)
    starts = rng.integers(0, 16000 * 60, a.utterances)
    cleans = [np.ascontiguousarray(pool[s:s + n]) for s, n in zip(starts, lengths)]
    noisys = [np.clip(c + rng.normal(0, 800.0, c.size), -32768, 32767).astype(np.int16) for c in cleans]
    res = {"workload": "scored list with STOI, enhance_waves 1799-2048^3-257 16 kHz", "utterances": a.utterances,
           "mean_seconds": a.seconds, "audio_s": round(float(lengths.sum()) / 16000.0, 1),
           "frames": int(pkg.enhance_waves_layout(lengths, 16)[1][-1]),
           "stoi_frames": int(sum(pkg.stoi_layout(int(n), 16)[1] for n in lengths)), "reps": a.reps}
    eng = pkg.BPGpu(1, a.gpu, ls, 512, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    got = {}
    t = best_of({"pass_scored_wall_s": lambda: eng.enhance_waves(noisys, mean, inv, cleans=cleans),
                 "pass_scored_stoi_wall_s": lambda: got.update(r=eng.enhance_waves(noisys, mean, inv, cleans=cleans,
                                                                                    stoi=True))}, a.reps)
    eng.close()
    res.update({k: round(v, 4) for k, v in t.items()})
    res["pass_stoi_device_s"] = round(t["pass_scored_stoi_wall_s"] - t["pass_scored_wall_s"], 4)
    res["stoi_share"] = round((t["pass_scored_stoi_wall_s"] - t["pass_scored_wall_s"]) / t["pass_scored_stoi_wall_s"], 4)
    stoi = got["r"][3]
    res["utterances_with_a_value"] = int(np.isfinite(stoi).sum())
    res["mean_stoi"] = round(float(np.nanmean(stoi)), 4)
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
