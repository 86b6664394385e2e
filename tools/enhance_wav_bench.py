"""Throughput of BPGpu.enhance_wave (the whole decode.m chain on the device) at the shipped shape 1799-2048^3-257 on
synthetic speech-like audio, in audio-seconds per second and frames per second.  One JSON line on stdout.

    python tools/enhance_wav_bench.py [--minutes 60] [--reps 2] [--gpu 0]

A list of short utterances, the batched call against the loop of single calls in the same process:

    python tools/enhance_wav_bench.py --utterances 1000 --seconds 3 [--reps 3] [--batch-s 300]

times BPGpu.enhance_waves over batches of --batch-s seconds of audio (the enhance_wav tool's default) and the loop of
enhance_wave calls over the same synthetic utterances, each the best of --reps repetitions after the same warm-up.
MLGGD_WAVES_LOOKUP=table in the environment selects the per-frame utterance table instead of the binary search.

The share of the spectral kernels in device time comes from a kernel trace of a run of this tool:

    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/enhance_wav_bench.py --minutes 10 --reps 1
    python tools/enhance_wav_bench.py --kernel-stats OUT/.../run_kernel_stats.csv
"""
import argparse
import csv
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
SPECTRAL = ("k_lps_analysis", "k_lps_stream", "k_lps_synthesis", "k_ola", "k_lps_analysis_seg", "k_lps_stream_seg",
            "k_ola_seg")


def kernel_shares(path):
    """{kernel: share of the total device time} from a rocprofv3 --stats kernel CSV, spectral kernels by name."""
    rows = list(csv.DictReader(open(path)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {k: 0.0 for k in SPECTRAL}
    for r in rows:
        for k in SPECTRAL:
            if r["Name"].startswith(k + "(") or r["Name"] == k:
                out[k] += float(r["TotalDurationNs"]) / tot
    out["spectral_total"] = sum(out[k] for k in SPECTRAL)
    out["device_ms"] = tot / 1e6
    return out


def utterance_list(pkg, spec64, a, ls, ws, bs, mean, inv):
    """N utterances of 0.67 .. 1.33 x --seconds, cut from one synthetic wave; batched call vs the loop of single calls"""
    rng = np.random.default_rng(2)
    lengths = rng.integers(int(a.seconds * 16000 * 2 / 3), int(a.seconds * 16000 * 4 / 3) + 1, a.utterances)
    pool = spec64.synth_speech(int(lengths.max()) + 16000 * 60, 16, seed=1)
    starts = rng.integers(0, 16000 * 60, a.utterances)
    waves = [np.ascontiguousarray(pool[s:s + n]) for s, n in zip(starts, lengths)]
    frames = int(pkg.enhance_waves_layout(lengths, 16)[1][-1])
    batches, cur, cur_n = [], [], 0
    for w in waves:
        cur.append(w)
        cur_n += w.size
        if cur_n >= a.batch_s * 16000:
            batches.append(cur)
            cur, cur_n = [], 0
    if cur:
        batches.append(cur)
    eng = pkg.BPGpu(1, a.gpu, ls, 512, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)

    def batched():
        return [o for b in batches for o in eng.enhance_waves(b, mean, inv)]

    def loop():
        return [eng.enhance_wave(w, mean, inv) for w in waves]

    res = {"workload": "enhance_waves 1799-2048^3-257 16 kHz", "utterances": a.utterances, "mean_seconds": a.seconds,
           "audio_s": round(float(lengths.sum()) / 16000.0, 1), "frames": frames, "batch_s": a.batch_s,
           "calls": len(batches), "reps": a.reps, "lookup": os.environ.get("MLGGD_WAVES_LOOKUP", "search")}
    outs = {}
    for name, fn in (("batched", batched), ("loop", loop)):
        if a.only not in ("both", name):
            continue
        fn()                                                  # warm-up: tables, buffers, code objects
        best = None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            outs[name] = fn()
            dt = time.perf_counter() - t0
            best = dt if best is None else min(best, dt)
        res[name + "_wall_s"] = round(best, 4)
        res[name + "_frames_per_s"] = round(frames / best, 1)
    if len(outs) == 2:
        res["bit_identical"] = all(np.array_equal(x, y) for x, y in zip(outs["batched"], outs["loop"]))
        res["loop_over_batched"] = round(res["loop_wall_s"] / res["batched_wall_s"], 2)
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=None, help="default 2; 3 with --utterances")
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--utterances", type=int, default=0, help="time a list of this many utterances")
    ap.add_argument("--seconds", type=float, default=3.0, help="mean utterance length of the list")
    ap.add_argument("--batch-s", type=float, default=300.0, help="seconds of audio per enhance_waves call")
    ap.add_argument("--only", choices=("both", "batched", "loop"), default="both", help="for a kernel trace of one form")
    a = ap.parse_args()
    if a.reps is None:
        a.reps = 3 if a.utterances else 2
    if a.kernel_stats:
        print(json.dumps({k: round(v, 5) for k, v in kernel_shares(a.kernel_stats).items()}))
        return
    pkg = importlib.import_module("speech-enhancement-based-on-a-maximum-likelihood-criterion_amd")
    import spec64
    rng = np.random.default_rng(0)
    ls = [7 * 257, 2048, 2048, 2048, 257]
    ws = [(rng.normal(0, 1.0, (ls[i], ls[i + 1])) / np.sqrt(ls[i])).astype(np.float32) for i in range(4)]
    bs = [rng.normal(0, 0.1, ls[i + 1]).astype(np.float32) for i in range(4)]
    mean = rng.normal(10, 2, 257).astype(np.float32)
    inv = (1.0 / rng.uniform(2, 4, 257)).astype(np.float32)
    n = int(a.minutes * 60 * 16000) if not a.utterances else 16000 * 10
    noisy = spec64.synth_speech(n, 16, seed=1)
    if a.utterances:
        print(json.dumps(utterance_list(pkg, spec64, a, ls, ws, bs, mean, inv)))
        return
    eng = pkg.BPGpu(1, a.gpu, ls, 512, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    eng.enhance_wave(noisy[:16000 * 10], mean, inv)          # warm-up: tables, buffers, code objects
    best = None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = eng.enhance_wave(noisy, mean, inv)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    F = (n - 256) // 256
    eng.close()
    print(json.dumps({"workload": "enhance_wave 1799-2048^3-257 16 kHz", "audio_s": n / 16000.0, "frames": F,
                      "wall_s": round(best, 4), "audio_s_per_s": round(n / 16000.0 / best, 1),
                      "frames_per_s": round(F / best, 1), "out_samples": int(out.size)}))


if __name__ == "__main__":
    main()
