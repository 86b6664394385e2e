"""Throughput of BPGpu.enhance_wave (the whole decode.m chain on the device) at the shipped shape 1799-2048^3-257 on
synthetic speech-like audio, in audio-seconds per second and frames per second.  One JSON line on stdout.

    python tools/enhance_wav_bench.py [--minutes 60] [--reps 2] [--gpu 0]

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
SPECTRAL = ("k_lps_analysis", "k_lps_stream", "k_lps_synthesis", "k_ola")


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--kernel-stats", default=None)
    a = ap.parse_args()
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
    n = int(a.minutes * 60 * 16000)
    noisy = spec64.synth_speech(n, 16, seed=1)
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
