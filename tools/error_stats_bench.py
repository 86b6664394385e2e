"""Cost of the error statistics of a CV chunk at the shipped shape 1799-2048^3-257, B = 128, a 7,920-sample chunk and the
default grid of 21 shapes (0.5:0.1:2.5): BPGpu.error_stats_frames (mlggd_error_stats_frames) and, beside it,
BPGpu.error_stats_signed_frames (mlggd_error_stats_signed_frames, the same grid) against
  * cv_all_frames with the device reduce (mlggd_cv_all_frames after set_cv_device_reduce): the same upload and the same
    forward pass with k_cv_reduce in the place of k_err_stats -- the comparator;
  * the path a user had before: forward_frames, the n x D outputs downloaded, the same sums in NumPy (float64).
Writes profiles/error_stats_bench.json and prints it as one JSON line.

    python tools/error_stats_bench.py [--samples 7920] [--reps 9] [--gpu 0] [--out FILE] [--pkg-root DIR]

--pkg-root DIR times another build with the same file (DIR holds its package, e.g. a built checkout of the parent
commit), for an A/B of two builds in processes of their own; its result is printed and, unless --out names a file,
not written.

Every arm is a host clock around a call that ends in a stream synchronise; each is warmed up once, then the arms
alternate inside every repetition and the MEDIAN over the repetitions is reported (with the fastest and slowest beside
it).  The device sums are compared with the NumPy ones before anything is written.  No figure is promised; the file
records what the run gave.  Needs a GPU: there is no CPU path."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "speech-enhancement-based-on-a-maximum-likelihood-criterion_amd"
DIM, CTX, TOFF, B = 257, 7, 3, 128


def numpy_sums(out, targ, betas):
    e = (out - targ).astype(np.float64)                   # the error in float32, as the device forms it
    e2 = e * e
    a = np.abs(e)
    return np.stack([e.sum(0), e2.sum(0), (e2 * e).sum(0), (e2 * e2).sum(0)] + [(a ** float(b)).sum(0) for b in betas])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7920)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pkg-root", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg_root))
    if a.out is None:  # the committed profile is this tree's: another build's figures go to it only when asked
        a.out = os.path.join(ROOT, "profiles", "error_stats_bench.json") if os.path.samefile(a.pkg_root, ROOT) else os.devnull
    pkg = importlib.import_module(PKG)
    rng = np.random.default_rng(0)
    ls = [CTX * DIM, 2048, 2048, 2048, DIM]
    ws = [(rng.normal(0, 1.0, (ls[i], ls[i + 1])) / np.sqrt(ls[i])).astype(np.float32) for i in range(4)]
    bs = [rng.normal(0, 0.1, ls[i + 1]).astype(np.float32) for i in range(4)]
    n = a.samples
    feat = rng.standard_normal((n + CTX - 1, DIM), dtype=np.float32)
    targ = (0.5 * feat + 0.5 * rng.standard_normal(feat.shape, dtype=np.float32)).astype(np.float32)
    first = np.arange(n, dtype=np.int32)                  # a CV chunk is not shuffled
    betas = np.array([np.float32(0.5 + 0.1 * i) for i in range(21)], np.float32)
    eng = pkg.BPGpu(1, a.gpu, ls, B, 0.1, 0.9, 1e-5, ws, bs, 1.2, 1)
    eng.set_scalefactor(np.ones(DIM, np.float32))
    eng.set_cv_device_reduce(True)
    got = {}
    arms = {
        "error_stats_frames_s": lambda: got.update(dev=eng.error_stats_frames(feat, targ, first, CTX, TOFF, betas)),
        "error_stats_signed_frames_s": lambda: eng.error_stats_signed_frames(feat, targ, first, CTX, TOFF, betas),
        "cv_all_frames_device_reduce_s": lambda: eng.cv_all_frames(feat, targ, first, CTX, TOFF),
        "forward_frames_plus_numpy_s": lambda: got.update(
            host=numpy_sums(eng.forward_frames(feat, first, CTX), targ[first + TOFF], betas)),
    }
    for f in arms.values():
        f()
    rel = float(np.max(np.abs(got["dev"] - got["host"]) / np.maximum(np.abs(got["host"]), 1.0)))
    assert rel < 1e-6, rel                                # the arms looked at the same errors (the powers differ: fp32 terms)
    times = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, f in arms.items():
            t0 = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t0)
    eng.close()
    res = {"workload": "error statistics of a CV chunk, 1799-2048^3-257, B 128, frame-stream chunk", "samples": n,
           "betas": "0.5:0.1:2.5", "n_betas": int(betas.size), "reps": a.reps,
           "command": "python tools/error_stats_bench.py", "package_of": os.path.relpath(a.pkg_root, ROOT), "device_vs_numpy_max_rel": rel}
    for k, v in times.items():
        res[k] = {"median": round(float(np.median(v)), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
    m = {k: res[k]["median"] for k in times}
    res["error_stats_over_cv_all"] = round(m["error_stats_frames_s"] / m["cv_all_frames_device_reduce_s"], 3)
    res["numpy_path_over_error_stats"] = round(m["forward_frames_plus_numpy_s"] / m["error_stats_frames_s"], 3)
    res["bytes_back"] = {"error_stats": int(got["dev"].nbytes), "forward_frames": int(n * DIM * 4)}
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
