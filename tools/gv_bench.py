"""Cost of global variance equalisation (csrc/gv_rule.h) at the shipped shape 2827-2048^3-257, B = 128:
  (a) the output statistics of a 7,920-sample CV chunk, BPGpu.output_stats_frames (mlggd_output_stats_frames), against
      cv_all_frames with the device reduce: the same upload and the same forward pass with k_cv_reduce in the place of
      k_out_stats -- the comparator; the ratio is recorded;
  (b) enhance_waves on one batch with the factors set and unset (k_lps_synthesis_gv / k_lps_synthesis), alternating
      windows in one session on one engine; the difference of the medians is stated next to the run-to-run spread;
  (c) bench.py's headline on the parent commit's build and on this one, measured by the caller with
      `python bench.py --gpus 1` on both trees, alternating, same machine, same session: --bench-parent / --bench-this
      name files that hold the JSON lines of those runs (every line is recorded); without them (c) says "not run".
Writes profiles/gv_bench.json and prints it as one JSON line.

    python tools/gv_bench.py [--samples 7920] [--utts 16] [--seconds 4] [--reps 9] [--gpu 0] [--out FILE]
                             [--bench-parent FILE] [--bench-this FILE] [--only-a] [--pkg-root DIR]

--only-a stops after (a); --pkg-root DIR times another build with the same file (DIR holds its package, e.g. a built
checkout of the parent commit), for an A/B of two builds in processes of their own; its result is printed and, unless --out names a file,
not written.

Every arm is a host clock around a call that ends in a stream synchronise; each is warmed up once, then the arms
alternate inside every repetition and the MEDIAN over the repetitions is reported (with the fastest and slowest beside
it).  No figure is promised; the file records what the run gave.  Needs a GPU: there is no CPU path."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "speech-enhancement-based-on-a-maximum-likelihood-criterion_amd"
DIM, CTX, TOFF, B = 257, 11, 5, 128


def headlines(path):
    if not path:
        return None
    out = []
    for line in open(path).read().splitlines():
        if line.startswith("{"):
            r = json.loads(line)
            out.append({k: r[k] for k in ("value", "ms_per_step", "unit", "metric") if k in r})
    return out or None


def stats(v):
    return {"median": round(float(np.median(v)), 5), "min": round(min(v), 5), "max": round(max(v), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=7920)
    ap.add_argument("--utts", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-parent", default=None, help="file with the JSON lines of `python bench.py` on the parent commit")
    ap.add_argument("--bench-this", default=None, help="file with the JSON lines of `python bench.py` on this commit")
    ap.add_argument("--only-a", action="store_true")
    ap.add_argument("--pkg-root", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.pkg_root))
    if a.out is None:  # the committed profile is this tree's: another build's figures go to it only when asked
        a.out = os.path.join(ROOT, "profiles", "gv_bench.json") if os.path.samefile(a.pkg_root, ROOT) else os.devnull
    pkg = importlib.import_module(PKG)
    rng = np.random.default_rng(0)
    ls = [CTX * DIM, 2048, 2048, 2048, DIM]
    ws = [(rng.normal(0, 1.0, (ls[i], ls[i + 1])) / np.sqrt(ls[i])).astype(np.float32) for i in range(4)]
    bs = [rng.normal(0, 0.1, ls[i + 1]).astype(np.float32) for i in range(4)]
    n = a.samples
    feat = rng.standard_normal((n + CTX - 1, DIM), dtype=np.float32)
    targ = (0.5 * feat + 0.5 * rng.standard_normal(feat.shape, dtype=np.float32)).astype(np.float32)
    first = np.arange(n, dtype=np.int32)                  # a CV chunk is not shuffled
    eng = pkg.BPGpu(1, a.gpu, ls, B, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    eng.set_cv_device_reduce(True)
    res = {"workload": "global variance equalisation, 2827-2048^3-257, B 128", "reps": a.reps,
           "command": "python tools/gv_bench.py"}

    # (a) the statistics against the CV pass
    got = {}
    arms = {
        "output_stats_frames_s": lambda: got.update(dev=eng.output_stats_frames(feat, targ, first, CTX, TOFF)),
        "cv_all_frames_device_reduce_s": lambda: eng.cv_all_frames(feat, targ, first, CTX, TOFF),
    }
    for f in arms.values():
        f()
    y, t = eng.forward_frames(feat, first, CTX).astype(np.float64), targ[first + TOFF].astype(np.float64)
    host = np.stack([y.sum(0), (y * y).sum(0), t.sum(0), (t * t).sum(0)])
    rel = float(np.max(np.abs(got["dev"] - host) / np.maximum(np.abs(host), 1.0)))
    assert rel < 1e-9, rel                                # the arms looked at the same outputs
    fit = pkg.gv_fit(n, got["dev"])
    times = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, f in arms.items():
            t0 = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t0)
    sa = {"samples": n, "bunches": -(-n // B), "device_vs_numpy_max_rel": rel, "bytes_back": int(got["dev"].nbytes)}
    for k, v in times.items():
        sa[k] = stats(v)
    sa["output_stats_over_cv_all"] = round(sa["output_stats_frames_s"]["median"] / sa["cv_all_frames_device_reduce_s"]["median"], 3)
    res["a_output_stats"] = sa
    if a.only_a:
        eng.close()
        line = json.dumps(res)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        print(line)
        return

    # (b) the decoders with and without factors
    mean = rng.normal(10, 2, DIM).astype(np.float32)
    inv = (1.0 / rng.uniform(2, 4, DIM)).astype(np.float32)
    waves = [(3000 * rng.standard_normal(int(a.seconds * 16000))).astype(np.int16) for _ in range(a.utts)]
    eta = np.where(fit.fitted, fit.eta, np.float32(1)).astype(np.float32)
    dec = lambda: eng.enhance_waves(waves, mean, inv, fs_khz=16, fea_context=CTX)

    for e in (eta, None):
        eng.set_gv(e)
        dec()
    times = {"enhance_waves_gv_s": [], "enhance_waves_plain_s": []}
    for _ in range(a.reps):
        for k, e in (("enhance_waves_gv_s", eta), ("enhance_waves_plain_s", None)):
            eng.set_gv(e)                                 # outside the clock: one upload of D floats
            t0 = time.perf_counter()
            dec()
            times[k].append(time.perf_counter() - t0)
    eng.close()
    sb = {"utterances": a.utts, "seconds_each": a.seconds, "frames": int(sum(pkg.enhance_waves_layout([w.size for w in waves], 16)[0]))}
    for k, v in times.items():
        sb[k] = stats(v)
    sb["gv_minus_plain_s"] = round(sb["enhance_waves_gv_s"]["median"] - sb["enhance_waves_plain_s"]["median"], 5)
    sb["spread_s"] = round(max(s["max"] - s["min"] for s in (sb["enhance_waves_gv_s"], sb["enhance_waves_plain_s"])), 5)
    sb["difference_within_spread"] = abs(sb["gv_minus_plain_s"]) <= sb["spread_s"]
    res["b_enhance_waves"] = sb

    # (c) the training headline, measured by the caller
    hp, ht = headlines(a.bench_parent), headlines(a.bench_this)
    if hp and ht:
        res["c_bench_py_headline"] = {"parent_commit": hp, "this_commit": ht, "order": "alternating, parent first"}
    else:
        res["c_bench_py_headline"] = "not run"
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
