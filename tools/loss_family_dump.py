"""Raw bits of everything the output-layer loss families produce, for an A/B of two builds on one GPU.

    python tools/loss_family_dump.py --out THIS.npz [--pkg-root DIR] [--gpu 0]
    python tools/loss_family_dump.py --compare A.npz B.npz

The first form runs a fixed, seeded set of small cases on the build under --pkg-root (default: this checkout; DIR is
the directory that holds another build's package, e.g. a built checkout of the parent commit) and writes one .npz.  Run
it once per build, each run a process of its own, then --compare: it prints "identical", or the first array that
differs with the index of its first differing element, and exits non-zero on a difference.  Every array is compared as
bytes, so -0.0 / 0.0 and NaN payloads count.

Cases -- the shapes of tests/test_gpu_shapefactors.py and tests/test_gpu_asymmetry.py, the smallest that reach every
edge of the kernels:
  net     40-64-D, D = 19 (Dp 32: a partly filled group of 8 units and an empty one) and D = 257 (a last group with
          one live unit); B = 160 (the fused kernel's 128-frame loop makes a second, partial pass) and B = 32;
  model   scalar beta = 0.8 (pow_det runs, not a self-case); a mixed shape vector that holds 1.0 and 2.0; a mixed skew
          vector without a power of two, alone (shapes from the scalar) and on top of the shape vector;
  path    fused; MLGGD_LOSS_FUSE=0; fake_world(2) (B = 32, as in the tests); fake_world(2, allreduce=True).
Per case: 3 training steps, then weights, biases, both momentum sets and scalefactor.  On the two single-device paths
also, over 200 frames (one full bunch and a trailing partial one): cv_all under the device reduce and in host order,
error_stats, error_stats_signed and output_stats -- the emulated worlds refuse the statistics by design.

Statistics cases (STATS) -- the column statistics alone, on a 24-H-D net fed 3-frame windows of 8-wide frames, each
through the chunk entries AND the _frames entries (error_stats, error_stats_signed, output_stats; the slab count of
the output layer is dumped beside them):
  D       5 (fewer bins than the 8 of a workgroup) and 13 (not a multiple of 8);
  n, B    a chunk of 1, 33 and 2 B + 7 samples at B = 32 and B = 128;
  K       a grid of 1 shape, of 3, and of MLGGD_MAX_BETAS = 32 (0.5 + k / 16: 1.0 and 2.0, the self-cases, are in it);
  H       16 (one output slab), 64 (two) and 256 (eight).
Needs a GPU: there is no CPU path."""
import argparse
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "speech-enhancement-based-on-a-maximum-likelihood-criterion_amd"
HP = (0.1, 0.9, 1e-5)
BETA = 0.8
SHAPES = [(19, 32), (19, 160), (257, 32), (257, 160)]
PATHS = ([(p, D, B) for p in ("fused", "unfused", "allreduce") for D, B in SHAPES]
         + [("gather", D, 32) for D in (19, 257)])
MODELS = ("scalar", "shapes", "skew", "shapes+skew")
GRID = (0.8, 1.0, 2.0)          # the statistics' own shape grid
CV_FRAMES = 200
# (D, H, B, n, K): see the docstring
STATS = [(5, 64, 32, 1, 1), (5, 64, 32, 33, 32), (5, 64, 32, 71, 3), (13, 64, 128, 1, 32), (13, 64, 128, 33, 1),
         (13, 64, 128, 263, 3), (13, 256, 32, 71, 32), (13, 256, 128, 263, 32), (5, 16, 128, 263, 1)]
STATS_DIM, STATS_CTX, STATS_TOFF = 8, 3, 1


def vectors(D):
    shapes = np.array([(0.8, 1.0, 1.3, 2.0, 0.6)[d % 5] for d in range(D)], np.float32)
    skews = np.array([(0.7, 1.0, 1.3, 0.9, 1.6, 1.1, 0.85)[d % 7] for d in range(D)], np.float32)
    return shapes, skews


def data(D, n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 40), dtype=np.float32), rng.standard_normal((n, D), dtype=np.float32)


def run_case(pkg, synth, gpu, path, D, B, model, out):
    ls = [40, 64, D]
    ws, bs = synth.make_weights(ls, seed=100 + D)
    os.environ.pop("MLGGD_LOSS_FUSE", None)
    if path == "unfused":
        os.environ["MLGGD_LOSS_FUSE"] = "0"      # read when the engine is created
    eng = pkg.BPGpu(1, gpu, ls, B, *HP, ws, bs, BETA, 1)
    try:
        if path == "gather":
            eng.fake_world(2)
        elif path == "allreduce":
            eng.fake_world(2, allreduce=True)
        shapes, skews = vectors(D)
        if "shapes" in model:
            eng.set_shapefactors(shapes)
        if "skew" in model:
            eng.set_asymmetry(skews)
        rows = (2 * B if path in ("gather", "allreduce") else B) * 3
        x, t = data(D, rows, 300 + D)
        assert eng.train(x, t) == 3
        key = "%s/D%d/B%d/%s/" % (path, D, B, model)
        W, b = eng.returnWeights()
        for l in range(len(W)):
            out[key + "W%d" % (l + 1)] = W[l]
            out[key + "b%d" % (l + 1)] = b[l]
            out[key + "delta_w%d" % (l + 1)] = eng.debug_tensor("delta_w", l + 1)
            out[key + "delta_b%d" % (l + 1)] = eng.debug_tensor("delta_b", l + 1)
        out[key + "scalefactor"] = eng.scalefactor()
        if path in ("fused", "unfused"):
            cx, ct = data(D, CV_FRAMES, 700 + D)
            for dev in (True, False):
                eng.set_cv_device_reduce(dev)
                out[key + ("cv_all_device" if dev else "cv_all_host")] = np.array(eng.cv_all(cx, ct), np.float32)
            out[key + "error_stats"] = eng.error_stats(cx, ct, GRID)
            out[key + "error_stats_signed"] = eng.error_stats_signed(cx, ct, GRID)
            out[key + "output_stats"] = eng.output_stats(cx, ct)
    finally:
        eng.close()
        os.environ.pop("MLGGD_LOSS_FUSE", None)


def run_stats_case(pkg, synth, gpu, D, H, B, n, K, out):
    ls = [STATS_CTX * STATS_DIM, H, D]
    ws, bs = synth.make_weights(ls, seed=500 + D + H)
    rng = np.random.default_rng(900 + D + H + B + n)
    feat = rng.standard_normal((n + STATS_CTX - 1, STATS_DIM), dtype=np.float32)
    targ = rng.standard_normal((n + STATS_CTX - 1, D), dtype=np.float32)
    first = rng.permutation(n).astype(np.int32)           # a window per sample, in scattered order
    rows = np.stack([feat[f:f + STATS_CTX].reshape(-1) for f in first])
    grid = np.array([0.5 + k / 16.0 for k in range(K)], np.float32)
    eng = pkg.BPGpu(1, gpu, ls, B, *HP, ws, bs, BETA, 1)
    try:
        key = "stats/D%d/H%d/B%d/n%d/K%d/" % (D, H, B, n, K)
        out[key + "out_slabs"] = np.array(eng.out_slabs(), np.int32)
        out[key + "error_stats"] = eng.error_stats(rows, targ[first + STATS_TOFF], grid)
        out[key + "error_stats_signed"] = eng.error_stats_signed(rows, targ[first + STATS_TOFF], grid)
        out[key + "output_stats"] = eng.output_stats(rows, targ[first + STATS_TOFF])
        fr = (feat, targ, first, STATS_CTX, STATS_TOFF)
        out[key + "error_stats_frames"] = eng.error_stats_frames(*fr, grid)
        out[key + "error_stats_signed_frames"] = eng.error_stats_signed_frames(*fr, grid)
        out[key + "output_stats_frames"] = eng.output_stats_frames(*fr)
    finally:
        eng.close()


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    if sorted(a.files) != sorted(b.files):
        print("different arrays: only in A %s, only in B %s" % (sorted(set(a.files) - set(b.files))[:5], sorted(set(b.files) - set(a.files))[:5]))
        return 1
    for k in sorted(a.files):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.dtype != y.dtype:
            print("%s: %s %s against %s %s" % (k, x.dtype, x.shape, y.dtype, y.shape))
            return 1
        bx, by = x.reshape(-1).view(np.uint8), y.reshape(-1).view(np.uint8)
        if not np.array_equal(bx, by):
            bad = (bx.reshape(-1, x.itemsize) != by.reshape(-1, x.itemsize)).any(axis=1)
            i = int(np.flatnonzero(bad)[0])
            print("%s differs first at flat index %d: %r against %r (%d of %d elements differ)"
                  % (k, i, x.reshape(-1)[i], y.reshape(-1)[i], int(bad.sum()), x.size))
            return 1
    n = sum(int(a[k].size) for k in a.files)
    print("identical: %d arrays, %d elements, compared as bytes" % (len(a.files), n))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--pkg-root", default=ROOT)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.compare:
        return compare(*a.compare)
    if not a.out:
        ap.error("--out FILE or --compare A B")
    sys.path.insert(0, os.path.abspath(a.pkg_root))
    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    out = {}
    for path, D, B in PATHS:
        for model in MODELS:
            run_case(pkg, synth, a.gpu, path, D, B, model, out)
    for case in STATS:
        run_stats_case(pkg, synth, a.gpu, *case, out)
    for k, v in out.items():
        assert np.isfinite(np.asarray(v, np.float64)).all(), k
    np.savez(a.out, **out)
    print("%d cases, %d arrays -> %s (package of %s)" % (len(PATHS) * len(MODELS) + len(STATS), len(out), a.out, os.path.abspath(a.pkg_root)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
