"""Training from waves at the shipped shape 1799-2048^3-257 (16 kHz, context 7), B = 128, a few minutes of audio:
  (a) BPGpu.train_waves (mlggd_train_waves): clean waves up, mixed with the resident noise bank, both waves analysed,
      normalised and trained on the device;
  (b) BPGpu.train_frames on the same rows prepared beforehand -- the unchanged path, the floor;
  (c) what a user did before: the mix in NumPy (the rule of csrc/mix_rule.h, float64), wave_to_lps twice per utterance,
      the normalisation in NumPy float32, then train_frames.
Writes profiles/train_waves_bench.json and prints it as one JSON line: the three frames/s figures, the front end's
share of (a) taken from (a) - (b), and beside them load_waves alone (upload, two analyses, normalisation) and
mix_waves alone, which say where the front end's time goes.

    python tools/train_waves_bench.py [--utts 40] [--seconds 6] [--reps 7] [--gpu 0] [--out FILE]

Every arm is a host clock around a call that ends in a stream synchronise; each is warmed up once, then the arms
alternate inside every repetition and the MEDIAN over the repetitions is reported (with the fastest and slowest beside
it).  Before anything is timed, (a) and (b) on fresh engines must leave the same bits in every weight, and the NumPy
mix must equal the device's in every sample.  No figure is promised; the file records what the run gave.  Needs a GPU:
there is no CPU path."""
import argparse
import importlib
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "speech-enhancement-based-on-a-maximum-likelihood-criterion_amd"
FS, HZ, DIM, CTX, TOFF, B = 16, 16000, 257, 7, 3, 128


def speech(n, seed):
    """a speech-like int16 wave: harmonics of a gliding pitch under a syllable envelope, plus a little noise"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / HZ
    ph = 2 * np.pi * np.cumsum(110.0 + 30.0 * np.sin(2 * np.pi * 0.7 * t + seed)) / HZ
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 2.3 * t + 0.1 * seed)
    s = sum(np.sin(k * ph + rng.uniform(0, 2 * np.pi)) / k for k in range(1, 12)) * env * 4000.0
    return np.clip(np.round(s + rng.normal(0, 300.0, n)), -32768, 32767).astype(np.int16)


def numpy_mix(clean, noise, lo, ln, start, snr_db):
    nz = noise[lo + (start + np.arange(clean.size, dtype=np.int64)) % ln]
    Ec = int(np.sum(clean.astype(np.int64) ** 2))
    En = int(np.sum(nz.astype(np.int64) ** 2))
    g = 0.0 if Ec == 0 or En == 0 else math.sqrt(float(Ec) / float(En)) * math.pow(10.0, -snr_db / 20.0)
    v = np.rint(clean.astype(np.float64) + g * nz.astype(np.float64))
    return np.clip(v, -32768.0, 32767.0).astype(np.int16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=40)
    ap.add_argument("--seconds", type=float, default=6.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_waves_bench.json"))
    a = ap.parse_args()
    pkg = importlib.import_module(PKG)
    rng = np.random.default_rng(0)
    ls = [CTX * DIM, 2048, 2048, 2048, DIM]
    ws = [(rng.normal(0, 1.0, (ls[i], ls[i + 1])) / np.sqrt(ls[i])).astype(np.float32) for i in range(4)]
    bs = [rng.normal(0, 0.1, ls[i + 1]).astype(np.float32) for i in range(4)]
    n_utts = a.utts
    cleans = [speech(int(a.seconds * HZ * rng.uniform(0.7, 1.3)), u) for u in range(n_utts)]
    noise = rng.integers(-3000, 3001, 60 * HZ).astype(np.int16)                 # a minute of noise in the bank
    seg = [(int(rng.integers(0, 30 * HZ)), int(rng.integers(2 * HZ, 30 * HZ))) for _ in range(n_utts)]
    start = [int(rng.integers(0, s[1])) for s in seg]
    snr = [(-5.0, 0.0, 5.0, 10.0, 15.0, 20.0)[u % 6] for u in range(n_utts)]
    table = pkg.wave_samples([w.size for w in cleans], CTX, FS)
    first = table[rng.permutation(table.size)]
    n = first.size

    def host_rows(noisys, mean, inv):
        rows_n = np.concatenate([pkg.wave_to_lps(w, fs_khz=FS, device=a.gpu) for w in noisys])
        rows_c = np.concatenate([pkg.wave_to_lps(w, fs_khz=FS, device=a.gpu) for w in cleans])
        return (rows_n - mean) * inv, (rows_c - mean) * inv

    noisys = pkg.mix_waves(cleans, noise, snr, start, noise_seg=seg, device=a.gpu)
    mean, inv = pkg.norm_from_stats(*pkg.lps_stats(noisys, fs_khz=FS, device=a.gpu))
    feat, targ = host_rows(noisys, mean, inv)
    mixed = [numpy_mix(c, noise, s[0], s[1], st, r) for c, s, st, r in zip(cleans, seg, start, snr)]
    numpy_mix_equal = all(np.array_equal(x, y) for x, y in zip(mixed, noisys))

    def engine():
        return pkg.BPGpu(1, a.gpu, ls, B, 0.001, 0.9, 1e-5, ws, bs, 1.2, 1)

    def arm_a(eng):
        return eng.train_waves(cleans, snr, start, mean, inv, first, TOFF, noise_seg=seg, fea_context=CTX, fs_khz=FS)

    def arm_b(eng):
        return eng.train_frames(feat, targ, first, CTX, TOFF)

    def arm_c(eng):
        ns = [numpy_mix(c, noise, s[0], s[1], st, r) for c, s, st, r in zip(cleans, seg, start, snr)]
        f, t = host_rows(ns, mean, inv)
        return eng.train_frames(f, t, first, CTX, TOFF)

    # the arms train the same thing: every bit of every weight after one pass on fresh engines
    states = []
    for arm in (arm_a, arm_b):
        eng = engine()
        eng.set_noise(noise)
        steps = arm(eng)
        states.append(eng.returnWeights())
        eng.close()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(states[0][0] + states[0][1], states[1][0] + states[1][1]))
    assert numpy_mix_equal

    eng = engine()
    eng.set_noise(noise)
    arms = {
        "a_train_waves_s": lambda: arm_a(eng),
        "b_train_frames_prepared_s": lambda: arm_b(eng),
        "c_numpy_mix_wave_to_lps_train_frames_s": lambda: arm_c(eng),
        "load_waves_alone_s": lambda: eng.load_waves(noisys, cleans, mean, inv, first, TOFF, CTX, FS),
        "mix_waves_alone_s": lambda: pkg.mix_waves(cleans, noise, snr, start, noise_seg=seg, device=a.gpu),
    }
    for f in arms.values():
        f()
    times = {k: [] for k in arms}
    for _ in range(a.reps):
        for k, f in arms.items():
            eng.sync()
            t0 = time.perf_counter()
            f()
            eng.sync()
            times[k].append(time.perf_counter() - t0)
    eng.close()
    trained = steps * B
    res = {"workload": "training from waves, 1799-2048^3-257, B 128, 16 kHz, ML-GGD", "utterances": n_utts,
           "audio_seconds": round(sum(w.size for w in cleans) / HZ, 1), "frames": int(feat.shape[0]), "samples": int(n),
           "steps_per_pass": int(steps), "reps": a.reps, "command": "python tools/train_waves_bench.py",
           "weights_equal_a_b": True, "numpy_mix_equals_device": bool(numpy_mix_equal)}
    for k, v in times.items():
        res[k] = {"median": round(float(np.median(v)), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
    m = {k: res[k]["median"] for k in times}
    res["frames_per_s"] = {"a_train_waves": round(trained / m["a_train_waves_s"], 1),
                           "b_train_frames_prepared": round(trained / m["b_train_frames_prepared_s"], 1),
                           "c_numpy_path": round(trained / m["c_numpy_mix_wave_to_lps_train_frames_s"], 1)}
    res["front_end_share_of_a"] = round((m["a_train_waves_s"] - m["b_train_frames_prepared_s"]) / m["a_train_waves_s"], 4)
    res["a_over_c_speedup"] = round(m["c_numpy_mix_wave_to_lps_train_frames_s"] / m["a_train_waves_s"], 3)
    res["bytes_up_per_pass"] = {"a_train_waves": int(2 * sum(w.size for w in cleans) + 4 * n),
                                "b_train_frames": int(feat.nbytes + targ.nbytes + 4 * n)}
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
