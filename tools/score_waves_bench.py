"""Cost of the quality report (segmental SNR, LSD) of a scored list at the shipped shape 1799-2048^3-257, 16 kHz:
enhance_wav score=host (the report in double on one host thread) against score=device (mlggd_enhance_waves_scored), on
the same synthetic list.  Writes profiles/score_waves_bench.json and prints it as one JSON line.

    python tools/score_waves_bench.py [--utterances 200] [--seconds 3] [--reps 3] [--gpu 0] [--out FILE]

Two measurements, each after a warm-up run of the same form, the forms alternating inside every repetition, best of
--reps:
* the tool: wall time of `enhance_wav scp=LIST` as a process (engine creation and wave file I/O included) with an
  unscored list, with score=host and with score=device.  host_report_s = score=host - unscored is the host-only time
  of the report; device_report_s = score=device - unscored (reading the clean waves included).
* the pass: wall time of BPGpu.enhance_waves in this process, which ends in a stream synchronise, without and with
  cleans=: the difference is the device time the report adds to the pass (clean upload, two kernels, 2 n floats back).
No ratio is promised; the file records what the run gave.  Needs a GPU: there is no CPU path."""
import argparse
import importlib
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "speech-enhancement-based-on-a-maximum-likelihood-criterion_amd"


def write_wav(path, w, rate=16000):
    w = np.asarray(w, "<i2")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + 2 * w.size) + b"WAVEfmt " +
                struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16) + b"data" + struct.pack("<I", 2 * w.size) +
                w.tobytes())


def best_of(forms, reps):
    """{name: best wall seconds}: one warm-up of every form, then reps rounds with the forms alternating"""
    for fn in forms.values():
        fn()
    best = {}
    for _ in range(reps):
        for name, fn in forms.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            best[name] = min(best.get(name, dt), dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utterances", type=int, default=200)
    ap.add_argument("--seconds", type=float, default=3.0, help="mean utterance length")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--gpu", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_waves_bench.json"))
    a = ap.parse_args()
    pkg = importlib.import_module(PKG)
    import hostlib
    import spec64
    rng = np.random.default_rng(0)
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
    frames = int(pkg.enhance_waves_layout(lengths, 16)[1][-1])
    res = {"workload": "scored list, enhance_wav 1799-2048^3-257 16 kHz", "utterances": a.utterances,
           "mean_seconds": a.seconds, "audio_s": round(float(lengths.sum()) / 16000.0, 1), "frames": frames,
           "reps": a.reps}

    eng = pkg.BPGpu(1, a.gpu, ls, 512, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    scores = {}
    t = best_of({"pass_unscored_wall_s": lambda: eng.enhance_waves(noisys, mean, inv),
                 "pass_scored_wall_s": lambda: scores.update(r=eng.enhance_waves(noisys, mean, inv, cleans=cleans))},
                a.reps)
    eng.close()
    res.update({k: round(v, 4) for k, v in t.items()})
    res["pass_report_device_s"] = round(t["pass_scored_wall_s"] - t["pass_unscored_wall_s"], 4)
    res["mean_segsnr_db"] = round(float(scores["r"][1].mean()), 4)
    res["mean_lsd_db"] = round(float(scores["r"][2].mean()), 4)

    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    with tempfile.TemporaryDirectory() as d:
        hostlib.write_wts(os.path.join(d, "mlp.wts"), ws, bs)
        hostlib.write_norm(os.path.join(d, "n.norm"), mean, inv)
        with open(os.path.join(d, "plain.scp"), "w") as plain, open(os.path.join(d, "scored.scp"), "w") as scored:
            for u, (c, n) in enumerate(zip(cleans, noisys)):
                p = os.path.join(d, "%d" % u)
                write_wav(p + ".n.wav", n)
                write_wav(p + ".c.wav", c)
                plain.write("%s.n.wav %s.out.wav\n" % (p, p))
                scored.write("%s.n.wav %s.out.wav %s.c.wav %s.info.txt\n" % (p, p, p, p))
        common = [os.path.join(hostlib.HOST, "enhance_wav"), "wts=" + os.path.join(d, "mlp.wts"),
                  "norm_file=" + os.path.join(d, "n.norm"), "gpu_used=%d" % a.gpu]

        def tool(scp, *extra):
            return lambda: subprocess.run(common + ["scp=" + os.path.join(d, scp), *extra], check=True,
                                          stdout=subprocess.DEVNULL)

        t = best_of({"tool_unscored_wall_s": tool("plain.scp"), "tool_score_host_wall_s": tool("scored.scp", "score=host"),
                     "tool_score_device_wall_s": tool("scored.scp", "score=device")}, a.reps)
    res.update({k: round(v, 4) for k, v in t.items()})
    res["host_report_s"] = round(t["tool_score_host_wall_s"] - t["tool_unscored_wall_s"], 4)
    res["device_report_s"] = round(t["tool_score_device_wall_s"] - t["tool_unscored_wall_s"], 4)
    line = json.dumps(res)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
