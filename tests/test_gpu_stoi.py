"""GPU: STOI on the device -- pkg.stoi_waves (mlggd_stoi_waves), BPGpu.enhance_waves(cleans=..., stoi=True)
(mlggd_enhance_waves_scored_stoi) and enhance_wav score=device stoi=1 -- against the float64 definition stoi64.stoi64.

Tolerance.  stoi64.stoi32 restates the measure in float32 on the CPU.  A case is one batch of utterances; its distance
to float64 is the largest |value - stoi64| over the batch's utterances that have a value.  The GPU's distance may be
16 x the model's on the same inputs: the rule and the factor of tests/test_gpu_score_waves.py, whose docstring says why
the batch and not the single utterance is the unit.  Before the device is touched every case asserts on the CPU that
its inputs decide nothing by a rounding: every frame's keep margin |e - max + 40| is at least 1e-3 dB in float64 (a
float32 energy is good to about 1e-5 dB) and no band of any segment has zero variance.  Each accuracy test prints its
row of the table in DESIGN.md section 8: case, model distance, GPU distance."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import hostlib
import stoi64
from test_gpu_score_waves import engine, norm_stats, same, small_net, write_wav

pytestmark = pytest.mark.gpu
F32 = np.float32
MARGIN = 16.0
MIN_KEEP_MARGIN_DB = 1e-3


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def batch(fs):
    """(cleans, procs, models): five utterances -- 30 frames (one too few: no value), 31 frames (30 compacted, one
    segment), 32 frames (two segments), 45 frames with a gap 70 dB down (kept < frames), about 2 s; noise at 10, 0, 15,
    5, -5 dB; models[u] = (stoi64, stoi32).  Built once, never written to."""
    n31 = stoi64.shortest_with_frames(31, fs)
    n45 = stoi64.shortest_with_frames(45, fs)
    rate = {8: 8000, 11: 11000, 16: 16000}[fs]
    lengths = [n31 - 1, n31, stoi64.shortest_with_frames(32, fs) + 3, n45 + 7, 2 * rate + 11]
    gaps = [(), (), (), ((n45 // 3, n45 // 3 + n45 // 6),), ((rate // 2, rate // 2 + rate // 5),)]
    cleans = [stoi64.speech(n, fs, seed=100 * fs + u, gaps=g) for u, (n, g) in enumerate(zip(lengths, gaps))]
    procs = [stoi64.add_noise(c, snr, seed=fs + u) for u, (c, snr) in enumerate(zip(cleans, (10, 0, 15, 5, -5)))]
    for a in cleans + procs:
        a.setflags(write=False)
    models = [(stoi64.stoi64(c, p, fs), stoi64.stoi32(c, p, fs)) for c, p in zip(cleans, procs)]
    return cleans, procs, models


def check_inputs(models):
    """the condition on the inputs, on the CPU: no keep decision and no correlation hangs on a rounding"""
    for m64, m32 in models:
        assert m64.min_margin >= MIN_KEEP_MARGIN_DB, m64
        assert (m64.frames, m64.kept, m64.segments) == (m32.frames, m32.kept, m32.segments)
        if m64.segments:
            assert m64.min_var > 1e-3, m64


def check_case(name, got, seg, models, muted=()):
    """the GPU's values against stoi64 with the model's bound; prints the case's row of the table.  muted: the rows
    whose processed wave has a band of exact zeros over a whole segment: NaN by the definition, with segments counted"""
    valued = [u for u, (m64, _) in enumerate(models) if m64.segments and u not in muted]
    for u, (m64, _) in enumerate(models):
        assert int(seg[u]) == m64.segments, (name, u)
        if u in muted:
            assert m64.segments > 0 and np.isnan(m64.value) and np.isnan(got[u]), (name, u, got[u])
        else:
            assert np.isnan(got[u]) == (m64.segments == 0), (name, u)
    dm = max(abs(models[u][1].value - models[u][0].value) for u in valued)
    dg = max(abs(float(got[u]) - models[u][0].value) for u in valued)
    print("stoi table | %-34s | model %.3g | GPU %.3g" % (name, dm, dg))
    assert np.isfinite(dg) and dg <= MARGIN * dm, (name, dm, dg)


# ---- accuracy at every rate
@pytest.mark.parametrize("fs", [8, 11, 16])
def test_a_batch_against_float64(pkg, fs):
    cleans, procs, models = batch(fs)
    check_inputs(models)
    m = [a for a, _ in models]
    assert [x.segments for x in m[:3]] == [0, 1, 2] and m[0].frames == 30 and m[1].M == 30 and m[2].M == 31
    assert m[3].kept < m[3].frames and m[4].kept < m[4].frames and m[4].segments > 100
    assert [pkg.stoi_layout(c.size, fs_khz=fs)[:2] for c in cleans] == [(x.len10, x.frames) for x in m]
    got, seg = pkg.stoi_waves(cleans, procs, fs_khz=fs, return_segments=True)
    assert got.dtype == np.float32 and got.shape == (5,) and seg.dtype == np.int32 and seg.shape == (5,)
    check_case("%d kHz, batch of 5" % fs, got, seg, models)
    assert 0.2 < got[4] < got[3] < 1.0                        # -5 dB is worse than 5 dB


@pytest.mark.parametrize("fs", [8, 16])
def test_a_wave_against_itself_and_a_silent_clean_wave(pkg, fs):
    cleans, procs, _ = batch(fs)
    got, seg = pkg.stoi_waves([cleans[4], np.zeros_like(cleans[4]), cleans[3]], [cleans[4], procs[4], cleans[3]],
                              fs_khz=fs, return_segments=True)
    assert abs(float(got[0]) - 1.0) < 2e-6 and abs(float(got[2]) - 1.0) < 2e-6
    assert np.isnan(got[1]) and seg[1] == 0 and seg[0] > 100


# ---- independence and determinism
def test_an_utterance_s_value_does_not_depend_on_the_batch(pkg):
    """alone, first, last and between other neighbours; twice in one process"""
    fs = 16
    cleans, procs, _ = batch(fs)
    full = pkg.stoi_waves(cleans, procs, fs_khz=fs)
    assert np.array_equal(bits(full), bits(pkg.stoi_waves(cleans, procs, fs_khz=fs)))
    n = len(cleans)
    for u in range(n):
        alone = pkg.stoi_waves([cleans[u]], [procs[u]], fs_khz=fs)
        order = [u] + [v for v in range(n) if v != u]
        first = pkg.stoi_waves([cleans[v] for v in order], [procs[v] for v in order], fs_khz=fs)
        order = order[1:] + [u]
        last = pkg.stoi_waves([cleans[v] for v in order], [procs[v] for v in order], fs_khz=fs)
        order = [(u + 2) % n, u, (u + 3) % n]
        mid = pkg.stoi_waves([cleans[v] for v in order], [procs[v] for v in order], fs_khz=fs)
        assert bits(alone)[0] == bits(first)[0] == bits(last)[n - 1] == bits(mid)[1] == bits(full)[u], u


# ---- stoi_samples
@pytest.mark.parametrize("fs", [11, 16])
def test_stoi_samples(pkg, fs):
    cleans, procs, _ = batch(fs)
    full = pkg.stoi_waves(cleans, procs, fs_khz=fs)
    whole = pkg.stoi_waves(cleans, procs, fs_khz=fs, stoi_samples=[c.size for c in cleans])
    assert np.array_equal(bits(full), bits(whole))
    n31 = stoi64.shortest_with_frames(31, fs)
    counts = [cleans[0].size, 0, n31, cleans[3].size - 301, cleans[4].size // 2]
    got, seg = pkg.stoi_waves(cleans, procs, fs_khz=fs, stoi_samples=counts, return_segments=True)
    cut, cseg = pkg.stoi_waves([c[:k] for c, k in zip(cleans, counts)], [p[:k] for p, k in zip(procs, counts)],
                               fs_khz=fs, return_segments=True)
    assert np.array_equal(bits(got), bits(cut)) and np.array_equal(seg, cseg)
    assert np.isnan(got[1]) and seg[1] == 0 and seg[2] == 1 and bits(got)[4] != bits(full)[4]
    models = [(stoi64.stoi64(c, p, fs, samples=k), stoi64.stoi32(c, p, fs, samples=k))
              for c, p, k in zip(cleans, procs, counts)]
    check_inputs(models)
    check_case("%d kHz, stoi_samples" % fs, got, seg, models)
    # a clean wave shorter than the processed one: scored over the samples both have
    short = pkg.stoi_waves([c[:k] for c, k in zip(cleans, counts)], procs, fs_khz=fs)
    assert np.array_equal(bits(short), bits(got))


# ---- the engine path
def test_engine_path_adds_stoi_and_changes_nothing_else(pkg):
    """capacity 4 cuts inside every utterance, 1000 holds the batch; the second call of an engine reuses its workspaces"""
    fs, ctx = 16, 7
    cleans, noisys, _ = batch(fs)
    rng = np.random.default_rng(81)
    ls, ws, bs = small_net(rng, ctx=ctx)
    mean, inv = norm_stats(rng)
    res = []
    for cap in (1000, 4):
        eng = engine(pkg, ls, ws, bs, 16, cap=cap)
        plain = eng.enhance_waves(noisys, mean, inv, fs_khz=fs, fea_context=ctx, return_f32=True, return_lps=True,
                                  cleans=cleans)
        assert len(plain) == 5
        with_stoi = eng.enhance_waves(noisys, mean, inv, fs_khz=fs, fea_context=ctx, return_f32=True, return_lps=True,
                                      cleans=cleans, stoi=True)
        assert len(with_stoi) == 6
        for g, w in zip(with_stoi[:3], plain[:3]):
            same(g, w)
        assert np.array_equal(bits(with_stoi[3]), bits(plain[3])) and np.array_equal(bits(with_stoi[4]), bits(plain[4]))
        stoi = with_stoi[5]
        assert stoi.dtype == np.float32 and stoi.shape == (5,)
        assert np.array_equal(bits(stoi), bits(pkg.stoi_waves(cleans, with_stoi[0], fs_khz=fs)))
        assert np.isnan(stoi[0]) and np.isfinite(stoi[2:]).all()     # the enhanced wave ends with its last whole frame
        again = eng.enhance_waves(noisys, mean, inv, fs_khz=fs, cleans=cleans, stoi=True)      # workspaces reused
        assert len(again) == 4 and np.array_equal(bits(again[3]), bits(stoi))
        same(again[0], plain[0])
        half = [c.size // 2 for c in cleans]
        part = eng.enhance_waves(noisys, mean, inv, fs_khz=fs, cleans=cleans, stoi=True, stoi_samples=half)
        assert np.array_equal(bits(part[3]), bits(pkg.stoi_waves(cleans, with_stoi[0], fs_khz=fs, stoi_samples=half)))
        same(eng.enhance_waves(noisys, mean, inv, fs_khz=fs), plain[0])                        # and the plain call after it
        with pytest.raises(pkg.MlggdError, match=r"error 1: utterance 2: stoi_samples %d is outside" % (cleans[2].size + 1)):
            eng.enhance_waves(noisys, mean, inv, fs_khz=fs, cleans=cleans, stoi=True,
                              stoi_samples=[0, 0, cleans[2].size + 1, 0, 0])
        eng.close()
        res.append(stoi)
    assert np.array_equal(bits(res[0]), bits(res[1]))


# ---- the tool
def test_enhance_wav_stoi(pkg, tmp_path):
    """three lines, the first and the third scored"""
    fs, ctx, B = 16, 7, 64
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    cleans, noisys, _ = batch(fs)
    cleans, noisys = [cleans[0], cleans[2], cleans[3]], [noisys[0], noisys[2], noisys[3]]
    rng = np.random.default_rng(82)
    ls, ws, bs = small_net(rng, ctx=ctx)
    mean, inv = norm_stats(rng)
    hostlib.write_wts(str(tmp_path / "mlp.wts"), ws, bs)
    hostlib.write_norm(str(tmp_path / "n.norm"), mean, inv)
    scored = (0, 2)
    with open(tmp_path / "list.scp", "w") as f:
        for u in range(3):
            write_wav(tmp_path / ("n%d.wav" % u), noisys[u])
            write_wav(tmp_path / ("c%d.wav" % u), cleans[u])
            f.write("%s %s" % (tmp_path / ("n%d.wav" % u), tmp_path / ("out%d.wav" % u)))
            f.write(" %s %s\n" % (tmp_path / ("c%d.wav" % u), tmp_path / ("info%d.txt" % u)) if u in scored else "\n")
    common = [os.path.join(hostlib.HOST, "enhance_wav"), "wts=%s" % (tmp_path / "mlp.wts"),
              "norm_file=%s" % (tmp_path / "n.norm"), "fea_context=%d" % ctx, "bunchsize=%d" % B,
              "scp=%s" % (tmp_path / "list.scp")]

    def run(extra):
        r = subprocess.run(common + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        names = ["out%d.wav" % u for u in range(3)] + ["info%d.txt" % u for u in scored]
        files = {n: open(tmp_path / n, "rb").read() for n in names}
        for n in names:
            os.remove(tmp_path / n)
        return r.stdout.split("\n"), files

    base, base_files = run(["score=device"])
    assert not any("stoi=" in l or "STOI" in l for l in base)       # (the directory's own name holds the word)
    off, off_files = run(["score=device", "stoi=0"])
    assert off == base and off_files == base_files
    lines, files = run(["score=device", "stoi=1"])
    assert files == base_files                                       # waves and info files: the same bytes
    assert len(lines) == len(base) == 5 and lines[1] == base[1] and lines[4] == ""
    eng = engine(pkg, ls, ws, bs, B)
    want = eng.enhance_waves(noisys, mean, inv, fs_khz=fs, fea_context=ctx, cleans=cleans, stoi=True)[3]
    eng.close()
    assert np.isnan(want[0]) and np.isfinite(want[2])
    assert lines[0] == base[0] + " stoi=nan"
    assert lines[2] == base[2] + " stoi=%f" % want[2]
    assert lines[3] == base[3] + ", mean STOI %f over 1 utterances" % want[2]
    r = subprocess.run(common + ["score=host", "stoi=1"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "stoi=1 needs score=device" in r.stderr
