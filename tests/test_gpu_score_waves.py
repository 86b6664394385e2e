"""GPU: the quality report on the device -- pkg.score_waves (mlggd_score_waves), BPGpu.enhance_waves(cleans=...)
(mlggd_enhance_waves_scored) and enhance_wav score=device -- against spec64.quality64.

Tolerance.  quality32 below restates the report in float32 on the CPU (spec64.analysis32 for both spectra, the inverse
transform of spec64.synthesis32, numpy's float32 log10; numpy's pairwise sums, not the kernels' trees).  A case is one
batch of utterances; its distance to float64 is the largest |value - quality64| over the batch's utterances, taken for
the segmental SNR and for the LSD separately.  The GPU's distance may be 16 x the model's on the same inputs: the
margin covers another equally valid summation order and the device's log10 and exp.  The batch, not the single
utterance, is the unit because a single float32 result can land next to the float64 value by chance (a distance far
below its typical size), which would turn 16 x into a bound no correct float32 evaluation meets; the largest of
several distances does not collapse like that.  Exact results (a clamped frame: -20 or 30) have distance 0 on both
sides.  Each accuracy test prints its rows of the table in DESIGN.md section 8: case, model distance, GPU distance."""
import functools
import os
import struct
import subprocess

import numpy as np
import pytest

import hostlib
import spec64

pytestmark = pytest.mark.gpu
F32 = np.float32
FRAMES = [1, 2, 5, 9]     # 1 + 2 share a workgroup of 4 frames with the start of 5; 5 and 9 each span two workgroups
MARGIN = 16.0


# ---- inputs
def n_samples(F, fs, extra=0):
    L, S, _ = spec64.params(fs)
    return F * S + L - S + extra


def add_noise(clean, snr_db, rng):
    """clean + Gaussian noise at snr_db, int16"""
    c = clean.astype(np.float64)
    noise = rng.normal(0.0, 1.0, c.size)
    noise *= np.sqrt((c * c).mean() / (noise * noise).mean() / 10.0 ** (snr_db / 10.0))
    return np.clip(np.round(c + noise), -32768, 32767).astype(np.int16)


def mixed_lps(clean, noisy, fs, rng):
    """0.7 lps_clean + 0.3 lps_noisy + N(0, 0.3), float32"""
    lc, ln = spec64.analysis32(clean, fs)[0], spec64.analysis32(noisy, fs)[0]
    return (0.7 * lc + 0.3 * ln + rng.normal(0.0, 0.3, lc.shape)).astype(F32)


@functools.lru_cache(maxsize=None)
def batch(fs, snr_db):
    """(cleans, noisys, lps) of utterances of FRAMES frames; built once, never written to"""
    rng = np.random.default_rng(1000 * fs + int(snr_db) + 50)
    cleans = [spec64.synth_speech(n_samples(F, fs, extra=3 * i), fs, seed=fs + 7 * i) for i, F in enumerate(FRAMES)]
    noisys = [add_noise(c, snr_db, rng) for c in cleans]
    lps = [mixed_lps(c, n, fs, rng) for c, n in zip(cleans, noisys)]
    for a in cleans + noisys + lps:
        a.setflags(write=False)
    return cleans, noisys, lps


# ---- the float32 restatement
def quality32(clean, noisy, lps, fs, per_frame=False):
    """(segmental SNR, LSD) of tool_io::quality / spec64.quality64 with every step in float32; per_frame: the two
    float32 arrays [F] before the means"""
    L, S, N = spec64.params(fs)
    M, D = N // 2, N // 2 + 1
    F = min(spec64.n_frames(len(clean), fs), spec64.n_frames(len(noisy), fs))
    n = F * S + L - S
    clean, noisy = np.asarray(clean)[:n], np.asarray(noisy)[:n]
    _, cr, ci = spec64.analysis32(clean, fs)
    _, xr, xi = spec64.analysis32(noisy, fs)
    v = np.asarray(lps, F32)[:F]
    pc = cr * cr + ci * ci
    pd = np.where(v < F32(-50.0), F32(np.exp(-50.0)), np.exp(v.astype(np.float64)).astype(F32)).astype(F32)
    mag, A = np.sqrt(pd), np.sqrt(xr * xr + xi * xi)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = mag / np.where(A > 0, A, F32(1.0))
    yr = np.where(A > 0, xr * g, mag).astype(F32)
    yi = np.where(A > 0, xi * g, F32(0.0)).astype(F32)
    k = np.arange(M)                                                  # the inverse split and FFT of spec64.synthesis32
    ar, ai, br_, bi_ = yr[:, k], yi[:, k], yr[:, M - k], -yi[:, M - k]
    h = F32(0.5)
    er, ei, dr, di = (ar + br_) * h, (ai + bi_) * h, (ar - br_) * h, (ai - bi_) * h
    wx, wy = spec64.twiddle32(k, N)
    br, bi = wx * dr + wy * di, wx * di - wy * dr
    re, im = np.empty((F, M), F32), np.empty((F, M), F32)
    p = spec64.bitrev(k, int(np.log2(M)))
    re[:, p], im[:, p] = er - bi, -(ei + br)
    spec64.fft32(re, im, M, spec64.twiddle32(np.arange(M // 2), M))
    nn = np.arange(L)
    raw = np.where((nn & 1) == 1, -im[:, nn >> 1] * F32(1.0 / M), re[:, nn >> 1] * F32(1.0 / M)).astype(F32)
    cf = spec64.frames(clean, fs).astype(F32)
    e = (raw / spec64.window(L)).astype(F32) - cf
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = F32(10.0) * np.log10((cf * cf).sum(axis=1, dtype=F32) / (e * e).sum(axis=1, dtype=F32))
        snr = np.where(snr > F32(30.0), F32(30.0), np.where(snr < F32(-20.0), F32(-20.0), snr)).astype(F32)
        mc, md = F32(1e-5) * pc.max(), F32(1e-5) * pd.max()
        d = F32(10.0) * np.log10(np.maximum(pd, md) / np.maximum(pc, mc))
        lsd = np.sqrt((d * d).sum(axis=1, dtype=F32) / F32(D))
    if per_frame:
        return snr, lsd
    return float(snr.mean(dtype=F32)), float(lsd.mean(dtype=F32))


def check_case(name, got, cleans, noisys, lps, fs, counts=None, extra=0.0):
    """the GPU's (segsnr [n], lsd [n]) against quality64 with the model's bound; prints the case's row of the table"""
    want, model = [], []
    for u, (c, n, l) in enumerate(zip(cleans, noisys, lps)):
        if counts is not None:
            if counts[u] == 0:
                assert got[0][u] == 0.0 and got[1][u] == 0.0
                continue
            m = n_samples(counts[u], fs)
            c, n, l = c[:m], n[:m], l[:counts[u]]
        want.append(spec64.quality64(c, n, l, fs) + (u,))
        model.append(quality32(c, n, l, fs))
    for q, label in ((0, "segSNR"), (1, "LSD")):
        dm = max(abs(m[q] - w[q]) for m, w in zip(model, want))
        dg = max(abs(float(got[q][w[2]]) - w[q]) for w in want)
        print("score table | %-34s | %-6s | model %.3g dB | GPU %.3g dB" % (name, label, dm, dg))
        assert np.isfinite(dg) and dg <= MARGIN * dm + extra, (name, label, dm, dg)
    return want


# ---- accuracy at every rate
@pytest.mark.parametrize("snr_db", [20, 5, -5])
@pytest.mark.parametrize("fs", [8, 11, 16])
def test_a_batch_against_float64(pkg, fs, snr_db):
    cleans, noisys, lps = batch(fs, snr_db)
    got = pkg.score_waves(cleans, noisys, lps, fs_khz=fs)
    assert got[0].dtype == got[1].dtype == np.float32 and got[0].shape == got[1].shape == (len(FRAMES),)
    check_case("%d kHz, noise at %d dB" % (fs, snr_db), got, cleans, noisys, lps, fs)


# ---- clamps and floors
@pytest.mark.parametrize("fs", [8, 16])
def test_a_silent_clean_frame_is_minus_20_exactly(pkg, fs):
    """a one-frame utterance of digital silence: exactly -20; and an utterance whose third frame is silent: that frame
    enters the mean as -20 (float64 agrees within the model's bound)"""
    cleans, noisys, lps = batch(fs, 5)
    L, S, _ = spec64.params(fs)
    silent = np.zeros_like(cleans[0])
    holed = cleans[3].copy()
    holed[2 * S:2 * S + L] = 0
    cl, no, lp = [silent, holed], [noisys[0], noisys[3]], [lps[0], lps[3]]
    got = pkg.score_waves(cl, no, lp, fs_khz=fs)
    assert got[0][0] == F32(-20.0)
    assert quality32(silent, noisys[0], lps[0], fs)[0] == -20.0 == spec64.quality64(silent, noisys[0], lps[0], fs)[0]
    check_case("%d kHz, a silent clean frame" % fs, ([got[0][1]], [got[1][1]]), cl[1:], no[1:], lp[1:], fs)


@pytest.mark.parametrize("fs", [8, 11, 16])
def test_noisy_equal_to_clean_with_its_own_analysis_is_30_and_a_small_lsd(pkg, fs):
    cleans, _, _ = batch(fs, 5)
    lps = [spec64.analysis32(c, fs)[0] for c in cleans]
    got = pkg.score_waves(cleans, cleans, lps, fs_khz=fs)
    assert (got[0] == F32(30.0)).all()
    want = check_case("%d kHz, noisy = clean, own LPS" % fs, got, cleans, cleans, lps, fs)
    assert all(w[0] == 30.0 and w[1] < 1e-4 for w in want) and (got[1] < 1e-4).all()


@pytest.mark.parametrize("fs", [8, 16])
def test_rows_at_the_floor(pkg, fs):
    """lps = -60 everywhere: pd is exp(-50) on every bin and md 1e-5 of that"""
    cleans, noisys, _ = batch(fs, 20)
    lps = [np.full((F, spec64.params(fs)[2] // 2 + 1), -60.0, F32) for F in FRAMES]
    got = pkg.score_waves(cleans, noisys, lps, fs_khz=fs)
    check_case("%d kHz, rows at the floor" % fs, got, cleans, noisys, lps, fs)


def test_the_floor_is_the_utterance_s_own(pkg):
    """utterance A has one frame 50 times as loud as its others, so the 1e-5 floors engage on A's quiet frames; its
    neighbour B is 60 dB below A's loud frame, so a floor taken over the batch would raise every bin of B: B's numbers
    must be the bits of B alone"""
    fs = 16
    L, S, N = spec64.params(fs)
    rng = np.random.default_rng(77)
    base = spec64.synth_speech(n_samples(6, fs), fs, seed=31).astype(np.float64) * 0.08
    gain = np.ones(base.size)
    gain[3 * S:3 * S + L] = 50.0
    A = np.clip(np.round(base * gain), -32768, 32767).astype(np.int16)
    B = np.round(spec64.synth_speech(n_samples(4, fs), fs, seed=32) * 0.004).astype(np.int16)
    An, Bn = add_noise(A, 10, rng), add_noise(B, 10, rng)
    la, lb = mixed_lps(A, An, fs, rng), mixed_lps(B, Bn, fs, rng)
    pa, pb = np.exp(la.astype(np.float64)), np.exp(lb.astype(np.float64))
    assert (pa < 1e-5 * pa.max()).mean() > 0.05            # the floor engages inside A
    assert (pb < 1e-5 * pa.max()).all() and not (pb < 1e-5 * pb.max()).all()
    alone = pkg.score_waves([B], [Bn], [lb], fs_khz=fs)
    for cl, no, lp, at in (([A, B], [An, Bn], [la, lb], 1), ([B, A], [Bn, An], [lb, la], 0)):
        got = pkg.score_waves(cl, no, lp, fs_khz=fs)
        assert got[0][at] == alone[0][0] and got[1][at] == alone[1][0]
    got = pkg.score_waves([A, B], [An, Bn], [la, lb], fs_khz=fs)
    check_case("16 kHz, one loud frame", got, [A, B], [An, Bn], [la, lb], fs)


# ---- score_frames
@pytest.mark.parametrize("fs", [11, 16])
def test_score_frames(pkg, fs):
    cleans, noisys, lps = batch(fs, 5)
    full = pkg.score_waves(cleans, noisys, lps, fs_khz=fs)
    same = pkg.score_waves(cleans, noisys, lps, fs_khz=fs, score_frames=FRAMES)
    assert np.array_equal(full[0], same[0]) and np.array_equal(full[1], same[1])
    counts = [1, 0, 3, 8]
    got = pkg.score_waves(cleans, noisys, lps, fs_khz=fs, score_frames=counts)
    assert got[0][0] == full[0][0] and got[1][0] == full[1][0]          # 1 of 1: unchanged by the others' counts
    assert got[0][1] == 0.0 and got[1][1] == 0.0
    keep = [0, 2, 3]
    cut = pkg.score_waves([cleans[u][:n_samples(counts[u], fs)] for u in keep],
                          [noisys[u][:n_samples(counts[u], fs)] for u in keep],
                          [lps[u][:counts[u]] for u in keep], fs_khz=fs)
    assert np.array_equal(got[0][keep], cut[0]) and np.array_equal(got[1][keep], cut[1])
    assert got[0][3] != full[0][3]
    check_case("%d kHz, score_frames 1 0 3 8" % fs, got, cleans, noisys, lps, fs, counts=counts)
    # a clean wave shorter than its noisy wave: zero-padded by the wrapper, scored over its own frames
    short = [c[:n_samples(k, fs) + 5] if k else c for c, k in zip(cleans, counts)]
    got2 = pkg.score_waves(short, noisys, lps, fs_khz=fs, score_frames=counts)
    assert np.array_equal(got2[0], got[0]) and np.array_equal(got2[1], got[1])


# ---- independence and determinism
def test_an_utterance_s_numbers_do_not_depend_on_the_batch(pkg):
    fs = 16
    cleans, noisys, lps = batch(fs, 5)
    full = pkg.score_waves(cleans, noisys, lps, fs_khz=fs)
    again = pkg.score_waves(cleans, noisys, lps, fs_khz=fs)
    assert np.array_equal(full[0], again[0]) and np.array_equal(full[1], again[1])
    n = len(FRAMES)
    for u in range(n):
        alone = pkg.score_waves([cleans[u]], [noisys[u]], [lps[u]], fs_khz=fs)
        order = [u] + [v for v in range(n) if v != u]
        first = pkg.score_waves([cleans[v] for v in order], [noisys[v] for v in order], [lps[v] for v in order], fs_khz=fs)
        order = order[1:] + [u]
        last = pkg.score_waves([cleans[v] for v in order], [noisys[v] for v in order], [lps[v] for v in order], fs_khz=fs)
        for q in (0, 1):
            assert alone[q][0] == first[q][0] == last[q][n - 1] == full[q][u], (u, q)


# ---- the engine path
def small_net(rng, ctx=7, hidden=(40, 24), D=257):
    ls = [ctx * D, *hidden, D]
    ws = [rng.normal(0, 0.05, (ls[i], ls[i + 1])).astype(F32) for i in range(len(ls) - 1)]
    bs = [rng.normal(0, 0.1, ls[i + 1]).astype(F32) for i in range(len(ls) - 1)]
    return ls, ws, bs


def norm_stats(rng, D=257):
    return rng.normal(10, 2, D).astype(F32), (1.0 / rng.uniform(2, 4, D)).astype(F32)


def engine(pkg, ls, ws, bs, B, cap=0):
    return pkg.BPGpu(1, 0, ls, B, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0, max_cache_frames=cap)


def same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)


def test_engine_path_equals_the_stateless_path_at_any_chunking(pkg):
    """capacity 4 over frame offsets 0 1 3 8 17 cuts inside the utterances of 5 and 9 frames; 1000 holds the batch"""
    fs, ctx = 16, 7
    cleans, noisys, _ = batch(fs, 5)
    rng = np.random.default_rng(78)
    ls, ws, bs = small_net(rng, ctx=ctx)
    mean, inv = norm_stats(rng)
    counts = [1, 2, 0, 7]
    res = []
    for cap in (1000, 4):
        eng = engine(pkg, ls, ws, bs, 16, cap=cap)
        plain = eng.enhance_waves(noisys, mean, inv, fs_khz=fs, fea_context=ctx, return_f32=True, return_lps=True)
        assert len(plain) == 3
        out, outf, lps, segsnr, lsd = eng.enhance_waves(noisys, mean, inv, fs_khz=fs, fea_context=ctx, return_f32=True,
                                                        return_lps=True, cleans=cleans)
        for g, w in zip((out, outf, lps), plain):
            same(g, w)
        stateless = pkg.score_waves(cleans, noisys, lps, fs_khz=fs)
        assert np.array_equal(segsnr, stateless[0]) and np.array_equal(lsd, stateless[1])
        only = eng.enhance_waves(noisys, mean, inv, fs_khz=fs, cleans=cleans)       # no float wave, no LPS rows asked for
        same(only[0], out)
        assert len(only) == 3 and np.array_equal(only[1], segsnr) and np.array_equal(only[2], lsd)
        part = eng.enhance_waves(noisys, mean, inv, fs_khz=fs, cleans=cleans, score_frames=counts)
        want = pkg.score_waves(cleans, noisys, lps, fs_khz=fs, score_frames=counts)
        assert np.array_equal(part[1], want[0]) and np.array_equal(part[2], want[1]) and part[1][2] == 0.0
        same(eng.enhance_waves(noisys, mean, inv, fs_khz=fs), out)                   # and the plain call after it
        eng.close()
        res.append((segsnr, lsd, lps))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    check_case("16 kHz, engine path, net output", res[0][:2], cleans, noisys, res[0][2], fs)


def test_engine_path_argument_errors(pkg):
    fs, ctx = 16, 7
    cleans, noisys, _ = batch(fs, 5)
    rng = np.random.default_rng(79)
    ls, ws, bs = small_net(rng, ctx=ctx)
    mean, inv = norm_stats(rng)
    eng = engine(pkg, ls, ws, bs, 16)
    with pytest.raises(pkg.MlggdError, match=r"error 1: utterance 2: score_frames 6 is outside 0\.\.5"):
        eng.enhance_waves(noisys, mean, inv, fs_khz=fs, cleans=cleans, score_frames=[1, 2, 6, 9])
    with pytest.raises(pkg.MlggdError, match=r"error 1: utterance 0: score_frames -1"):
        eng.enhance_waves(noisys, mean, inv, fs_khz=fs, cleans=cleans, score_frames=[-1, 2, 5, 9])
    with pytest.raises(pkg.MlggdError, match=r"error 1: utterance 1: 511 samples is shorter than one frame"):
        eng.enhance_waves([noisys[0], noisys[1][:511]], mean, inv, fs_khz=fs, cleans=cleans[:2])
    assert eng.enhance_waves([], mean, inv, cleans=[])[0] == []
    eng.fake_world(2, allreduce=True)
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_enhance_waves_scored runs on a single-device engine"):
        eng.enhance_waves(noisys, mean, inv, fs_khz=fs, cleans=cleans)
    eng.close()


# ---- the tools
def write_wav(path, w, rate=16000):
    w = np.asarray(w, "<i2")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + 2 * w.size) + b"WAVEfmt " +
                struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16) + b"data" + struct.pack("<I", 2 * w.size) +
                w.tobytes())


def parse_info(text):
    lines = text.decode().split("\n")
    assert lines[0] == "Segmental SNR:" and lines[2] == "Log-Spectral Distortion:" and lines[4:] == [""]
    for v in (lines[1], lines[3]):
        assert len(v.split(".")[1]) == 6
    return float(lines[1]), float(lines[3])


def test_enhance_wav_score_device(pkg, tmp_path):
    """four lines, the second and the fourth scored, the fourth's clean wave three frames shorter than its noisy wave"""
    fs, ctx, B = 16, 7, 64
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    cleans, noisys, _ = batch(fs, 5)
    cleans = list(cleans[:3]) + [cleans[3][:n_samples(6, fs) + 11]]
    rng = np.random.default_rng(80)
    ls, ws, bs = small_net(rng, ctx=ctx)
    mean, inv = norm_stats(rng)
    hostlib.write_wts(str(tmp_path / "mlp.wts"), ws, bs)
    hostlib.write_norm(str(tmp_path / "n.norm"), mean, inv)
    scored = (1, 3)
    with open(tmp_path / "list.scp", "w") as f:
        for u in range(4):
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
        names = ["out%d.wav" % u for u in range(4)] + ["info%d.txt" % u for u in scored]
        files = {n: open(tmp_path / n, "rb").read() for n in names}
        assert not any((tmp_path / ("info%d.txt" % u)).exists() for u in range(4) if u not in scored)
        for n in names:
            os.remove(tmp_path / n)
        return r.stdout, files

    default, host_files = run([])
    host, host_files2 = run(["score=host"])
    assert default == host and host_files == host_files2 and "scored" not in host
    dev_out, dev_files = run(["score=device"])
    for u in range(4):
        assert dev_files["out%d.wav" % u] == host_files["out%d.wav" % u]
    assert dev_out.startswith(host) and dev_out[len(host):].startswith("scored 2 utterances: mean segmental SNR ")
    single, _ = run(["score=device", "batch_s=0"])
    assert single == dev_out
    eng = engine(pkg, ls, ws, bs, B)
    _, lps = eng.enhance_waves(noisys, mean, inv, fs_khz=fs, fea_context=ctx, return_lps=True)
    eng.close()
    got = [parse_info(dev_files["info%d.txt" % u]) for u in scored]
    hostv = [parse_info(host_files["info%d.txt" % u]) for u in scored]
    sel = lambda a: [a[u] for u in scored]
    want = check_case("16 kHz, enhance_wav score=device", ([g[0] for g in got], [g[1] for g in got]), sel(cleans),
                      sel(noisys), sel(lps), fs, extra=5e-7)
    for h, w in zip(hostv, want):                                     # the host report is the float64 value, printed
        assert abs(h[0] - w[0]) <= 1e-6 and abs(h[1] - w[1]) <= 1e-6
    mean_line = dev_out[len(host):].split()
    assert abs(float(mean_line[6]) - np.mean([g[0] for g in got])) < 1e-5
    assert abs(float(mean_line[10]) - np.mean([g[1] for g in got])) < 1e-5
