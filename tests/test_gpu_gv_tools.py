"""GPU: the tools of global variance equalisation.  BPtrain_Sigmoid with MLGGD_GVFILE=FILE on the original project's
10-sentence sample (tests/golden/tools_pfile*): the opt-in pass over the CV chunks changes neither the weights file nor
the log, and the file it writes holds pkg.gv_fit of BPGpu.output_stats_frames over the same CV rows (read through the
trainer's own host IO, summed chunk by chunk as the trainer does), parsed back through pkg.read_gv.  enhance_wav
gv=FILE writes the bytes of BPGpu.enhance_wave with those factors in single, scp= and live= modes, gv_mode=shared those
of the shared factor, and a malformed file ends the run with its path and line; enhance_lps gv=FILE writes the
equalised rows."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import gv64
import hostlib
import spec64

pytestmark = pytest.mark.gpu
DIM, CTX, B, TOFF = 257, 3, 32, 1
LS = [DIM * CTX, 64, DIM]
HP = dict(lrate=0.1, momentum=0.9, weightcost=1e-5)
EXE = os.path.join(hostlib.HOST, "BPtrain_Sigmoid")


def run_trainer(cwd, kv, **env):
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([EXE] + ["%s=%s" % (k, v) for k, v in kv.items()], capture_output=True, text=True, timeout=300,
                          cwd=cwd, env=dict(os.environ, **env))


def log_of(path):
    return re.sub(r"Total cost time: [\d.]+ s\.", "Total cost time: T s.", open(path).read())


def parse(path):
    head, rows = {}, []
    for line in open(path):
        if line.startswith("#"):
            w = line[1:].split()
            if w and w[0] in ("n", "D", "shared_eta", "gv_ref_shared", "gv_est_shared"):
                head[w[0]] = w[1]
        else:
            rows.append(line.split())
    return head, rows


@pytest.fixture(scope="module")
def trained(tmp_path_factory):
    """the sample pfiles, initial weights, the command line; one epoch without the variable and one with it"""
    d = tmp_path_factory.mktemp("gv_tools")
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    sample = hostlib.sample_pfiles(d / "tools_pfile")
    rng = np.random.default_rng(5)
    ws = [rng.normal(0, 0.05, (LS[i], LS[i + 1])).astype(np.float32) for i in range(2)]
    bs = [rng.normal(0, 0.1, LS[i + 1]).astype(np.float32) for i in range(2)]
    hostlib.write_wts(str(d / "init.wts"), ws, bs)
    kv = dict(gpu_used=0, numlayers=3, layersizes=",".join(map(str, LS)), bunchsize=B, MLflag=1, shapefactor=1.2,
              fea_dim=DIM, fea_context=CTX, traincache=500, init_randem_seed=27870775, targ_offset=TOFF,
              initwts_file=d / "init.wts", norm_file=os.path.join(sample, "train_noisy.norm"),
              fea_file=os.path.join(sample, "train_noisy.pfile"), targ_file=os.path.join(sample, "train_clean.pfile"),
              outwts_file="mlp.wts", log_file="mlp.log", train_sent_range="0-7", cv_sent_range="8-9", dropoutflag=0,
              visible_omit=0.1, hid_omit=0.1, **HP)
    plain = run_trainer(d / "plain", kv)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    gv = run_trainer(d / "gv", kv, MLGGD_GVFILE=str(d / "gv.txt"))
    assert gv.returncode == 0, gv.stdout + gv.stderr
    return d, kv, plain, gv, sample


def test_the_file_is_the_fit_of_the_cv_set_and_nothing_else_changes(pkg, trained):
    d, kv, plain, res, _ = trained
    assert "global variance" not in plain.stdout
    assert open(d / "gv" / "mlp.wts", "rb").read() == open(d / "plain" / "mlp.wts", "rb").read()
    assert os.path.getsize(d / "gv" / "mlp.wts") > 4 * LS[0] * LS[1]
    assert log_of(d / "gv" / "mlp.log") == log_of(d / "plain" / "mlp.log")
    assert "CV2 over. CV log likelihood" in log_of(d / "gv" / "mlp.log")

    io = hostlib.HostIO(**dict(kv, log_file=d / "io.log", outwts_file=d / "io.wts"))
    cvs, cvtotal = io.plan(kv["cv_sent_range"], cv=True)
    ws, bs = hostlib.read_wts(str(d / "gv" / "mlp.wts"), LS)
    eng = pkg.BPGpu(1, 0, LS, B, HP["lrate"], HP["momentum"], HP["weightcost"], ws, bs, 1.2, 1)
    total, n = np.zeros((4, DIM)), 0
    for ci in range(len(cvs)):
        feat, targ, first = io.read_chunk_frames(ci, DIM, DIM, 4000, 4000, cv=True)
        total += eng.output_stats_frames(feat, targ, first, CTX, TOFF)
        n += first.size
    io.close()
    eng.close()
    assert n == cvtotal and n > 0
    fit = pkg.gv_fit(n, total)
    assert fit.fitted.all() and fit.fitted_shared

    path = str(d / "gv.txt")
    assert pkg.read_gv(path, DIM).tobytes() == fit.eta.tobytes()
    assert pkg.read_gv(path, DIM, shared=True).tobytes() == np.full(DIM, fit.eta_shared, np.float32).tobytes()
    head, rows = parse(path)
    assert head["n"] == str(n) and head["D"] == str(DIM)
    assert np.float32(head["shared_eta"]) == fit.eta_shared
    assert float(head["gv_ref_shared"]) == fit.gv_ref_shared and float(head["gv_est_shared"]) == fit.gv_est_shared
    assert len(rows) == DIM
    for dd, row in enumerate(rows):
        assert row[0] == str(dd) and len(row) == 4
        assert float(row[1]) == fit.gv_ref[dd] and float(row[2]) == fit.gv_est[dd] and np.float32(row[3]) == fit.eta[dd]
    line = [l for l in res.stdout.splitlines() if l.startswith("global variance:")]
    assert len(line) == 1 and path in line[0] and "%d CV samples" % n in line[0]
    assert "shared eta %.9g" % fit.eta_shared in line[0]
    assert res.stdout.index("cur_chunk_samples") < res.stdout.index("global variance:") < res.stdout.index("all finish!")


def test_both_files_in_one_run_the_expanded_path_and_a_dropout_run(pkg, trained):
    d, kv, _, _, _ = trained
    res = run_trainer(d / "both", kv, MLGGD_GVFILE=str(d / "both.gv"), MLGGD_ERRMODEL=str(d / "both.errmodel"),
                      MLGGD_EXPANDED="1")
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.index("error model:") < res.stdout.index("global variance:") < res.stdout.index("all finish!")
    assert os.path.getsize(d / "both.errmodel") > 0
    # the expanded entry forms the same statistics from the same rows
    assert pkg.read_gv(str(d / "both.gv"), DIM).tobytes() == pkg.read_gv(str(d / "gv.txt"), DIM).tobytes()
    assert open(d / "both" / "mlp.wts", "rb").read() == open(d / "plain" / "mlp.wts", "rb").read()
    res = run_trainer(d / "drop", dict(kv, dropoutflag=1), MLGGD_GVFILE=str(d / "drop.gv"))
    assert res.returncode == 0, res.stdout + res.stderr
    assert "MLGGD_GVFILE is not available with dropoutflag != 0" in res.stdout and "all finish!" in res.stdout
    assert os.path.getsize(d / "drop" / "mlp.wts") > 0 and not os.path.exists(d / "drop.gv")


# ---- the decoders
def write_wav(path, w, rate):
    w = np.asarray(w, "<i2")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + 2 * w.size) + b"WAVEfmt " +
                struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16) + b"data" + struct.pack("<I", 2 * w.size) +
                w.tobytes())


def read_wav(path):
    d = open(path, "rb").read()
    assert d[:4] == b"RIFF" and d[8:16] == b"WAVEfmt " and d[36:40] == b"data"
    return np.frombuffer(d[44:], "<i2").astype(np.int16)


def test_enhance_wav_with_a_gv_file(pkg, trained, tmp_path):
    d, kv, _, _, sample = trained
    wts, norm, gvf = str(d / "gv" / "mlp.wts"), os.path.join(sample, "train_noisy.norm"), str(d / "gv.txt")
    ws, bs = hostlib.read_wts(wts, LS)
    mean, inv = (np.asarray(v, np.float32) for v in hostlib.HostNorm.read(norm, DIM))
    waves = [spec64.synth_speech(3000 + 777 * i, 16, seed=40 + i) for i in range(3)]
    for i, w in enumerate(waves):
        write_wav(tmp_path / ("n%d.wav" % i), w, 16000)
    common = [os.path.join(hostlib.HOST, "enhance_wav"), "wts=" + wts, "norm_file=" + norm, "fea_context=%d" % CTX,
              "bunchsize=%d" % B]

    def tool(tag, extra, single=False):
        os.makedirs(tmp_path / tag)
        if single:
            args = ["in=%s" % (tmp_path / "n0.wav"), "out=%s" % (tmp_path / tag / "e0.wav")]
        else:
            with open(tmp_path / tag / "list.scp", "w") as f:
                for i in range(3):
                    f.write("%s %s\n" % (tmp_path / ("n%d.wav" % i), tmp_path / tag / ("e%d.wav" % i)))
            args = ["scp=%s" % (tmp_path / tag / "list.scp")]
        r = subprocess.run(common + args + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return [read_wav(tmp_path / tag / ("e%d.wav" % i)) for i in range(1 if single else 3)]

    eng = pkg.BPGpu(1, 0, LS, B, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    dec = lambda: [eng.enhance_wave(w, mean, inv, fea_context=CTX) for w in waves]
    off = dec()
    eng.set_gv(pkg.read_gv(gvf, DIM))
    per_bin = dec()
    eng.set_gv(pkg.read_gv(gvf, DIM, shared=True))
    shared = dec()
    eng.close()
    assert all(a.tobytes() != b.tobytes() for a, b in zip(off, per_bin))
    assert all(a.tobytes() != b.tobytes() for a, b in zip(shared, per_bin))

    same = lambda got, want: all(g.tobytes() == w.tobytes() for g, w in zip(got, want)) and len(got) <= len(want)
    assert same(tool("off", []), off)
    assert same(tool("single", ["gv=" + gvf], single=True), per_bin)
    assert same(tool("scp", ["gv=" + gvf, "gv_mode=bin"]), per_bin)
    assert same(tool("line", ["gv=" + gvf, "batch_s=0"]), per_bin)
    assert same(tool("live", ["gv=" + gvf, "live=200", "sessions=2"]), per_bin)
    assert same(tool("shared", ["gv=" + gvf, "gv_mode=shared"]), shared)
    assert same(tool("sharedlive", ["gv=" + gvf, "gv_mode=shared", "live=1000"]), shared)

    # a malformed file, a bad mode: the run ends before a wave is written
    bad = tmp_path / "bad.txt"
    lines = open(gvf).read().splitlines()
    row = next(i for i, l in enumerate(lines) if l.startswith("5 "))
    lines[row] = "5 1 1 -3"
    bad.write_text("\n".join(lines) + "\n")
    for extra, msg in ((["gv=%s" % bad], "%s line %d: eta -3 of bin 5" % (bad, row + 1)),
                       (["gv=%s" % (tmp_path / "none.txt")], "%s line 1: cannot read" % (tmp_path / "none.txt")),
                       (["gv=" + gvf, "gv_mode=both"], "gv_mode=both")):
        out = tmp_path / "never.wav"
        r = subprocess.run(common + ["in=%s" % (tmp_path / "n0.wav"), "out=%s" % out] + extra, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 1 and msg in r.stderr and not os.path.exists(out), r.stderr


def test_the_device_report_is_the_one_of_the_equalised_rows(pkg, trained, tmp_path):
    """score=device stoi=1 gv=FILE: the info file holds the scores enhance_waves(cleans=...) returns with the factors set"""
    d, kv, _, _, sample = trained
    wts, norm, gvf = str(d / "gv" / "mlp.wts"), os.path.join(sample, "train_noisy.norm"), str(d / "gv.txt")
    ws, bs = hostlib.read_wts(wts, LS)
    mean, inv = (np.asarray(v, np.float32) for v in hostlib.HostNorm.read(norm, DIM))
    noisy, clean = spec64.synth_speech(9000, 16, seed=50), spec64.synth_speech(9000, 16, seed=51)
    write_wav(tmp_path / "n.wav", noisy, 16000), write_wav(tmp_path / "c.wav", clean, 16000)
    common = [os.path.join(hostlib.HOST, "enhance_wav"), "wts=" + wts, "norm_file=" + norm, "fea_context=%d" % CTX,
              "bunchsize=%d" % B, "in=%s" % (tmp_path / "n.wav"), "clean=%s" % (tmp_path / "c.wav")]
    infos = {}
    for tag, extra in (("off", []), ("gv", ["gv=" + gvf])):
        for score in ("device", "host"):
            r = subprocess.run(common + ["out=%s" % (tmp_path / (tag + score + ".wav")),
                                         "info=%s" % (tmp_path / (tag + score + ".info")), "score=" + score] +
                               (["stoi=1"] if score == "device" else []) + extra, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            infos[tag, score] = open(tmp_path / (tag + score + ".info")).read()
        assert open(tmp_path / (tag + "device.wav"), "rb").read() == open(tmp_path / (tag + "host.wav"), "rb").read()
    assert infos["gv", "device"] != infos["off", "device"] and infos["gv", "host"] != infos["off", "host"]
    eng = pkg.BPGpu(1, 0, LS, B, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    eng.set_gv(pkg.read_gv(gvf, DIM))
    out, segsnr, lsd = eng.enhance_waves([noisy], mean, inv, fs_khz=16, fea_context=CTX, cleans=[clean])
    eng.close()
    assert read_wav(tmp_path / "gvdevice.wav").tobytes() == out[0].tobytes()
    # the tool writes the two scores as the engine returned them; its own run without factors wrote other ones
    r = subprocess.run(common + ["out=%s" % (tmp_path / "again.wav"), "info=%s" % (tmp_path / "again.info"), "score=device",
                                 "gv=" + gvf], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and open(tmp_path / "again.info").read() == infos["gv", "device"]
    assert infos["gv", "device"] == "Segmental SNR:\n%f\nLog-Spectral Distortion:\n%f\n" % (segsnr[0], lsd[0])


def test_enhance_lps_with_a_gv_file(pkg, trained, tmp_path):
    d, kv, _, _, sample = trained
    wts, norm, gvf = str(d / "gv" / "mlp.wts"), os.path.join(sample, "train_noisy.norm"), str(d / "gv.txt")
    ws, bs = hostlib.read_wts(wts, LS)
    mean, inv = (np.asarray(v, np.float32) for v in hostlib.HostNorm.read(norm, DIM))
    lps = pkg.wave_to_lps(spec64.synth_speech(5000, 16, seed=60), fs_khz=16)
    F = lps.shape[0]
    with open(tmp_path / "in.lps", "wb") as f:
        f.write(struct.pack(">iihh", F, 160000, 4 * DIM, 9) + lps.astype(">f4").tobytes())
    common = [os.path.join(hostlib.HOST, "enhance_lps"), "wts=" + wts, "norm_file=" + norm, "fea_context=%d" % CTX,
              "bunchsize=%d" % B, "in=%s" % (tmp_path / "in.lps")]
    rows = {}
    for tag, extra in (("off", []), ("bin", ["gv=" + gvf]), ("shared", ["gv=" + gvf, "gv_mode=shared"])):
        r = subprocess.run(common + ["out=%s" % (tmp_path / (tag + ".htk"))] + extra, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        rows[tag] = np.frombuffer(open(tmp_path / (tag + ".htk"), "rb").read()[12:], ">f4").reshape(F, DIM).astype(np.float32)
    eng = pkg.BPGpu(1, 0, LS, B, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    x = ((lps - mean) * inv).astype(np.float32)
    y = eng.forward_frames(x[np.clip(np.arange(F + 2) - 1, 0, F - 1)], np.arange(F, dtype=np.int32), CTX)
    eng.close()
    assert rows["off"].tobytes() == gv64.apply32(y, None, inv, mean).tobytes()
    assert rows["bin"].tobytes() == gv64.apply32(y, pkg.read_gv(gvf, DIM), inv, mean).tobytes()
    assert rows["shared"].tobytes() == gv64.apply32(y, pkg.read_gv(gvf, DIM, shared=True), inv, mean).tobytes()
    r = subprocess.run(common + ["out=%s" % (tmp_path / "x.htk"), "gv=%s" % (tmp_path / "none.txt")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 1 and "none.txt line 1" in r.stderr
