"""GPU: BPtrain_Sigmoid with MLGGD_ERRMODEL=FILE.  The opt-in second pass over the CV chunks changes neither the weights
file nor the log, and the file it writes is pkg.ggd_fit of BPGpu.error_stats_frames over the same CV samples (read
through the trainer's own host IO, summed chunk by chunk as the trainer does) to the 9 printed digits -- on the
frame-stream path and with MLGGD_EXPANDED=1."""
import os
import re
import subprocess

import numpy as np
import pytest

import ggd64
import hostlib

pytestmark = pytest.mark.gpu
DIM, CTX, B, TOFF = 20, 5, 16, 2
LS = [DIM * CTX, 48, 40, DIM]
EXE = os.path.join(hostlib.HOST, "BPtrain_Sigmoid")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """a tiny synthetic pfile pair, norm file and initial weights; kv: the finetune.pl-style command line"""
    d = tmp_path_factory.mktemp("errmodel")
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    rng = np.random.default_rng(31)
    lens = [int(x) for x in rng.integers(30, 90, 24)]
    nfr = sum(lens)
    noisy = rng.normal(3, 2, (nfr, DIM)).astype(np.float32)
    clean = (0.6 * noisy + rng.laplace(0, 1, (nfr, DIM))).astype(np.float32)
    hostlib.write_pfile(str(d / "n.pfile"), lens, noisy)
    hostlib.write_pfile(str(d / "c.pfile"), lens, clean)
    hostlib.write_norm(str(d / "n.norm"), noisy.mean(0), 1.0 / noisy.std(0))
    ws = [rng.normal(0, 0.1, (LS[i], LS[i + 1])).astype(np.float32) for i in range(3)]
    bs = [rng.normal(0, 0.1, LS[i + 1]).astype(np.float32) for i in range(3)]
    hostlib.write_wts(str(d / "init.wts"), ws, bs)
    kv = dict(gpu_used=0, numlayers=4, layersizes=",".join(map(str, LS)), bunchsize=B, MLflag=1, shapefactor=1.2,
              momentum=0.9, weightcost=1e-5, lrate=0.1, fea_dim=DIM, fea_context=CTX, traincache=300,
              init_randem_seed=27870775, targ_offset=TOFF, initwts_file=d / "init.wts", norm_file=d / "n.norm",
              fea_file=d / "n.pfile", targ_file=d / "c.pfile", outwts_file="mlp.wts", log_file="mlp.log",
              train_sent_range="0-13", cv_sent_range="14-23", dropoutflag=0, visible_omit=0.1, hid_omit=0.1)
    return d, kv


def run(cwd, kv, **env):
    """one epoch in the directory cwd (the output names are relative, so the logs of two runs can be compared)"""
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([EXE] + ["%s=%s" % (k, v) for k, v in kv.items()], capture_output=True, text=True, timeout=300,
                          cwd=cwd, env=dict(os.environ, **env))


def log_of(path):
    """the log with the one wall-clock figure it holds masked"""
    return re.sub(r"Total cost time: [\d.]+ s\.", "Total cost time: T s.", open(path).read())


def parse(path):
    head, rows = {}, []
    for line in open(path):
        if line.startswith("#"):
            w = line[1:].split()
            if w and w[0] in ("n", "D", "betas", "shared_beta", "loglik_per_frame"):
                head[w[0]] = w[1:]
        else:
            rows.append(line.split())
    return head, rows


@pytest.mark.parametrize("expanded,grid", [(False, None), (True, "0.6:0.2:2.0")])
def test_the_file_is_the_fit_of_the_cv_set_and_nothing_else_changes(pkg, data, tmp_path, expanded, grid):
    d, kv = data
    env = {"MLGGD_EXPANDED": "1"} if expanded else {}
    plain = run(tmp_path / "plain", kv, **env)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    assert "error model" not in plain.stdout
    env_model = dict(env, MLGGD_ERRMODEL=str(tmp_path / "cv.errmodel"))
    if grid:
        env_model["MLGGD_ERRMODEL_BETAS"] = grid
    res = run(tmp_path / "model", kv, **env_model)
    assert res.returncode == 0, res.stdout + res.stderr
    # neither the weights nor the log know about the second pass
    assert open(tmp_path / "model" / "mlp.wts", "rb").read() == open(tmp_path / "plain" / "mlp.wts", "rb").read()
    assert log_of(tmp_path / "model" / "mlp.log") == log_of(tmp_path / "plain" / "mlp.log")
    assert "CV2 over. CV log likelihood" in log_of(tmp_path / "model" / "mlp.log")

    # the same statistics from Python: the trainer's host IO for the CV samples, the trained weights, the same bunchsize
    betas = ggd64.grid(*map(float, grid.split(":"))) if grid else ggd64.grid()
    assert betas.size == (8 if grid else 21)
    io = hostlib.HostIO(**dict(kv, log_file=tmp_path / "io.log", outwts_file=tmp_path / "io.wts"))
    cvs, cvtotal = io.plan(kv["cv_sent_range"], cv=True)
    assert len(cvs) >= 2                                             # the trainer has chunks to add
    ws, bs = hostlib.read_wts(str(tmp_path / "model" / "mlp.wts"), LS)
    eng = pkg.BPGpu(1, 0, LS, B, 0.1, 0.9, 1e-5, ws, bs, 1.2, 1)
    total, n = np.zeros((4 + betas.size, DIM)), 0
    for ci in range(len(cvs)):
        feat, targ, first = io.read_chunk_frames(ci, DIM, DIM, 4000, 4000, cv=True)
        total += eng.error_stats_frames(feat, targ, first, CTX, TOFF, betas)
        n += first.size
    io.close()
    eng.close()
    assert n == cvtotal
    fit = pkg.ggd_fit(n, total, betas)

    head, rows = parse(tmp_path / "cv.errmodel")
    g9 = lambda x: "%.9g" % x
    assert head["n"] == [str(n)] and head["D"] == [str(DIM)]
    assert head["betas"] == [g9(b) for b in betas]
    assert head["shared_beta"] == [g9(betas[fit.best_shared])]
    assert head["loglik_per_frame"] == [g9(v / n) for v in fit.loglik_shared]
    assert len(rows) == DIM
    for dd, row in enumerate(rows):
        k = int(fit.best[dd])
        assert row == [str(dd), g9(fit.mean[dd]), g9(fit.var[dd]), g9(fit.kurt[dd]), g9(betas[k]), g9(fit.alpha[k, dd]),
                       g9(fit.alpha[fit.best_shared, dd])], dd
    line = [l for l in res.stdout.splitlines() if l.startswith("error model:")]
    assert len(line) == 1 and str(tmp_path / "cv.errmodel") in line[0]
    assert "shared beta %s" % g9(betas[fit.best_shared]) in line[0]
    assert res.stdout.index("cur_chunk_samples") < res.stdout.index("error model:") < res.stdout.index("all finish!")


def test_a_bad_grid_and_a_dropout_run(data, tmp_path):
    d, kv = data
    # more than 32 shapes, a malformed grid: the run ends before the epoch and the message names the variable
    for spec in ("0.1:0.01:2.0", "0.5:0.1", "0:0.1:1", "1:0:2"):
        res = run(tmp_path / "bad", kv, MLGGD_ERRMODEL=str(tmp_path / "bad.errmodel"), MLGGD_ERRMODEL_BETAS=spec)
        assert res.returncode == 1 and "MLGGD_ERRMODEL_BETAS=" + spec in res.stderr, (spec, res.stderr)
        assert os.path.getsize(tmp_path / "bad" / "mlp.wts") == 0 and not os.path.exists(tmp_path / "bad.errmodel")
        assert "MLGGD_ERRMODEL_BETAS=" + spec in open(tmp_path / "bad" / "mlp.log").read()   # like every error of the trainer
    # 32 shapes are accepted (checked on the dropout run, which needs no fit); dropout: said so, and the run carries on
    res = run(tmp_path / "drop", dict(kv, dropoutflag=1), MLGGD_ERRMODEL=str(tmp_path / "drop.errmodel"),
              MLGGD_ERRMODEL_BETAS="0.5:0.05:2.05")
    assert res.returncode == 0, res.stdout + res.stderr
    assert "error model: not available with dropoutflag != 0" in res.stdout and "all finish!" in res.stdout
    assert os.path.getsize(tmp_path / "drop" / "mlp.wts") > 0 and not os.path.exists(tmp_path / "drop.errmodel")
