"""GPU: BPtrain_Sigmoid with MLGGD_ASYMMODEL=FILE and MLGGD_ASYMMETRY=FILE on the original project's 10-sentence sample
(tests/golden/tools_pfile*), run the way tests/test_gpu_shapefactors_exe.py runs the trainer: writing the fit changes
neither the weights file nor the log, a file of ones is the run without the variable, the fitted file -- read both as
a shape file and as a skew file -- trains the net that BPGpu trains on the same chunks under the same two vectors, and
a beta-norm run refuses the variable before it trains."""
import os
import re
import subprocess

import numpy as np
import pytest

import hostlib

pytestmark = pytest.mark.gpu
DIM, CTX, B, TOFF = 257, 3, 32, 1
LS = [DIM * CTX, 64, DIM]
HP = dict(lrate=0.1, momentum=0.9, weightcost=1e-5)
BETA = 1.2
EXE = os.path.join(hostlib.HOST, "BPtrain_Sigmoid")


def run(cwd, kv, **env):
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([EXE] + ["%s=%s" % (k, v) for k, v in kv.items()], capture_output=True, text=True, timeout=300,
                          cwd=cwd, env=dict(os.environ, **env))


def wts(d, name):
    return open(d / name / "mlp.wts", "rb").read()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the sample pfiles, initial weights, the command line, and the two runs that the tests compare with (no variable;
    MLGGD_ASYMMODEL with a short grid), made once"""
    d = tmp_path_factory.mktemp("asym_exe")
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    sample = hostlib.sample_pfiles(d / "tools_pfile")
    rng = np.random.default_rng(5)
    ws = [rng.normal(0, 0.05, (LS[i], LS[i + 1])).astype(np.float32) for i in range(2)]
    bs = [rng.normal(0, 0.1, LS[i + 1]).astype(np.float32) for i in range(2)]
    hostlib.write_wts(str(d / "init.wts"), ws, bs)
    kv = dict(gpu_used=0, numlayers=3, layersizes=",".join(map(str, LS)), bunchsize=B, MLflag=1, shapefactor=BETA,
              fea_dim=DIM, fea_context=CTX, traincache=500, init_randem_seed=27870775, targ_offset=TOFF,
              initwts_file=d / "init.wts", norm_file=os.path.join(sample, "train_noisy.norm"),
              fea_file=os.path.join(sample, "train_noisy.pfile"), targ_file=os.path.join(sample, "train_clean.pfile"),
              outwts_file="mlp.wts", log_file="mlp.log", train_sent_range="0-7", cv_sent_range="8-9", dropoutflag=0,
              visible_omit=0.1, hid_omit=0.1, **HP)
    plain = run(d / "plain", kv)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    fitted = run(d / "fitted", kv, MLGGD_ASYMMODEL=str(d / "fit.txt"), MLGGD_ERRMODEL_BETAS="0.6:0.2:2.0")
    assert fitted.returncode == 0, fitted.stdout + fitted.stderr
    return d, kv, plain, fitted


def log_of(path):
    """the log with the one wall-clock figure it holds masked"""
    return re.sub(r"Total cost time: [\d.]+ s\.", "Total cost time: T s.", open(path).read())


def test_writing_the_fit_leaves_the_weights_and_the_log(pkg, runs):
    d, kv, plain, fitted = runs
    assert "asymmetr" not in plain.stderr and "asymmetric error model" not in plain.stdout
    assert "asymmetric error model: %s written" % (d / "fit.txt") in fitted.stdout
    assert wts(d, "fitted") == wts(d, "plain") and len(wts(d, "plain")) > 4 * LS[0] * LS[1]
    assert log_of(d / "fitted" / "mlp.log") == log_of(d / "plain" / "mlp.log")
    assert "CV2 over. CV log likelihood" in log_of(d / "fitted" / "mlp.log")
    kap = pkg.read_asymmetry(str(d / "fit.txt"), DIM)
    bet = pkg.read_shapefactors(str(d / "fit.txt"), DIM, BETA)
    assert kap.shape == bet.shape == (DIM,) and np.isfinite(kap).all() and (kap > 0).all()
    assert len(set(kap.tolist())) > DIM // 2 and len(set(bet.tolist())) > 1
    grid = (0.6 + 0.2 * np.arange(8)).astype(np.float32)
    assert set(bet.tolist()) <= set(grid.tolist())


def test_a_file_of_ones_is_the_run_without_the_variable(runs):
    d, kv, plain, _ = runs
    (d / "ones.txt").write_text("\n".join(["1"] * DIM) + "\n")
    res = run(d / "ones", kv, MLGGD_ASYMMETRY=str(d / "ones.txt"))
    assert res.returncode == 0, res.stdout + res.stderr
    assert wts(d, "ones") == wts(d, "plain")
    line = [l for l in res.stderr.splitlines() if l.startswith("asymmetry:")]
    assert len(line) == 1 and str(d / "ones.txt") in line[0] and "min 1 max 1 mean 1" in line[0]


def test_the_fitted_file_is_the_net_the_python_engine_trains(pkg, runs):
    """... on the same chunks: the trainer's own host IO gives the chunk order and the rows, BPGpu the steps, both under
    the shape and the skew vector read from the one fitted file"""
    d, kv, plain, _ = runs
    fit = str(d / "fit.txt")
    res = run(d / "next", kv, MLGGD_SHAPEFACTORS=fit, MLGGD_ASYMMETRY=fit)
    assert res.returncode == 0, res.stdout + res.stderr
    assert wts(d, "next") != wts(d, "plain")
    io = hostlib.HostIO(**dict(kv, log_file=d / "io.log", outwts_file=d / "io.wts"))
    w0, b0 = hostlib.read_wts(str(d / "init.wts"), LS)
    eng = pkg.BPGpu(1, 0, LS, B, HP["lrate"], HP["momentum"], HP["weightcost"], w0, b0, BETA, 1)
    try:
        eng.set_shapefactors(pkg.read_shapefactors(fit, DIM, BETA))
        eng.set_asymmetry(pkg.read_asymmetry(fit, DIM))
        starts, _ = io.plan(kv["train_sent_range"])
        order = io.shuffle(len(starts))
        assert len(starts) >= 3
        for ci in order:
            inp, tg = io.read_chunk(ci, LS[0], DIM, 600)
            eng.train(inp, tg)
        we, be = eng.returnWeights()
    finally:
        io.close()
        eng.close()
    ws, bs = hostlib.read_wts(str(d / "next" / "mlp.wts"), LS)
    for l in range(2):
        assert np.array_equal(ws[l].view(np.uint32), we[l].view(np.uint32)), l
        assert np.array_equal(bs[l].view(np.uint32), be[l].view(np.uint32)), l


def test_a_beta_norm_run_refuses_the_variable_before_training(runs):
    d, kv, _, _ = runs
    (d / "ones.txt").write_text("\n".join(["1"] * DIM) + "\n")
    res = run(d / "mmse", dict(kv, MLflag=0, shapefactor=2.0), MLGGD_ASYMMETRY=str(d / "ones.txt"))
    assert res.returncode != 0 and "MLGGD_ASYMMETRY" in res.stderr
    assert "Starting chunk" not in open(d / "mmse" / "mlp.log").read()
    assert os.path.getsize(d / "mmse" / "mlp.wts") == 0
    (d / "short.txt").write_text("1 1.5 2\n")
    res = run(d / "short", kv, MLGGD_ASYMMETRY=str(d / "short.txt"))
    assert res.returncode != 0 and "MLGGD_ASYMMETRY" in res.stderr and "line 1" in res.stderr
