"""GPU: BPtrain_Sigmoid with MLGGD_SHAPEFACTORS=FILE on the original project's 10-sentence sample (tests/golden/
tools_pfile*), run the way tests/test_gpu_error_model_file.py runs the trainer: a uniform file is the run without the
variable, a mixed file is the net that BPGpu.set_shapefactors trains on the same chunks, the file MLGGD_ERRMODEL
writes is accepted by the next epoch, and a beta-norm run refuses the variable before it trains."""
import os
import re
import subprocess

import numpy as np
import pytest

import hostlib
import shapes64 as s6

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
    """the sample pfiles, initial weights, the command line, the three shape files, and the two runs that several tests
    compare with (no variable; the mixed file), made once"""
    d = tmp_path_factory.mktemp("shapes_exe")
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
    (d / "uniform.txt").write_text("\n".join(["%.9g" % np.float32(BETA)] * DIM) + "\n")
    (d / "mixed.txt").write_text(" ".join("%.9g" % v for v in s6.mixed(DIM)) + "\n")
    plain = run(d / "plain", kv)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    mixed = run(d / "mixed", kv, MLGGD_SHAPEFACTORS=str(d / "mixed.txt"))
    assert mixed.returncode == 0, mixed.stdout + mixed.stderr
    return d, kv, plain, mixed


def test_a_uniform_file_is_the_run_without_the_variable(runs):
    d, kv, plain, _ = runs
    assert "shape factors" not in plain.stderr
    res = run(d / "uniform", kv, MLGGD_SHAPEFACTORS=str(d / "uniform.txt"))
    assert res.returncode == 0, res.stdout + res.stderr
    assert wts(d, "uniform") == wts(d, "plain") and len(wts(d, "plain")) > 4 * LS[0] * LS[1]
    g9 = "%.9g" % np.float32(BETA)
    line = [l for l in res.stderr.splitlines() if l.startswith("shape factors:")]
    assert len(line) == 1 and str(d / "uniform.txt") in line[0]
    assert "min %s max %s mean %s" % (g9, g9, g9) in line[0]


def test_a_mixed_file_is_the_net_set_shapefactors_trains(pkg, runs):
    """... on the same chunks: the trainer's own host IO gives the chunk order and the rows, BPGpu the steps"""
    d, kv, plain, mixed = runs
    assert wts(d, "mixed") != wts(d, "plain")
    assert "min 0.600000024 max 2 " in mixed.stderr
    log = open(d / "mixed" / "mlp.log").read()
    for pat in (r"^CV over\. squared error: -?[\d.]+$", r"^CV over\. square root squared error: -?[\d.]+$",
                r"^CV2 over\. CV log likelihood: -?[\d.]+$"):
        assert re.search(pat, log, re.M), pat                     # the log lines keep their form
    ll = lambda p: re.search(r"CV log likelihood: (-?[\d.]+)", open(p).read()).group(1)
    assert ll(d / "mixed" / "mlp.log") != ll(d / "plain" / "mlp.log")     # ... and carry the vector's value
    io = hostlib.HostIO(**dict(kv, log_file=d / "io.log", outwts_file=d / "io.wts"))
    w0, b0 = hostlib.read_wts(str(d / "init.wts"), LS)
    eng = pkg.BPGpu(1, 0, LS, B, HP["lrate"], HP["momentum"], HP["weightcost"], w0, b0, BETA, 1)
    try:
        eng.set_shapefactors(pkg.read_shapefactors(str(d / "mixed.txt"), DIM, BETA))
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
    ws, bs = hostlib.read_wts(str(d / "mixed" / "mlp.wts"), LS)
    for l in range(2):
        assert np.array_equal(ws[l].view(np.uint32), we[l].view(np.uint32)), l
        assert np.array_equal(bs[l].view(np.uint32), be[l].view(np.uint32)), l


def test_the_error_model_file_of_one_epoch_is_the_shape_file_of_the_next(pkg, runs):
    d, kv, _, _ = runs
    a = d / "a.errmodel"
    first = run(d / "epoch1", kv, MLGGD_ERRMODEL=str(a))
    assert first.returncode == 0 and os.path.getsize(a) > 0, first.stdout + first.stderr
    betas = pkg.read_shapefactors(str(a), DIM, BETA)              # what the next epoch is going to read
    assert betas.shape == (DIM,) and len(set(betas.tolist())) > 1
    kv2 = dict(kv, initwts_file=d / "epoch1" / "mlp.wts")
    second = run(d / "epoch2", kv2, MLGGD_SHAPEFACTORS=str(a), MLGGD_ERRMODEL=str(d / "b.errmodel"))   # both in one run
    assert second.returncode == 0 and "all finish!" in second.stdout, second.stdout + second.stderr
    assert "shape factors: %s, %d bins, beta min %.9g max %.9g" % (a, DIM, betas.min(), betas.max()) in second.stderr
    assert len(wts(d, "epoch2")) == len(wts(d, "epoch1")) and wts(d, "epoch2") != wts(d, "epoch1")
    assert os.path.getsize(d / "b.errmodel") > 0


def test_a_beta_norm_run_refuses_the_variable_before_training(runs):
    d, kv, _, _ = runs
    res = run(d / "mmse", dict(kv, MLflag=0, shapefactor=2.0), MLGGD_SHAPEFACTORS=str(d / "mixed.txt"))
    assert res.returncode != 0 and "MLGGD_SHAPEFACTORS" in res.stderr
    assert "Starting chunk" not in open(d / "mmse" / "mlp.log").read()
    assert os.path.getsize(d / "mmse" / "mlp.wts") == 0
    # ... and so does a file that does not fit the output layer
    (d / "short.txt").write_text("1 1.5 2\n")
    res = run(d / "short", kv, MLGGD_SHAPEFACTORS=str(d / "short.txt"))
    assert res.returncode != 0 and "MLGGD_SHAPEFACTORS" in res.stderr and "line 1" in res.stderr
