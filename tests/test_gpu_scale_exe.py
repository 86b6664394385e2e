"""GPU: BPtrain_Sigmoid with MLGGD_SCALE=learned and MLGGD_SCALE_FILE=FILE on the original project's 10-sentence sample
(tests/golden/tools_pfile*), run the way tests/test_gpu_asymmetry_exe.py runs the trainer: the state file an epoch
writes holds the (alpha, v) of a BPGpu fed the same chunks, a second epoch reads it and continues, a beta-norm run
refuses the variable before it trains, and a run without the variables is the run it was."""
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
RATES = dict(lrate=0.1, momentum=0.25, vmax=0.5)
EXE = os.path.join(hostlib.HOST, "BPtrain_Sigmoid")


def run(cwd, kv, **env):
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([EXE] + ["%s=%s" % (k, v) for k, v in kv.items()], capture_output=True, text=True, timeout=300,
                          cwd=cwd, env=dict(os.environ, **env))


def wts(d, name):
    return open(d / name / "mlp.wts", "rb").read()


def log_of(path):
    """the log with the one wall-clock figure it holds masked"""
    return re.sub(r"Total cost time: [\d.]+ s\.", "Total cost time: T s.", open(path).read())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the sample pfiles, initial weights, the command line, the run without a variable and two learned epochs, the second
    starting from the first one's weights and state file, made once"""
    d = tmp_path_factory.mktemp("scale_exe")
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
    env = dict(MLGGD_SCALE="learned", MLGGD_SCALE_FILE=str(d / "scale.txt"), MLGGD_SCALE_LRATE=str(RATES["lrate"]),
               MLGGD_SCALE_MOMENTUM=str(RATES["momentum"]), MLGGD_SCALE_VMAX=str(RATES["vmax"]))
    plain = run(d / "plain", kv)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    one = run(d / "one", kv, **env)
    assert one.returncode == 0, one.stdout + one.stderr
    state1 = open(d / "scale.txt").read()
    two = run(d / "two", dict(kv, initwts_file=d / "one" / "mlp.wts"), **env)
    assert two.returncode == 0, two.stdout + two.stderr
    return d, kv, plain, one, two, state1


def python_epoch(pkg, d, kv, init, state):
    """one epoch of BPGpu over the trainer's own chunks; returns (weights, bias, alpha, v, steps)"""
    io = hostlib.HostIO(**dict(kv, log_file=d / "io.log", outwts_file=d / "io.wts"))
    w0, b0 = hostlib.read_wts(str(init), LS)
    eng = pkg.BPGpu(1, 0, LS, B, HP["lrate"], HP["momentum"], HP["weightcost"], w0, b0, BETA, 1)
    try:
        eng.set_scale_mode("learned", **RATES)
        if state is not None:
            eng.set_scale_state(*state)
        starts, _ = io.plan(kv["train_sent_range"])
        order = io.shuffle(len(starts))
        assert len(starts) >= 3
        for ci in order:
            inp, tg = io.read_chunk(ci, LS[0], DIM, 600)
            eng.train(inp, tg)
        we, be = eng.returnWeights()
        a, v = eng.scale_state()
        return we, be, a, v, eng.scale_mode().steps
    finally:
        io.close()
        eng.close()


def same_net(path, we, be):
    ws, bs = hostlib.read_wts(str(path), LS)
    for l in range(2):
        assert np.array_equal(bits(ws[l]), bits(we[l])), l
        assert np.array_equal(bits(bs[l]), bits(be[l])), l


def steps_of(text):
    return int(re.search(r"^# steps (\d+)$", text, re.M).group(1))


def test_the_state_file_is_the_python_engines_state_and_the_next_epoch_continues(pkg, runs, tmp_path):
    d, kv, plain, one, two, state1 = runs
    line = [l for l in one.stderr.splitlines() if l.startswith("learned scale:")]
    assert len(line) == 1 and "lrate 0.100000001 momentum 0.25 vmax 0.5" in line[0] and "seeds" in line[0]
    assert "learned scale: %s written" % (d / "scale.txt") in one.stdout
    assert wts(d, "one") != wts(d, "plain")
    we, be, a, v, steps = python_epoch(pkg, d, kv, d / "init.wts", None)
    (tmp_path / "s1.txt").write_text(state1)
    fa, fv = pkg.read_scale_state(str(tmp_path / "s1.txt"), DIM)
    assert np.array_equal(bits(fa), bits(a)) and np.array_equal(bits(fv), bits(v)) and v.any() and (a > 0).all()
    assert steps_of(state1) == steps > 3
    same_net(d / "one" / "mlp.wts", we, be)
    # the second epoch: the first one's weights and state
    line = [l for l in two.stderr.splitlines() if l.startswith("learned scale:")]
    assert len(line) == 1 and "state of %s after %d steps" % (d / "scale.txt", steps) in line[0]
    we2, be2, a2, v2, steps2 = python_epoch(pkg, d, dict(kv, initwts_file=d / "one" / "mlp.wts"), d / "one" / "mlp.wts", (fa, fv))
    state2 = open(d / "scale.txt").read()
    ga, gv = pkg.read_scale_state(str(d / "scale.txt"), DIM)
    assert np.array_equal(bits(ga), bits(a2)) and np.array_equal(bits(gv), bits(v2))
    assert not np.array_equal(bits(ga), bits(fa))
    assert steps_of(state2) == steps + steps2
    same_net(d / "two" / "mlp.wts", we2, be2)
    # the log keeps its form; its likelihood line is the learned scale's
    assert "CV2 over. CV log likelihood" in log_of(d / "one" / "mlp.log")
    assert log_of(d / "one" / "mlp.log") != log_of(d / "plain" / "mlp.log")


def test_a_beta_norm_run_and_bad_values_end_before_training(runs):
    d, kv, *_ = runs
    res = run(d / "mmse", dict(kv, MLflag=0, shapefactor=2.0), MLGGD_SCALE="learned")
    assert res.returncode != 0 and "MLGGD_SCALE=learned" in res.stderr and "MLflag=1" in res.stderr
    assert "Starting chunk" not in open(d / "mmse" / "mlp.log").read()
    assert os.path.getsize(d / "mmse" / "mlp.wts") == 0
    for name, env, what in (("mode", dict(MLGGD_SCALE="both"), "must be learned or alternating"),
                            ("rate", dict(MLGGD_SCALE="learned", MLGGD_SCALE_LRATE="-1"), "MLGGD_SCALE_LRATE"),
                            ("word", dict(MLGGD_SCALE="learned", MLGGD_SCALE_VMAX="big"), "MLGGD_SCALE_VMAX=big: not a number"),
                            ("file", dict(MLGGD_SCALE_FILE=str(d / "x.txt")), "needs MLGGD_SCALE=learned")):
        res = run(d / name, kv, **env)
        assert res.returncode != 0 and what in res.stderr, (name, res.stderr)
        assert "Starting chunk" not in open(d / name / "mlp.log").read()
    (d / "short.txt").write_text("0 1 0\n1 1 0\n")
    res = run(d / "short", kv, MLGGD_SCALE="learned", MLGGD_SCALE_FILE=str(d / "short.txt"))
    assert res.returncode != 0 and "MLGGD_SCALE_FILE" in res.stderr and "line 2" in res.stderr
    assert "Starting chunk" not in open(d / "short" / "mlp.log").read()


def test_without_the_variables_the_run_is_what_it_was(runs):
    """no word of the mode on stdout or stderr, and MLGGD_SCALE=alternating is that run byte for byte: weights, log, stdout"""
    d, kv, plain, *_ = runs
    assert "learned scale" not in plain.stdout and "learned scale" not in plain.stderr
    res = run(d / "alt", kv, MLGGD_SCALE="alternating")
    assert res.returncode == 0, res.stdout + res.stderr
    assert wts(d, "alt") == wts(d, "plain") and len(wts(d, "plain")) > 4 * LS[0] * LS[1]
    assert log_of(d / "alt" / "mlp.log") == log_of(d / "plain" / "mlp.log")
    assert res.stdout == plain.stdout and "learned scale" not in res.stderr
