"""GPU: BPtrain_Sigmoid with MLGGD_OPTIMIZER=adam and MLGGD_OPT_FILE=FILE on the original project's 10-sentence sample
(tests/golden/tools_pfile*), run the way tests/test_gpu_scale_exe.py runs the trainer: two epochs, the second starting from
the first one's weights and state file.  Both weights files and the final state file hold what a BPGpu gives when it is
driven over the same chunks through the trainer's own host IO; a second epoch started without the file differs, so the
file is really read; a state file for another net ends the run with status 1 before anything is trained."""
import os
import subprocess

import numpy as np
import pytest

import hostlib

pytestmark = pytest.mark.gpu
DIM, CTX, B, TOFF = 257, 3, 32, 1
LS = [DIM * CTX, 64, DIM]
HP = dict(lrate=0.002, momentum=0.9, weightcost=1e-5)
BETA = 1.2
ADAM = dict(beta1=0.8, beta2=0.99, eps=1e-6)
EXE = os.path.join(hostlib.HOST, "BPtrain_Sigmoid")


def run(cwd, kv, **env):
    os.makedirs(cwd, exist_ok=True)
    return subprocess.run([EXE] + ["%s=%s" % (k, v) for k, v in kv.items()], capture_output=True, text=True, timeout=300,
                          cwd=cwd, env=dict(os.environ, **env))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the sample pfiles, initial weights, the command line and two Adam epochs, made once"""
    d = tmp_path_factory.mktemp("adam_exe")
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
    env = dict(MLGGD_OPTIMIZER="adam", MLGGD_OPT_FILE=str(d / "adam.opt"), MLGGD_ADAM_BETA1=str(ADAM["beta1"]),
               MLGGD_ADAM_BETA2=str(ADAM["beta2"]), MLGGD_ADAM_EPS=str(ADAM["eps"]))
    one = run(d / "one", kv, **env)
    assert one.returncode == 0, one.stdout + one.stderr
    state1 = open(d / "adam.opt", "rb").read()
    two = run(d / "two", dict(kv, initwts_file=d / "one" / "mlp.wts"), **env)
    assert two.returncode == 0, two.stdout + two.stderr
    return d, kv, env, one, two, state1


def python_epoch(pkg, d, kv, init, state):
    """one epoch of BPGpu over the trainer's own chunks; returns (weights, bias, OptimizerState)"""
    io = hostlib.HostIO(**dict(kv, log_file=d / "io.log", outwts_file=d / "io.wts"))
    w0, b0 = hostlib.read_wts(str(init), LS)
    eng = pkg.BPGpu(1, 0, LS, B, HP["lrate"], HP["momentum"], HP["weightcost"], w0, b0, BETA, 1)
    try:
        eng.set_optimizer("adam", **ADAM)
        if state is not None:
            eng.set_optimizer_state(state.m_w, state.v_w, state.m_b, state.v_b, state.steps)
        starts, _ = io.plan(kv["train_sent_range"])
        order = io.shuffle(len(starts))
        assert len(starts) >= 3
        for ci in order:
            inp, tg = io.read_chunk(ci, LS[0], DIM, 600)
            eng.train(inp, tg)
        we, be = eng.returnWeights()
        return we, be, eng.optimizer_state()
    finally:
        io.close()
        eng.close()


def same_net(path, we, be):
    ws, bs = hostlib.read_wts(str(path), LS)
    for l in range(2):
        assert np.array_equal(bits(ws[l]), bits(we[l])), l
        assert np.array_equal(bits(bs[l]), bits(be[l])), l


def same_state(f, st):
    assert f.steps == st.steps
    for got, want in ((f.m_w, st.m_w), (f.v_w, st.v_w), (f.m_b, st.m_b), (f.v_b, st.v_b)):
        for l in range(2):
            assert np.array_equal(bits(got[l]), bits(want[l])), l


def test_two_epochs_equal_the_python_engine_and_the_file_is_really_read(pkg, runs, tmp_path):
    d, kv, env, one, two, state1 = runs
    line = [l for l in one.stderr.splitlines() if l.startswith("adam:")]
    assert len(line) == 1 and "beta1 0.800000012 beta2 0.99000001 eps 9.99999997e-07" in line[0] and "start from zero" in line[0]
    assert "adam: %s written" % (d / "adam.opt") in one.stdout
    we, be, st = python_epoch(pkg, d, kv, d / "init.wts", None)
    assert st.steps > 3
    same_net(d / "one" / "mlp.wts", we, be)
    (tmp_path / "s1.opt").write_bytes(state1)
    f1 = pkg.read_optimizer_state(str(tmp_path / "s1.opt"))
    assert f1.layersizes == LS and (np.float32(f1.beta1), np.float32(f1.beta2), np.float32(f1.eps)) == tuple(
        np.float32(ADAM[k]) for k in ("beta1", "beta2", "eps"))
    same_state(f1, st)
    assert all(a.any() for a in f1.m_w + f1.v_w + f1.m_b + f1.v_b)
    # the second epoch: the first one's weights and state
    line = [l for l in two.stderr.splitlines() if l.startswith("adam:")]
    assert len(line) == 1 and "state of %s after %d steps" % (d / "adam.opt", st.steps) in line[0]
    we2, be2, st2 = python_epoch(pkg, d, dict(kv, initwts_file=d / "one" / "mlp.wts"), d / "one" / "mlp.wts", f1)
    assert st2.steps == 2 * st.steps
    same_net(d / "two" / "mlp.wts", we2, be2)
    same_state(pkg.read_optimizer_state(str(d / "adam.opt")), st2)
    # ... and the same second epoch without the file: other weights
    cold = run(d / "cold", dict(kv, initwts_file=d / "one" / "mlp.wts"), **dict(env, MLGGD_OPT_FILE=str(d / "cold.opt")))
    assert cold.returncode == 0, cold.stdout + cold.stderr
    assert open(d / "cold" / "mlp.wts", "rb").read() != open(d / "two" / "mlp.wts", "rb").read()
    assert pkg.read_optimizer_state(str(d / "cold.opt")).steps == st.steps
    # the log keeps its form
    assert "CV over. squared error" in open(d / "one" / "mlp.log").read()


def test_a_state_for_another_net_and_bad_values_end_before_training(pkg, runs):
    d, kv, env, *_ = runs
    other = [LS[0], 48, LS[2]]
    z = lambda l, wide: np.zeros((other[l], other[l + 1]) if wide else other[l + 1], np.float32)
    pkg.write_optimizer_state(str(d / "other.opt"), other, [z(0, 1), z(1, 1)], [z(0, 1), z(1, 1)], [z(0, 0), z(1, 0)],
                              [z(0, 0), z(1, 0)], steps=5)
    res = run(d / "other", kv, **dict(env, MLGGD_OPT_FILE=str(d / "other.opt")))
    assert res.returncode == 1 and "MLGGD_OPT_FILE" in res.stderr
    assert "771,48,257" in res.stderr and "771,64,257" in res.stderr
    assert "Starting chunk" not in open(d / "other" / "mlp.log").read()
    assert os.path.getsize(d / "other" / "mlp.wts") == 0
    (d / "short.opt").write_bytes(open(d / "adam.opt", "rb").read()[:1000])
    for name, e, what in (("kind", dict(MLGGD_OPTIMIZER="adamw"), "must be adam or sgd"),
                          ("beta", dict(MLGGD_OPTIMIZER="adam", MLGGD_ADAM_BETA1="1"), "MLGGD_ADAM_BETA1"),
                          ("word", dict(MLGGD_OPTIMIZER="adam", MLGGD_ADAM_EPS="tiny"), "MLGGD_ADAM_EPS=tiny: not a number"),
                          ("file", dict(MLGGD_OPT_FILE=str(d / "x.opt")), "needs MLGGD_OPTIMIZER=adam"),
                          ("ranks", dict(MLGGD_OPTIMIZER="adam", WORLD_SIZE="2", RANK="0"), "MLGGD_OPTIMIZER=adam"),
                          ("short", dict(MLGGD_OPTIMIZER="adam", MLGGD_OPT_FILE=str(d / "short.opt")), "the file ends inside")):
        res = run(d / name, kv, **e)
        assert res.returncode == 1 and what in res.stderr, (name, res.stderr)
        assert "Starting chunk" not in open(d / name / "mlp.log").read()
    assert not os.path.exists(d / "x.opt")


def test_sgd_by_name_is_the_run_without_the_variable(runs):
    d, kv, *_ = runs
    plain = run(d / "plain", kv)
    named = run(d / "named", kv, MLGGD_OPTIMIZER="sgd")
    assert plain.returncode == 0 and named.returncode == 0, plain.stderr + named.stderr
    assert open(d / "plain" / "mlp.wts", "rb").read() == open(d / "named" / "mlp.wts", "rb").read()
    assert named.stdout == plain.stdout and "adam" not in named.stderr and "adam" not in plain.stdout
