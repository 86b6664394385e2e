"""CPU: what BPtrain_Sigmoid decides from its environment before it trains (host/train_options.cc), on the fixture of
tests/test_gpu_scale_exe.py: the original project's 10-sentence sample and a 771-64-257 net.

Part A runs the executable.  A refused run never opens a device: it ends with status 1, the one message line on stderr
and in the log, no chunk started and an empty weights file.  Two faults at once pin the order of the checks, since only
the first one is reported.

Part B reads the accepted cases back through the hook (tests/host_api.cc: mlggd_host_train_options), which runs the
trainer's own reader over a table of NAME=VALUE strings and prints every field; the values are compared with what this
file computes itself."""
import os
import subprocess

import numpy as np
import pytest

import hostlib

DIM, CTX, B, TOFF = 257, 3, 32, 1
LS = [DIM * CTX, 64, DIM]
OTHER = [LS[0], 48, LS[2]]
HP = dict(lrate=0.1, momentum=0.9, weightcost=1e-5)
BETA = 1.2
EXE = os.path.join(hostlib.HOST, "BPtrain_Sigmoid")
F = np.float32
# the trainer's own variables: a test's environment holds the ones it names and none it inherited
OWN = ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MLGGD_EXPANDED", "MLGGD_PINNED", "MLGGD_WATCHDOG_S", "MLGGD_TIMING", "MLGGD_ID_FILE",
       "MLGGD_RENDEZVOUS_TIMEOUT", "MLGGD_ERRMODEL", "MLGGD_ERRMODEL_BETAS", "MLGGD_ASYMMODEL", "MLGGD_GVFILE",
       "MLGGD_SHAPEFACTORS", "MLGGD_ASYMMETRY", "MLGGD_SCALE", "MLGGD_SCALE_FILE", "MLGGD_SCALE_LRATE", "MLGGD_SCALE_MOMENTUM",
       "MLGGD_SCALE_VMAX", "MLGGD_OPTIMIZER", "MLGGD_OPT_FILE", "MLGGD_ADAM_BETA1", "MLGGD_ADAM_BETA2", "MLGGD_ADAM_EPS")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def g9(x):
    """a float as the hook prints it"""
    return "%.9g" % float(F(x))


def zeros(ls, l, wide):
    return np.zeros((ls[l], ls[l + 1]) if wide else ls[l + 1], F)


@pytest.fixture(scope="module")
def fx(pkg, tmp_path_factory):
    """the sample pfiles, initial weights, the command line and the files the cases name, made once"""
    d = tmp_path_factory.mktemp("trainer_options")
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    sample = hostlib.sample_pfiles(d / "tools_pfile")
    rng = np.random.default_rng(5)
    ws = [rng.normal(0, 0.05, (LS[i], LS[i + 1])).astype(F) for i in range(2)]
    bs = [rng.normal(0, 0.1, LS[i + 1]).astype(F) for i in range(2)]
    hostlib.write_wts(str(d / "init.wts"), ws, bs)
    kv = dict(gpu_used=0, numlayers=3, layersizes=",".join(map(str, LS)), bunchsize=B, MLflag=1, shapefactor=BETA,
              fea_dim=DIM, fea_context=CTX, traincache=500, init_randem_seed=27870775, targ_offset=TOFF,
              initwts_file=d / "init.wts", norm_file=os.path.join(sample, "train_noisy.norm"),
              fea_file=os.path.join(sample, "train_noisy.pfile"), targ_file=os.path.join(sample, "train_clean.pfile"),
              outwts_file="mlp.wts", log_file="mlp.log", train_sent_range="0-7", cv_sent_range="8-9", dropoutflag=0,
              visible_omit=0.1, hid_omit=0.1, **HP)
    (d / "word.txt").write_text("abc\n" + "1.5\n" * (DIM - 1))
    (d / "two_rows.txt").write_text("0 1 0\n1 1 0\n")
    pkg.write_optimizer_state(str(d / "other.opt"), OTHER, [zeros(OTHER, 0, 1), zeros(OTHER, 1, 1)], [zeros(OTHER, 0, 1), zeros(OTHER, 1, 1)],
                              [zeros(OTHER, 0, 0), zeros(OTHER, 1, 0)], [zeros(OTHER, 0, 0), zeros(OTHER, 1, 0)], steps=5)
    (d / "other_cut.opt").write_bytes(open(d / "other.opt", "rb").read()[:1000])
    mom = [[rng.normal(0, 1, (LS[l], LS[l + 1]) if wide else LS[l + 1]).astype(F) ** (2 if second else 1) for l in range(2)]
           for wide, second in ((1, 0), (1, 1), (0, 0), (0, 1))]  # m_w, v_w, m_b, v_b
    pkg.write_optimizer_state(str(d / "right.opt"), LS, *mom, beta1=0.7, beta2=0.95, eps=1e-5, steps=77)
    (d / "right_cut.opt").write_bytes(open(d / "right.opt", "rb").read()[:1000])
    return d, kv, mom


# ---------------------------------------------------------------- part A: refusals through the executable
def run(cwd, kv, env):
    os.makedirs(cwd, exist_ok=True)
    base = {k: v for k, v in os.environ.items() if k not in OWN}
    return subprocess.run([EXE] + ["%s=%s" % (k, v) for k, v in kv.items()], capture_output=True, text=True, timeout=120,
                          cwd=cwd, env=dict(base, **env))


MMSE = dict(MLflag=0, shapefactor=2.0)
GRID = "MLGGD_ERRMODEL_BETAS=oops: expected lo:step:hi"
SCALE_RATES = ("MLGGD_SCALE=learned: MLGGD_SCALE_LRATE must be finite and >= 0, MLGGD_SCALE_MOMENTUM in [0, 1), MLGGD_SCALE_VMAX "
               "finite and > 0")
ADAM_PARAMS = ("MLGGD_OPTIMIZER=adam: MLGGD_ADAM_BETA1 and MLGGD_ADAM_BETA2 must lie in [0, 1), MLGGD_ADAM_EPS must be finite "
               "and > 0")
OTHER_NET = "the state is of a net with layer sizes 771,48,257, this run's net has 771,64,257"
BODY = 4 * sum(2 * LS[l] * LS[l + 1] + 2 * LS[l + 1] for l in range(2))  # bytes of moments behind a header of 44
# name, changes to the command line, environment ({d}: the fixture's directory), the one message line
REFUSALS = [
    ("errmodel_grid", {}, dict(MLGGD_ERRMODEL="x", MLGGD_ERRMODEL_BETAS="oops"), GRID),
    ("asymmodel_grid", {}, dict(MLGGD_ASYMMODEL="x", MLGGD_ERRMODEL_BETAS="oops"), GRID),
    ("shapes_mmse", MMSE, dict(MLGGD_SHAPEFACTORS="f"), "MLGGD_SHAPEFACTORS=f: per-bin shape factors need MLflag=1, this run has MLflag=0"),
    ("shapes_word", {}, dict(MLGGD_SHAPEFACTORS="{d}/word.txt"), "MLGGD_SHAPEFACTORS: {d}/word.txt line 1: 'abc' is not a number"),
    ("skews_mmse", MMSE, dict(MLGGD_ASYMMETRY="f"), "MLGGD_ASYMMETRY=f: a skew per bin needs MLflag=1, this run has MLflag=0"),
    ("skews_word", {}, dict(MLGGD_ASYMMETRY="{d}/word.txt"), "MLGGD_ASYMMETRY: {d}/word.txt line 1: 'abc' is not a number"),
    ("scale_mode", {}, dict(MLGGD_SCALE="both"), "MLGGD_SCALE=both: must be learned or alternating"),
    ("scale_file_alone", {}, dict(MLGGD_SCALE_FILE="x"), "MLGGD_SCALE_FILE=x: needs MLGGD_SCALE=learned"),
    ("scale_mmse", MMSE, dict(MLGGD_SCALE="learned"), "MLGGD_SCALE=learned: a learned scale needs MLflag=1, this run has MLflag=0"),
    ("scale_rate", {}, dict(MLGGD_SCALE="learned", MLGGD_SCALE_LRATE="-1"), SCALE_RATES),
    ("scale_word", {}, dict(MLGGD_SCALE="learned", MLGGD_SCALE_VMAX="big"), "MLGGD_SCALE_VMAX=big: not a number"),
    ("scale_two_rows", {}, dict(MLGGD_SCALE="learned", MLGGD_SCALE_FILE="{d}/two_rows.txt"),
     "MLGGD_SCALE_FILE: {d}/two_rows.txt line 2: 2 rows, the output layer has 257"),
    ("opt_kind", {}, dict(MLGGD_OPTIMIZER="adamw"), "MLGGD_OPTIMIZER=adamw: must be adam or sgd"),
    ("opt_file_alone", {}, dict(MLGGD_OPT_FILE="x"), "MLGGD_OPT_FILE=x: needs MLGGD_OPTIMIZER=adam"),
    ("opt_ranks", {}, dict(MLGGD_OPTIMIZER="adam", WORLD_SIZE="2", RANK="0"),
     "MLGGD_OPTIMIZER=adam: Adam runs on a single rank, this run has WORLD_SIZE=2"),
    ("opt_beta", {}, dict(MLGGD_OPTIMIZER="adam", MLGGD_ADAM_BETA1="1"), ADAM_PARAMS),
    ("opt_word", {}, dict(MLGGD_OPTIMIZER="adam", MLGGD_ADAM_EPS="tiny"), "MLGGD_ADAM_EPS=tiny: not a number"),
    ("opt_other_net", {}, dict(MLGGD_OPTIMIZER="adam", MLGGD_OPT_FILE="{d}/other.opt"), "MLGGD_OPT_FILE: {d}/other.opt: " + OTHER_NET),
    # that file cut to 1000 bytes: its header is whole, so the net is still what is named ...
    ("opt_other_net_cut", {}, dict(MLGGD_OPTIMIZER="adam", MLGGD_OPT_FILE="{d}/other_cut.opt"),
     "MLGGD_OPT_FILE: {d}/other_cut.opt: " + OTHER_NET),
    # ... and a cut file for this run's net, where the length is
    ("opt_right_net_cut", {}, dict(MLGGD_OPTIMIZER="adam", MLGGD_OPT_FILE="{d}/right_cut.opt"),
     "MLGGD_OPT_FILE: {d}/right_cut.opt: the file ends inside the moments: 956 bytes behind the header, %d belong there" % BODY),
    # two faults at once: the first check in the order reports
    ("shapes_before_opt", MMSE, dict(MLGGD_SHAPEFACTORS="f", MLGGD_OPTIMIZER="adamw"),
     "MLGGD_SHAPEFACTORS=f: per-bin shape factors need MLflag=1, this run has MLflag=0"),
    ("scale_before_opt", {}, dict(MLGGD_SCALE="both", MLGGD_OPTIMIZER="adamw"), "MLGGD_SCALE=both: must be learned or alternating"),
]


@pytest.mark.parametrize("name,args,env,message", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_a_refused_run_ends_with_status_1_and_the_one_message(fx, name, args, env, message):
    d, kv, _ = fx
    env = {k: v.format(d=d) for k, v in env.items()}
    message = message.format(d=d)
    res = run(d / name, dict(kv, **args), env)
    print(res.stderr)
    assert res.returncode == 1
    assert res.stderr == message + "\n"
    log = open(d / name / "mlp.log").read()
    assert message + "\n" in log and "Starting chunk" not in log
    assert os.path.getsize(d / name / "mlp.wts") == 0
    assert not os.path.exists(d / name / "x") and not os.path.exists(d / name / "f")


# ---------------------------------------------------------------- part B: accepted cases through the hook
@pytest.fixture(scope="module")
def io(fx):
    d, kv, _ = fx
    h = hostlib.HostIO(**dict(kv, log_file=d / "io.log", outwts_file=d / "io.wts"))
    yield h
    h.close()


def floats(tokens):
    """a vector field of the hook's text: its length, then its values"""
    assert int(tokens[0]) == len(tokens) - 1
    return np.array([float(t) for t in tokens[1:]], np.float64).astype(F)


OFF = dict(world=["1"], rank=["0"], local_rank=["0"], frames=["1"], pinned=["1"], watchdog_s=["900"], timing=["0"], id_file=[],
           rendezvous_timeout=["600"], errmodel_fn=[], asymmodel_fn=[], gv_fn=[], model_betas=["0"], shapes_fn=[], shapes=["0"],
           asym_fn=[], skews=["0"], scale_learned=["0"], scale_fn=[], scale_alpha=["0"], scale_velocity=["0"], scale_steps0=["0"],
           adam=["0"], opt_fn=[], opt_restored=["0"])


def test_without_a_variable_every_feature_is_off(io):
    got = io.train_options({})
    for k, v in OFF.items():
        assert got[k] == v, k
    assert [got[k] for k in ("scale_lrate", "scale_momentum", "scale_vmax")] == [["0.0500000007"], ["0.5"], ["1"]]
    assert [got[k] for k in ("adam_beta1", "adam_beta2", "adam_eps")] == [[g9(0.9)], [g9(0.999)], [g9(1e-8)]]
    # an empty value is an unset one, and the default mode by name is the default
    assert io.train_options_text(dict(MLGGD_SCALE="")) == io.train_options_text({})
    assert io.train_options_text(dict(MLGGD_SCALE="alternating")) == io.train_options_text({})
    assert io.train_options_text({k: "" for k in OWN if k != "MLGGD_TIMING"}) == io.train_options_text({})


def test_the_plain_knobs_and_the_local_rank(io):
    got = io.train_options(dict(RANK="3", WORLD_SIZE="4"))
    assert (got["world"], got["rank"], got["local_rank"]) == (["4"], ["3"], ["3"])
    got = io.train_options(dict(RANK="3", WORLD_SIZE="4", LOCAL_RANK="1", MLGGD_EXPANDED="1", MLGGD_PINNED="0", MLGGD_WATCHDOG_S="5",
                                MLGGD_TIMING="1", MLGGD_ID_FILE="/tmp/id", MLGGD_RENDEZVOUS_TIMEOUT="7", MLGGD_GVFILE="gv.txt"))
    assert got["local_rank"] == ["1"] and got["frames"] == ["0"] and got["pinned"] == ["0"] and got["watchdog_s"] == ["5"]
    assert got["timing"] == ["1"] and got["id_file"] == ["/tmp/id"] and got["rendezvous_timeout"] == ["7"] and got["gv_fn"] == ["gv.txt"]


SCALE_ENV = dict(MLGGD_SCALE="learned", MLGGD_SCALE_LRATE="0.1", MLGGD_SCALE_MOMENTUM="0.25", MLGGD_SCALE_VMAX="0.5")


def test_the_learned_scale_its_rates_and_its_state_file(pkg, fx, io):
    d, *_ = fx
    for env in (SCALE_ENV, dict(SCALE_ENV, MLGGD_SCALE_FILE=str(d / "no_such_scale.txt"))):
        got = io.train_options(env)
        assert got["scale_learned"] == ["1"] and got["scale_fn"] == ([env["MLGGD_SCALE_FILE"]] if "MLGGD_SCALE_FILE" in env else [])
        assert [got[k] for k in ("scale_lrate", "scale_momentum", "scale_vmax")] == [[g9(0.1)], ["0.25"], ["0.5"]]
        assert got["scale_alpha"] == ["0"] and got["scale_velocity"] == ["0"] and got["scale_steps0"] == ["0"]
    assert not os.path.exists(d / "no_such_scale.txt")
    rng = np.random.default_rng(11)
    a, v = rng.uniform(0.1, 3.0, DIM).astype(F), rng.normal(0, 0.01, DIM).astype(F)
    a[0] = 0.0  # a bin that still seeds
    pkg.write_scale_state(str(d / "scale.txt"), a, v, lrate=0.3, momentum=0.1, vmax=2.0, steps=1234)
    got = io.train_options(dict(SCALE_ENV, MLGGD_SCALE_FILE=str(d / "scale.txt")))
    assert np.array_equal(bits(floats(got["scale_alpha"])), bits(a)) and np.array_equal(bits(floats(got["scale_velocity"])), bits(v))
    assert got["scale_steps0"] == ["1234"]
    # the file's own rates describe the run that wrote it: this run's are the ones in effect
    assert [got[k] for k in ("scale_lrate", "scale_momentum", "scale_vmax")] == [[g9(0.1)], ["0.25"], ["0.5"]]


@pytest.mark.parametrize("var,name_key,key", [("MLGGD_SHAPEFACTORS", "shapes_fn", "shapes"), ("MLGGD_ASYMMETRY", "asym_fn", "skews")])
def test_a_plain_list_of_257_numbers_comes_back_as_those_floats(fx, io, var, name_key, key):
    d, *_ = fx
    vals = np.random.default_rng(12).uniform(0.6, 2.4, DIM).astype(F)
    path = d / (key + ".txt")
    path.write_text("".join("%.9g\n" % x for x in vals))
    got = io.train_options({var: str(path)})
    assert got[name_key] == [str(path)] and np.array_equal(bits(floats(got[key])), bits(vals))
    other = "skews" if key == "shapes" else "shapes"
    assert got[other] == ["0"]


def test_adam_its_parameters_and_its_state_file(fx, io):
    d, _, mom = fx
    env = dict(MLGGD_OPTIMIZER="adam", MLGGD_ADAM_BETA1="0.8", MLGGD_ADAM_BETA2="0.99", MLGGD_ADAM_EPS="1e-6")
    got = io.train_options(env)
    assert got["adam"] == ["1"] and got["opt_fn"] == [] and got["opt_restored"] == ["0"]
    assert [got[k] for k in ("adam_beta1", "adam_beta2", "adam_eps")] == [[g9(0.8)], [g9(0.99)], [g9(1e-6)]]
    got = io.train_options(dict(env, MLGGD_OPT_FILE=str(d / "no_such.opt")))
    assert got["adam"] == ["1"] and got["opt_restored"] == ["0"] and not os.path.exists(d / "no_such.opt")
    got = io.train_options(dict(env, MLGGD_OPT_FILE=str(d / "right.opt")))
    assert got["opt_fn"] == [str(d / "right.opt")] and got["opt_restored"] == ["1"] and got["opt_steps"] == ["77"]
    # this run's parameters are the ones in effect, not the file's
    assert [got[k] for k in ("adam_beta1", "adam_beta2", "adam_eps")] == [[g9(0.8)], [g9(0.99)], [g9(1e-6)]]
    for kind, arrays in zip(("m_w", "v_w", "m_b", "v_b"), mom):
        for l, want in enumerate(arrays, start=1):
            n, first, last = got["opt_%s%d" % (kind, l)]  # a moment array: its length, its first and its last value
            assert int(n) == want.size
            assert np.array_equal(bits([float(first), float(last)]), bits([want.ravel()[0], want.ravel()[-1]])), (kind, l)
    assert io.train_options(dict(MLGGD_OPTIMIZER="sgd")) == io.train_options({})


def test_the_model_grid_is_rank_0s(io):
    got = io.train_options(dict(MLGGD_ERRMODEL="x"))
    want = np.array([0.5 + i * 0.1 for i in range(21)], np.float64).astype(F)
    assert got["errmodel_fn"] == ["x"] and got["asymmodel_fn"] == []
    assert np.array_equal(bits(floats(got["model_betas"])), bits(want)) and want[0] == F(0.5) and want[-1] == F(2.5)
    got = io.train_options(dict(MLGGD_ASYMMODEL="y", MLGGD_ERRMODEL_BETAS="1:0.5:2"))
    assert got["asymmodel_fn"] == ["y"] and np.array_equal(floats(got["model_betas"]), np.array([1, 1.5, 2], F))
    # a bad grid on another rank is not looked at
    got = io.train_options(dict(MLGGD_ERRMODEL="x", MLGGD_ERRMODEL_BETAS="oops", RANK="1", WORLD_SIZE="2"))
    assert got["errmodel_fn"] == ["x"] and got["model_betas"] == ["0"]
    with pytest.raises(hostlib.HostError, match="MLGGD_ERRMODEL_BETAS=oops: expected lo:step:hi"):
        io.train_options(dict(MLGGD_ERRMODEL="x", MLGGD_ERRMODEL_BETAS="oops"))


def test_the_hook_reports_a_refusal_with_the_executables_message(io):
    with pytest.raises(hostlib.HostError) as e:
        io.train_options(dict(MLGGD_SCALE="both", MLGGD_OPTIMIZER="adamw"))
    assert str(e.value) == "MLGGD_SCALE=both: must be learned or alternating"
