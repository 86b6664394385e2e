"""GPU: rectified-linear hidden units (BPGpu(..., activation="relu")) through every layer of the engine.

Beside the bit-for-bit runs against the oracle's twin (tests/test_gpu_twin_relu_bins.py: 4-wave and 64 x 64 kernels), the
ReLU kernels are held to the float64 model of tests/relu64.py: every kernel of a
training step against its own fp32 inputs with derived per-element bounds (tests/test_relu_model.py shows on the CPU
that the bounds pass the rules and refuse the slips they are meant for), one step on exactly representable data with no
bound at all, the special values of the rule itself, and then the features built on run_forward / the dX launcher --
dropout, the four data-parallel exchanges, decoding (single, batched, live), wave training, the error statistics, the
executables -- each by the property its sigmoid test checks.  A table of the worst ratios is printed at the end (-s)."""
import os
import subprocess

import numpy as np
import pytest

import bounds64 as b6
import hostlib
import relu64 as r6
import spec64
from test_gpu_dp_vs_float64 import MODES, read_dp_step, set_world
from test_gpu_error_stats import pin
from test_gpu_live import feed, same_as
from test_gpu_spectral import chain_from_pieces, norm_stats, read_wav, write_wav
from test_gpu_vs_float64 import KNOBS, fail_lines, read_step, state

pytestmark = pytest.mark.gpu
TABLE = {}


def record(case, reps):
    for r in reps:
        key = (case, r.name)
        h, t, lim = TABLE.get(key, (0.0, 0.0, r.limit))
        TABLE[key] = (max(h, r.hard), max(t, r.tight), r.limit)


@pytest.fixture(scope="module", autouse=True)
def print_table():
    yield
    print("\n%-44s %-22s %10s %10s %8s" % ("case", "kernel", "hard", "tight", "limit"))
    for (case, name), (h, t, lim) in TABLE.items():
        print("%-44s %-22s %10.4f %10.2f %8.1f" % (case, name, h, t, lim))


def new_engine(pkg, monkeypatch, ls, B, hp, beta, ml, W, b, env=None, activation="relu", **kw):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    eng = pkg.BPGpu(1, 0, ls, B, *hp, W, b, beta, ml, activation=activation, **kw)
    assert eng.activation == activation
    return eng


def one_step(eng, x, t, hp, beta, ml, L, lr=None):
    pre = state(eng, L)
    assert eng.train(x, t) == 1
    return read_step(eng, x, t, pre, hp[0] if lr is None else lr, hp, beta, ml, L)


# ---------------------------------------------------------------------------------------------------------------------
# 1. per-kernel bounds
@pytest.mark.parametrize("ml,beta", [(0, 2.0), (0, 1.0), (1, 0.9)], ids=["MMSE", "betanorm1", "ML0.9"])
@pytest.mark.parametrize("B", [24, 128])
def test_every_kernel_of_three_steps_within_its_bound(pkg, monkeypatch, B, ml, beta):
    """[45, 70, 33, 9]: edge tiles in every layer, a one-row strip, B = 24 a partial frame tile.  Biases U(+-0.5) and
    normal inputs put both signs of z into every layer: between 20 % and 80 % of each hidden layer's y are exactly 0 in
    every step (shown for this seed in float64 by tests/test_relu_model.py::test_the_gpu_case_is_not_degenerate)."""
    ls, hp = r6.CASE_LS, r6.CASE_HP
    L = len(ls)
    W, b = b6.make_net(ls, r6.CASE_SEED)
    x, t = b6.make_data(ls, 3 * B, r6.CASE_SEED + 1)
    eng = new_engine(pkg, monkeypatch, ls, B, hp, beta, ml, W, b)
    case = "relu B%d ML%d beta %g" % (B, ml, beta)
    bad = []
    try:
        for k in range(3):
            s = one_step(eng, x[k * B:(k + 1) * B], t[k * B:(k + 1) * B], hp, beta, ml, L)
            reps = r6.check_step_relu(s)
            record(case, reps)
            bad += ["step %d %s" % (k + 1, ln) for ln in fail_lines(reps)]
            for l, f in r6.zero_fractions(s).items():
                print("%s step %d layer %d: %.3f of y are zero" % (case, k + 1, l, f))
                assert r6.ZERO_FRACTION[0] <= f <= r6.ZERO_FRACTION[1], (k, l, f)
                assert (s.dedx[l][s.y[l] == 0] == 0).all() and not np.signbit(s.dedx[l][s.y[l] == 0]).any()
    finally:
        eng.close()
    assert not bad, case + "\n" + "\n".join(bad)


def test_the_64x64_kernels(pkg, monkeypatch):
    """MLGGD_TILE64=2 at [96, 128, 128, 40], B = 64: k_fwd64<FWD_RELU> for both hidden layers and k_dx64<ACT_RELU> for
    both dX launches -- the plan must say so -- within the bounds (one chain per output element: another order than the
    32 x 32 kernels', so no bit identity with them)"""
    ls, B, hp = [96, 128, 128, 40], 64, r6.CASE_HP
    W, b = b6.make_net(ls, 41)
    x, t = b6.make_data(ls, 2 * B, 42)
    eng = new_engine(pkg, monkeypatch, ls, B, hp, 1.2, 1, W, b, {"MLGGD_TILE64": "2"})
    bad = []
    try:
        plan = eng.gemm_plan()
        assert plan[0][0] == 1 and plan[1] == (1, 1) and plan[2][1] == 1, plan
        for k in range(2):
            s = one_step(eng, x[k * B:(k + 1) * B], t[k * B:(k + 1) * B], hp, 1.2, 1, len(ls))
            reps = r6.check_step_relu(s)
            record("TILE64=2", reps)
            bad += fail_lines(reps)
            assert all(0.2 <= f <= 0.8 for f in r6.zero_fractions(s).values())
    finally:
        eng.close()
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# 3. exact data
def test_one_step_on_exactly_representable_data_equals_float64(pkg, monkeypatch):
    """[587, 96, 577], 128 rows, MMSE: inputs in {-1, 0, 1}, weights multiples of 1/8, targets multiples of 1/4, lrate
    and momentum powers of two, no weight cost.  The test first asserts the condition that makes the step exact: at
    every GEMM and every update, sum |a||b| per element in units of the common quantum is below 2^24, so every product
    and every partial sum in any order is an fp32 number.  Then out, y, both dedx, delta_w, delta_b and the new weights
    equal the float64 model's values, the ReLU mask included -- no bound."""
    c = r6.exact_case()
    rows, m = r6.exact_case_quanta(c)
    for name, worst in rows:
        assert worst < 2.0 ** 24, (name, worst)
    ls, n, hp = c["ls"], c["n"], (c["lr"], c["mom"], c["wc"])
    eng = new_engine(pkg, monkeypatch, ls, n, hp, c["beta"], c["ml"], c["W"], c["b"])
    try:
        s = one_step(eng, c["x"], c["t"], hp, c["beta"], c["ml"], len(ls))
    finally:
        eng.close()

    def same(name, got, want):
        want32 = want.astype(np.float32)
        assert np.array_equal(want32.astype(np.float64), want), name        # the model's value is an fp32 number
        bad = np.argwhere(got != want32)
        assert bad.size == 0, "%s: first differing %s of %d" % (name, bad[:5].tolist(), len(bad))

    same("y 1", s.y[1], m["y"][1])
    assert np.array_equal(s.y[1] == 0, m["y"][1] == 0) and 0.2 <= (s.y[1] == 0).mean() <= 0.8
    same("out", s.out, m["out"])
    same("dedx 2", s.dedx[2], m["dedx"][2])
    same("dedx 1", s.dedx[1], m["dedx"][1])
    assert np.array_equal(s.dedx[1] == 0, (m["y"][1] == 0) | (m["dedx"][1] == 0))
    for l in (0, 1):
        same("delta_w %d" % (l + 1), s.dW_new[l], m["dW_new"][l])
        same("delta_b %d" % (l + 1), s.db_new[l], m["db_new"][l])
        same("W %d" % (l + 1), s.W_new[l], m["W_new"][l])
        same("b %d" % (l + 1), s.b_new[l], m["b_new"][l])
    assert np.abs(s.dW_new[0][576:, :]).max() > 0 and np.abs(s.dW_new[1][:, 576]).max() > 0   # the edge strips moved


# ---------------------------------------------------------------------------------------------------------------------
# 4. special values
def test_special_values_of_the_rule(pkg, monkeypatch):
    W, b = b6.make_net([8, 4, 3], 1)
    eng = new_engine(pkg, monkeypatch, [8, 4, 3], 8, r6.CASE_HP, 2.0, 0, W, b)
    sub = np.float32(2.0 ** -140)
    x = np.array([np.nan, -0.0, -sub, sub, -np.inf, np.inf, 1.5, -1.5, 0.0], np.float32)
    try:
        y = eng.debug_math("relu", x)
    finally:
        eng.close()
    assert np.isnan(y[0])                                   # a diverged net stays visible
    assert y[1] == 0 and y[2] == 0 and not np.signbit(y[2])
    assert y[3].tobytes() == sub.tobytes()                  # a positive subnormal passes unchanged
    assert y[4] == 0 and y[5] == np.inf and y[6] == np.float32(1.5) and y[7] == 0 and y[8] == 0


def test_kernel_work_does_not_depend_on_the_activation(pkg, monkeypatch):
    """the figures are the GEMM's multiply-adds and tensors; no epilogue is counted for either activation"""
    ls = [96, 128, 128, 40]
    W, b = b6.make_net(ls, 1)
    got = {}
    for act in ("sigmoid", "relu"):
        eng = new_engine(pkg, monkeypatch, ls, 64, r6.CASE_HP, 2.0, 0, W, b, activation=act)
        got[act] = [eng.kernel_work(c, l) for c in ("fwd", "dx", "dw") for l in (0, 1, 2, 3)]
        eng.close()
    assert got["relu"] == got["sigmoid"] and got["relu"][1][0] == 2.0 * 64 * 96 * 128


# ---------------------------------------------------------------------------------------------------------------------
# 5. dropout
def test_dropout_masks_are_the_sigmoid_engine_s(pkg, monkeypatch):
    """The mask generator does not look at values: with one seed, shape and step a ReLU and a sigmoid engine drop the
    same units.  The sigmoid of these nets never rounds to 0, so its y == 0 IS its mask: there the ReLU engine's y is
    exactly 0, everywhere else it meets the ReLU bound on its own masked inputs; dX gives a dropped unit no gradient."""
    ls, B, hp = [45, 70, 33, 9], 128, r6.CASE_HP
    L = len(ls)
    W, b = b6.make_net(ls, 51)
    x, t = b6.make_data(ls, 2 * B, 52)
    kw = dict(dropoutflag=1, visible_omit=0.0, hid_omit=0.5)
    engs = {a: new_engine(pkg, monkeypatch, ls, B, hp, 2.0, 0, W, b, activation=a, **kw) for a in ("relu", "sigmoid")}
    bad = []
    try:
        for k in range(2):
            xb, tb = x[k * B:(k + 1) * B], t[k * B:(k + 1) * B]
            pre = state(engs["relu"], L)
            for e in engs.values():
                assert e.train(xb, tb) == 1
            s = read_step(engs["relu"], xb, tb, pre, hp[0], hp, 2.0, 0, L)
            reps = []
            for l in (1, 2):
                dropped = engs["sigmoid"].debug_tensor("y", l) == 0
                assert 0.4 <= dropped.mean() <= 0.6
                assert (s.y[l][dropped] == 0).all()
                exp = r6.expect_relu_dropout_layer(xb if l == 1 else s.y[l - 1], s.W[l - 1], s.b[l - 1], dropped)
                reps.append(b6.compare("dropout fwd %d" % l, s.y[l], exp))
                reps.append(b6.compare("dropout dx %d" % l, s.dedx[l], r6.expect_dx_relu(s.dedx[l + 1], s.W[l], s.y[l])))
                assert (s.dedx[l][dropped] == 0).all()
                assert ((s.y[l] > 0) & ~dropped).mean() > 0.1              # kept and on: the bound is exercised
            record("dropout 0.5", reps)
            bad += fail_lines(reps)
    finally:
        for e in engs.values():
            e.close()
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# 6. data parallel, emulated
@pytest.mark.parametrize("mode", list(MODES))
def test_emulated_world_of_two(pkg, monkeypatch, mode):
    """fake_world(2) x 32 rows for each exchange: the ranks' rows stacked in rank order are one step of 64 rows
    (tests/bounds64.py: the any-order bounds cover the per-rank chains), checked by check_step_relu -- an exchange with
    an activation of its own would show in y, dedx or dW.  An emulated world holds one copy of the weights, so that the
    replicas are identical is checked on what the ranks compute: in the second step both ranks get the same 32 rows and
    must produce the same bits of y, out and dedx."""
    ls, B, world, hp, beta, ml = r6.CASE_LS, 32, 2, r6.CASE_HP, 0.9, 1
    L, n = len(ls), 64
    W, b = b6.make_net(ls, 61)
    x, t = b6.make_data(ls, n + B, 62)
    steps = [(x[:n], t[:n]), (np.vstack([x[n:], x[n:]]), np.vstack([t[n:], t[n:]]))]
    eng = new_engine(pkg, monkeypatch, ls, B, hp, beta, ml, W, b)
    bad = []
    try:
        set_world(eng, mode, world)
        assert eng.dp_mode() == MODES[mode]
        eng.keep_ranks()
        for k, (xb, tb) in enumerate(steps):
            pre = state(eng, L)
            assert eng.train(xb, tb) == 1
            s = read_dp_step(eng, xb, tb, pre, hp, beta, ml, L, world, set(range(1, L)))
            reps = r6.check_step_relu(s)
            record("emulated 2 x 32 %s" % mode, reps)
            bad += ["step %d %s" % (k + 1, ln) for ln in fail_lines(reps)]
            assert all(0.2 <= f <= 0.8 for f in r6.zero_fractions(s).values())
        for a in [s.y[1], s.y[2], s.out, s.dedx[1], s.dedx[2], s.dedx[3]]:
            assert a[:B].tobytes() == a[B:].tobytes()
    finally:
        eng.close()
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------
# 7. decoding
@pytest.fixture(scope="module")
def decoder(pkg):
    rng = np.random.default_rng(71)
    ls = [7 * 257, 64, 257]
    ws = [rng.normal(0, 0.05, (ls[i], ls[i + 1])).astype(np.float32) for i in range(2)]
    bs = [rng.normal(0, 0.1, ls[i + 1]).astype(np.float32) for i in range(2)]
    mean, inv = norm_stats(rng)
    eng = pkg.BPGpu(1, 0, ls, 16, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0, activation="relu")
    yield eng, mean, inv, (ls, ws, bs)
    eng.close()


def test_enhance_wave_equals_the_public_pieces(pkg, decoder):
    eng, mean, inv, (ls, ws, bs) = decoder
    noisy = spec64.synth_speech(4800, 16, seed=72)                    # 0.3 s: 17 frames, two bunches of 16
    out, outf = eng.enhance_wave(noisy, mean, inv, fea_context=7, return_float=True)
    (pout, poutf), lps, _ = chain_from_pieces(pkg, eng, noisy, mean, inv, 7)
    assert out.size == 17 * 256 + 256 and np.array_equal(outf, poutf) and np.array_equal(out, pout)
    y1 = eng.debug_tensor("y", 1)
    assert (y1 == 0).any() and (y1 > 0).any()                         # ... of a net whose rectifier does cut
    sig = pkg.BPGpu(1, 0, ls, 16, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0)
    assert not np.array_equal(sig.enhance_wave(noisy, mean, inv), out)
    sig.close()


def test_a_live_group_emits_enhance_wave_s_samples(pkg, decoder):
    eng, mean, inv, _ = decoder
    w = spec64.synth_speech(4800, 16, seed=73)
    want = eng.enhance_wave(w, mean, inv, fea_context=7, return_float=True)
    live = eng.live(mean, inv, 1, fea_context=7)
    steps = [(700, False), (0, False), (1, False), (2300, False), (255, False), (w.size - 3256, True)]
    same_as(feed(live, [w], [steps])[0], want)
    live.close()


def test_enhance_waves_equals_the_single_calls(pkg, decoder):
    eng, mean, inv, _ = decoder
    waves = [spec64.synth_speech(n, 16, seed=74 + i) for i, n in enumerate((4800, 512, 3000))]
    outs, outfs = eng.enhance_waves(waves, mean, inv, return_f32=True)
    for w, o, f in zip(waves, outs, outfs):
        same_as((o, f), eng.enhance_wave(w, mean, inv, fea_context=7, return_float=True))


# ---------------------------------------------------------------------------------------------------------------------
# 8. wave training and the error model
def test_train_waves_equals_train_frames_on_host_built_rows(pkg, synth):
    fs, ctx, B, D = 16, 7, 32, 257
    L, S, _ = spec64.params(fs)
    cleans = [spec64.synth_speech(F * S + L - S + i, fs, seed=81 + i) for i, F in enumerate((50, 40))]
    noise = np.random.default_rng(82).integers(-2500, 2501, 9000).astype(np.int16)
    snr, start, seg = [0.0, 10.0], [17, 300], [(0, 4000), (1000, 5000)]
    noisys = pkg.mix_waves(cleans, noise, snr, start, noise_seg=seg)
    rowsN = np.concatenate([pkg.wave_to_lps(w, fs_khz=fs) for w in noisys])
    rowsC = np.concatenate([pkg.wave_to_lps(w, fs_khz=fs) for w in cleans])
    mean, inv = rowsN.mean(0).astype(np.float32), (1.0 / rowsN.std(0)).astype(np.float32)
    feat, targ = (rowsN - mean) * inv, (rowsC - mean) * inv
    table = pkg.wave_samples([w.size for w in cleans], ctx, fs)
    first = table[np.random.default_rng(83).permutation(table.size)]
    assert first.size // B == 2
    ls = [ctx * D, 64, D]
    ws, bs = synth.make_weights(ls, seed=84)
    bs = [np.random.default_rng(85 + i).uniform(-0.3, 0.3, v.size).astype(np.float32) for i, v in enumerate(bs)]
    make = lambda: pkg.BPGpu(1, 0, ls, B, 0.01, 0.9, 1e-5, ws, bs, 0.9, 1, activation="relu")
    ref = make()
    assert ref.train_frames(feat, targ, first, ctx, ctx // 2) == 2
    want = sum(ref.returnWeights(), []) + [ref.scalefactor()]
    y1 = ref.debug_tensor("y", 1)
    ref.close()
    assert (y1 == 0).any() and (y1 > 0).any() and not np.array_equal(want[0], ws[0])
    eng = make()
    eng.set_noise(noise)
    assert eng.train_waves(cleans, snr, start, mean, inv, first, ctx // 2, noise_seg=seg, fea_context=ctx, fs_khz=fs) == 2
    got = sum(eng.returnWeights(), []) + [eng.scalefactor()]
    eng.close()
    for i, (a, w) in enumerate(zip(got, want)):
        assert a.tobytes() == w.tobytes(), "tensor %d" % i


def test_error_stats_are_sums_over_forward_s_outputs(pkg, pyoracle, monkeypatch):
    ls, B, n = [99, 64, 33], 32, 2 * 32 + 7
    W, b = b6.make_net(ls, 91)
    x, t = b6.make_data(ls, n, 92)
    betas = np.array([0.9, 1.0, 2.0], np.float32)
    eng = new_engine(pkg, monkeypatch, ls, B, r6.CASE_HP, 1.2, 1, W, b)
    try:
        out = eng.forward(x)
        got = eng.error_stats(x, t, betas)
        y1 = eng.debug_tensor("y", 1)
    finally:
        eng.close()
    assert (y1 == 0).any() and (y1 > 0).any()
    want, bound = pin(pyoracle, out, t, betas)
    mag = bound / (2.0 * n * 2.0 ** -53)                               # sum |term| per entry
    assert (np.abs(got - want) <= 1e-12 * mag).all()


# ---------------------------------------------------------------------------------------------------------------------
# 9. executables
DIM, CTX, EB, TOFF = 257, 3, 32, 1
ELS = [DIM * CTX, 64, DIM]


def run_tool(argv, cwd):
    os.makedirs(cwd, exist_ok=True)
    r = subprocess.run([str(a) for a in argv], capture_output=True, text=True, timeout=300, cwd=cwd)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def test_the_executables(pkg, tmp_path):
    """BPtrain_ReLU and BPtrain_Sigmoid activation=relu train the same net from the original project's sample for one
    epoch -- identical weights files, different from the sigmoid run's -- and enhance_wav activation=relu decodes with
    it to the bytes of the Python call"""
    d = tmp_path
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    sample = hostlib.sample_pfiles(d / "tools_pfile")
    rng = np.random.default_rng(5)
    ws = [rng.normal(0, 0.05, (ELS[i], ELS[i + 1])).astype(np.float32) for i in range(2)]
    bs = [rng.normal(0, 0.1, ELS[i + 1]).astype(np.float32) for i in range(2)]
    hostlib.write_wts(str(d / "init.wts"), ws, bs)
    kv = dict(gpu_used=0, numlayers=3, layersizes=",".join(map(str, ELS)), bunchsize=EB, MLflag=1, shapefactor=1.2,
              fea_dim=DIM, fea_context=CTX, traincache=500, init_randem_seed=27870775, targ_offset=TOFF,
              initwts_file=d / "init.wts", norm_file=os.path.join(sample, "train_noisy.norm"),
              fea_file=os.path.join(sample, "train_noisy.pfile"), targ_file=os.path.join(sample, "train_clean.pfile"),
              outwts_file="mlp.wts", log_file="mlp.log", train_sent_range="0-7", cv_sent_range="8-9", dropoutflag=0,
              visible_omit=0.1, hid_omit=0.1, lrate=0.01, momentum=0.9, weightcost=1e-5)
    args = ["%s=%s" % kvp for kvp in kv.items()]
    exe = lambda name: os.path.join(hostlib.HOST, name)
    by_name = run_tool([exe("BPtrain_ReLU")] + args, d / "by_name")
    by_key = run_tool([exe("BPtrain_Sigmoid")] + args + ["activation=relu"], d / "by_key")
    plain = run_tool([exe("BPtrain_Sigmoid")] + args, d / "plain")
    assert "is relu" in by_name.stdout and "is relu" in by_key.stdout and "is sigmoid" in plain.stdout
    wts = lambda name: open(d / name / "mlp.wts", "rb").read()
    assert wts("by_name") == wts("by_key") and len(wts("by_name")) > 4 * ELS[0] * ELS[1]
    assert wts("by_name") != wts("plain")
    assert run_tool([exe("BPtrain_ReLU")] + args + ["activation=sigmoid"], d / "back") and wts("back") == wts("plain")

    w = spec64.synth_speech(4800, 16, seed=95)
    write_wav(d / "n.wav", w)
    norm = os.path.join(sample, "train_noisy.norm")
    run_tool([exe("enhance_wav"), "wts=%s" % (d / "by_name" / "mlp.wts"), "norm_file=%s" % norm, "fea_context=%d" % CTX,
              "bunchsize=64", "activation=relu", "in=%s" % (d / "n.wav"), "out=%s" % (d / "e.wav")], d)
    mean, inv = hostlib.HostNorm.read(norm, DIM)
    tw, tb = hostlib.read_wts(str(d / "by_name" / "mlp.wts"), ELS)
    eng = pkg.BPGpu(1, 0, ELS, 64, 0.1, 0.9, 1e-5, tw, tb, 2.0, 0, activation="relu")
    want = eng.enhance_wave(w, np.asarray(mean, np.float32), np.asarray(inv, np.float32), fea_context=CTX)
    eng.close()
    got, rate = read_wav(d / "e.wav")
    assert rate == 16000 and np.array_equal(got, want)
