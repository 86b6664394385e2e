"""GPU: noise-aware training through the frames entries -- forward_frames_nat / cv_all_frames_nat / train_frames_nat /
load_frames_nat on a NAT engine against forward / cv_all / train on rows [window | noise row] expanded on the host
(tests/nat_model.py).  Staging is a copy, so every comparison is bit for bit; and the argument and state errors, after
which the engine still gives those bits.  The corners at the end: the chunk capacity at n_samples and one below it, the
64 x 64 kernels at bunches of 64 and 128, every launch knob, per-bin shape factors, the error model's sums and the
expanded and the NAT entries in turn on one engine."""
import ctypes as C

import numpy as np
import pytest

import bounds64 as b6
import ggd64
import nat_model
from test_gpu_vs_float64 import KNOBS

pytestmark = pytest.mark.gpu
T = 6
# (fdim, ctx): 13 x 3 = 39 -- the noise row starts inside a 32-column tile and the pad follows it (52 -> 64); 40 x 1 --
# the noise row crosses a tile boundary (40..79); 257 x 7 -- the shipped bin count.  Bunches of 32 and of 40 (Bp = 64).
SHAPES = [(13, 3), (40, 1), (257, 7)]
FRAMES = [9, 1, 30, T - 1, T, T + 1, 12, 3, 25, 40, 18]


class Data:
    """a chunk of utterances: normalised rows, targets, a shuffled sample table with repeats and its noise rows"""

    def __init__(self, fdim, ctx, seed=0, twice=7, hidden=64):
        rng = np.random.default_rng(100 * fdim + ctx + seed)
        self.fdim, self.ctx = fdim, ctx
        self.fo = np.concatenate([[0], np.cumsum(FRAMES)]).astype(np.int32)
        n = int(self.fo[-1])
        self.feat = rng.standard_normal((n, fdim)).astype(np.float32)
        self.targ = rng.standard_normal((n, fdim)).astype(np.float32)
        table = np.array([f for u in range(len(FRAMES)) for f in range(self.fo[u], self.fo[u + 1] - ctx + 1)], np.int32)
        first = table[rng.permutation(table.size)]
        self.first = np.concatenate([first, first[:twice]])              # some samples twice
        self.toff = ctx // 2
        self.nat = nat_model.noise_rows(self.feat, self.fo, T)
        self.nat_row = nat_model.utt_of_frames(self.fo, self.first)
        assert len(set(self.nat_row.tolist())) >= 3 and (np.diff(self.nat_row) < 0).any()   # repeated, out of order
        self.rows = nat_model.expand(self.feat, self.first, ctx, self.nat, self.nat_row)
        self.trows = self.targ[self.first + self.toff]
        self.n = self.first.size
        self.ls = [(ctx + 1) * fdim, hidden, hidden, fdim]


HP = (0.01, 0.9, 1e-5)
NO_MOM = (0.01, 0.0, 1e-5)         # weights, biases and the scale are then all a step hands to the next one


def engine(pkg, synth, d, B, nat=T, ml=1, act="sigmoid", drop=0, beta=1.2, cap=0, hp=HP, net=None):
    ws, bs = net or synth.make_weights(d.ls, seed=11)
    return pkg.BPGpu(3, 0, d.ls, B, *hp, ws, bs, beta, ml, dropoutflag=drop, visible_omit=0.1, hid_omit=0.2,
                     activation=act, nat_frames=nat, max_cache_frames=cap)


def state(eng):
    ws, bs = eng.returnWeights()
    return ws + bs + [eng.scalefactor()]


def same_bits(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), "tensor %d" % i


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "%dx%d" % s)
def data(request):
    return Data(*request.param)


@pytest.mark.parametrize("B", [32, 40])
def test_forward_and_cv_equal_the_expanded_rows(pkg, synth, data, B):
    d = data
    assert d.n % B != 0 and d.n > 2 * B                                     # more than one bunch and a trailing partial one
    eng = engine(pkg, synth, d, B)
    assert eng.nat_frames == T
    assert eng.train(d.rows, d.trows) == d.n // B                           # a scale per bin: the log-likelihood is finite
    want = eng.forward(d.rows)
    got = eng.forward_frames_nat(d.feat, d.first, d.ctx, d.nat, d.nat_row)
    assert got.shape == (d.n, d.fdim) and np.isfinite(got).all() and got.tobytes() == want.tobytes()
    # the noise row matters: with another table the outputs move
    other = eng.forward_frames_nat(d.feat, d.first, d.ctx, d.nat[::-1].copy(), d.nat_row)
    assert other.tobytes() != want.tobytes()
    for on in (False, True):                                                 # sums in host order, then on the device
        eng.set_cv_device_reduce(on)
        ref = eng.cv_all(d.rows, d.trows)
        cv = eng.cv_all_frames_nat(d.feat, d.targ, d.first, d.ctx, d.toff, d.nat, d.nat_row)
        print("cv", on, cv, ref)
        assert np.isfinite(cv).all()
        assert np.array(cv, np.float32).tobytes() == np.array(ref, np.float32).tobytes()
    eng.close()


TRAIN = [(fdim, ctx, B) for (fdim, ctx), B in (((13, 3), 32), ((40, 1), 40))]


@pytest.mark.parametrize("drop", [0, 1], ids=["nodrop", "dropout"])
@pytest.mark.parametrize("act", ["sigmoid", "relu"])
@pytest.mark.parametrize("loss", ["mmse", "mlggd"])
@pytest.mark.parametrize("shape", TRAIN, ids=lambda s: "%dx%d_B%d" % s)
def test_training_equals_training_on_the_expanded_rows(pkg, synth, shape, loss, act, drop):
    """weights, biases and scalefactor after train_frames_nat = those after train on [window | noise row]: MMSE
    (the 2-norm) and ML-GGD at beta = 1.2, both activations, with and without dropout"""
    fdim, ctx, B = shape
    d = Data(fdim, ctx)
    ml, beta = (1, 1.2) if loss == "mlggd" else (0, 2.0)
    ref = engine(pkg, synth, d, B, ml=ml, act=act, drop=drop, beta=beta)
    start = state(ref)
    assert ref.train(d.rows, d.trows) == d.n // B >= 3
    want = state(ref)
    ref.close()
    assert all(np.isfinite(a).all() for a in want) and any(a.tobytes() != b.tobytes() for a, b in zip(want, start))
    eng = engine(pkg, synth, d, B, ml=ml, act=act, drop=drop, beta=beta)
    assert eng.train_frames_nat(d.feat, d.targ, d.first, d.ctx, d.toff, d.nat, d.nat_row) == d.n // B
    same_bits(state(eng), want)
    eng.close()
    # load_frames_nat + train_resident over the same samples: the same steps
    eng = engine(pkg, synth, d, B, ml=ml, act=act, drop=drop, beta=beta)
    eng.load_frames_nat(d.feat, d.targ, d.first, d.ctx, d.toff, d.nat, d.nat_row)
    assert eng.train_resident(0, d.n) == d.n // B
    eng.sync()
    same_bits(state(eng), want)
    eng.close()


def test_errors_leave_the_engine_usable_and_its_weights_unchanged(pkg, synth):
    d = Data(13, 3)
    B = 32
    eng = engine(pkg, synth, d, B)
    start = state(eng)
    nat_args = (d.feat, d.targ, d.first, d.ctx, d.toff, d.nat, d.nat_row)
    bad = d.nat_row.copy()
    bad[5] = d.nat.shape[0]
    with pytest.raises(pkg.MlggdError, match=r"error 1: sample 5: nat_row %d outside the %d noise rows" % (bad[5], bad[5])):
        eng.train_frames_nat(d.feat, d.targ, d.first, d.ctx, d.toff, d.nat, bad)
    bad[5] = -1
    with pytest.raises(pkg.MlggdError, match=r"error 1: sample 5: nat_row -1"):
        eng.forward_frames_nat(d.feat, d.first, d.ctx, d.nat, bad)
    # NULL pointers and a context that does not fit layer 0, straight through the C entry
    L = pkg.load()
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    first, rows = d.first.ctypes.data_as(ip), d.nat_row.ctypes.data_as(ip)
    feat, targ, nat = (a.ctypes.data_as(fp) for a in (d.feat, d.targ, d.nat))
    n_fr, n_nat = d.feat.shape[0], d.nat.shape[0]
    trained = C.c_int(0)
    for a_nat, a_rows in ((None, rows), (nat, None)):
        assert L.mlggd_train_frames_nat(eng._h, n_fr, d.ctx, feat, targ, d.n, first, d.toff, n_nat, a_nat, a_rows,
                                        C.byref(trained)) == 1
        assert "nat/nat_row is NULL" in L.mlggd_last_error().decode()
    assert L.mlggd_load_frames_nat(eng._h, n_fr, d.ctx, None, targ, d.n, first, d.toff, n_nat, nat, rows) == 1
    assert L.mlggd_load_frames_nat(eng._h, n_fr, d.ctx + 1, feat, targ, d.n, first, d.toff, n_nat, nat, rows) == 1
    assert "(fea_context 4 + 1) does not divide layersizes[0] = 52" in L.mlggd_last_error().decode()
    # the plain frames entries have no noise rows: a state error on a NAT engine, each of them
    for call in (lambda: L.mlggd_load_frames(eng._h, n_fr, d.ctx, feat, targ, d.n, first, d.toff),
                 lambda: L.mlggd_train_frames(eng._h, n_fr, d.ctx, feat, targ, d.n, first, d.toff, C.byref(trained)),
                 lambda: L.mlggd_train_frames_async(eng._h, n_fr, d.ctx, feat, targ, d.n, first, d.toff, C.byref(trained)),
                 lambda: L.mlggd_cv_all_frames(eng._h, n_fr, d.ctx, feat, targ, d.n, first, d.toff, C.byref(C.c_float()),
                                               C.byref(C.c_float()), C.byref(C.c_float())),
                 lambda: L.mlggd_forward_frames(eng._h, n_fr, d.ctx, feat, d.n, first, targ),
                 lambda: L.mlggd_error_stats_frames(eng._h, n_fr, d.ctx, feat, targ, d.n, first, d.toff, 1,
                                                    np.array([1.2], np.float32).ctypes.data_as(fp),
                                                    np.zeros((5, d.fdim)).ctypes.data_as(C.POINTER(C.c_double)))):
        assert call() == 4
        assert "mlggd_*_frames_nat" in L.mlggd_last_error().decode()
    with pytest.raises(pkg.MlggdError, match="error 4: mlggd_debug_fake_world"):
        eng.fake_world(2)
    with pytest.raises(pkg.MlggdError, match="error 4: mlggd_comm_init"):
        eng.comm_init(bytes(pkg.UNIQUE_ID_BYTES), 1, 0)
    same_bits(state(eng), start)                                             # nothing moved ...
    ref = engine(pkg, synth, d, B)
    ref.train(d.rows, d.trows)
    assert eng.train_frames_nat(*nat_args) == d.n // B                       # ... and the engine trains as a fresh one
    same_bits(state(eng), state(ref))
    ref.close()
    eng.close()


def test_an_engine_without_nat_frames_refuses_the_nat_entries(pkg, synth):
    d = Data(13, 3)
    eng = engine(pkg, synth, d, 32, nat=0)
    assert eng.nat_frames == 0
    start = state(eng)
    with pytest.raises(pkg.MlggdError, match="error 4: mlggd_load_frames_nat needs an engine with nat_frames > 0"):
        eng.load_frames_nat(d.feat, d.targ, d.first, d.ctx, d.toff, d.nat, d.nat_row)
    with pytest.raises(pkg.MlggdError, match="error 4: mlggd_train_frames_nat"):
        eng.train_frames_nat(d.feat, d.targ, d.first, d.ctx, d.toff, d.nat, d.nat_row)
    with pytest.raises(pkg.MlggdError, match="error 4: mlggd_cv_all_frames_nat"):
        eng.cv_all_frames_nat(d.feat, d.targ, d.first, d.ctx, d.toff, d.nat, d.nat_row)
    with pytest.raises(pkg.MlggdError, match="error 4: mlggd_forward_frames_nat"):
        eng.forward_frames_nat(d.feat, d.first, d.ctx, d.nat, d.nat_row)
    same_bits(state(eng), start)
    # the same layer sizes without NAT are a plain engine of context ctx + 1 over the same stream: still served
    first = d.first[d.first + d.ctx + 1 <= d.feat.shape[0]]
    out = eng.forward_frames(d.feat, first, d.ctx + 1)
    assert out.shape == (first.size, d.fdim) and np.isfinite(out).all()
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# corners: the chunk capacity, the 64 x 64 kernels, the launch knobs, per-bin shapes, the error model, mixed entries
def test_the_chunk_capacity_admits_n_samples_and_refuses_one_more(pkg, synth):
    """load_frames_nat with n_samples == max_cache_frames trains to the uncapped bits; with one sample more it is an
    argument error that moves nothing, after which the engine trains the chunk without its last sample -- the trailing
    partial bunch is skipped either way -- to the same bits"""
    d = Data(13, 3)
    B = 32
    assert d.n % B > 1
    ref = engine(pkg, synth, d, B)
    start = state(ref)
    assert ref.train(d.rows, d.trows) == d.n // B
    want = state(ref)
    ref.close()
    args = (d.feat, d.targ, d.first, d.ctx, d.toff, d.nat, d.nat_row)
    eng = engine(pkg, synth, d, B, cap=d.n)
    eng.load_frames_nat(*args)
    assert eng.train_resident(0, d.n) == d.n // B
    eng.sync()
    same_bits(state(eng), want)
    eng.close()
    eng = engine(pkg, synth, d, B, cap=d.n - 1)
    for call in (eng.load_frames_nat, eng.train_frames_nat, eng.cv_all_frames_nat):
        with pytest.raises(pkg.MlggdError, match=r"error 1: n_frames %d exceeds the chunk capacity %d" % (d.n, d.n - 1)):
            call(*args)
    with pytest.raises(pkg.MlggdError, match=r"error 1: .*exceeds the chunk capacity"):
        eng.forward_frames_nat(d.feat, d.first, d.ctx, d.nat, d.nat_row)
    same_bits(state(eng), start)
    eng.load_frames_nat(d.feat, d.targ, d.first[:-1], d.ctx, d.toff, d.nat, d.nat_row[:-1])
    assert eng.train_resident(0, d.n - 1) == d.n // B
    eng.sync()
    same_bits(state(eng), want)
    eng.close()


@pytest.mark.parametrize("B", [64, 128])
def test_the_64_tile_kernels_and_a_bunch_of_128(pkg, synth, monkeypatch, B):
    """MLGGD_TILE64=2 on 52-128-128-13: layer 0 is 52 wide (no multiple of 32; the noise row begins at column 39) and
    the hidden layers run the 64 x 64 forward and dX kernels.  Training, forward and both CV reductions against the
    expanded entries bit for bit, the forward also against float64."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MLGGD_TILE64", "2")
    d = Data(13, 3, twice=135, hidden=128)
    assert d.ls == [52, 128, 128, 13] and d.n > 2 * B and d.n % B != 0
    net = b6.make_net(d.ls, 21)
    ref = engine(pkg, synth, d, B, net=net)
    plan = ref.gemm_plan()
    assert plan[0][0] == 1 and plan[1] == (1, 1), plan
    assert ref.train(d.rows, d.trows) == d.n // B >= 2
    want = state(ref)
    eng = engine(pkg, synth, d, B, net=net)
    assert eng.train_frames_nat(d.feat, d.targ, d.first, d.ctx, d.toff, d.nat, d.nat_row) == d.n // B
    same_bits(state(eng), want)
    out = eng.forward_frames_nat(d.feat, d.first, d.ctx, d.nat, d.nat_row)
    assert out.tobytes() == ref.forward(d.rows).tobytes()
    W, b = eng.returnWeights()
    rep = b6.compare("forward TILE64=2 B%d" % B, out, b6.expect_forward_chain(d.rows, W, b, eng.out_slabs()))
    print(rep.line())
    assert rep.ok, rep.line()
    for on in (False, True):
        for e in (eng, ref):
            e.set_cv_device_reduce(on)
        cv = eng.cv_all_frames_nat(d.feat, d.targ, d.first, d.ctx, d.toff, d.nat, d.nat_row)
        assert np.isfinite(cv).all()
        assert np.array(cv, np.float32).tobytes() == np.array(ref.cv_all(d.rows, d.trows), np.float32).tobytes()
    ref.close()
    eng.close()


NON_DEFAULT = {"MLGGD_TILE64": "2", "MLGGD_S_OUT": "3", "MLGGD_LOSS_FUSE": "0", "MLGGD_DW_MERGE": "0",
               "MLGGD_STAGE_AHEAD": "0", "MLGGD_CV_DEVICE": "1", "MLGGD_DW_TILE": "2", "MLGGD_DW_PERSIST": "0",
               "MLGGD_DWP_PER_CU": "1", "MLGGD_TILE_MAP": "1"}
assert set(NON_DEFAULT) == set(KNOBS)


@pytest.mark.parametrize("knob", KNOBS)
def test_every_launch_knob_leaves_the_nat_entries_on_the_expanded_bits(pkg, synth, monkeypatch, knob):
    """a NAT engine stages its rows in a launch of its own, outside the loss launch, so the knobs that move staging
    (MLGGD_STAGE_AHEAD, MLGGD_LOSS_FUSE) must not reach it; nor any other.  Both engines are created under the knob."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv(knob, NON_DEFAULT[knob])
    d = Data(13, 3)
    B = 32
    ref = engine(pkg, synth, d, B)
    if knob == "MLGGD_S_OUT":
        assert ref.out_slabs() == 3
    start = state(ref)
    assert ref.train(d.rows, d.trows) == d.n // B >= 3
    want = state(ref)
    ref.close()
    assert any(a.tobytes() != b.tobytes() for a, b in zip(want, start))
    eng = engine(pkg, synth, d, B)
    assert eng.train_frames_nat(d.feat, d.targ, d.first, d.ctx, d.toff, d.nat, d.nat_row) == d.n // B
    same_bits(state(eng), want)
    eng.close()


def uneven_shapes(D):
    return (0.8 + 0.9 * ((7 * np.arange(D)) % D) / D).astype(np.float32)      # 0.8 .. 1.7, no two neighbours alike


def test_per_bin_shape_factors_on_a_nat_engine(pkg, synth):
    d = Data(13, 3)
    B = 32
    betas = uneven_shapes(d.fdim)
    assert len(set(betas.tolist())) == d.fdim
    ref, eng = engine(pkg, synth, d, B), engine(pkg, synth, d, B)
    for e in (ref, eng):
        e.set_shapefactors(betas)
        assert e.shapefactors().tobytes() == betas.tobytes()
    assert ref.train(d.rows, d.trows) == d.n // B
    assert eng.train_frames_nat(d.feat, d.targ, d.first, d.ctx, d.toff, d.nat, d.nat_row) == d.n // B
    same_bits(state(eng), state(ref))
    uniform = engine(pkg, synth, d, B)
    uniform.train(d.rows, d.trows)
    assert any(a.tobytes() != b.tobytes() for a, b in zip(state(uniform), state(ref)))   # the vector is in the result
    uniform.close()
    for on in (False, True):
        for e in (eng, ref):
            e.set_cv_device_reduce(on)
        cv = eng.cv_all_frames_nat(d.feat, d.targ, d.first, d.ctx, d.toff, d.nat, d.nat_row)
        print("cv per bin", on, cv)
        assert np.isfinite(cv).all()
        assert np.array(cv, np.float32).tobytes() == np.array(ref.cv_all(d.rows, d.trows), np.float32).tobytes()
    ref.close()
    eng.close()


def test_error_stats_of_a_nat_engine(pkg, synth):
    """error_stats on the expanded rows of a NAT engine: the bits of a plain engine with the same layer sizes and
    weights (to the forward pass a NAT net is a net with a wider layer 0).  Against tests/ggd64.py with the bound of
    test_gpu_error_stats.py -- a double sum of n terms in any order is within 2 n 2^-53 sum|term| of math.fsum -- where
    float64 of the fp32 error IS the term: the four moments, and |e|^1 (the device's power returns its argument at
    shape 1).  The other powers are fp32 powers of the device, which that file pins; here they are compared with the
    plain engine's."""
    d = Data(13, 3)
    B = 32
    grid = np.array([0.5, 0.9, 1.0, 1.2, 2.0, 2.5], np.float32)
    nat, plain = engine(pkg, synth, d, B), engine(pkg, synth, d, B, nat=0)
    for e in (nat, plain):
        assert e.train(d.rows, d.trows) == d.n // B                             # weights that have moved
    same_bits(state(nat), state(plain))
    got = nat.error_stats(d.rows, d.trows, grid)
    assert got.shape == (4 + grid.size, d.fdim) and got.dtype == np.float64 and np.isfinite(got).all()
    assert got.tobytes() == plain.error_stats(d.rows, d.trows, grid).tobytes()
    out = nat.forward_frames_nat(d.feat, d.first, d.ctx, d.nat, d.nat_row)
    nat.close()
    plain.close()
    e = (out - d.trows).astype(np.float32)
    one = np.array([1.0], np.float32)
    want, mag = ggd64.sums(e, one), ggd64.sums(np.abs(e), one)
    bound = 2.0 * d.n * 2.0 ** -53 * mag
    rows = [0, 1, 2, 3, 4 + int(np.flatnonzero(grid == 1.0)[0])]
    err = np.abs(got[rows] - want)
    print("error_stats of a NAT engine: max |got - want| / bound = %.3g" % (err / np.maximum(bound, 1e-300)).max())
    assert (err <= bound).all(), np.argwhere(err > bound)[:5]


def test_expanded_and_nat_entries_alternate_on_one_engine(pkg, synth):
    """train on the expanded rows, then train_frames_nat on another chunk, on ONE engine (the expanded entry stages
    from the chunk buffer, the NAT entry from a raw set and its noise table) = the same two calls on two fresh engines,
    the second begun with the first one's weights, biases and scale; without momentum that is the whole state"""
    d1, d2 = Data(13, 3), Data(13, 3, seed=5)
    B = 32
    eng = engine(pkg, synth, d1, B, hp=NO_MOM)
    assert eng.train(d1.rows, d1.trows) == d1.n // B
    assert eng.train_frames_nat(d2.feat, d2.targ, d2.first, d2.ctx, d2.toff, d2.nat, d2.nat_row) == d2.n // B
    assert eng.train(d1.rows, d1.trows) == d1.n // B                          # ... and back
    got = state(eng)
    eng.close()
    st = None
    for k, d in enumerate((d1, d2, d1)):
        ref = engine(pkg, synth, d, B, hp=NO_MOM)
        if st is not None:
            ref.set_weights(st[:3], st[3:6])
            ref.set_scalefactor(st[6])
        if k == 1:
            assert ref.train_frames_nat(d.feat, d.targ, d.first, d.ctx, d.toff, d.nat, d.nat_row) == d.n // B
        else:
            assert ref.train(d.rows, d.trows) == d.n // B
        st = state(ref)
        ref.close()
    same_bits(got, st)
