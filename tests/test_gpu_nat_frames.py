"""GPU: noise-aware training through the frames entries -- forward_frames_nat / cv_all_frames_nat / train_frames_nat /
load_frames_nat on a NAT engine against forward / cv_all / train on rows [window | noise row] expanded on the host
(tests/nat_model.py).  Staging is a copy, so every comparison is bit for bit; and the argument and state errors, after
which the engine still gives those bits."""
import ctypes as C

import numpy as np
import pytest

import nat_model

pytestmark = pytest.mark.gpu
T = 6
# (fdim, ctx): 13 x 3 = 39 -- the noise row starts inside a 32-column tile and the pad follows it (52 -> 64); 40 x 1 --
# the noise row crosses a tile boundary (40..79); 257 x 7 -- the shipped bin count.  Bunches of 32 and of 40 (Bp = 64).
SHAPES = [(13, 3), (40, 1), (257, 7)]
FRAMES = [9, 1, 30, T - 1, T, T + 1, 12, 3, 25, 40, 18]


class Data:
    """a chunk of utterances: normalised rows, targets, a shuffled sample table with repeats and its noise rows"""

    def __init__(self, fdim, ctx, seed=0):
        rng = np.random.default_rng(100 * fdim + ctx + seed)
        self.fdim, self.ctx = fdim, ctx
        self.fo = np.concatenate([[0], np.cumsum(FRAMES)]).astype(np.int32)
        n = int(self.fo[-1])
        self.feat = rng.standard_normal((n, fdim)).astype(np.float32)
        self.targ = rng.standard_normal((n, fdim)).astype(np.float32)
        table = np.array([f for u in range(len(FRAMES)) for f in range(self.fo[u], self.fo[u + 1] - ctx + 1)], np.int32)
        first = table[rng.permutation(table.size)]
        self.first = np.concatenate([first, first[:7]])                  # some samples twice
        self.toff = ctx // 2
        self.nat = nat_model.noise_rows(self.feat, self.fo, T)
        self.nat_row = nat_model.utt_of_frames(self.fo, self.first)
        assert len(set(self.nat_row.tolist())) >= 3 and (np.diff(self.nat_row) < 0).any()   # repeated, out of order
        self.rows = nat_model.expand(self.feat, self.first, ctx, self.nat, self.nat_row)
        self.trows = self.targ[self.first + self.toff]
        self.n = self.first.size
        self.ls = [(ctx + 1) * fdim, 64, 64, fdim]


def engine(pkg, synth, d, B, nat=T, ml=1, act="sigmoid", drop=0, beta=1.2):
    ws, bs = synth.make_weights(d.ls, seed=11)
    return pkg.BPGpu(3, 0, d.ls, B, 0.01, 0.9, 1e-5, ws, bs, beta, ml, dropoutflag=drop, visible_omit=0.1, hid_omit=0.2,
                     activation=act, nat_frames=nat)


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
