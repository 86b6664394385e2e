"""GPU: the output statistics of a CV chunk (BPGpu.output_stats / output_stats_frames, csrc/colstats.hip.h).

The pin: out = eng.forward(inp), the four terms y, y*y, t, t*t in float64 from the fp32 values, every sum by
math.fsum.  A double sum of n terms in ANY order is within 2 n 2^-53 sum|term| of that, and nothing else separates the
two sides (tests/test_gpu_error_stats.py's argument), so that is the bound of every entry.  Beyond the pin: the two
entries return the same bits for the same rows, a call repeats its bits -- also after other calls have used the
engine's workspaces and without a new allocation --, chunks add up, and every refusal leaves an engine whose next
forward is unchanged bit for bit.

Shapes: those of tests/test_gpu_error_stats.py -- D = 33 (one bin past a 32-bin strip), context 3, net 99-64-33,
B = 32 and 128, n in {0, 1, 31, 32, 33, 2B + 7}; one net whose output layer is summed from several split-K slabs, one
ReLU engine, one NAT engine (the expanded entry)."""
import numpy as np
import pytest

import gv64
import nat_model
from test_gpu_error_stats import CTX, FDIM, LS, TOFF, make_chunk, make_engine, same_bits

pytestmark = pytest.mark.gpu
BETAS = np.array([0.5, 1.0, 2.0], np.float32)


@pytest.fixture(scope="module")
def engines(pkg, synth):
    made = {B: make_engine(pkg, synth, LS, B)[0] for B in (32, 128)}
    yield made
    for e in made.values():
        e.close()


def check_pin(got, out, targ, what):
    assert got.shape == (4, targ.shape[1]) and got.dtype == np.float64
    want, bound = gv64.pin(out, targ)
    err = np.abs(got - want)
    print("%s: max |got - want| / bound = %.3g" % (what, (err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all(), (what, np.argwhere(err > bound)[:5])


@pytest.mark.parametrize("B", [32, 128])
@pytest.mark.parametrize("n", [0, 1, 31, 32, 33, "2B+7"])
def test_sums_against_the_pin_and_both_entries_agree(pkg, engines, B, n):
    eng = engines[B]
    n = 2 * B + 7 if n == "2B+7" else n
    feat, tstream, first, inp, targ = make_chunk(n, seed=200 + n)
    out = eng.forward(inp) if n else np.zeros((0, FDIM), np.float32)
    got = eng.output_stats(inp, targ)
    check_pin(got, out, targ, "B %d n %d" % (B, n))
    assert same_bits(got, eng.output_stats(inp, targ))                               # a call repeats its bits
    assert same_bits(got, eng.output_stats_frames(feat, tstream, first, CTX, TOFF))  # the same rows
    if n == 0:
        assert not got.any()
    elif n > 1:
        assert pkg.gv_fit(n, got).fitted.all()


def test_an_output_layer_of_several_slabs(pkg, synth):
    B = 32
    eng, _, _ = make_engine(pkg, synth, [FDIM * CTX, 512, FDIM], B)
    try:
        assert eng.out_slabs() > 1
        n = B + 5
        feat, tstream, first, inp, targ = make_chunk(n, seed=7)
        got = eng.output_stats(inp, targ)
        check_pin(got, eng.forward(inp), targ, "slabs")
        assert same_bits(got, eng.output_stats_frames(feat, tstream, first, CTX, TOFF))
    finally:
        eng.close()


def test_a_relu_engine(pkg, synth):
    B = 32
    eng, _, _ = make_engine(pkg, synth, LS, B, activation="relu")
    try:
        n = 2 * B + 7
        feat, tstream, first, inp, targ = make_chunk(n, seed=17)
        got = eng.output_stats(inp, targ)
        check_pin(got, eng.forward(inp), targ, "relu")
        assert same_bits(got, eng.output_stats_frames(feat, tstream, first, CTX, TOFF))
    finally:
        eng.close()


def test_a_nat_engine_takes_the_expanded_entry_and_refuses_the_frames_entry(pkg, synth):
    B, T = 32, 4
    ls = [FDIM * (CTX + 1), 64, FDIM]
    eng, _, _ = make_engine(pkg, synth, ls, B, nat_frames=T)
    try:
        n = B + 9
        feat, tstream, first, _, targ = make_chunk(n, seed=18)
        z = nat_model.noise_rows(feat, [0, feat.shape[0]], T)
        rows = nat_model.expand(feat, first, CTX, z, np.zeros(n, np.int32))
        before = eng.forward(rows)
        got = eng.output_stats(rows, targ)
        check_pin(got, before, targ, "nat")
        with pytest.raises(pkg.MlggdError, match=r"error 4: the plain frames entries have no noise rows"):
            # to a NAT engine a stream of FDIM columns looks like a context of CTX + 1 frames: the state decides
            eng.output_stats_frames(feat, tstream, np.minimum(first, feat.shape[0] - CTX - 1), CTX + 1, TOFF)
        assert eng.forward(rows).tobytes() == before.tobytes()
        assert same_bits(eng.output_stats(rows, targ), got)
    finally:
        eng.close()


def test_chunks_add_up(pkg, engines):
    B = 32
    eng = engines[B]
    n = 3 * B + 9
    _, _, _, inp, targ = make_chunk(n, seed=8)
    whole = eng.output_stats(inp, targ)
    cut = 2 * B
    parts = eng.output_stats(inp[:cut], targ[:cut]) + eng.output_stats(inp[cut:], targ[cut:])
    _, bound = gv64.pin(eng.forward(inp), targ)
    assert (np.abs(parts - whole) <= bound).all()


def test_the_same_bits_after_other_calls_used_the_workspaces_and_no_new_allocation(pkg, synth):
    """error_stats, cv_all and an enhance_waves call in between"""
    fs, ctx, D, B = 8, 3, 129, 32
    eng, ws, bs = make_engine(pkg, synth, [D * ctx, 64, D], B)
    try:
        n = 2 * B + 7
        feat, tstream, first, inp, targ = make_chunk(n, seed=9, fdim=D, ctx=ctx, toff=1)
        eng.set_scalefactor(np.full(D, 0.7, np.float32))
        first_cv = eng.cv_all(inp, targ)
        want = eng.output_stats(inp, targ)
        assert eng.cv_all(inp, targ) == first_cv                       # output_stats leaves cv_all's results alone
        es = eng.error_stats(inp, targ, BETAS)
        assert same_bits(eng.output_stats(inp, targ), want)
        assert same_bits(eng.error_stats(inp, targ, BETAS), es)        # ... and error_stats'
        assert same_bits(eng.output_stats_frames(feat, tstream, first, ctx, 1), want)
        rng = np.random.default_rng(10)
        waves = [(3000 * rng.standard_normal(m)).astype(np.int16) for m in (2100, 900)]
        eng.enhance_waves(waves, np.zeros(D, np.float32), np.ones(D, np.float32), fs_khz=fs, fea_context=ctx)
        assert same_bits(eng.output_stats(inp, targ), want)
        # the factors are the decoders' business: setting them changes no statistic
        eng.set_gv(gv64.draw_eta(D, 2))
        assert same_bits(eng.output_stats(inp, targ), want)
        eng.set_gv(None)
        # a repeated call allocates nothing (frame-stream chunks alternate between the engine's two raw sets: two
        # calls have sized both)
        for _ in range(2):
            eng.output_stats_frames(feat, tstream, first, ctx, 1)
        allocs = eng.buffer_stats()[0]
        for _ in range(3):
            assert same_bits(eng.output_stats(inp, targ), want)
            assert same_bits(eng.output_stats_frames(feat, tstream, first, ctx, 1), want)
        assert eng.buffer_stats()[0] == allocs
    finally:
        eng.close()


def test_every_refusal_leaves_the_next_forward_unchanged(pkg, synth, engines):
    B = 32
    feat, tstream, first, inp, targ = make_chunk(B + 3, seed=12)
    # an emulated world
    fake, _, _ = make_engine(pkg, synth, LS, B)
    fake.fake_world(2, allreduce=True)
    before = fake.forward(inp)
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_output_stats runs on a single-device engine"):
        fake.output_stats(inp, targ)
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_output_stats_frames runs on a single-device engine"):
        fake.output_stats_frames(feat, tstream, first, CTX, TOFF)
    assert fake.forward(inp).tobytes() == before.tobytes()
    assert fake.train(np.tile(inp, (2, 1)), np.tile(targ, (2, 1))) == 1      # one global minibatch of 2 x B rows
    fake.close()
    # dropout
    # (a forward pass of a dropout engine scales W by the keep rate and back, as the reference does, so two passes of
    # one engine differ in the last bit: the engine is held to a twin that makes the same passes without the refusals)
    drop, _, _ = make_engine(pkg, synth, LS, B, dropoutflag=1, visible_omit=0.1, hid_omit=0.2)
    twin, _, _ = make_engine(pkg, synth, LS, B, dropoutflag=1, visible_omit=0.1, hid_omit=0.2)
    assert drop.forward(inp).tobytes() == twin.forward(inp).tobytes()
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_output_stats: .*not available with dropoutflag"):
        drop.output_stats(inp, targ)
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_output_stats_frames: .*not available with dropoutflag"):
        drop.output_stats_frames(feat, tstream, first, CTX, TOFF)
    assert drop.forward(inp).tobytes() == twin.forward(inp).tobytes()
    drop.close()
    twin.close()
    # bad arguments
    eng = engines[B]
    before = eng.forward(inp)
    want = eng.output_stats(inp, targ)
    with pytest.raises(pkg.MlggdError, match=r"error 1: targ_offset 3"):
        eng.output_stats_frames(feat, tstream, first, CTX, 3)
    with pytest.raises(pkg.MlggdError, match=r"error 1: sample 0: window"):
        eng.output_stats_frames(feat, tstream, first + 1000, CTX, TOFF)
    with pytest.raises(ValueError):
        eng.output_stats(inp[:, :-1], targ)
    with pytest.raises(ValueError):
        eng.output_stats(inp, targ[:, :-1])
    L = pkg.load()
    assert L.mlggd_output_stats(eng._h, 4, None, None, None) == 1 and "NULL" in L.mlggd_last_error().decode()
    assert L.mlggd_output_stats(None, 4, None, None, None) == 1
    assert L.mlggd_output_stats_frames(eng._h, 4, CTX, None, None, 2, None, TOFF, None) == 1
    sums = np.zeros((4, FDIM))
    import ctypes as C
    assert L.mlggd_output_stats(eng._h, 4, None, None, sums.ctypes.data_as(C.POINTER(C.c_double))) == 1
    assert "in/targ is NULL" in L.mlggd_last_error().decode()
    assert eng.forward(inp).tobytes() == before.tobytes()
    assert same_bits(eng.output_stats(inp, targ), want)
