"""GPU: mlggd_mix_waves against the model of the mixing rule (tests/mix64.py): every sample, the clipped counts and the
gains of a batch of 70 utterances whose lengths, noise segments, starts and SNRs take every path of the kernels."""
import ctypes as C
import math

import numpy as np
import pytest

import mix64

pytestmark = pytest.mark.gpu
SP, LP, IP, DP = (C.POINTER(t) for t in (C.c_int16, C.c_int64, C.c_int32, C.c_double))
N_NOISE, SILENT = 21000, (15000, 600)            # the noise has a silent stretch [15000, 15600)
BLOCK = 4096                                     # mix_rule::kBlock


def batch():
    """70 utterances: (clean, (lo, len), start, snr_db)"""
    rng = np.random.default_rng(2024)
    noise = rng.integers(-3000, 3001, N_NOISE).astype(np.int16)
    noise[SILENT[0]:SILENT[0] + SILENT[1]] = 0
    lengths = [1, 255, 256, 257, 2 * BLOCK + 809, BLOCK, BLOCK + 1, BLOCK - 1, 7, 8, 9, 15, 16, 17, 3000, 2999]
    lengths += rng.integers(2, 9000, 70 - len(lengths)).tolist()
    snrs = [-40.0, -5.0, 0.0, 20.0, math.inf]
    utts = []
    for u, n in enumerate(lengths):
        clean = rng.integers(-6000, 6001, n).astype(np.int16)
        kind = u % 7
        if kind == 0:
            seg = (int(rng.integers(0, N_NOISE)), 1)                      # one sample, repeated
        elif kind == 1:
            seg = (int(rng.integers(0, N_NOISE - 7)), 7)                  # wraps many times
        elif kind == 2:
            seg = (int(rng.integers(0, 5000)), n + int(rng.integers(1, 4000)))   # longer than the utterance
        elif kind == 3:
            seg = (0, N_NOISE)                                            # the whole noise
        elif kind == 4:
            seg = (int(rng.integers(0, 9000)), max(1, n - 1))             # wraps once, at the last sample
        elif kind == 5:
            seg = (int(rng.integers(0, 9000)), max(1, n // 3 + 1))        # wraps inside blocks, often shorter than one
        else:
            seg = (int(rng.integers(0, 9000)), BLOCK + 5)                 # just longer than a block
        start = seg[1] - 1 if u % 3 == 0 else int(rng.integers(0, seg[1]))
        utts.append([clean, seg, start, snrs[u % 5]])
    utts[4][1], utts[4][2] = (100, 5000), 4999                            # > 2 blocks over a segment that is >= a block and wraps
    utts[20][0] = np.zeros_like(utts[20][0])                              # a silent clean utterance
    utts[21][1], utts[21][2], utts[21][3] = (SILENT[0] + 10, 500), 499, 0.0    # a silent noise segment
    utts[14][0] = rng.integers(-28000, 28001, 3000).astype(np.int16)      # loud: at 0 dB the sum leaves int16 often
    utts[14][1], utts[14][2], utts[14][3] = (2000, 6000), 17, 0.0
    return noise, utts


def run(pkg, noise, utts, base=3):
    """mlggd_mix_waves through the C entry point, the packed batch starting at offsets[0] = base"""
    n = len(utts)
    off = (base + np.concatenate([[0], np.cumsum([u[0].size for u in utts])])).astype(np.int64)
    packed = np.concatenate([np.full(base, 12345, np.int16)] + [u[0] for u in utts])
    lo = np.array([u[1][0] for u in utts], np.int64)
    ln = np.array([u[1][1] for u in utts], np.int64)
    st = np.array([u[2] for u in utts], np.int64)
    snr = np.array([u[3] for u in utts], np.float64)
    out = np.full(packed.size, -77, np.int16)
    gain, clipped = np.full(n, -1.0), np.full(n, -1, np.int32)
    rc = pkg.load().mlggd_mix_waves(0, n, packed.ctypes.data_as(SP), off.ctypes.data_as(LP), noise.ctypes.data_as(SP),
                                    noise.size, lo.ctypes.data_as(LP), ln.ctypes.data_as(LP), st.ctypes.data_as(LP),
                                    snr.ctypes.data_as(DP), out.ctypes.data_as(SP), gain.ctypes.data_as(DP),
                                    clipped.ctypes.data_as(IP))
    assert rc == 0, pkg.load().mlggd_last_error().decode()
    assert (out[:base] == -77).all()                                       # nothing in front of the batch is written
    return [out[off[u]:off[u + 1]] for u in range(n)], gain, clipped, out.tobytes()


@pytest.fixture(scope="module")
def mixed(pkg):
    noise, utts = batch()
    return noise, utts, run(pkg, noise, utts)


def test_the_batch_takes_every_path():
    noise, utts = batch()
    lens = [u[0].size for u in utts]
    assert len(utts) == 70 and {1, 255, 256, 257}.issubset(lens) and max(lens) > 2 * BLOCK
    assert {u[1][1] for u in utts} >= {1, 7} and any(u[1][1] > u[0].size for u in utts)
    assert any(u[2] == u[1][1] - 1 and u[1][1] > 1 for u in utts)
    assert {u[3] for u in utts} == {-40.0, -5.0, 0.0, 20.0, math.inf}
    assert any(u[1][1] < BLOCK < u[0].size for u in utts) and any(BLOCK <= u[1][1] < u[0].size for u in utts)
    assert not utts[20][0].any() and not mix64.paired(noise, *utts[21][1], utts[21][2], utts[21][0].size).any()


def test_every_sample_and_count_equals_the_model_at_the_returned_gain(mixed):
    noise, utts, (waves, gain, clipped, _) = mixed
    for u, (clean, seg, start, snr) in enumerate(utts):
        want, _, want_clipped = mix64.mix_utt(clean, noise, seg[0], seg[1], start, snr, g=float(gain[u]))
        assert waves[u].dtype == np.int16 and np.array_equal(waves[u], want), "utterance %d" % u
        assert int(clipped[u]) == want_clipped, "utterance %d" % u
    assert 100 <= int(clipped[14]) < 3000                                  # the loud one clips a few hundred samples
    assert mix64.mix_utt(utts[14][0], noise, *utts[14][1], utts[14][2], utts[14][3])[2] >= 100   # ... in the model itself


def test_the_gain_is_the_models_within_four_ulps(mixed):
    noise, utts, (_, gain, _, _) = mixed
    for u, (clean, seg, start, snr) in enumerate(utts):
        g = mix64.mix_utt(clean, noise, seg[0], seg[1], start, snr)[1]
        print("utterance %d: gain %r model %r" % (u, float(gain[u]), g))
        assert abs(float(gain[u]) - g) <= 4 * 2.0 ** -52 * abs(g), "utterance %d" % u
        if snr == math.inf or u in (20, 21):
            assert gain[u] == 0.0 and np.array_equal(mixed[2][0][u], clean)   # the noisy wave is the clean wave


def test_two_calls_return_the_same_bytes(pkg, mixed):
    noise, utts, (_, gain, clipped, raw) = mixed
    _, gain2, clipped2, raw2 = run(pkg, noise, utts)
    assert raw2 == raw and gain2.tobytes() == gain.tobytes() and clipped2.tobytes() == clipped.tobytes()


def test_an_utterance_does_not_depend_on_its_neighbours_or_position(pkg, mixed):
    noise, utts, (waves, gain, clipped, _) = mixed
    rev = utts[::-1]
    waves2, gain2, clipped2, _ = run(pkg, noise, rev, base=0)
    for u in range(len(utts)):
        assert np.array_equal(waves2[len(utts) - 1 - u], waves[u]), "utterance %d" % u
    assert gain2[::-1].tobytes() == gain.tobytes() and clipped2[::-1].tobytes() == clipped.tobytes()


def test_the_python_call_returns_the_same(pkg, mixed):
    noise, utts, (waves, gain, clipped, _) = mixed
    got, g, c = pkg.mix_waves([u[0] for u in utts], noise, [u[3] for u in utts], [u[2] for u in utts],
                              noise_seg=[u[1] for u in utts], return_info=True)
    for a, b in zip(got, waves):
        assert np.array_equal(a, b)
    assert g.tobytes() == gain.tobytes() and c.tobytes() == clipped.tobytes()
    assert pkg.mix_waves([], noise, 0.0, 0) == []
