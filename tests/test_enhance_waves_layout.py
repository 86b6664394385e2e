"""CPU: the layout of a packed batch of utterances (mlggd_enhance_waves_layout, pkg.enhance_waves_layout) -- frames per
utterance, offsets into the packed frames and into the packed output -- against spec64.n_frames, and its argument
checks.  A host call: no device is touched."""
import ctypes as C

import numpy as np
import pytest

import spec64


def expected(lengths, fs):
    L, S, _ = spec64.params(fs)
    frames = np.array([spec64.n_frames(n, fs) for n in lengths], np.int64)
    frame_off = np.concatenate([[0], np.cumsum(frames)])
    out_off = np.concatenate([[0], np.cumsum(frames * S + L - S)])
    return frames, frame_off, out_off


def boundary_lengths(fs):
    """L - 1 is too short; from L on: each frame count's first and last length, and a few more"""
    L, S, _ = spec64.params(fs)
    out = []
    for k in range(0, 5):
        out += [L + k * S, L + k * S + 1, L + (k + 1) * S - 1]
    return out + [L + 300 * S + 7, 3 * fs * 1000, 4 * fs * 1000 + 13]


@pytest.mark.parametrize("fs", [8, 11, 16])
def test_layout_agrees_with_spec64_around_the_frame_boundaries(pkg, fs):
    lengths = boundary_lengths(fs)
    frames, frame_off, out_off = pkg.enhance_waves_layout(lengths, fs)
    want = expected(lengths, fs)
    assert frames.tolist() == want[0].tolist() and min(frames) == 1
    assert frame_off.dtype == np.int32 and frame_off.tolist() == want[1].tolist()
    assert out_off.dtype == np.int64 and out_off.tolist() == want[2].tolist()
    for n in lengths:                                              # one utterance at a time
        f, fo, oo = pkg.enhance_waves_layout([n], fs)
        assert f.tolist() == [spec64.n_frames(n, fs)] and fo.tolist() == [0, f[0]]
        L, S, _ = spec64.params(fs)
        assert oo.tolist() == [0, f[0] * S + L - S]


@pytest.mark.parametrize("fs", [8, 11, 16])
def test_layout_of_an_empty_list(pkg, fs):
    frames, frame_off, out_off = pkg.enhance_waves_layout([], fs)
    assert frames.size == 0 and frame_off.tolist() == [0] and out_off.tolist() == [0]


@pytest.mark.parametrize("fs", [8, 11, 16])
def test_layout_drops_trailing_samples(pkg, fs):
    L, S, _ = spec64.params(fs)
    base = [L + 3 * S, L, L + 40 * S]
    for extra in (1, S // 2, S - 1):
        a = pkg.enhance_waves_layout(base, fs)
        b = pkg.enhance_waves_layout([n + extra for n in base], fs)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
    assert pkg.enhance_waves_layout([L + 3 * S + S], fs)[0].tolist() == [5]


def raw_layout(pkg, fs, offsets):
    off = np.asarray(offsets, np.int64)
    n = off.size - 1
    fo, oo = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int64)
    lp = C.POINTER(C.c_int64)
    rc = pkg.load().mlggd_enhance_waves_layout(fs, n, off.ctypes.data_as(lp), fo.ctypes.data_as(C.POINTER(C.c_int32)),
                                               oo.ctypes.data_as(lp))
    return rc, pkg.load().mlggd_last_error().decode(), fo, oo


def test_layout_takes_offsets_that_do_not_start_at_zero(pkg):
    rc, _, fo, oo = raw_layout(pkg, 16, [1000, 1000 + 512, 1000 + 512 + 1024])
    assert rc == 0 and fo.tolist() == [0, 1, 4] and oo.tolist() == [0, 512, 512 + 1024]


def test_layout_rejects_offsets_that_decrease(pkg):
    rc, msg, _, _ = raw_layout(pkg, 16, [0, 4000, 3000, 9000])
    assert rc == 1 and "offsets decrease at utterance 1" in msg                 # MLGGD_ERR_ARG


@pytest.mark.parametrize("fs", [8, 11, 16])
def test_layout_names_the_utterance_that_is_shorter_than_one_frame(pkg, fs):
    L, S, _ = spec64.params(fs)
    with pytest.raises(pkg.MlggdError, match=r"error 1: utterance 2: %d samples is shorter than one frame" % (L - 1)):
        pkg.enhance_waves_layout([L, 5 * L, L - 1, L], fs)
    with pytest.raises(pkg.MlggdError, match=r"error 1: utterance 0: 0 samples"):
        pkg.enhance_waves_layout([0], fs)


def test_layout_checks_that_the_frames_fit_int32(pkg):
    rc, msg, _, _ = raw_layout(pkg, 8, [0, 2 ** 37, 2 ** 38 + 2 ** 37])            # 2^30 + 2^31 frames of 128 samples
    assert rc == 1 and "frames" in msg and "utterance 1" in msg


def test_layout_rejects_an_unknown_rate_and_a_negative_count(pkg):
    rc, msg, _, _ = raw_layout(pkg, 12, [0, 1000])
    assert rc == 1 and "fs_khz 12" in msg
    lp = C.POINTER(C.c_int64)
    assert pkg.load().mlggd_enhance_waves_layout(16, -1, lp(), C.POINTER(C.c_int32)(), lp()) == 1
    assert pkg.load().mlggd_enhance_waves_layout(16, 2, lp(), C.POINTER(C.c_int32)(), lp()) == 1   # offsets NULL
    assert pkg.load().mlggd_enhance_waves_layout(16, 0, lp(), C.POINTER(C.c_int32)(), lp()) == 0   # nothing to lay out
