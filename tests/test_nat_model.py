"""CPU: the host-only half of noise-aware training (csrc/nat_rule.h) -- pkg.nat_estimate and pkg.nat_rows against the
numpy model tests/nat_model.py bit for bit, the size of the config struct, and the argument checks that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import nat_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 6


def rows_of(frames, D, seed):
    """normalised rows whose sum depends on the order of the additions: a wide range of magnitudes and both signs"""
    rng = np.random.default_rng(seed)
    n = int(np.sum(frames))
    return (rng.standard_normal((n, D)) * 10.0 ** rng.integers(-3, 4, (n, D))).astype(np.float32)


def offsets(frames):
    return np.concatenate([[0], np.cumsum(frames)]).astype(np.int32)


def test_nat_estimate_equals_the_model(pkg):
    """F_u in {1, T - 1, T, T + 1}, an utterance without frames in the middle and a long one"""
    frames = [1, T - 1, 0, T, T + 1, 40]
    for D in (1, 13, 257):
        rows, fo = rows_of(frames, D, 3 + D), offsets(frames)
        want = nat_model.noise_rows(rows, fo, T)
        got = pkg.nat_estimate(rows, fo, T)
        assert got.dtype == np.float32 and got.shape == (len(frames), D)
        assert got.tobytes() == want.tobytes()
        assert not got[2].any() and np.array_equal(got[0], rows[0])            # no frames: zeros; one frame: x / 1
    # the order is the rule: the same T rows added from the last to the first give other bits somewhere
    rows, fo = rows_of([T + 1], 257, 9), offsets([T + 1])
    back = nat_model.noise_rows(rows[:T][::-1], offsets([T]), T)
    assert pkg.nat_estimate(rows, fo, T).tobytes() != back.tobytes()
    # T = 1 is the first row, and only the first T rows are read
    assert np.array_equal(pkg.nat_estimate(rows, fo, 1)[0], rows[0])
    later = rows.copy()
    later[T:] = np.nan
    assert pkg.nat_estimate(later, fo, T).tobytes() == pkg.nat_estimate(rows, fo, T).tobytes()


def test_nat_rows_equals_the_model(pkg):
    frames = [3, 0, 1, 0, 0, 7, 2]
    fo = offsets(frames)
    first = np.random.default_rng(2).permutation(np.arange(fo[-1], dtype=np.int32))
    first = np.concatenate([first, first[:5]])                                  # repeats, any order
    got = pkg.nat_rows(fo, first)
    assert got.dtype == np.int32 and np.array_equal(got, nat_model.utt_of_frames(fo, first))
    assert set(got.tolist()) == {0, 2, 5, 6}                                     # never an utterance without frames
    assert pkg.nat_rows(fo, np.zeros(0, np.int32)).size == 0


def test_host_entries_reject_bad_arguments(pkg):
    rows, fo = rows_of([4, 4], 5, 1), offsets([4, 4])
    with pytest.raises(pkg.MlggdError, match="error 1: nat_frames 0 < 1"):
        pkg.nat_estimate(rows, fo, 0)
    with pytest.raises(pkg.MlggdError, match="error 1: frame_off decreases at utterance 1"):
        pkg.nat_estimate(rows, np.array([0, 4, 2], np.int32), T)
    with pytest.raises(pkg.MlggdError, match="error 1: sample 1: frame 8 outside the 8 packed frames"):
        pkg.nat_rows(fo, np.array([0, 8], np.int32))
    with pytest.raises(pkg.MlggdError, match="error 1: sample 0: frame -1 outside"):
        pkg.nat_rows(fo, np.array([-1], np.int32))


def test_config_struct_keeps_its_size_and_nat_frames_takes_a_reserved_slot(pkg):
    """the layout of every earlier field is unchanged: nat_frames sits where reserved[0] was, and a zeroed struct says off"""
    C = pkg._Config
    assert ctypes.sizeof(C) == 4 * (4 + 10 + 1 + 4 + 2 + 2 + 1 + 7)
    assert C.activation.offset == 4 * 24 and C.nat_frames.offset == 4 * 25 and C.reserved.offset == 4 * 26
    assert C.reserved.size == 4 * 5 and C().nat_frames == 0
    hdr = open(os.path.join(ROOT, "include", "mlggd.h")).read()
    body = re.search(r"typedef struct mlggd_config \{(.*?)\} mlggd_config;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(\w+)(?:\[(\w+)\])?;", body)
    assert fields[-3:] == [("activation", ""), ("nat_frames", ""), ("reserved", "5")]


def test_create_rejects_a_negative_nat_frames_before_touching_a_device(pkg):
    L = pkg.load()
    fp = ctypes.POINTER(ctypes.c_float)
    arr = (fp * pkg.MAXLAYER)()  # never dereferenced: the checks come first
    cfg = pkg._Config()
    cfg.struct_size = ctypes.sizeof(pkg._Config)
    cfg.numlayers = 3
    for i, v in enumerate([28, 8, 7]):
        cfg.layersizes[i] = v
    cfg.bunchsize = 8
    cfg.nat_frames = -1
    h = ctypes.c_void_p()
    rc = L.mlggd_create(ctypes.byref(cfg), arr, arr, ctypes.byref(h))
    assert rc == 1 and "nat_frames -1 < 0" in L.mlggd_last_error().decode() and not h
