"""CPU: mlggd_stoi_layout (pkg.stoi_layout) against the counts of the float64 model tests/stoi64.py at every rate and
around every boundary, and the argument checks of mlggd_stoi_waves / mlggd_enhance_waves_scored_stoi.  Every error is
MLGGD_ERR_ARG (1) with the utterance named where there is one; a device call on a machine without a GPU would come back
as MLGGD_ERR_DEVICE (2) instead, so status 1 also shows that the check came before any device call."""
import ctypes as C

import numpy as np
import pytest

import stoi64

RATES = [8, 11, 16]
FP, SP, LP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int16), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
ERR_ARG = 1


def shortest_with_len10(l10, fs):
    n = 0
    while stoi64.len10(n, fs) < l10:
        n += 1
    return n


def boundaries(fs):
    """sample counts around: no samples, len10 = N and N + 1 (the first frame), and the shortest lengths with 2, 30, 31
    and 32 frames (the first segment and the second), each plus and minus one sample"""
    pts = {0, 1, 2}
    for n in [shortest_with_len10(stoi64.N, fs), shortest_with_len10(stoi64.N + 1, fs)] + \
             [stoi64.shortest_with_frames(F, fs) for F in (1, 2, 30, 31, 32, 77)]:
        pts |= {n - 1, n, n + 1}
    return sorted(pts)


@pytest.mark.parametrize("fs", RATES)
def test_layout_equals_the_model_around_every_boundary(pkg, fs):
    seen = set()
    for n in boundaries(fs):
        want = stoi64.layout(n, fs)
        assert pkg.stoi_layout(n, fs_khz=fs) == want, (fs, n)
        seen.add(want[1:])
    # the boundaries are boundaries: no frame / one frame, 30 frames without a segment, 31 with one, 32 with two
    assert {(0, 0), (1, 0), (30, 0), (31, 1), (32, 2)} <= seen


@pytest.mark.parametrize("fs", RATES)
def test_the_model_s_own_counts_are_the_layout_s(fs):
    """stoi64 on a signal that keeps every frame reports the layout's len10, frames and segments"""
    n = stoi64.shortest_with_frames(33, fs) + 5
    x = stoi64.speech(n, fs, seed=fs)
    r = stoi64.stoi64(x, x, fs)
    assert r.kept == r.frames
    assert (r.len10, r.frames, r.segments) == stoi64.layout(n, fs) and r.segments == 3


def test_layout_argument_errors(pkg):
    L = pkg.load()
    a = C.c_int64(7)
    assert L.mlggd_stoi_layout(12, 100, C.byref(a), None, None) == ERR_ARG and "fs_khz 12" in L.mlggd_last_error().decode()
    assert L.mlggd_stoi_layout(16, -1, C.byref(a), None, None) == ERR_ARG and "n_samples -1" in L.mlggd_last_error().decode()
    assert a.value == 7
    assert L.mlggd_stoi_layout(16, 16000, None, None, None) == 0          # every output is optional
    with pytest.raises(pkg.MlggdError, match="fs_khz 44"):
        pkg.stoi_layout(1000, fs_khz=44)


def call(pkg, fs=16, lengths=(900, 300, 1200), offsets=None, stoi_samples=None, null=None, n_utts=None):
    """mlggd_stoi_waves on zero waves of these lengths; `null` names the pointer passed as NULL"""
    off = np.asarray(offsets if offsets is not None else np.concatenate([[0], np.cumsum(lengths)]), np.int64)
    n = off.size - 1
    wave = np.zeros(max(int(off.max()), 1), np.int16)
    ss = None if stoi_samples is None else np.asarray(stoi_samples, np.int64)
    a, b = np.full(n, 7, np.float32), np.full(n, 7, np.int32)
    args = {"clean": wave.ctypes.data_as(SP), "proc": wave.ctypes.data_as(SP), "offsets": off.ctypes.data_as(LP),
            "stoi": a.ctypes.data_as(FP)}
    if null:
        args[null] = None
    rc = pkg.load().mlggd_stoi_waves(0, fs, n if n_utts is None else n_utts, args["clean"], args["proc"],
                                     args["offsets"], ss.ctypes.data_as(LP) if ss is not None else None, args["stoi"],
                                     b.ctypes.data_as(IP))
    assert (a == 7).all() and (b == 7).all()          # nothing was written
    return rc, pkg.load().mlggd_last_error().decode()


@pytest.mark.parametrize("null", ["clean", "proc", "offsets", "stoi"])
def test_a_null_pointer_is_an_argument_error(pkg, null):
    rc, msg = call(pkg, null=null)
    assert rc == ERR_ARG and "NULL" in msg


def test_offsets_that_decrease_name_the_utterance(pkg):
    rc, msg = call(pkg, offsets=[0, 4000, 3000, 9000])
    assert rc == ERR_ARG and "offsets decrease at utterance 1" in msg


@pytest.mark.parametrize("ss,u", [([900, 301, 1200], 1), ([900, 300, -1], 2), ([901, 0, 0], 0)])
def test_stoi_samples_out_of_range_names_the_utterance(pkg, ss, u):
    rc, msg = call(pkg, stoi_samples=ss)
    assert rc == ERR_ARG and "utterance %d: stoi_samples %d is outside 0..%d" % (u, ss[u], (900, 300, 1200)[u]) in msg


def test_a_bad_rate_and_a_negative_count(pkg):
    rc, msg = call(pkg, fs=12)
    assert rc == ERR_ARG and "fs_khz 12" in msg
    rc, msg = call(pkg, n_utts=-1)
    assert rc == ERR_ARG and "n_utts -1" in msg
    assert call(pkg, n_utts=0)[0] == 0                # nothing to score: no device is touched either


def test_the_python_wrapper_raises_the_same_errors(pkg):
    w = [np.zeros(900, np.int16), np.zeros(300, np.int16)]
    with pytest.raises(pkg.MlggdError, match=r"error 1: utterance 1: stoi_samples 301 is outside 0\.\.300"):
        pkg.stoi_waves(w, w, stoi_samples=[900, 301])
    with pytest.raises(ValueError):
        pkg.stoi_waves(w, w, stoi_samples=[900])
    with pytest.raises(ValueError):
        pkg.stoi_waves(w[:1], w)
    with pytest.raises(pkg.MlggdError, match="fs_khz 12"):
        pkg.stoi_waves(w, w, fs_khz=12)


def test_the_engine_entry_point_refuses_a_null_handle(pkg):
    fn = pkg.load().mlggd_enhance_waves_scored_stoi
    rc = fn(None, 16, 7, None, None, 1, None, None, None, None, None, None, None, None, None, None, None, None)
    assert rc == ERR_ARG and "NULL handle" in pkg.load().mlggd_last_error().decode()
