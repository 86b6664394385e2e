"""CPU: the argument checks of mlggd_score_waves and mlggd_enhance_waves_scored, and the tools' score= key.  Every error
is MLGGD_ERR_ARG (1) with the utterance named where there is one; a device call on a machine without a GPU would come
back as MLGGD_ERR_DEVICE (2) instead, so status 1 also shows that the check came before any device call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hostlib
import spec64

FP, SP, LP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int16), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
ERR_ARG = 1


def call(pkg, fs=16, frames=(3, 1, 4), offsets=None, score_frames=None, null=None, n_utts=None):
    """mlggd_score_waves on zero waves of these frame counts; `null` names the pointer passed as NULL"""
    lfs = fs if fs in spec64.PARAMS else 16
    N = spec64.params(lfs)[2]
    off = np.asarray(offsets if offsets is not None else spec64.waves_layout64(frames, lfs)[0], np.int64)
    n = off.size - 1
    wave = np.zeros(max(int(off.max()), 1), np.int16)
    lps = np.zeros((max(sum(frames), 1), N // 2 + 1), np.float32)
    sf = None if score_frames is None else np.asarray(score_frames, np.int32)
    a, b = np.full(n, 7, np.float32), np.full(n, 7, np.float32)
    args = {"clean": wave.ctypes.data_as(SP), "noisy": wave.ctypes.data_as(SP), "offsets": off.ctypes.data_as(LP),
            "lps": lps.ctypes.data_as(FP), "segsnr": a.ctypes.data_as(FP), "lsd": b.ctypes.data_as(FP)}
    if null:
        args[null] = None
    rc = pkg.load().mlggd_score_waves(0, fs, n if n_utts is None else n_utts, args["clean"], args["noisy"],
                                      args["offsets"], args["lps"], sf.ctypes.data_as(IP) if sf is not None else None,
                                      args["segsnr"], args["lsd"])
    assert (a == 7).all() and (b == 7).all()          # nothing was written
    return rc, pkg.load().mlggd_last_error().decode()


@pytest.mark.parametrize("null", ["clean", "noisy", "offsets", "lps", "segsnr", "lsd"])
def test_a_null_pointer_is_an_argument_error(pkg, null):
    rc, msg = call(pkg, null=null)
    assert rc == ERR_ARG and "NULL" in msg


def test_offsets_that_decrease_name_the_utterance(pkg):
    rc, msg = call(pkg, frames=(3, 1, 4), offsets=[0, 4000, 3000, 9000])
    assert rc == ERR_ARG and "offsets decrease at utterance 1" in msg


@pytest.mark.parametrize("fs", [8, 11, 16])
def test_an_utterance_shorter_than_one_frame_is_named(pkg, fs):
    L = spec64.params(fs)[0]
    rc, msg = call(pkg, fs=fs, frames=(1, 1, 1), offsets=[0, L, 2 * L, 3 * L - 1])
    assert rc == ERR_ARG and "utterance 2: %d samples is shorter than one frame" % (L - 1) in msg


@pytest.mark.parametrize("sf,u", [([3, 2, 4], 1), ([3, 1, -1], 2), ([4, 1, 4], 0), ([0, 0, 5], 2)])
def test_score_frames_out_of_range_names_the_utterance(pkg, sf, u):
    rc, msg = call(pkg, frames=(3, 1, 4), score_frames=sf)
    assert rc == ERR_ARG and "utterance %d: score_frames %d" % (u, sf[u]) in msg


def test_a_bad_rate_and_a_negative_count(pkg):
    rc, msg = call(pkg, fs=12)
    assert rc == ERR_ARG and "fs_khz 12" in msg
    rc, msg = call(pkg, n_utts=-1)
    assert rc == ERR_ARG and "n_utts -1" in msg
    assert call(pkg, n_utts=0)[0] == 0                # nothing to score: no device is touched either


def test_the_python_wrapper_raises_the_same_errors(pkg):
    L, S, _ = spec64.params(16)
    w = [np.zeros(L + 2 * S, np.int16), np.zeros(L, np.int16)]
    lps = [np.zeros((3, 257), np.float32), np.zeros((1, 257), np.float32)]
    with pytest.raises(pkg.MlggdError, match=r"error 1: utterance 1: score_frames 2 is outside 0\.\.1"):
        pkg.score_waves(w, w, lps, score_frames=[3, 2])
    with pytest.raises(pkg.MlggdError, match=r"error 1: utterance 1: 511 samples is shorter than one frame"):
        pkg.score_waves(w, [w[0], w[1][:511]], lps)
    with pytest.raises(ValueError):
        pkg.score_waves(w, w, lps, score_frames=[3])
    with pytest.raises(ValueError):
        pkg.score_waves(w[:1], w, lps)


def test_the_engine_entry_point_refuses_a_null_handle(pkg):
    fn = pkg.load().mlggd_enhance_waves_scored
    rc = fn(None, 16, 7, None, None, 1, None, None, None, None, None, None, None, None, None)
    assert rc == ERR_ARG and "NULL handle" in pkg.load().mlggd_last_error().decode()


@pytest.mark.parametrize("tool,argv", [
    ("enhance_wav", ["wts=a.wts", "norm_file=a.norm", "in=a.wav", "out=b.wav", "score=bogus"]),
    ("lps2wav", ["clean.raw", "noisy.raw", "feat.htk", "info.txt", "out.raw", "score=bogus"])])
def test_a_tool_refuses_an_unknown_score_mode_with_its_usage(pkg, tool, argv):
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    r = subprocess.run([os.path.join(hostlib.HOST, tool)] + argv, capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "score=bogus" in r.stderr and "usage: %s" % tool in r.stderr and "score=host|device" in r.stderr
