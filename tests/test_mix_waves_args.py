"""CPU: the argument checks of mlggd_mix_waves, mlggd_lps_stats, mlggd_wave_samples and mlggd_norm_from_stats, and
of the mix_wav tool's list.  Every
error is MLGGD_ERR_ARG (1) with the utterance or bin named; a device call on a machine without a GPU would come back as
MLGGD_ERR_DEVICE (2) instead, so status 1 also shows that the check came before any device call."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import hostlib

FP, SP, LP, IP, DP = (C.POINTER(t) for t in (C.c_float, C.c_int16, C.c_int64, C.c_int32, C.c_double))
ERR_ARG = 1


def mix(pkg, offsets=(3, 13, 13, 40), n_noise=50, lo=(0, 10, 20), ln=(50, 1, 30), start=(49, 0, 29),
        snr=(0.0, 5.0, math.inf), null=None, n_utts=None):
    """mlggd_mix_waves on zero waves; `null` names the pointer passed as NULL"""
    off = np.asarray(offsets, np.int64)
    n = off.size - 1
    clean = np.zeros(max(int(off.max()), 1), np.int16)
    noisy = np.full(clean.size, 7, np.int16)
    noise = np.zeros(max(n_noise, 1), np.int16)
    a = {"clean": clean.ctypes.data_as(SP), "offsets": off.ctypes.data_as(LP), "noise": noise.ctypes.data_as(SP),
         "noise_lo": np.asarray(lo, np.int64).ctypes.data_as(LP), "noise_len": np.asarray(ln, np.int64).ctypes.data_as(LP),
         "noise_start": np.asarray(start, np.int64).ctypes.data_as(LP),
         "snr_db": np.asarray(snr, np.float64).ctypes.data_as(DP), "noisy": noisy.ctypes.data_as(SP)}
    if null:
        a[null] = None
    rc = pkg.load().mlggd_mix_waves(0, n if n_utts is None else n_utts, a["clean"], a["offsets"], a["noise"], n_noise,
                                    a["noise_lo"], a["noise_len"], a["noise_start"], a["snr_db"], a["noisy"], None, None)
    assert (noisy == 7).all()                          # nothing was written
    return rc, pkg.load().mlggd_last_error().decode()


@pytest.mark.parametrize("null", ["clean", "offsets", "noise", "noise_lo", "noise_len", "noise_start", "snr_db", "noisy"])
def test_mix_waves_a_null_pointer_is_an_argument_error(pkg, null):
    rc, msg = mix(pkg, null=null)
    assert rc == ERR_ARG and "NULL" in msg


@pytest.mark.parametrize("kw,text", [
    (dict(offsets=(0, 20, 10, 40)), "offsets decrease at utterance 1"),
    (dict(ln=(50, 0, 30)), "utterance 1: noise_len 0 < 1"),
    (dict(ln=(50, 1, -2)), "utterance 2: noise_len -2 < 1"),
    (dict(lo=(0, 10, 21)), "utterance 2: noise segment [21, 51) is outside the 50 noise samples"),
    (dict(lo=(-1, 10, 20), ln=(5, 1, 30), start=(0, 0, 0)), "utterance 0: noise segment [-1, 4) is outside"),
    (dict(lo=(0, 50, 20)), "utterance 1: noise segment [50, 51) is outside"),
    (dict(start=(50, 0, 29)), "utterance 0: noise_start 50 is outside its segment of 50 samples"),
    (dict(start=(49, 0, -1)), "utterance 2: noise_start -1 is outside its segment of 30 samples"),
    (dict(snr=(0.0, math.nan, 1.0)), "utterance 1: snr_db nan"),
    (dict(snr=(0.0, 5.0, -math.inf)), "utterance 2: snr_db -inf"),
    (dict(n_noise=-1), "n_noise -1"),
    (dict(n_utts=-1), "n_utts -1"),
])
def test_mix_waves_names_the_utterance(pkg, kw, text):
    rc, msg = mix(pkg, **kw)
    assert rc == ERR_ARG and text in msg, msg


def test_mix_waves_with_nothing_to_mix_touches_no_device(pkg):
    assert mix(pkg, n_utts=0)[0] == 0
    assert mix(pkg, offsets=(5, 5, 5, 5))[0] == 0      # three empty utterances


def test_the_python_wrapper_raises_the_same_errors(pkg):
    w = [np.zeros(10, np.int16), np.zeros(4, np.int16)]
    noise = np.zeros(20, np.int16)
    with pytest.raises(pkg.MlggdError, match=r"error 1: utterance 1: noise_start 20 is outside"):
        pkg.mix_waves(w, noise, 0.0, [0, 20])
    with pytest.raises(pkg.MlggdError, match=r"error 1: utterance 0: noise segment \[15, 21\) is outside the 20"):
        pkg.mix_waves(w, noise, [0.0, 1.0], 0, noise_seg=[(15, 6), (0, 1)])
    with pytest.raises(pkg.MlggdError, match=r"error 1: utterance 1: snr_db nan"):
        pkg.mix_waves(w, noise, [0.0, math.nan], 0)
    with pytest.raises(ValueError):
        pkg.mix_waves(w, noise, 0.0, 0, noise_seg=[(0, 1)])
    with pytest.raises(ValueError):
        pkg.mix_waves([np.zeros(4, np.float32)], noise, 0.0, 0)


def stats(pkg, fs=16, offsets=(0, 600, 1300), null=None, n_utts=None):
    off = np.asarray(offsets, np.int64)
    wave = np.zeros(max(int(off.max()), 1), np.int16)
    sums = np.full((2, 257), 7.0)
    n = C.c_int64(-7)
    a = {"wave": wave.ctypes.data_as(SP), "offsets": off.ctypes.data_as(LP), "sums": sums.ctypes.data_as(DP),
         "n_frames": C.byref(n)}
    if null:
        a[null] = None
    rc = pkg.load().mlggd_lps_stats(0, fs, off.size - 1 if n_utts is None else n_utts, a["wave"], a["offsets"], a["sums"],
                                    a["n_frames"])
    return rc, pkg.load().mlggd_last_error().decode(), sums, n.value


@pytest.mark.parametrize("null", ["wave", "offsets", "sums", "n_frames"])
def test_lps_stats_a_null_pointer_is_an_argument_error(pkg, null):
    rc, msg, sums, n = stats(pkg, null=null)
    assert rc == ERR_ARG and "NULL" in msg and (sums == 7.0).all()


def test_lps_stats_bad_rate_decreasing_offsets_and_nothing_to_do(pkg):
    rc, msg, _, _ = stats(pkg, fs=12)
    assert rc == ERR_ARG and "fs_khz 12" in msg
    rc, msg, sums, _ = stats(pkg, offsets=(0, 900, 600, 1300))
    assert rc == ERR_ARG and "offsets decrease at utterance 1" in msg and (sums == 7.0).all()
    rc, msg, _, _ = stats(pkg, n_utts=-1)
    assert rc == ERR_ARG and "n_utts -1" in msg
    rc, _, sums, n = stats(pkg, n_utts=0)                  # no wave: zeros, no device
    assert rc == 0 and n == 0 and (sums == 0.0).all()
    rc, _, sums, n = stats(pkg, offsets=(0, 511, 600))     # no utterance reaches one frame
    assert rc == 0 and n == 0 and (sums == 0.0).all()


def samples(pkg, fs=16, ctx=3, offsets=(0, 2000, 5000), null=None, n_utts=None):
    off = np.asarray(offsets, np.int64)
    n = C.c_int64(-7)
    a = {"offsets": off.ctypes.data_as(LP), "n_samples": C.byref(n)}
    if null:
        a[null] = None
    rc = pkg.load().mlggd_wave_samples(fs, ctx, off.size - 1 if n_utts is None else n_utts, a["offsets"], None,
                                       a["n_samples"])
    return rc, pkg.load().mlggd_last_error().decode()


def test_wave_samples_argument_errors(pkg):
    for null in ("offsets", "n_samples"):
        rc, msg = samples(pkg, null=null)
        assert rc == ERR_ARG and "NULL" in msg
    rc, msg = samples(pkg, fs=44)
    assert rc == ERR_ARG and "fs_khz 44" in msg
    rc, msg = samples(pkg, ctx=0)
    assert rc == ERR_ARG and "fea_context 0" in msg
    rc, msg = samples(pkg, offsets=(0, 2000, 1999))
    assert rc == ERR_ARG and "offsets decrease at utterance 1" in msg
    rc, msg = samples(pkg, n_utts=-2)
    assert rc == ERR_ARG and "n_utts -2" in msg
    with pytest.raises(pkg.MlggdError, match="error 1: fea_context -1"):
        pkg.wave_samples([5000], -1)


def test_norm_from_stats_equals_the_float32_rounding_of_numpy(pkg):
    x = np.random.default_rng(11).integers(-40, 25, (4000, 129)).astype(np.float64)   # integers: the sums are exact
    sums = np.stack([x.sum(0), (x * x).sum(0)])
    mean, inv = pkg.norm_from_stats(x.shape[0], sums)
    assert mean.dtype == np.float32 and inv.dtype == np.float32
    assert np.array_equal(mean, x.mean(0).astype(np.float32))
    assert np.array_equal(inv, (1.0 / x.std(0)).astype(np.float32))


def test_norm_from_stats_argument_errors(pkg):
    L = pkg.load()
    sums = np.array([[4.0, 6.0, 9.0], [8.0, 18.0, 27.0]])       # n = 2: bin 0 = {2, 2}, bin 1 = {3, 3}: no variance
    m, v = np.full(3, 7, np.float32), np.full(3, 7, np.float32)
    args = lambda **k: (k.get("D", 3), k.get("n", 2), k.get("sums", sums.ctypes.data_as(DP)),
                        k.get("mean", m.ctypes.data_as(FP)), k.get("inv", v.ctypes.data_as(FP)))
    assert L.mlggd_norm_from_stats(*args()) == ERR_ARG and "bin 0" in L.mlggd_last_error().decode()
    assert (m == 7).all() and (v == 7).all()                    # nothing was written
    for k in ("sums", "mean", "inv"):
        assert L.mlggd_norm_from_stats(*args(**{k: None})) == ERR_ARG and "NULL" in L.mlggd_last_error().decode()
    assert L.mlggd_norm_from_stats(*args(D=0)) == ERR_ARG and "D 0" in L.mlggd_last_error().decode()
    assert L.mlggd_norm_from_stats(*args(n=0)) == ERR_ARG and "n 0" in L.mlggd_last_error().decode()
    with pytest.raises(pkg.MlggdError, match="error 1: bin 1"):
        pkg.norm_from_stats(2, np.array([[4.0, 6.0], [10.0, 18.0]]))
    with pytest.raises(ValueError):
        pkg.norm_from_stats(2, np.zeros(6))


def test_the_engine_entry_points_refuse_a_null_handle(pkg):
    L = pkg.load()
    assert L.mlggd_load_waves(None, 16, 7, None, None, 1, None, None, None, 1, None, 0) == ERR_ARG
    assert "NULL handle" in L.mlggd_last_error().decode()
    assert L.mlggd_cv_all_waves(None, 16, 7, None, None, 1, None, None, None, 1, None, 0, None, None, None) == ERR_ARG
    assert L.mlggd_set_noise(None, 0, None) == ERR_ARG
    assert L.mlggd_train_waves(None, 16, 7, None, None, 1, None, None, None, None, None, None, 1, None, 0, None, None,
                               None, None) == ERR_ARG
    assert "NULL handle" in L.mlggd_last_error().decode()


def test_mix_wav_refuses_a_bad_list_with_the_line_named(pkg, tmp_path):
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s", "mix_wav"])
    exe = os.path.join(hostlib.HOST, "mix_wav")
    scp = tmp_path / "bad.scp"
    scp.write_text("a.wav n.wav 5 0\n")
    r = subprocess.run([exe, "scp=%s" % scp], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "line 1" in r.stderr
    scp.write_text("a.wav n.wav loud 0 out.wav\n")
    r = subprocess.run([exe, "scp=%s" % scp], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "line 1: snr_db 'loud' is no number" in r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "usage: mix_wav scp=LIST" in r.stderr
    r = subprocess.run([exe, "scp=%s" % scp, "fs=12"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "invalid sampling frequency 12" in r.stderr
