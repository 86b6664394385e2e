"""CPU: mlggd_wave_samples, the sample table of load_waves / train_waves, against a restatement in Python."""
import ctypes as C

import numpy as np
import pytest

import mix64
import spec64

LP, IP = C.POINTER(C.c_int64), C.POINTER(C.c_int32)


def restated(lengths, ctx, fs):
    L, S, _ = spec64.params(fs)
    out, at = [], 0
    for n in lengths:
        F = 0 if n < L else (n - (L - S)) // S
        for t in range(F):
            if t + ctx <= F:
                out.append(at + t)
        at += F
    return out


def lengths_for(fs, ctx):
    """fewer than one frame, exactly ctx - 1, ctx and ctx + 1 frames, with samples to spare that make no frame"""
    L, S, _ = spec64.params(fs)
    of = lambda F, extra=0: F * S + L - S + extra
    return [L - 1, of(ctx - 1), of(ctx, S - 1), 0, of(ctx + 1, 1), 1, of(1), of(3 * ctx)]


@pytest.mark.parametrize("fs", [8, 11, 16])
@pytest.mark.parametrize("ctx", [1, 3, 7])
def test_wave_samples_equals_the_restatement(pkg, fs, ctx):
    lengths = lengths_for(fs, ctx)
    got = pkg.wave_samples(lengths, ctx, fs)
    want = restated(lengths, ctx, fs)
    assert got.dtype == np.int32 and got.tolist() == want
    assert got.tolist() == mix64.wave_samples(lengths, ctx, fs).tolist()
    if ctx > 1:                                   # the utterance of exactly ctx - 1 frames has no window
        F = np.array([mix64.frames(n, fs) for n in lengths])
        assert F[1] == ctx - 1 and F[2] == ctx and F[4] == ctx + 1
        assert len(want) == sum(max(0, f - ctx + 1) for f in F)


@pytest.mark.parametrize("fs", [8, 11, 16])
def test_a_batch_whose_offsets_do_not_start_at_zero(pkg, fs):
    lengths = lengths_for(fs, 3)
    off = np.concatenate([[3], 3 + np.cumsum(lengths)]).astype(np.int64)
    n = C.c_int64(-1)
    assert pkg.load().mlggd_wave_samples(fs, 3, len(lengths), off.ctypes.data_as(LP), None, C.byref(n)) == 0
    want = restated(lengths, 3, fs)
    assert n.value == len(want)                                   # count only
    first = np.full(n.value + 1, -7, np.int32)
    assert pkg.load().mlggd_wave_samples(fs, 3, len(lengths), off.ctypes.data_as(LP), first.ctypes.data_as(IP),
                                         C.byref(n)) == 0
    assert first[:-1].tolist() == want and first[-1] == -7        # nothing past the count is written


def test_no_utterances_and_no_windows(pkg):
    assert pkg.wave_samples([], 3, 16).size == 0
    assert pkg.wave_samples([100, 511, 512 + 256], 3, 16).size == 0
