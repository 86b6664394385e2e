"""The model of the mixing rule (csrc/mix_rule.h) the tests compare the device with: numpy only, Python integers for the
energies, float64 for the gain and the mix, math.pow for the ratio.  Written for the tests; the original project has no
mixer."""
import math

import numpy as np

from spec64 import params


def ratio(snr_db):
    """r = 10^(-snr_db / 20); +inf gives 0"""
    return 0.0 if snr_db == math.inf else math.pow(10.0, -snr_db / 20.0)


def paired(noise, lo, ln, start, n):
    """the n noise samples an utterance of n samples is paired with: noise[lo + (start + i) mod ln]"""
    return noise[lo + (start + np.arange(n, dtype=np.int64)) % ln]


def energies(clean, nz):
    """(Ec, En) as Python integers: exact"""
    return (sum(int(c) * int(c) for c in clean.tolist()), sum(int(z) * int(z) for z in nz.tolist()))


def gain(Ec, En, r):
    if Ec == 0 or En == 0 or r == 0.0:
        return 0.0
    return math.sqrt(float(Ec) / float(En)) * r          # float(int) rounds to nearest


def unrounded(clean, nz, g):
    return clean.astype(np.float64) + g * nz.astype(np.float64)     # two float64 operations


def mix(clean, nz, g):
    """(noisy int16, clipped): rint to nearest even, then the clamp; clipped counts what the clamp changed"""
    v = np.rint(unrounded(clean, nz, g))
    clipped = int(np.count_nonzero((v > 32767.0) | (v < -32768.0)))
    return np.clip(v, -32768.0, 32767.0).astype(np.int16), clipped


def mix_utt(clean, noise, lo, ln, start, snr_db, g=None):
    """(noisy, gain, clipped) of one utterance; g: use this gain instead of the model's own"""
    nz = paired(noise, lo, ln, start, clean.size)
    if g is None:
        g = gain(*energies(clean, nz), ratio(snr_db))
    out, clipped = mix(clean, nz, g)
    return out, g, clipped


def frames(n, fs_khz):
    L, S, _ = params(fs_khz)
    return 0 if n < L else (n - (L - S)) // S


def wave_samples(lengths, ctx, fs_khz):
    """every window of ctx frames inside one utterance, as indices into the packed frames"""
    out, at = [], 0
    for n in lengths:
        F = frames(n, fs_khz)
        out += [at + t for t in range(F - ctx + 1)]
        at += F
    return np.array(out, np.int32)
