"""Inputs of the STOI edge tests (tests/test_gpu_stoi_edges.py on the device, their CPU companions in
tests/test_stoi_model.py): utterances whose kept frames lie where k_stoi_select, stoi_compacted and k_stoi_utt could be
wrong without the short batch of tests/test_gpu_stoi.py noticing.  Every builder is cached and its arrays read-only.

Gaps are given in 10 kHz frame units: frame t covers the 10 kHz samples [128 t, 128 t + 256), a gap [a, b) the samples
[128 a, 128 b), scaled by q / p to input samples.  A gap is 70 dB down, which rounds to exact zeros in int16: its frames
have e = -inf.  k_stoi_select scans in trips of 256 frames."""
import functools

import numpy as np

import stoi64

TRIP = 256                                          # 64 * STOI_SELECT_WAVES
RATE = {8: 8000, 11: 11000, 16: 16000}
A_GAPS = ((0, 248), (264, 504), (520, 602))
B_GAPS = ((0, 5), (200, 520), (690, 702)) + tuple((a, a + 3) for a in range(560, 640, 8))
# C: (bursts of one frame, bursts of a frame and a half) every 19 frames from frame 4 -> kept frames
C_VARIANTS = {32: (16, 0), 31: (14, 1), 30: (15, 0)}


def frozen(a):
    a.setflags(write=False)
    return a


def to_samples(frame_gaps, fs, n):
    """[a, b) in 10 kHz frame units (halves allowed) -> input sample ranges inside 0..n"""
    p, q = stoi64.RATES[fs]
    return [(min(n, int(stoi64.K * a) * q // p), min(n, int(stoi64.K * b) * q // p)) for a, b in frame_gaps]


def utterance(frames, fs, seed, frame_gaps):
    n = stoi64.shortest_with_frames(frames, fs)
    return frozen(stoi64.speech(n, fs, seed=seed, gaps=to_samples(frame_gaps, fs, n)))


def impulsive(clean, starts, seed):
    """noise at 20 dB plus a burst of 400 samples with sigma 8000 from every start, saturated to int16: a few frames
    of a segment far above the segment's rms ratio, which is what the clipping is for"""
    rng = np.random.default_rng(seed)
    v = stoi64.add_noise(clean, 20, seed=seed + 1).astype(np.float64)
    for a in starts:
        v[a:a + 400] += rng.normal(0.0, 8000.0, 400)
    return frozen(np.clip(np.round(v), -32768, 32767).astype(np.int16))


@functools.lru_cache(maxsize=None)
def case_a(fs, snr):
    """600 frames, loud in frames 247..263 and 503..519 alone: trip 1 keeps only its tail, trip 2 both ends, trip 3
    only its head; 34 kept, 4 segments.  snr: of the added noise in dB, or "impulsive": a burst in each loud stretch"""
    c = utterance(600, fs, 700 + fs, A_GAPS)
    if snr == "impulsive":
        return c, impulsive(c, [a + 1000 for _, a in to_samples(A_GAPS, fs, c.size)[:2]], seed=712 + fs)
    return c, frozen(stoi64.add_noise(c, snr, seed=710 + fs + (snr < 0)))


@functools.lru_cache(maxsize=None)
def case_b(fs):
    """700 frames, mostly kept: the first frames dropped (compacted frame 0 is not frame 0), trip 2's interior empty,
    ten short gaps in trip 3, the last frames dropped"""
    c = utterance(700, fs, 720 + fs, B_GAPS)
    return c, frozen(stoi64.add_noise(c, 5, seed=730 + fs))


def c_bursts(variant):
    ones, longs = C_VARIANTS[variant]
    return [(4 + 19 * i, 4 + 19 * i + (1 if i < ones else 1.5)) for i in range(ones + longs)]


@functools.lru_cache(maxsize=None)
def case_c(fs, variant):
    """300 frames, loud only in short bursts 19 frames apart: a burst of one frame keeps 2 frames, one of a frame and
    a half 3, so every compacted frame is rebuilt from frames that are no neighbours.  variant = the kept count: 32
    (2 segments), 31 (one segment), 30 (no value, although 300 frames >= 31)"""
    bursts = c_bursts(variant)
    edges = [0] + [v for b in bursts for v in b] + [302]
    c = utterance(300, fs, 740 + fs + variant, list(zip(edges[0::2], edges[1::2])))
    return c, frozen(stoi64.add_noise(c, 5, seed=750 + fs + variant))


@functools.lru_cache(maxsize=None)
def case_d(fs, n):
    """n samples: 1 is shorter than every filter tap range, 100 gives 10 kHz samples and no frame, 0 nothing"""
    c = frozen(stoi64.speech(n, fs, seed=760 + n))
    return c, frozen(stoi64.add_noise(c, 5, seed=761 + n)) if n else c


E_ZEROED = {2: 10000, 3: 2048}                      # samples set to zero from sample 9000 of the processed wave


@functools.lru_cache(maxsize=None)
def case_e(fs, kind):
    """2 s; the processed wave: 0 = noisy at 5 dB; 1 = all zeros; 2 = noisy with a zeroed stretch so long that whole
    segments have Y = 0 in every band (no value by the definition); 3 = noisy with a zeroed stretch of about 10 frames
    (exact zeros in Y, every segment's sum of squares positive: a value); 4 = impulsive: noise at 20 dB plus bursts of
    400 samples with sigma 8000 every 4000 samples, saturated"""
    assert fs == 16
    c = frozen(stoi64.speech(2 * RATE[fs], fs, seed=770))
    if kind == 1:
        return c, frozen(np.zeros_like(c))
    if kind == 4:
        return c, impulsive(c, range(1000, c.size - 400, 4000), seed=772)
    p = stoi64.add_noise(c, 5, seed=771)
    if kind in E_ZEROED:
        p[9000:9000 + E_ZEROED[kind]] = 0
    return c, frozen(p)


@functools.lru_cache(maxsize=None)
def models(builder, *args):
    """(stoi64, stoi32) of a case, evaluated once"""
    c, p = builder(*args)
    fs = args[0]
    return stoi64.stoi64(c, p, fs), stoi64.stoi32(c, p, fs)


def rows(spec):
    """[(builder, args...), ...] -> cleans, procs, models"""
    pairs = [b(*a) for b, *a in spec]
    return [c for c, _ in pairs], [p for _, p in pairs], [models(b, *a) for b, *a in spec]


def trips_batch(fs):
    """A at +5 and -5 dB, the three C variants, and the short utterances first, in the middle and last"""
    return [(case_d, fs, 1), (case_a, fs, 5), (case_a, fs, -5), (case_d, fs, 100), (case_c, fs, 32), (case_c, fs, 31),
            (case_c, fs, 30), (case_d, fs, 0)]


def long_batch(fs):
    return [(case_d, fs, 0), (case_b, fs), (case_d, fs, 1), (case_a, fs, 5), (case_c, fs, 32), (case_d, fs, 100)]


def model_distance(ms, muted=()):
    """the batch's distance of stoi32 to stoi64: the largest over its utterances that have a value"""
    return max(abs(m32.value - m64.value) for u, (m64, m32) in enumerate(ms) if m64.segments and u not in muted)
