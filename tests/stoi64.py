"""STOI (Taal, Hendriks, Heusdens, Jensen: "An Algorithm for Intelligibility Prediction of Time-Frequency Weighted Noisy
Speech", IEEE TASL 2011) of a processed int16 wave against the clean int16 wave: the definition the device kernels of
csrc/stoi.hip.h are built against.

stoi64 is the published algorithm in float64 (numpy's FFT, numpy's sums).  stoi32 restates it the way the kernels run
it: every operation in float32 (the FFT in the kernels' radix-2 form, spec64.fft32), only log10 in double, and the
reductions in the kernels' order (a lane's strided partial sum, the 64-lane xor butterfly, 16 per-wave partials and a
halving tree).  Both return a Result; `value` is NaN and `segments` 0 when the utterance is too short or its clean wave
is silent.  A segment in which a band of the processed signal is exactly zero has alpha = inf and alpha Y = NaN, which
the minimum keeps: `value` is NaN, with the segments still counted.

Hooks for the tests: `kept` replaces the kept frames' list (in the order given: what a wrong scan would have written)
and `clip=False` leaves the minimum out.

Steps: resample both waves to 10 kHz by p/q with a Kaiser-windowed sinc; drop the frames (256 samples, hop 128, open
Hann window) whose clean energy is more than 40 dB below the loudest and overlap-add the kept ones; 512-point spectra
of the compacted signals' frames; 15 third-octave band magnitudes; per band and per segment of 30 frames, the
correlation coefficient of the clean band with the normalised and clipped processed band; the mean of those."""
import collections

import numpy as np

import spec64

F32 = np.float32
FS = 10000
N, K, NFFT, J, SEG = 256, 128, 512, 15, 30
BETA_DB, DYN_DB = -15.0, 40.0
RATES = {16: (5, 8), 8: (5, 4), 11: (10, 11)}     # fs_khz -> p / q; "11" is 11 000 Hz as in SPECTRAL_PARAMS
BANDS = [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87),
         (87, 109), (109, 138), (138, 174), (174, 219)]
WAVES = 16                                          # wavefronts of a k_stoi_utt workgroup

Result = collections.namedtuple("Result", "value len10 frames kept M segments min_margin min_var")


def thirdoct_rule(fs=FS, nfft=NFFT, bands=J, mn=150.0):
    """(lo, hi) per band by the rule of the original script's thirdoct(): the bins nearest to the band edges
    cf 2^(-1/6) and cf 2^(1/6), cf = mn 2^(j/3); band j sums the bins lo <= k < hi"""
    f = np.arange(nfft // 2 + 1) * (fs / nfft)
    out = []
    for j in range(bands):
        fl = np.sqrt((2.0 ** (j / 3.0) * mn) * (2.0 ** ((j - 1) / 3.0) * mn))
        fr = np.sqrt((2.0 ** (j / 3.0) * mn) * (2.0 ** ((j + 1) / 3.0) * mn))
        out.append((int(np.argmin((f - fl) ** 2)), int(np.argmin((f - fr) ** 2))))
    return out


def window():
    n = np.arange(N)
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * (n + 1) / (N + 1)))


def bessel_i0(x):
    """sum ((x/2)^k / k!)^2, in double"""
    x = np.asarray(x, np.float64)
    term, s = np.ones_like(x), np.ones_like(x)
    for k in range(1, 60):
        term = term * (x / 2.0) / k
        s = s + term * term
    return s


def resample_filter(p, q):
    """h[t + Lh], t = -Lh..Lh: 2 fc sinc(2 fc t) kaiser(2 Lh + 1, 5), scaled to sum p; float64"""
    m = max(p, q)
    Lh, fc = 10 * m, 1.0 / (2.0 * m)
    t = np.arange(-Lh, Lh + 1, dtype=np.float64)
    kais = bessel_i0(5.0 * np.sqrt(1.0 - (t / Lh) ** 2)) / bessel_i0(5.0)
    h = 2.0 * fc * np.sinc(2.0 * fc * t) * kais
    return h * (p / h.sum())


def len10(n, fs_khz):
    p, q = RATES[fs_khz]
    return -(-n * p // q)


def n_frames(length):
    """frame starts 0, K, 2K, ... <= length - N - 1 (the original's 1:K:(len-N))"""
    return 0 if length <= N else (length - N - 1) // K + 1


def layout(n, fs_khz):
    """(len10, frames, segments if every frame is kept) of an utterance of n samples"""
    l10 = len10(n, fs_khz)
    F = n_frames(l10)
    return l10, F, max(0, n_frames((F - 1) * K + N if F > 0 else 0) - (SEG - 1))


def shortest_with_frames(F, fs_khz):
    """the smallest sample count that gives F >= 1 frames"""
    p, q = RATES[fs_khz]
    want = (F - 1) * K + N + 1
    n = (want - 1) * q // p
    while len10(n, fs_khz) < want:
        n += 1
    return n


def resample(x, fs_khz, dtype=np.float64):
    """y[n] = sum_k h[n q - k p + Lh] x[k], summed in increasing k from 0, n < ceil(len p / q); dtype float32: h
    rounded to float32 and every product and sum in float32"""
    p, q = RATES[fs_khz]
    Lh = 10 * max(p, q)
    h = resample_filter(p, q).astype(dtype)
    x = np.asarray(x).astype(dtype)
    n = np.arange(len10(x.size, fs_khz), dtype=np.int64)
    acc = np.zeros(n.size, dtype)
    if x.size == 0:
        return acc
    kmin, kmax = -((Lh - n * q) // p), (n * q + Lh) // p
    for j in range(2 * Lh // p + 1):
        k = kmin + j
        ok = (k <= kmax) & (k >= 0) & (k < x.size)
        kk = np.where(ok, k, 0)
        idx = np.where(ok, n * q - kk * p + Lh, 0)
        acc = acc + np.where(ok, h[idx] * x[kk], dtype(0))
    return acc


def _frames(x, count):
    return x[np.arange(count)[:, None] * K + np.arange(N)[None, :]]


def _nan_result(l10, F, kept, M, margin):
    return Result(float("nan"), l10, F, kept, M, 0, margin, float("inf"))


def _cut(clean, proc, samples):
    clean, proc = np.asarray(clean), np.asarray(proc)
    assert clean.dtype == np.int16 and proc.dtype == np.int16
    n = min(clean.size, proc.size) if samples is None else int(samples)
    assert 0 <= n <= min(clean.size, proc.size)
    return clean[:n], proc[:n]


def stoi64(clean, proc, fs_khz=16, samples=None, proc_gain=1.0, kept=None, clip=True):
    """proc_gain: a gain on the processed signal applied in float64, after the int16 samples were read; kept: the kept
    frames' indices in compacted order instead of the rule's; clip=False: Y' = alpha Y, without the minimum"""
    clean, proc = _cut(clean, proc, samples)
    x, y = resample(clean, fs_khz), resample(proc, fs_khz) * proc_gain
    l10, w = x.size, window()
    F = n_frames(l10)
    if F == 0:
        return _nan_result(l10, 0, 0, 0, float("inf"))
    xf, yf = _frames(x, F) * w, _frames(y, F) * w
    with np.errstate(divide="ignore", invalid="ignore"):
        e = 20.0 * np.log10(np.sqrt((xf * xf).sum(axis=1)) / 16.0)
        rel = e - e.max() + DYN_DB
    keep = rel > 0
    margin = float(np.abs(rel[np.isfinite(rel)]).min()) if np.isfinite(rel).any() else float("inf")
    idx = np.flatnonzero(keep) if kept is None else np.asarray(kept, np.int64)
    kept = int(idx.size)
    if kept == 0:
        return _nan_result(l10, F, 0, 0, margin)
    xs, ys = np.zeros((kept - 1) * K + N), np.zeros((kept - 1) * K + N)
    for i, t in enumerate(idx):
        xs[i * K:i * K + N] += xf[t]
        ys[i * K:i * K + N] += yf[t]
    M = n_frames(xs.size)
    if M < SEG:
        return _nan_result(l10, F, kept, M, margin)
    PX = np.abs(np.fft.rfft(_frames(xs, M) * w, NFFT, axis=1)) ** 2
    PY = np.abs(np.fft.rfft(_frames(ys, M) * w, NFFT, axis=1)) ** 2
    X = np.sqrt(np.stack([PX[:, lo:hi].sum(axis=1) for lo, hi in BANDS]))      # [J][M]
    Y = np.sqrt(np.stack([PY[:, lo:hi].sum(axis=1) for lo, hi in BANDS]))
    c = 10.0 ** (-BETA_DB / 20.0)
    d, min_var = [], float("inf")
    for m in range(SEG - 1, M):
        Xs, Ys = X[:, m - SEG + 1:m + 1], Y[:, m - SEG + 1:m + 1]
        with np.errstate(divide="ignore", invalid="ignore"):      # a zero band: alpha = inf, alpha Y = NaN, kept
            alpha = np.sqrt((Xs * Xs).sum(axis=1, keepdims=True) / (Ys * Ys).sum(axis=1, keepdims=True))
            Yp = np.minimum(alpha * Ys, Xs + Xs * c) if clip else alpha * Ys
            xn, yn = Xs - Xs.mean(axis=1, keepdims=True), Yp - Yp.mean(axis=1, keepdims=True)
            nx, ny = np.sqrt((xn * xn).sum(axis=1)), np.sqrt((yn * yn).sum(axis=1))
            min_var = min(min_var, float((nx / np.sqrt((Xs * Xs).sum(axis=1))).min()),
                          float((ny / np.sqrt((Yp * Yp).sum(axis=1))).min()))
            d.append(((xn / nx[:, None]) * (yn / ny[:, None])).sum(axis=1))
    d = np.array(d)
    return Result(float(d.mean()), l10, F, kept, M, M - SEG + 1, margin, min_var)


# ---- the float32 restatement, in the kernels' order
def wave_sum32(v):
    """score_wave_sum over the last axis of 64 float32 lanes: v += v[lane ^ o] for o = 32, 16, ..., 1; lane 0"""
    v = np.asarray(v, F32)
    lane = np.arange(64)
    o = 32
    while o:
        v = v + v[..., lane ^ o]
        o >>= 1
    return v[..., 0]


def tree_mean32(values, count):
    """k_stoi_utt's mean: partial w of 16 adds values[w], values[w + 16], ... from 0.0f; the partials combine as
    s[i] += s[i + h], h = 8, 4, 2, 1; the result is s[0] / float(count)"""
    v = np.asarray(values, F32).ravel()
    s = np.zeros(WAVES, F32)
    for a in range(0, v.size, WAVES):
        row = v[a:a + WAVES]
        s[:row.size] = s[:row.size] + row
    h = WAVES // 2
    while h:
        s[:h] = s[:h] + s[h:2 * h]
        h >>= 1
    return F32(s[0] / F32(count))


def _power32(fr):
    """|rfft(frame, 512)|^2 of float32 frames [F][256] as the kernels form it: 256-point complex radix-2 FFT of the
    zero-padded even / odd samples and the real split step (spec64.analysis32's operations)"""
    Mh = NFFT // 2
    D = Mh + 1
    x = np.zeros((fr.shape[0], NFFT), F32)
    x[:, :N] = fr
    re, im = np.empty((x.shape[0], Mh), F32), np.empty((x.shape[0], Mh), F32)
    r = spec64.bitrev(np.arange(Mh), 8)
    re[:, r], im[:, r] = x[:, 0::2], x[:, 1::2]
    spec64.fft32(re, im, Mh, spec64.twiddle32(np.arange(Mh // 2), Mh))
    k = np.arange(D)
    ka, kb = np.where(k == Mh, 0, k), np.where(k == 0, 0, Mh - k)
    zr, zi, cr, ci = re[:, ka], im[:, ka], re[:, kb], -im[:, kb]
    h = F32(0.5)
    er, ei, orr, oi = (zr + cr) * h, (zi + ci) * h, (zr - cr) * h, (zi - ci) * h
    wx, wy = spec64.twiddle32(k, NFFT)
    pr, pi = wx * orr - wy * oi, wx * oi + wy * orr
    xr, xi = er + pi, ei - pr
    return xr * xr + xi * xi


def _bands32(P):
    out = np.empty((J, P.shape[0]), F32)
    for j, (lo, hi) in enumerate(BANDS):
        s = np.zeros(P.shape[0], F32)
        for k in range(lo, hi):
            s = s + P[:, k]
        out[j] = np.sqrt(s)
    return out


def stoi32(clean, proc, fs_khz=16, samples=None, kept=None):
    """kept: as in stoi64"""
    clean, proc = _cut(clean, proc, samples)
    x, y = resample(clean, fs_khz, F32), resample(proc, fs_khz, F32)
    l10, w = x.size, window().astype(F32)
    F = n_frames(l10)
    if F == 0:
        return _nan_result(l10, 0, 0, 0, float("inf"))
    xf, yf = _frames(x, F) * w, _frames(y, F) * w
    sq = (xf * xf).reshape(F, 4, 64)
    part = np.zeros((F, 64), F32)
    for r in range(4):                                      # a lane's elements lane, lane + 64, ... in index order
        part = part + sq[:, r]
    with np.errstate(divide="ignore", invalid="ignore"):
        nrm = np.sqrt(wave_sum32(part)) / F32(16.0)
        e = F32(20.0) * np.log10(nrm.astype(np.float64)).astype(F32)
        rel = (e - e.max()) + F32(DYN_DB)
    keep = rel > 0
    margin = float(np.abs(rel[np.isfinite(rel)]).min()) if np.isfinite(rel).any() else float("inf")
    idx = np.flatnonzero(keep) if kept is None else np.asarray(kept, np.int64)
    kept = int(idx.size)
    M = max(kept - 1, 0)
    if M < SEG:
        return _nan_result(l10, F, kept, M, margin)

    def compact(f):
        """frame m of the overlap-added kept frames: first half = second half of kept m - 1 (m >= 1) + first half of
        kept m, second half = second half of kept m + first half of kept m + 1; then the window again"""
        a = f[idx[:M]]
        out = a.copy()
        out[1:, :K] = f[idx[:M - 1], K:] + a[1:, :K]
        out[:, K:] = a[:, K:] + f[idx[1:M + 1], :K]
        return out * w

    X, Y = _bands32(_power32(compact(xf))), _bands32(_power32(compact(yf)))    # [J][M]
    c = F32(10.0 ** (-BETA_DB / 20.0))
    S = M - SEG + 1
    at = np.arange(S)[:, None] + np.arange(SEG)[None, :]                        # [S][30]
    Xs, Ys = X[:, at], Y[:, at]                                                 # [J][S][30]
    z = np.zeros((J, S), F32)
    ex, ey, sx = z.copy(), z.copy(), z.copy()
    for f in range(SEG):
        ex, ey, sx = ex + Xs[..., f] * Xs[..., f], ey + Ys[..., f] * Ys[..., f], sx + Xs[..., f]
    with np.errstate(divide="ignore", invalid="ignore"):          # a zero band: as in stoi64
        alpha = np.sqrt(ex / ey)
        Yp = np.minimum(alpha[..., None] * Ys, Xs + Xs * c)
    sy = z.copy()
    for f in range(SEG):
        sy = sy + Yp[..., f]
    mx, my = sx / F32(SEG), sy / F32(SEG)
    sxx, syy, sxy = z.copy(), z.copy(), z.copy()
    for f in range(SEG):
        a, b = Xs[..., f] - mx, Yp[..., f] - my
        sxx, syy, sxy = sxx + a * a, syy + b * b, sxy + a * b
    d = sxy / (np.sqrt(sxx) * np.sqrt(syy))                                     # [J][S]
    lanes = np.zeros((S, 64), F32)
    lanes[:, :J] = d.T
    value = tree_mean32(wave_sum32(lanes), J * S)
    return Result(float(value), l10, F, kept, M, S, margin, float("nan"))


# ---- test signals
def speech(n, fs_khz, seed, gaps=()):
    """spec64.synth_speech with the sample ranges gaps = [(a, b), ...] scaled down by 70 dB"""
    s = spec64.synth_speech(n, fs_khz, seed=seed).astype(np.float64)
    for a, b in gaps:
        s[a:b] *= 10.0 ** (-70.0 / 20.0)
    return np.round(s).astype(np.int16)


def add_noise(clean, snr_db, seed):
    c = clean.astype(np.float64)
    noise = np.random.default_rng(seed).normal(0.0, 1.0, c.size)
    noise *= np.sqrt((c * c).mean() / (noise * noise).mean() / 10.0 ** (snr_db / 10.0))
    return np.clip(np.round(c + noise), -32768, 32767).astype(np.int16)
