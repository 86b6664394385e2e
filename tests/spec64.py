"""Float64 restatement of the spectral front end and back end (Wav2LPS_be / LPS2Wav_be of the original project,
Wav2LogSpec_be.c / LogSpec2Wav.c / FEfunc.c) with a hard per-element error bound for an fp32 FFT (CPU only).

Notation as in bounds64.py: u = 2^-24.

Analysis, per frame t (samples [t S, t S + L), window w rounded to float, zero padding to N):
    x_t = frame * w (exact in float64: 16-bit integers times 24-bit mantissas), X = DFT_N(x_t), P = |X|^2,
    lps = log(P) where P >= float(exp(-50)), else exactly -50.

FFT bound (`fft_bound`).  A radix-2 FFT of n points in fp32 with twiddles of relative error mu satisfies
    ||fl(FFT x) - FFT x||_2 <= log2(n) eta / (1 - log2(n) eta) ||FFT x||_2,   eta = mu + gamma_4 (sqrt(2) + mu)
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm. 24.2).  The kernels form the real N-point
spectrum as an N/2-point complex FFT of z_m = x_2m + i x_2m+1 (log2(N) - 1 stages) followed by the real split step
X_k = (Z_k + conj Z_{N/2-k}) / 2 - i W^k (Z_k - conj Z_{N/2-k}) / 2, one more butterfly stage of the same form.  With
twiddles computed in double and rounded to float, mu = u, eta = u + gamma_4 (sqrt(2) + u) < 6.66 u.  Per bin
|dX_k| <= |dZ_k| + |dZ_{N/2-k}| <= sqrt(2) ||dZ||_2 and ||Z||_2 = sqrt(N/2) ||x||_2, so the complex stages give
(log2(N) - 1) eta sqrt(N) ||x||_2 per bin, the split step eta sqrt(N) ||x||_2 more, and the rounding of x * w (u per
element) sqrt(N) u ||x||_2 (|sum_n dx_n e^..| <= ||dx||_1 <= sqrt(N) ||dx||_2).  In all
    |fl(X_k) - X_k| <= (log2(N) eta + u) sqrt(N) ||x_t||_2 <= C_FFT log2(N) u sqrt(N) ||x_t||_2,   C_FFT = 7
(9 * 6.66 + 1 = 61 < 63 for N = 512; 8 * 6.66 + 1 = 54.3 < 56 for N = 256; the 1 / (1 - log2(N) eta) factor is below
1 + 1e-5).  Any correct fp32 FFT of this form meets it; the original project's own split-radix FFT meets it on its
recorded data too (tests/test_spec64.py).

Log domain (`lps_ok`).  With E = the bound above and A = |X_k| (float64), a computed power P^ = |X^|^2 (1 + d),
|d| <= 3 u (two products and a sum), lies in [(A - E)^2, (A + E)^2] (1 +- 3u); log(P^) is formed in double and rounded
to float (half an ulp of |lps|).  So where A > E:
    |lps - log A^2| <= -2 log(1 - E / A) + 3.01 u + u |lps|.
Where A <= E (the bin may have cancelled to the noise of the FFT, or to exactly zero: digital silence), the value is
checked in the amplitude domain: lps == -50 exactly, or exp(lps / 2) <= (A + E)(1 + 2 u + u |lps|).

Synthesis (`synthesis64`; LogSpec2Wav.c with OLA_KIND 1, POSTPROCESS 0, SMOOTHPROCESS 0): P^ = exp(lps), floored at
exp(-50) below lps < -50; Y_k = X_k sqrt(P^_k) / |X_k| (noisy phase; phase 0 where |X_k| = 0, a deliberate deviation:
the original divides 0 by 0 there); y_t = IDFT_N(Y)[:L] * w; the output is sum_t y_t / sum_t w^2 over the frames that
cover each sample, F S + L - S samples, truncated toward zero and saturated to int16.

Quality (`quality64`; LogSpec2Wav.c:597-613, 700-712, 747-797, 828-842): segmental SNR compares each clean frame with
the de-windowed synthesised frame (IDFT_N(Y)[:L]), 10 log10(sum clean^2 / sum err^2) clamped to [-20, 30], averaged over
frames; log-spectral distortion floors the clean power and the enhanced power (exp of the LPS) at 1e-5 times their
own maxima (50 dB) and averages, over frames, sqrt(mean_k (10 log10(P_enh / P_clean))^2).
"""
import numpy as np

U = 2.0 ** -24
C_FFT = 7.0
C_NORM = 9.0   # the normwise bound of the whole error spectrum (synthesis_bound)
FLOOR_P = float(np.float32(np.exp(-50.0)))  # (float) exp(-50.0), the analysis floor
PARAMS = {8: (256, 128, 256), 11: (256, 110, 256), 16: (512, 256, 512)}  # fs_khz -> frame L, hop S, FFT N


def params(fs_khz):
    if fs_khz not in PARAMS:
        raise ValueError("fs_khz must be 8, 11 or 16")
    return PARAMS[fs_khz]


def window(L):
    """float32 Hamming: the half table (float)(0.54 - 0.46 cos(2 pi i / (L - 1))), mirrored (FEfunc.c)."""
    i = np.arange(L // 2)
    half = (0.54 - 0.46 * np.cos(2.0 * np.pi * i / (L - 1))).astype(np.float32)
    return np.concatenate([half, half[::-1]])


def n_frames(n_samples, fs_khz):
    L, S, _ = params(fs_khz)
    return max(0, (int(n_samples) - (L - S)) // S)


def frames(wave, fs_khz):
    """[F][L] float64 frames of the int16 wave, trailing samples dropped."""
    L, S, _ = params(fs_khz)
    F = n_frames(len(wave), fs_khz)
    idx = np.arange(F)[:, None] * S + np.arange(L)[None, :]
    return np.asarray(wave, np.float64)[idx]


def spectrum64(wave, fs_khz):
    """X [F][N/2+1] complex128 of the windowed frames, and ||x_t * w||_2 per frame."""
    L, S, N = params(fs_khz)
    xw = frames(wave, fs_khz) * window(L).astype(np.float64)
    return np.fft.rfft(xw, n=N, axis=1), np.sqrt((xw * xw).sum(axis=1))


def fft_bound(norm_xw, fs_khz):
    """The per-bin amplitude bound of an fp32 FFT of one frame, for every frame (module docstring)."""
    N = params(fs_khz)[2]
    return C_FFT * np.log2(N) * U * np.sqrt(N) * np.asarray(norm_xw, np.float64)


def fft_norm_bound(norm_xw, fs_khz):
    """The weighted 2-norm bound sqrt(sum_k w_k |dX_k|^2) of an fp32 FFT's whole error spectrum, for every frame
    (derived in synthesis_bound)"""
    N = params(fs_khz)[2]
    return C_NORM * np.log2(N) * U * np.sqrt(N) * np.asarray(norm_xw, np.float64)


def analysis64(wave, fs_khz=16):
    """lps [F][N/2+1] float64 (the float rounding of the original left out), X, per-frame amplitude bound E."""
    X, nrm = spectrum64(wave, fs_khz)
    P = np.abs(X) ** 2
    with np.errstate(divide="ignore"):
        lps = np.where(P >= FLOOR_P, np.log(np.maximum(P, 1e-300)), -50.0)
    return lps, X, fft_bound(nrm, fs_khz)


def lps_ok(lps, X, E):
    """Boolean mask: every fp32 lps element within the analysis bound of the float64 spectrum X (module docstring)."""
    lps = np.asarray(lps, np.float64)
    A = np.abs(X)
    E = np.broadcast_to(np.asarray(E, np.float64).reshape(-1, 1), A.shape)
    rnd = 3.01 * U + U * np.abs(lps)
    far = A > E
    with np.errstate(divide="ignore", invalid="ignore"):
        d_log = np.abs(lps - 2.0 * np.log(np.where(A > 0, A, 1.0)))
        tol = -2.0 * np.log1p(-np.where(far, E / np.where(far, A, 1.0), 0.0)) + rnd
    ok_far = far & (d_log <= tol)
    near = ~far
    ok_near = near & ((lps == -50.0) | (np.exp(lps / 2.0) <= (A + E) * (1.0 + 2 * U + U * np.abs(lps))))
    return ok_far | ok_near


def lps_err_ratio(lps, X, E):
    """max over the far-from-floor elements of |lps - log A^2| / tolerance (<= 1 passes): how close to the bound."""
    lps = np.asarray(lps, np.float64)
    A = np.abs(X)
    E = np.broadcast_to(np.asarray(E, np.float64).reshape(-1, 1), A.shape)
    far = A > 2 * E
    tol = -2.0 * np.log1p(-E[far] / A[far]) + 3.01 * U + U * np.abs(lps[far])
    return float((np.abs(lps[far] - 2.0 * np.log(A[far])) / tol).max())


def trunc_sat(y):
    """(short) of the original with saturation instead of the undefined wrap-around (a deliberate deviation)."""
    return np.clip(np.trunc(np.asarray(y, np.float64)), -32768, 32767).astype(np.int16)


def _modified_spectrum(X, lps):
    lps = np.asarray(lps, np.float64)
    Ph = np.where(lps < -50.0, np.exp(-50.0), np.exp(lps))
    mag = np.sqrt(Ph)
    A = np.abs(X)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(A > 0, X * (mag / np.where(A > 0, A, 1.0)), mag + 0j)


def synthesis64(noisy, lps, fs_khz=16, return_frames=False):
    """float64 output wave (before the int16 cast) of LogSpec2Wav.c; lps [F][N/2+1] with F = n_frames(noisy)."""
    L, S, N = params(fs_khz)
    X, _ = spectrum64(noisy, fs_khz)
    F = X.shape[0]
    lps = np.asarray(lps, np.float64)
    if lps.shape != X.shape:
        raise ValueError("lps must be [%d][%d]" % X.shape)
    raw = np.fft.irfft(_modified_spectrum(X, lps), n=N, axis=1)[:, :L]   # rifft (divides by N)
    w = window(L).astype(np.float64)
    y = raw * w
    out = np.zeros(F * S + L - S)
    cnt = np.zeros_like(out)
    for t in range(F):
        out[t * S:t * S + L] += y[t]
        cnt[t * S:t * S + L] += w * w
    with np.errstate(invalid="ignore", divide="ignore"):
        out = out / cnt
    return (out, raw / w) if return_frames else out


def ola_norm(F, fs_khz):
    """sum_t w^2 over the frames covering each output sample (float64)."""
    L, S, _ = params(fs_khz)
    w = window(L).astype(np.float64)
    cnt = np.zeros(F * S + L - S)
    for t in range(F):
        cnt[t * S:t * S + L] += w * w
    return cnt


def synthesis_bound(noisy, lps, fs_khz=16, lps_eps=0.0):
    """Per-sample bound on |fp32 synthesis - synthesis64| for LPS rows `lps` given exactly, plus `lps_eps` of error in
    the log domain (a scalar or a per-element [F][N/2+1] array: the chain's bound of `decode64`).

    Derivation, per frame t and bin k (Y = the modified spectrum of `synthesis64`, mag = sqrt(exp(lps))):
    * noisy phase: X^ / |X^| is within 2 |dX_k| / |X_k| of X / |X| (dX = X^ - X, the analysis error), and within 2
      (the diameter of the unit circle) outright, which is what is taken where |X| <= E_t: the bin may have cancelled.
      The analysis error is bounded normwise as well (`fft_norm_bound`): the weighted 2-norm
      sqrt(sum_k w_k |dX_k|^2) of the error spectrum (w_k as below: the norm of the conjugate-symmetric N-point
      extension) is at most C_NORM log2(N) u sqrt(N) ||x_t||_2, C_NORM = 9.  Derivation: Higham's theorem bounds the
      complex stages normwise, ||dZ||_2 <= (log2(M) eta + u) sqrt(M) ||x_t||_2 (the rounding of x * w included; ||Z||_2
      = sqrt(M) ||x_t||_2).  The exact split step maps Z onto the N-point spectrum with norm ratio sqrt(2) (N ||x||^2
      against M ||x||^2), which gives (log2(M) eta + u) sqrt(N) ||x_t||.  Its own roundings per bin: E and O one
      rounding each (u |E|, u |O|), W^k O a complex product with a rounded twiddle (sqrt(2) gamma_2 + u, < 4.9 u, plus
      O's u), the final sum u (|E| + |P|): below 8 u (|E| + |O|) <= 8 u (|Z_k| + |Z_{M-k}|).  Weighted over the bins,
      sum_k w_k (|Z_k| + |Z_{M-k}|)^2 <= 2 sum_k w_k (|Z_k|^2 + |Z_{M-k}|^2) <= 8 ||Z||^2, so these add
      2 * 8 u sqrt(N) ||x_t||.  In all (log2(N) - 1) 6.66 u + 17 u per sqrt(N) ||x_t||: 70.3 u < 9 * 9 u at N = 512,
      63.6 u < 9 * 8 u at N = 256.  So by Cauchy-Schwarz the phase error reaches a time sample with at most
      2 sqrt(sum_k w_k (mag_k / |X_k|)^2) E_norm / N, summed over the bins with |X| > E_t (any threshold is sound
      there; below it the cap 2 is taken): a factor ~sqrt(N) below the per-bin E_t summed bin by bin;
    * magnitude: exp in double rounded to float, sqrtf, |X^| (two products, a sum, sqrtf), mag / A, X * g: fewer than
      10 roundings, 10 u relative;
    * an lps error eps moves mag by a factor exp(+-eps / 2): expm1(eps / 2) relative, counted twice for the
      second-order term and the float rounding of the chain's output;
    so |dY_k| <= mag (10 u + 2 expm1(eps / 2)) besides the phase term.  The inverse real split and the M-point inverse FFT are the
    forward form run backwards (the conjugate trick): a per-sample error of at most sum_k w_k |dY_k| / N (w_k = 2 for the
    bins that appear twice in the real spectrum, 1 for DC and Nyquist) from the input, and C_FFT log2(N) u ||Y||_2 /
    sqrt(N) from the arithmetic (the forward bound of the module docstring, scaled by the exact 1 / M and the split's
    1 / 2), with ||Y|| taken at mag (1 + ph) to cover the perturbed phase.  The window multiply adds u |raw|.  The
    overlap-add sums at most ceil(L / S) = 3 terms (2 at 8 and 16 kHz) in frame order, divides by sum w^2 formed the
    same way (3 roundings more) and the division rounds once: 6 u of the sum of |terms|.  1.01 covers the second-order
    products.  A slip below these margins -- one ulp in one twiddle, the floor compare `<` against `<=` at exactly
    -50 (which changes exp(-50) by nothing: the floor IS exp(-50)) -- is below what the bound can resolve."""
    L, S, N = params(fs_khz)
    X, nrm = spectrum64(noisy, fs_khz)
    E = fft_bound(nrm, fs_khz)[:, None]
    lps = np.asarray(lps, np.float64)
    mag = np.sqrt(np.where(lps < -50, np.exp(-50.0), np.exp(lps)))
    A = np.abs(X)
    far = A > E
    with np.errstate(divide="ignore", invalid="ignore"):
        ph = np.where(far, np.minimum(2.0, 2.0 * E / np.where(A > 0, A, 1.0)), 2.0)
        q = np.where(far, mag / np.where(far, A, 1.0), 0.0)
    dY = mag * (np.where(far, 0.0, 2.0) + 10 * U + 2 * np.expm1(np.asarray(lps_eps, np.float64) / 2.0))
    wts = np.full(dY.shape[1], 2.0)
    wts[0] = wts[-1] = 1.0
    Ymax = mag * (1 + ph)
    e_phase = 2.0 * np.sqrt((q * q * wts).sum(axis=1)) * fft_norm_bound(nrm, fs_khz) / N
    e = (dY * wts).sum(axis=1) / N + e_phase + \
        C_FFT * np.log2(N) * U * np.sqrt((Ymax ** 2 * wts).sum(axis=1)) / np.sqrt(N)
    _, raw = synthesis64(noisy, lps, fs_khz, return_frames=True)
    w = window(L).astype(np.float64)
    F = X.shape[0]
    acc, mag_acc = np.zeros(F * S + L - S), np.zeros(F * S + L - S)
    for t in range(F):
        acc[t * S:t * S + L] += w * (e[t] + U * np.abs(raw[t]).max())
        mag_acc[t * S:t * S + L] += np.abs(raw[t] * w) + w * e[t]
    cnt = ola_norm(F, fs_khz)
    return 1.01 * (acc / cnt + 6 * U * mag_acc / cnt)


def synthesis_ratio(out_f, noisy, lps, fs_khz=16, lps_eps=0.0):
    """worst |out_f - synthesis64| / synthesis_bound over the samples (<= 1 passes; NaN / inf count as inf)"""
    want = synthesis64(noisy, lps, fs_khz)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(np.asarray(out_f, np.float64) - want)
    err = np.where(np.isfinite(err), err, np.inf)
    return float((err / synthesis_bound(noisy, lps, fs_khz, lps_eps)).max())


# ---------------------------------------------------------------------------------------------------------------------
# float32 restatements of the kernels (spectral.hip.h): every step the IEEE fp32 operation the kernel performs, in the
# same order, vectorised across frames.  They serve as the "correct fp32 twin" that the bounds must pass and as the
# body into which the mutation tests plant one-line slips.
F32 = np.float32


def twiddle32(k, n):
    """exp(-2 pi i k / n) in double, exact zeros where the value is 0, rounded to float (engine.hip twiddle())"""
    k = np.asarray(k)
    a = -2.0 * np.pi * k / n
    c, s = np.cos(a), np.sin(a)
    c = np.where((4 * k == n) | (4 * k == 3 * n), 0.0, c)
    s = np.where((2 * k == n) | (k == 0), 0.0, s)
    return c.astype(F32), s.astype(F32)


def bitrev(m, logM):
    m = np.asarray(m)
    r = np.zeros_like(m)
    for b in range(logM):
        r |= ((m >> b) & 1) << (logM - 1 - b)
    return r


def round_bits(a, bits):
    """round float32 values to `bits` explicit mantissa bits, to nearest even (bf16: 7, a 10-bit mantissa: 10)"""
    u = np.asarray(a, F32).view(np.uint32).astype(np.uint64)
    drop = 23 - bits
    half = (1 << (drop - 1)) - 1
    u = (u + half + ((u >> drop) & 1)) & ~np.uint64((1 << drop) - 1)
    return u.astype(np.uint32).view(F32)


def fft32(re, im, M, tw, bf16_stage=None):
    """spec_fft_rows: radix-2 DIT butterflies in place on [F][M] rows already in bit-reversed order; twiddle pair tw;
    bf16_stage: that stage's operands rounded to bf16 (a mutation)"""
    logM = int(np.log2(M))
    b = np.arange(M // 2)
    for s in range(logM):
        h, tstep = 1 << s, M >> (s + 1)
        j = b & (h - 1)
        i0 = ((b >> s) << (s + 1)) + j
        i1 = i0 + h
        wx, wy = tw[0][j * tstep], tw[1][j * tstep]
        ar, ai, br, bi = re[:, i0], im[:, i0], re[:, i1], im[:, i1]
        if s == bf16_stage:
            ar, ai, br, bi = (round_bits(v, 7) for v in (ar, ai, br, bi))
        cr = br * wx - bi * wy
        ci = br * wy + bi * wx
        re[:, i0], im[:, i0] = ar + cr, ai + ci
        re[:, i1], im[:, i1] = ar - cr, ai - ci
    return re, im


def analysis32(wave, fs_khz=16):
    """k_lps_analysis in float32: (lps [F][D] float32, X real and imaginary parts [F][D] float32)"""
    L, S, N = params(fs_khz)
    M, D = N // 2, N // 2 + 1
    logM = int(np.log2(M))
    x = np.zeros((n_frames(len(wave), fs_khz), N), F32)
    x[:, :L] = frames(wave, fs_khz).astype(F32) * window(L)
    re, im = np.empty((x.shape[0], M), F32), np.empty((x.shape[0], M), F32)
    r = bitrev(np.arange(M), logM)
    re[:, r], im[:, r] = x[:, 0::2], x[:, 1::2]
    fft32(re, im, M, twiddle32(np.arange(M // 2), M))
    k = np.arange(D)
    ka, kb = np.where(k == M, 0, k), np.where(k == 0, 0, M - k)
    zr, zi, cr, ci = re[:, ka], im[:, ka], re[:, kb], -im[:, kb]
    h = F32(0.5)
    er, ei, orr, oi = (zr + cr) * h, (zi + ci) * h, (zr - cr) * h, (zi - ci) * h
    wx, wy = twiddle32(k, N)
    pr, pi = wx * orr - wy * oi, wx * oi + wy * orr
    xr, xi = er + pi, ei - pr
    P = xr * xr + xi * xi
    with np.errstate(divide="ignore"):
        lps = np.where(P < F32(FLOOR_P), F32(-50.0), np.log(P.astype(np.float64)).astype(F32)).astype(F32)
    return lps, xr, xi


SYNTH_MUTATIONS = ["window_n_plus_1", "ola_norm_missing_frame", "block_one_sample_late", "split_W_not_conj",
                   "nyquist_dropped", "no_final_conj", "phase_of_next_frame", "bf16_butterfly_stage",
                   "twiddle_10bit"]


def synthesis32(noisy, lps, fs_khz=16, mean=None, inv=None, mut=None):
    """k_lps_synthesis + k_ola in float32: (int16 wave, float32 wave before the cast).  With mean / inv the rows are
    de-normalised first (fl(fl(y / inv) + mean)), as in enhance_wave.  `mut` plants one of SYNTH_MUTATIONS."""
    L, S, N = params(fs_khz)
    M, D = N // 2, N // 2 + 1
    logM = int(np.log2(M))
    _, xr, xi = analysis32(noisy, fs_khz)
    Fn = xr.shape[0]
    if mut == "phase_of_next_frame":
        nxt = np.minimum(np.arange(Fn) + 1, Fn - 1)
        xr, xi = xr[nxt], xi[nxt]
    v = np.asarray(lps, F32)
    if v.shape != (Fn, D):
        raise ValueError("lps must be [%d][%d]" % (Fn, D))
    if mean is not None:
        v = v / np.asarray(inv, F32) + np.asarray(mean, F32)
    # magnitude substitution: exp in double rounded to float, floor below -50, phase 0 where |X| = 0
    ph = np.where(v < F32(-50.0), F32(np.exp(-50.0)), np.exp(v.astype(np.float64)).astype(F32)).astype(F32)
    mag = np.sqrt(ph)
    A = np.sqrt(xr * xr + xi * xi)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = mag / np.where(A > 0, A, F32(1.0))
    yr = np.where(A > 0, xr * g, mag).astype(F32)
    yi = np.where(A > 0, xi * g, F32(0.0)).astype(F32)
    if mut == "nyquist_dropped":
        yr[:, M] = yi[:, M] = 0
    # inverse split, loaded conjugated and bit-reversed
    k = np.arange(M)
    ar, ai, cr, ci = yr[:, k], yi[:, k], yr[:, M - k], -yi[:, M - k]
    h = F32(0.5)
    er, ei, dr, di = (ar + cr) * h, (ai + ci) * h, (ar - cr) * h, (ai - ci) * h
    wx, wy = twiddle32(k, N)
    if mut == "split_W_not_conj":
        br, bi = wx * dr - wy * di, wx * di + wy * dr
    else:
        br, bi = wx * dr + wy * di, wx * di - wy * dr
    zr, zi = er - bi, ei + br
    re, im = np.empty((Fn, M), F32), np.empty((Fn, M), F32)
    p = bitrev(k, logM)
    re[:, p], im[:, p] = zr, -zi
    tw = twiddle32(np.arange(M // 2), M)
    if mut == "twiddle_10bit":
        tw = (round_bits(tw[0], 10), round_bits(tw[1], 10))
    fft32(re, im, M, tw, bf16_stage=1 if mut == "bf16_butterfly_stage" else None)
    scale = F32(1.0 / M)
    n = np.arange(L)
    odd = (n & 1) == 1
    sgn = F32(1.0) if mut == "no_final_conj" else F32(-1.0)
    raw = np.where(odd, (sgn * im[:, n >> 1]) * scale, re[:, n >> 1] * scale).astype(F32)
    win = window(L)
    wn = win[np.minimum(n + 1, L - 1)] if mut == "window_n_plus_1" else win
    blk = (raw * wn).astype(F32)
    # overlap-add in frame order, / sum w^2 formed in the same order
    n_out = Fn * S + L - S
    acc, cnt = np.zeros(n_out, F32), np.zeros(n_out, F32)
    w2 = (win * win).astype(F32)
    last = np.minimum(np.arange(n_out) // S, Fn - 1)           # the last frame that covers each sample (k_ola's hi)
    first = np.maximum(0, (np.arange(n_out) - L + 1 + S - 1) // S)
    for t in range(Fn):
        sl = slice(t * S, t * S + L)
        if mut == "block_one_sample_late" and t == Fn // 2:
            acc[t * S + 1:t * S + L] = acc[t * S + 1:t * S + L] + blk[t, :L - 1]
        else:
            acc[sl] = acc[sl] + blk[t]
        if mut == "ola_norm_missing_frame":                  # hi off by one in the normaliser where 2+ frames cover
            keep = (t < last[sl]) | (first[sl] == last[sl])
            cnt[sl] = np.where(keep, cnt[sl] + w2, cnt[sl])
        else:
            cnt[sl] = cnt[sl] + w2
    out_f = (acc / cnt).astype(F32)
    c = np.trunc(out_f)
    return np.clip(c, -32768, 32767).astype(np.int16), out_f


# ---------------------------------------------------------------------------------------------------------------------
# decode.m downstream of the analysis: edge-replicated context, normalisation, the network, de-normalisation
def context_index(F, ctx, mut=None):
    """[F][ctx] frame index of the edge-replicated context window; mut "shift" / "wrap" plant a slip"""
    half = (ctx - 1) // 2
    idx = np.arange(F)[:, None] + np.arange(-half, half + 1)[None, :]
    if mut == "shift":
        idx = idx + 1
    if mut == "wrap":
        return idx % F
    return np.clip(idx, 0, F - 1)


def decode64(lps, mean, inv, ctx, Ws, bs, slabs=1, nat=None):
    """float64 decode.m target LPS [F][D] from the engine's own fp32 analysis rows `lps` (exact input: the analysis is
    bounded on its own), and a per-element bound lps_eps on any correct fp32 evaluation of the same chain:
    * x = fl(fl(lps - mean) * inv): two roundings, |dx| <= (2 u + u^2) |x|, which enter the network as x_err;
    * the forward chain: bounds64.expect_forward_chain, propagated through the layers;
    * out = fl(fl(y / inv) + mean) of the network's y = z + dz: |dz| / |inv| propagated, one rounding of the quotient
      and one of the sum.
    nat: on a noise-aware net the utterance's fp32 noise row [D] (tests/nat_model.py fixes its every bit from the fp32
    normalised rows), which closes every input row: an exact input like `lps`, no error of its own.
    Returns (target LPS float64, lps_eps) -- the inputs of synthesis_bound."""
    import bounds64
    lps = np.asarray(lps, np.float64)
    mean, inv = np.asarray(mean, np.float64), np.asarray(inv, np.float64)
    F, D = lps.shape
    x = (lps - mean) * inv
    idx = context_index(F, ctx)
    a = x[idx].reshape(F, ctx * D)
    a_err = (2.0 * U + U * U) * np.abs(a)
    if nat is not None:
        a = np.concatenate([a, np.broadcast_to(np.asarray(nat, np.float64).reshape(1, D), (F, D))], axis=1)
        a_err = np.concatenate([a_err, np.zeros((F, D))], axis=1)
    ex = bounds64.expect_forward_chain(a, Ws, bs, slabs=slabs, x_err=a_err)
    z, Ez = ex.ref, ex.bound * bounds64.SECOND_ORDER
    ainv = np.abs(inv)
    q = z / inv
    Eq = Ez / ainv + U * (np.abs(q) + Ez / ainv)
    want = q + mean
    eps = Eq + U * (np.abs(want) + Eq)
    return want, eps * bounds64.SECOND_ORDER


def decode32(lps, mean, inv, ctx, Ws, bs, mut=None):
    """the same chain in float32 (numpy's float32 matmul, the engine's sigmoid formula); mut: "raw" (the network's
    output, not de-normalised: the input of synthesis32(mean=, inv=)), "denorm_order"
    (y * inv + mean), "shift" (context one frame late), "wrap" (edges wrap around instead of clamping)"""
    lps = np.asarray(lps, F32)
    mean, inv = np.asarray(mean, F32), np.asarray(inv, F32)
    F, D = lps.shape
    x = ((lps - mean) * inv).astype(F32)
    y = x[context_index(F, ctx, mut if mut in ("shift", "wrap") else None)].reshape(F, ctx * D)
    for i, (W, b) in enumerate(zip(Ws, bs)):
        z = (np.matmul(y, np.asarray(W, F32)).astype(F32) + np.asarray(b, F32)).astype(F32)
        if i < len(Ws) - 1:
            with np.errstate(over="ignore"):
                z = (F32(1) / (F32(1) + np.exp(-z))).astype(F32)
        y = z
    if mut == "raw":
        return y
    if mut == "denorm_order":
        return (y * inv + mean).astype(F32)
    return (y / inv + mean).astype(F32)


def score_floors64(pc, pd, first=None):
    """(mc, md): the 50 dB floors of the log-spectral distortion, 1e-5 of the largest clean power pc [F][D] and of the
    largest enhanced power pd [F][D] over the first `first` scored frames (None: over all of them, which is the
    report; a number: the slip of a reduction that stops early)"""
    pc, pd = np.asarray(pc, np.float64), np.asarray(pd, np.float64)
    return float(pc[:first].max()) * 1e-5, float(pd[:first].max()) * 1e-5


def quality64(clean, noisy, lps, fs_khz=16, floors_first=None):
    """(segmental SNR, log-spectral distortion) of LogSpec2Wav.c in float64, over min(frames of clean, of noisy).
    floors_first: score_floors64's `first`, a planted slip."""
    F = min(n_frames(len(clean), fs_khz), n_frames(len(noisy), fs_khz))
    L, S, _ = params(fs_khz)
    n = F * S + L - S
    clean, noisy = np.asarray(clean)[:n], np.asarray(noisy)[:n]
    lps = np.asarray(lps, np.float64)[:F]
    _, est = synthesis64(noisy, lps, fs_khz, return_frames=True)
    cf = frames(clean, fs_khz)
    with np.errstate(divide="ignore", invalid="ignore"):
        snr = 10.0 * np.log10((cf * cf).sum(axis=1) / ((est - cf) ** 2).sum(axis=1))
    snr = np.where(snr > 30.0, 30.0, np.where(snr < -20.0, -20.0, snr))
    Xc, _ = spectrum64(clean, fs_khz)
    pc = np.abs(Xc) ** 2
    pd = np.where(lps < -50.0, np.exp(-50.0), np.exp(lps))
    mc, md = score_floors64(pc, pd, floors_first)
    pc = np.maximum(pc, mc)
    pd = np.maximum(pd, md)
    lsd = np.sqrt(((10.0 * np.log10(pd / pc)) ** 2).mean(axis=1))
    return float(snr.mean()), float(lsd.mean())


# The two means of k_score_utt (score.hip.h) in float32, in the order DESIGN.md section 8 documents, with switchable
# planted slips as in the waves_* models below.
SCORE_WAVES = 16                 # SCORE_UTT_WAVES
SCORE_TREE_SLIPS = [
    "first_trip_only",           # only the frames t < 16 enter the partial sums (the frame loop never comes round again)
    "divide_by_padded_count",    # the mean divides by ceil(n / 16) * 16, the frames the 16 wavefronts step over
    "left_to_right",             # the 16 partials are added 0, 1, ..., 15, not by the halving tree
]


def score_tree_mean32(values, slip=None):
    """float32 mean of `values` as k_score_utt forms it: partial w of 16 adds values[w], values[w + 16], ... in that
    order from 0.0f; the partials combine as s[i] += s[i + h] for h = 8, 4, 2, 1; the result is s[0] / float(n)"""
    v = np.asarray(values, F32).ravel()
    n = v.size
    s = np.zeros(SCORE_WAVES, F32)
    for a in range(0, SCORE_WAVES if slip == "first_trip_only" else n, SCORE_WAVES):
        row = v[a:a + SCORE_WAVES]
        s[:row.size] = s[:row.size] + row
    if slip == "left_to_right":
        for i in range(1, SCORE_WAVES):
            s[0] = s[0] + s[i]
    else:
        h = SCORE_WAVES // 2
        while h > 0:
            s[:h] = s[:h] + s[h:2 * h]
            h >>= 1
    count = -(-n // SCORE_WAVES) * SCORE_WAVES if slip == "divide_by_padded_count" else n
    return F32(s[0] / F32(count))


def synth_speech(n, fs_khz, seed=0):
    """Speech-like int16 test signal: a few harmonics of a gliding pitch under an envelope, plus noise."""
    rng = np.random.default_rng(seed)
    fs = {8: 8000.0, 11: 11000.0, 16: 16000.0}[fs_khz]
    t = np.arange(n) / fs
    f0 = 110.0 + 30.0 * np.sin(2 * np.pi * 0.7 * t)
    ph = 2 * np.pi * np.cumsum(f0) / fs
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 2.3 * t)
    s = sum(np.sin(k * ph + rng.uniform(0, 2 * np.pi)) / k for k in range(1, 12)) * env * 4000.0
    s += rng.normal(0, 300.0, n)
    return np.clip(np.round(s), -32768, 32767).astype(np.int16)


def load_fixture(path):
    z = np.load(path)
    return {k: z[k] for k in z.files}


# ---------------------------------------------------------------------------------------------------------------------
# mlggd_enhance_waves: the index arithmetic of a packed batch of utterances.
#
# Twice.  waves_*_model builds every mapping utterance by utterance from what the mapping means (the frames an
# utterance owns, the rows its section of a chunk's stream holds, the frames that cover an output sample); no search.
# waves_*_kernel computes the same quantities the way the *_seg kernels and the engine's chunk loop do: binary
# searches over the offset tables (or the per-frame table), rs(u), the clamps.  `slip` plants one mistake in the
# kernel-way form; the tests show on the CPU that the inputs of each GPU test would see it, so nothing has to be
# planted in device code.
WAVES_DEFAULT_CAP = 200000   # MLGGD_MAXCACHEFRAME
WAVES_SLIPS = [
    "search_bias",            # mid = (lo + hi) >> 1 without the + 1 (a lane may then never end: reported as -1)
    "lt_for_le",              # table[mid] < x for <= in the searches
    "ctx_for_ctx_minus_1",    # rs(u) advances by ctx rows per utterance, not ctx - 1
    "ga_not_clamped",         # rs(u) formed from frame_off[u], not max(frame_off[u], a), while the first local frame
                              # stays (ga - fo); dropping the clamp from both at once cancels in t and shows nowhere
    "fu_wrong_utterance",     # F_u, the clamp of the context and of the covering frames, from the next utterance
    "hi_not_clamped",         # the covering frames of an output sample not clamped to F_u - 1
    "table_plus_1",           # the per-frame table filled one frame early: an utterance's last frame says u + 1
    "wave_off_not_rebased",   # wave_off[u] = offsets[u], though the uploaded buffer starts at offsets[0]
]


def waves_layout64(frames_per_utt, fs_khz, base=0):
    """(offsets, frame_off, out_off) of utterances of exactly these frame counts packed from sample `base`"""
    L, S, _ = params(fs_khz)
    f = np.asarray(frames_per_utt, np.int64)
    z = np.zeros(1, np.int64)
    return (base + np.concatenate([z, np.cumsum(f * S + L - S)]), np.concatenate([z, np.cumsum(f)]),
            np.concatenate([z, np.cumsum(f * S + L - S)]))


def waves_chunks(frame_off, cap):
    FT = int(frame_off[-1])
    cap = cap if cap > 0 else WAVES_DEFAULT_CAP
    return [(a, min(cap, FT - a)) for a in range(0, FT, cap)]


def waves_analysis_model(offsets, frame_off, fs_khz):
    """[FT]: the index into the caller's packed buffer of the first sample of every packed frame"""
    S = params(fs_khz)[1]
    return np.concatenate([offsets[u] + np.arange(frame_off[u + 1] - frame_off[u], dtype=np.int64) * S
                           for u in range(len(frame_off) - 1)])


def waves_stream_model(frame_off, ctx, cap):
    """per chunk: (src [rows], first [n]).  Utterance u owns frames [f0, f1); of the chunk [a, a + n) it holds
    [lo, hi), and its section of the chunk's stream is those frames with half a context on either side, clamped into
    the utterance; the sections follow one another in utterance order; first[i] is the row where the context window
    of frame a + i starts."""
    fo = [int(x) for x in frame_off]
    half = (ctx - 1) // 2
    chunks = waves_chunks(frame_off, cap)
    cap = chunks[0][1]                                                # the capacity, or every frame in one chunk
    src = [[] for _ in chunks]
    first = [np.full(n, -1, np.int64) for _, n in chunks]
    used = [0] * len(chunks)
    for u in range(len(fo) - 1):
        f0, f1 = fo[u], fo[u + 1]
        for c in range(f0 // cap, (f1 - 1) // cap + 1):
            a, n = chunks[c]
            lo, hi = max(f0, a), min(f1, a + n)
            src[c].append(f0 + np.clip(np.arange(lo - f0 - half, hi - f0 + half, dtype=np.int64), 0, f1 - f0 - 1))
            first[c][lo - a:hi - a] = used[c] + np.arange(hi - lo)
            used[c] += hi - lo + ctx - 1
    return [(np.concatenate(s), f) for s, f in zip(src, first)]


def waves_ola_model(frame_off, fs_khz):
    """(utt, lo, hi) [n_out]: the utterance of every packed output sample and the first and last packed frame whose
    block covers it; frame t of an F-frame utterance covers its samples [t S, t S + L)"""
    L, S, _ = params(fs_khz)
    utt, los, his = [], [], []
    for u in range(len(frame_off) - 1):
        f0, F = int(frame_off[u]), int(frame_off[u + 1] - frame_off[u])
        n = F * S + L - S
        lo, hi = np.full(n, F, np.int64), np.full(n, -1, np.int64)
        for t in range(F):
            lo[t * S:t * S + L] = np.minimum(lo[t * S:t * S + L], t)
            hi[t * S:t * S + L] = t
        utt.append(np.full(n, u, np.int64))
        los.append(f0 + lo)
        his.append(f0 + hi)
    return np.concatenate(utt), np.concatenate(los), np.concatenate(his)


def _waves_search(table, x, lo0, hi0, slip, key=None):
    """the kernels' search, every lane at once: the largest m in [lo0, hi0] with key(m) <= x (key(m) = table[m] when
    not given).  A lane that has not ended after 64 rounds never would: -1."""
    lo, hi = np.full(x.shape, lo0, np.int64), np.full(x.shape, hi0, np.int64)
    for _ in range(64):
        act = lo < hi
        if not act.any():
            return lo
        mid = (lo + hi + (0 if slip == "search_bias" else 1)) >> 1
        k = table[mid] if key is None else key(mid)
        ok = (k < x) if slip == "lt_for_le" else (k <= x)
        lo, hi = np.where(act & ok, mid, lo), np.where(act & ~ok, mid - 1, hi)
    return np.where(lo < hi, -1, lo)


def waves_table(frame_off, slip=None):
    """the per-frame table of MLGGD_WAVES_LOOKUP=table"""
    n_utts = len(frame_off) - 1
    t = np.zeros(int(frame_off[-1]), np.int64)
    for u in range(n_utts):
        shift = 1 if slip == "table_plus_1" and u > 0 else 0
        t[frame_off[u] - shift:frame_off[u + 1]] = u
    return t


def _waves_seg_of_frame(frame_off, g, table, slip):
    if table is not None:
        return table[g]
    return _waves_search(frame_off, g, 0, len(frame_off) - 2, slip)


def _waves_other(u, n_utts):
    """the utterance the slip fu_wrong_utterance reads F_u from"""
    return np.where(u + 1 < n_utts, u + 1, np.maximum(u - 1, 0))


def waves_analysis_kernel(offsets, frame_off, fs_khz, lookup="search", slip=None):
    S = params(fs_khz)[1]
    offsets, frame_off = np.asarray(offsets, np.int64), np.asarray(frame_off, np.int64)
    table = waves_table(frame_off, slip) if lookup == "table" else None
    g = np.arange(int(frame_off[-1]), dtype=np.int64)
    u = _waves_seg_of_frame(frame_off, g, table, slip)
    wave_off = offsets - (0 if slip == "wave_off_not_rebased" else offsets[0])
    start = offsets[0] + wave_off[u] + (g - frame_off[u]) * S        # the uploaded buffer starts at offsets[0]
    return np.where(u < 0, -1, start)


def waves_stream_kernel(frame_off, ctx, cap, lookup="search", slip=None):
    """per chunk (src [rows], first [n]) as the engine's chunk loop and k_lps_stream_seg form them"""
    fo = np.asarray(frame_off, np.int64)
    n_utts, half = len(fo) - 1, (ctx - 1) // 2
    table = waves_table(fo, slip) if lookup == "table" else None
    c1 = ctx if slip == "ctx_for_ctx_minus_1" else ctx - 1
    out, u0 = [], 0
    for a, n in waves_chunks(fo, cap):
        while fo[u0 + 1] <= a:
            u0 += 1
        u1 = u0
        while fo[u1 + 1] < a + n:
            u1 += 1
        rows = n + (u1 - u0 + 1) * (ctx - 1)
        seg = _waves_seg_of_frame(fo, a + np.arange(n, dtype=np.int64), table, slip)
        first = np.where(seg < 0, -1, np.arange(n) + (seg - u0) * (ctx - 1))
        r = np.arange(rows, dtype=np.int64)
        clamp = (lambda f: f) if slip == "ga_not_clamped" else (lambda f: np.maximum(f, a))
        u = _waves_search(None, r, u0, u1, slip, key=lambda m: clamp(fo[m]) - a + (m - u0) * c1)
        uu = np.maximum(u, 0)
        f0 = fo[uu]
        w = _waves_other(uu, n_utts) if slip == "fu_wrong_utterance" else uu
        Fu = fo[w + 1] - fo[w]
        ga = np.maximum(f0, a)
        t = (ga - f0) - half + (r - (clamp(f0) - a + (uu - u0) * c1))
        t = np.where(t < 0, 0, np.where(t >= Fu, Fu - 1, t))
        out.append((np.where(u < 0, -1, f0 + t), first))
    return out


def waves_ola_kernel(frame_off, fs_khz, slip=None):
    """(utt, lo, hi) [n_out] as k_ola_seg forms them"""
    L, S, _ = params(fs_khz)
    fo = np.asarray(frame_off, np.int64)
    n_utts = len(fo) - 1
    out_off = np.concatenate([np.zeros(1, np.int64), np.cumsum(np.diff(fo) * S + L - S)])
    gi = np.arange(int(out_off[-1]), dtype=np.int64)
    u = _waves_search(out_off, gi, 0, n_utts - 1, slip)
    uu = np.maximum(u, 0)
    w = _waves_other(uu, n_utts) if slip == "fu_wrong_utterance" else uu
    f0, F = fo[uu], fo[w + 1] - fo[w]
    i = gi - out_off[uu]
    lo = i - L + 1
    lo = np.where(lo <= 0, 0, (lo + S - 1) // S)
    hi = i // S
    if slip != "hi_not_clamped":
        hi = np.where(hi > F - 1, F - 1, hi)
    bad = u < 0
    return np.where(bad, -1, uu), np.where(bad, -1, f0 + lo), np.where(bad, -1, f0 + hi)


def waves_index_model(frames_per_utt, fs_khz, ctx, cap, base=0):
    """every mapped index of one configuration, built per utterance: a flat list of arrays"""
    offsets, frame_off, _ = waves_layout64(frames_per_utt, fs_khz, base)
    res = [waves_analysis_model(offsets, frame_off, fs_khz)]
    for src, first in waves_stream_model(frame_off, ctx, cap):
        res += [src, first]
    return res + list(waves_ola_model(frame_off, fs_khz))


def waves_index_kernel(frames_per_utt, fs_khz, ctx, cap, base=0, lookup="search", slip=None):
    """the same list the kernels' way, with one planted slip"""
    offsets, frame_off, _ = waves_layout64(frames_per_utt, fs_khz, base)
    res = [waves_analysis_kernel(offsets, frame_off, fs_khz, lookup, slip)]
    for src, first in waves_stream_kernel(frame_off, ctx, cap, lookup, slip):
        res += [src, first]
    return res + list(waves_ola_kernel(frame_off, fs_khz, slip))


def waves_same_index(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def waves_rows_per_chunk(frame_off, ctx, cap):
    """[(n, rows, utterances touched)] of every chunk, from the per-utterance model"""
    fo = np.asarray(frame_off, np.int64)
    res = []
    for (a, n), (src, _) in zip(waves_chunks(fo, cap), waves_stream_model(fo, ctx, cap)):
        touched = int(np.count_nonzero((fo[:-1] < a + n) & (fo[1:] > a)))
        res.append((n, len(src), touched))
    return res


def waves_many_frames(n_utts, seed, n_long=6):
    """frame counts of the many-utterance batches: 1 to 4 frames (short ones the likelier), and n_long utterances of
    200 to 400 frames spread through the batch, never first or last"""
    rng = np.random.default_rng(seed)
    f = rng.choice([1, 2, 3, 4], n_utts, p=[0.4, 0.3, 0.2, 0.1])
    at = np.linspace(n_utts // 9, n_utts - n_utts // 7, n_long).astype(int)
    f[at] = rng.integers(200, 401, n_long)
    return [int(x) for x in f], [int(x) for x in at]


# The batches of tests/test_gpu_enhance_waves.py: name -> fs_khz, ctx, frames per utterance, chunk capacities (0 = the
# default), lookups, wave bases, the test that runs it and the planted slips its inputs are claimed to discriminate
# (tests/test_enhance_waves_model.py holds each claim to the models above).
def waves_gpu_configs():
    many_odd, _ = waves_many_frames(2187, 1)
    many_even, _ = waves_many_frames(2048, 2)
    cap1 = ["search_bias", "lt_for_le", "fu_wrong_utterance", "hi_not_clamped", "table_plus_1"]   # one utterance a chunk
    every_search = ["search_bias", "lt_for_le", "ctx_for_ctx_minus_1", "fu_wrong_utterance", "hi_not_clamped"]
    return {
        "table_mixed": dict(fs=16, ctx=7, frames=[1, 2, 3, 5, 17, 300], caps=[0], lookups=["table"], bases=[0],
                            test="test_table_lookup_equals_the_search_and_the_single_call",
                            slips=["table_plus_1", "ctx_for_ctx_minus_1", "fu_wrong_utterance", "hi_not_clamped"]),
        "table_chunks": dict(fs=16, ctx=7, frames=[10, 20, 5, 30, 1, 14], caps=[1, 7, 33, 1000], lookups=["table"],
                             bases=[0], test="test_table_lookup_equals_the_search_and_the_single_call",
                             slips=["table_plus_1", "ga_not_clamped", "ctx_for_ctx_minus_1", "fu_wrong_utterance",
                                    "hi_not_clamped"]),
        "many_odd": dict(fs=8, ctx=11, frames=many_odd, caps=[0, 257, 1000], lookups=["search", "table"], bases=[0],
                         test="test_thousands_of_utterances", slips=every_search + ["ga_not_clamped", "table_plus_1"]),
        "many_even": dict(fs=8, ctx=11, frames=many_even, caps=[0, 257, 1000], lookups=["search", "table"], bases=[0],
                          test="test_thousands_of_utterances", slips=every_search + ["ga_not_clamped", "table_plus_1"]),
        "many_odd_cap1": dict(fs=8, ctx=11, frames=many_odd[:301], caps=[1], lookups=["search", "table"], bases=[0],
                              test="test_thousands_of_utterances", slips=cap1),
        "many_even_cap1": dict(fs=8, ctx=11, frames=many_even[:300], caps=[1], lookups=["search", "table"], bases=[0],
                               test="test_thousands_of_utterances", slips=cap1),
        "wave_base": dict(fs=16, ctx=7, frames=[3, 1, 9, 2, 40], caps=[0], lookups=["search"], bases=[1, 1000, 12345],
                          test="test_a_wave_base_other_than_zero", slips=["wave_off_not_rebased"]),
        "degenerate": dict(fs=16, ctx=7, frames=[12, 9, 20, 1, 15, 30, 8], caps=[0, 16], lookups=["search"],
                           bases=[0], test="test_degenerate_utterances_as_subjects",
                           slips=["hi_not_clamped", "fu_wrong_utterance", "ga_not_clamped"]),
    }
