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


def quality64(clean, noisy, lps, fs_khz=16):
    """(segmental SNR, log-spectral distortion) of LogSpec2Wav.c in float64, over min(frames of clean, of noisy)."""
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
    pc = np.maximum(pc, pc.max() * 1e-5)
    pd = np.maximum(pd, pd.max() * 1e-5)
    lsd = np.sqrt(((10.0 * np.log10(pd / pc)) ** 2).mean(axis=1))
    return float(snr.mean()), float(lsd.mean())


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
