"""The model of noise-aware training (csrc/nat_rule.h) the tests compare the library with: numpy float32 only.

An utterance u of F_u frames uses its first T_u = min(T, F_u); with x_t its NORMALISED rows its noise row is
z_u = (((x_0 + x_1) + x_2) + ... + x_{T_u-1}) / float32(T_u): an explicit loop of float32 additions from left to right,
then one float32 division (numpy's own reductions promise no order).  An utterance without frames has
a zero row.  The input row of a sample is its window of fea_context frames followed by its utterance's noise row."""
import numpy as np


def normalise(lps, mean, inv):
    """(lps - mean) * inv_std: two float32 operations, the stream's own"""
    x = (np.asarray(lps, np.float32) - np.asarray(mean, np.float32)) * np.asarray(inv, np.float32)
    assert x.dtype == np.float32
    return x


def noise_rows(rows, frame_off, T):
    """[n_utts][D] float32 from normalised rows [sum F][D]; utterance u is rows[frame_off[u]:frame_off[u+1]]"""
    rows = np.asarray(rows, np.float32)
    assert T >= 1 and rows.ndim == 2
    n = len(frame_off) - 1
    out = np.zeros((n, rows.shape[1]), np.float32)
    for u in range(n):
        lo, F = int(frame_off[u]), int(frame_off[u + 1]) - int(frame_off[u])
        Tu = min(T, F)
        if Tu < 1:
            continue
        s = rows[lo].copy()
        for t in range(1, Tu):
            s = s + rows[lo + t]                       # float32 + float32, one rounding per element
        out[u] = s / np.float32(Tu)
        assert out.dtype == np.float32 and s.dtype == np.float32
    return out


def utt_of_frames(frame_off, first_frame):
    """the utterance that holds each frame: the last u with frame_off[u] <= f, utterances without frames stepped over"""
    fo = np.asarray(frame_off, np.int64)
    out = np.zeros(len(first_frame), np.int32)
    for i, f in enumerate(first_frame):
        assert fo[0] <= f < fo[-1]
        u = [k for k in range(len(fo) - 1) if fo[k] <= f < fo[k + 1]]
        assert len(u) == 1
        out[i] = u[0]
    return out


def expand(feat, first_frame, ctx, nat, nat_row):
    """rows [n_samples][(ctx + 1) * D] float32: [window of ctx frames | nat[nat_row[i]]] -- copies, no arithmetic"""
    feat, nat = np.asarray(feat, np.float32), np.asarray(nat, np.float32)
    D = feat.shape[1]
    out = np.empty((len(first_frame), (ctx + 1) * D), np.float32)
    for i, (f, r) in enumerate(zip(first_frame, nat_row)):
        out[i, :ctx * D] = feat[f:f + ctx].reshape(-1)
        out[i, ctx * D:] = nat[r]
    return out


def edge_stream(x, ctx):
    """the decoder's stream of one utterance: (ctx - 1) / 2 copies of the first / last row on either side"""
    F, half = x.shape[0], (ctx - 1) // 2
    return x[np.clip(np.arange(F + 2 * half) - half, 0, F - 1)]
