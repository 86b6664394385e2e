"""GPU: multi-objective nets -- ratio-mask targets from waves and the mask post-filter of the decoders (csrc/mask_rule.h,
k_lps_norm_pair_mask, k_mask_targets, k_lps_synthesis_mask / _mask_gv).

Targets: pkg.mask_targets equals s min(1, pyoracle.exp_det(0.5 (c - y))) bit for bit and stays within the derived bound
of tests/mask64.py of the float64 value.  Training: train_waves and load_waves + resident training on a mask engine
leave the weights of train_frames on rows [normalised clean LPS | pkg.mask_targets] assembled on the host.  Decoding is
pinned from the public pieces as tests/test_gpu_gv_decode.py pins it: wave_to_lps, the normalised edge-replicated
stream, forward_frames (2 D outputs), gv_rule's de-normalisation in NumPy float32, pkg.mask_select (itself equal to the
NumPy model), lps_to_wave -- every bit of the rows, the int16 and the float32 wave.

Shapes: 8 kHz (D = 129, odd), context 3, net 387-32-258, bunches of 16, one case at 16 kHz (771-32-514).  Decoded
utterances of 1, 2, 9 and 40 frames (one frame exactly; 1, 2 and 9 are no multiple of SPEC_FRAMES = 4) through a chunk
capacity of 16 frames, so that the 52 packed frames take four chunks whose boundaries fall inside utterances: a
post-filter that indexed the noisy rows by the chunk-local frame would read the wrong utterance.  An utterance shorter
than a frame cannot be decoded (the decoders refuse it as they always did); it is part of the training batch, where
it contributes no frame.  The compositions are computed once per case and shared."""
import os
import struct
import subprocess

import numpy as np
import pytest

import gv64
import hostlib
import mask64
import nat_model
import spec64

pytestmark = pytest.mark.gpu
CTX, B, HID, CAP = 3, 16, 32, 16
FRAMES = [1, 2, 9, 40]
LO, HI = 0.25, 0.75


def frames_wave(F, fs, seed, extra=5):
    L, S, _ = spec64.params(fs)
    return spec64.synth_speech(F * S + L - S + extra, fs, seed=seed)


def same(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


def state(eng):
    ws, bs = eng.returnWeights()
    return ws + bs + [eng.scalefactor()]


def same_bits(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), "tensor %d" % i


class Decode:
    """a mask net whose mask-half biases span [-0.2, 1.2] s, a few mask units cut off from the hidden layer with biases
    of exactly lo s and hi s (s a power of two: the products are exact), and its compositions"""

    def __init__(self, pkg, fs, s=0.5):
        self.pkg, self.fs, self.s = pkg, fs, np.float32(s)
        D = self.D = spec64.params(fs)[2] // 2 + 1
        rng = np.random.default_rng(200 + fs)
        self.ls = [CTX * D, HID, 2 * D]
        self.ws = [rng.normal(0, 0.05, (self.ls[i], self.ls[i + 1])).astype(np.float32) for i in range(2)]
        self.bs = [rng.normal(0, 0.1, self.ls[i + 1]).astype(np.float32) for i in range(2)]
        self.ws[1][:, D:] *= self.s
        self.bs[1][D:] = (np.linspace(-0.2, 1.2, D) * s).astype(np.float32)
        self.at_lo, self.at_hi = [5, 6, 70], [9, 64, 128]
        self.ws[1][:, [D + k for k in self.at_lo + self.at_hi]] = 0.0
        self.bs[1][[D + k for k in self.at_lo]] = np.float32(LO) * self.s
        self.bs[1][[D + k for k in self.at_hi]] = np.float32(HI) * self.s
        self.mean = rng.normal(10, 2, D).astype(np.float32)
        self.inv = (1.0 / rng.uniform(2, 4, D)).astype(np.float32)
        self.eta = gv64.draw_eta(2 * D, 9 + fs)                     # one factor per output; the decoders read the first D
        self.waves = [frames_wave(F, fs, seed=30 + i, extra=3 * i) for i, F in enumerate(FRAMES)]
        assert pkg.enhance_waves_layout([w.size for w in self.waves], fs)[0].tolist() == FRAMES
        assert sum(FRAMES) > 2 * CAP and any(F % 4 for F in FRAMES) and 1 in FRAMES
        eng = self.engine(cap=0)                                    # forward_frames takes an utterance in one chunk
        self.sel = [self.compose(eng, w, "select", None) for w in self.waves]
        self.off = [self.compose(eng, w, "off", None) for w in self.waves]
        self.sel_gv = [self.compose(eng, w, "select", self.eta) for w in self.waves]
        eng.close()

    def engine(self, cap=CAP, **kw):
        e = self.pkg.BPGpu(1, 0, self.ls, B, 0.1, 0.9, 1e-5, self.ws, self.bs, 2.0, 0, max_cache_frames=cap,
                           mask_bins=self.D, **kw)
        e.set_mask("select", LO, HI, float(self.s))
        return e

    def outputs(self, eng, w):
        lps = self.pkg.wave_to_lps(w, fs_khz=self.fs)
        F, half = lps.shape[0], (CTX - 1) // 2
        x = ((lps - self.mean) * self.inv).astype(np.float32)
        stream = x[np.clip(np.arange(F + 2 * half) - half, 0, F - 1)]
        return lps, eng.forward_frames(stream, np.arange(F, dtype=np.int32), CTX)

    def compose(self, eng, w, mode, eta):
        """(int16 wave, float32 wave, rows v, branch of every bin, m) of one utterance from the public pieces"""
        D = self.D
        lps, y = self.outputs(eng, w)
        assert y.shape == (lps.shape[0], 2 * D)
        x = gv64.apply32(y[:, :D], None if eta is None else eta[:D], self.inv, self.mean)
        br, m = mask64.branches(y[:, D:], self.s, LO, HI)
        v = x
        if mode == "select":
            v = self.pkg.mask_select(lps, x, m, LO, HI)
            same(v, mask64.select32(lps, x, y[:, D:], self.s, LO, HI), "mask_select against the model")
        out, outf = self.pkg.lps_to_wave(w, v, fs_khz=self.fs, return_float=True)
        return out, outf, v, br, m

    def decode(self, eng, **kw):
        return eng.enhance_waves(self.waves, self.mean, self.inv, fs_khz=self.fs, fea_context=CTX, return_f32=True,
                                 return_lps=True, **kw)

    def check(self, got, want):
        for u in range(len(FRAMES)):
            same(got[2][u], want[u][2], "rows of utterance %d" % u)
            same(got[1][u], want[u][1], "float wave %d" % u), same(got[0][u], want[u][0], "wave %d" % u)


@pytest.fixture(scope="module")
def dec8(pkg):
    return Decode(pkg, 8)


@pytest.fixture(scope="module")
def dec16(pkg):
    return Decode(pkg, 16)


# ---- 5: targets -----------------------------------------------------------------------------------------------

def test_mask_targets_equal_the_model_and_stay_within_the_derived_bound(pkg, pyoracle):
    c, y, _ = mask64.target_table()
    D = 129
    assert 4 * D < c.size < 5 * D
    c, y = np.resize(c, (5, D)), np.resize(y, (5, D))             # the whole table, its head repeated to fill the last row
    fin = np.isfinite(c) & np.isfinite(y)
    assert (c[fin] > y[fin]).sum() > 50 and (c == y).sum() >= 10 and (c == -50).sum() >= 20 and (~fin).sum() >= 6
    for s in (1.0, 0.5, 3.0):
        got = pkg.mask_targets(y, c, scale=s)
        want = mask64.target32(c, y, s, pyoracle.exp_det)
        # IEEE 754 leaves the sign and payload of a NaN RESULT open (3 - NaN comes back with the sign bit set from the
        # device's subtraction and clear from the host's): a NaN must be a NaN in the same place, every other bit equal
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and nan.sum() >= 5
        same(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want), "scale %g" % s)
        ref, bound = mask64.target64(c, y, s), mask64.target_bound(c, y, s)
        err = np.abs(got.astype(np.float64) - ref)
        print("scale %g: max error %.3g, max error / bound %.3g" % (s, err[fin].max(), (err[fin] / bound[fin]).max()))
        assert (err[fin] <= bound[fin]).all()
        assert bound[fin].max() < 7e-7 * s                                 # a few ulps of s: the bound is worth something
        assert np.isnan(got[np.isnan(c) | np.isnan(y)]).all()
        assert (got[fin & (c >= y)] == np.float32(s)).all()                # the cap, and c == y
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(pkg.MlggdError, match="error 1: scale"):
            pkg.mask_targets(y, c, scale=bad)
    assert pkg.mask_targets(np.zeros((0, 7)), np.zeros((0, 7))).shape == (0, 7)


# ---- 6: training from waves -----------------------------------------------------------------------------------

TRAIN_FRAMES = [3, 40, 1, 5, 12, 2, 7, 33, 9, 6, 17, 4]


class Train:
    def __init__(self, pkg, synth, fs, nat=0):
        self.pkg, self.fs, self.nat = pkg, fs, nat
        L, S, N = spec64.params(fs)
        D = self.D = N // 2 + 1
        rng = np.random.default_rng(11 * fs + nat)
        self.cleans = [spec64.synth_speech(F * S + L - S + i, fs, seed=5 * fs + i) for i, F in enumerate(TRAIN_FRAMES)]
        self.cleans.insert(3, spec64.synth_speech(L - 1, fs, seed=1))            # shorter than one frame
        self.cleans[6] = np.zeros_like(self.cleans[6])                           # digital silence: floor-valued clean rows
        n = len(self.cleans)
        self.noise = rng.integers(-2500, 2501, 9000).astype(np.int16)
        self.snr = [(-5.0, 0.0, 5.0, 10.0, 20.0)[u % 5] for u in range(n)]
        self.seg = [(int(rng.integers(0, 4000)), int(rng.integers(1, 5000))) for _ in range(n)]
        self.start = [int(rng.integers(0, s[1])) for s in self.seg]
        self.noisys = pkg.mix_waves(self.cleans, self.noise, self.snr, self.start, noise_seg=self.seg)
        rows = lambda ws: np.concatenate([pkg.wave_to_lps(w, fs_khz=fs) for w in ws if w.size >= L])
        self.rowsN, self.rowsC = rows(self.noisys), rows(self.cleans)
        assert (self.rowsC == -50).any()
        self.mean = self.rowsN.mean(0).astype(np.float32)
        self.inv = (1.0 / self.rowsN.std(0)).astype(np.float32)
        self.feat = (self.rowsN - self.mean) * self.inv
        self.lps_targ = (self.rowsC - self.mean) * self.inv
        table = pkg.wave_samples([w.size for w in self.cleans], CTX, fs)
        self.first = table[np.random.default_rng(5).permutation(table.size)]
        self.n = self.first.size
        assert self.n % B != 0 and self.n // B >= 3
        self.ls = [(CTX + (1 if nat else 0)) * D, HID, 2 * D]
        self.ws, self.bs = synth.make_weights(self.ls, seed=13)
        self.toff = CTX // 2
        self.betas = np.concatenate([np.full(D, 1.2), np.full(D, 2.0)]).astype(np.float32)   # the mask half: beta = 2

    def targ(self, s):
        return np.concatenate([self.lps_targ, self.pkg.mask_targets(self.rowsN, self.rowsC, scale=s)], axis=1)

    def engine(self, ml, s, cap=0):
        e = self.pkg.BPGpu(1, 0, self.ls, B, 0.01, 0.9, 1e-5, self.ws, self.bs, 1.2, ml, max_cache_frames=cap,
                           mask_bins=self.D, nat_frames=self.nat)
        e.set_mask(scale=s)
        if ml:
            e.set_shapefactors(self.betas)
        return e

    def reference(self, ml, s):
        """(weights after train_frames on the host rows, cv host order, cv device order)"""
        ref = self.engine(ml, s)
        t = self.targ(s)
        if self.nat:
            frame_off = np.concatenate([[0], np.cumsum([max(0, F) for F in self.frames()])])
            z = nat_model.noise_rows(self.feat, frame_off, self.nat)
            row = np.searchsorted(frame_off, self.first, side="right") - 1
            assert ref.train_frames_nat(self.feat, t, self.first, CTX, self.toff, z, row.astype(np.int32)) == self.n // B
            st = state(ref)
            ref.close()
            return st, None, None
        assert ref.train_frames(self.feat, t, self.first, CTX, self.toff) == self.n // B
        st = state(ref)
        cv = ref.cv_all_frames(self.feat, t, self.first, CTX, self.toff)
        ref.set_cv_device_reduce(True)
        cv_dev = ref.cv_all_frames(self.feat, t, self.first, CTX, self.toff)
        ref.close()
        return st, cv, cv_dev

    def frames(self):
        L, S, _ = spec64.params(self.fs)
        return [(w.size - (L - S)) // S for w in self.cleans if w.size >= L]

    def pair(self):
        return (self.noisys, self.cleans, self.mean, self.inv, self.first, self.toff, CTX, self.fs)


@pytest.fixture(scope="module")
def train8(pkg, synth):
    return Train(pkg, synth, 8)


@pytest.mark.parametrize("ml,s", [(0, 1.0), (0, 0.5), (1, 1.0), (1, 0.5)])
def test_training_from_waves_equals_train_frames_on_host_rows(train8, ml, s):
    t = train8
    want, cv, cv_dev = t.reference(ml, s)
    assert all(np.isfinite(a).all() for a in want) and any(not np.array_equal(a, b) for a, b in zip(want, t.ws))
    eng = t.engine(ml, s)
    eng.load_waves(*t.pair())
    assert eng.train_resident(0, t.n) == t.n // B
    eng.sync()
    same_bits(state(eng), want)
    eng.close()
    eng = t.engine(ml, s, cap=t.n + 1)
    eng.set_noise(t.noise)
    assert eng.train_waves(t.cleans, t.snr, t.start, t.mean, t.inv, t.first, t.toff, noise_seg=t.seg, fea_context=CTX,
                           fs_khz=t.fs) == t.n // B
    same_bits(state(eng), want)
    got = eng.cv_all_waves(*t.pair())                                   # on the trained weights, as the reference's
    print("cv (host order)", got, cv)
    assert np.array(got, np.float32).tobytes() == np.array(cv, np.float32).tobytes()
    eng.set_cv_device_reduce(True)
    got = eng.cv_all_waves(*t.pair())
    assert np.array(got, np.float32).tobytes() == np.array(cv_dev, np.float32).tobytes()
    eng.close()


def test_the_scale_reaches_the_targets(train8):
    a, b = train8.reference(0, 1.0)[0], train8.reference(0, 0.5)[0]
    assert any(x.tobytes() != y.tobytes() for x, y in zip(a, b))


def test_training_from_waves_on_a_noise_aware_mask_engine(pkg, synth):
    t = Train(pkg, synth, 8, nat=4)
    want = t.reference(0, 1.0)[0]
    eng = t.engine(0, 1.0)
    eng.set_noise(t.noise)
    assert eng.train_waves(t.cleans, t.snr, t.start, t.mean, t.inv, t.first, t.toff, noise_seg=t.seg, fea_context=CTX,
                           fs_khz=t.fs) == t.n // B
    same_bits(state(eng), want)
    eng.close()


def test_training_from_waves_at_16_khz(pkg, synth):
    t = Train(pkg, synth, 16)
    want = t.reference(1, 0.5)[0]
    eng = t.engine(1, 0.5)
    eng.load_waves(*t.pair())
    assert eng.train_resident(0, t.n) == t.n // B
    eng.sync()
    same_bits(state(eng), want)
    eng.close()


# ---- 7: decoding ----------------------------------------------------------------------------------------------

def branch_condition(c):
    """on the model's side: each branch takes at least 10 % of the bins and both equalities occur"""
    br = np.concatenate([r[3] for r in c.sel])
    m = np.concatenate([r[4] for r in c.sel])
    share = [float((br == k).mean()) for k in (0, 1, 2)]
    print("fs %d: estimate %.3f, mean %.3f, noisy %.3f of %d bins; m == lo %d, m == hi %d"
          % (c.fs, share[0], share[1], share[2], br.size, (m == np.float32(LO)).sum(), (m == np.float32(HI)).sum()))
    assert min(share) >= 0.10
    assert (m[:, c.at_lo] == np.float32(LO)).all() and (m[:, c.at_hi] == np.float32(HI)).all()
    assert (br[:, c.at_lo] == 1).all() and (br[:, c.at_hi] == 1).all()      # m == lo and m == hi both take the mean


def test_decoding_equals_the_composition_across_four_chunks(dec8):
    c = dec8
    branch_condition(c)
    eng = c.engine()
    assert eng.mask_bins == c.D and eng.mask() == (("select", LO, HI, float(c.s)))
    got = c.decode(eng)
    c.check(got, c.sel)
    for u, w in enumerate(c.waves):                                        # 8: the packed batch equals the single calls
        out, outf = eng.enhance_wave(w, c.mean, c.inv, fea_context=CTX, fs_khz=c.fs, return_float=True)
        same(outf, got[1][u], "enhance_wave %d" % u), same(out, got[0][u])
    assert all(a[2].tobytes() != b[2].tobytes() for a, b in zip(c.sel, c.off))
    eng.close()
    one = c.engine(cap=0)                                                  # one chunk: the same bits
    c.check(c.decode(one), c.sel)
    one.close()


def test_decoding_at_16_khz(dec16):
    c = dec16
    branch_condition(c)
    eng = c.engine()
    c.check(c.decode(eng), c.sel)
    eng.set_mask("off", LO, HI, float(c.s))
    c.check(c.decode(eng), c.off)
    eng.close()


def test_mode_off_decodes_the_lps_half_alone(dec8):
    c = dec8
    eng = c.engine()
    eng.set_mask("off", LO, HI, float(c.s))
    assert eng.mask().mode == "off"
    c.check(c.decode(eng), c.off)
    eng.set_mask("select", LO, HI, float(c.s))
    c.check(c.decode(eng), c.sel)
    eng.close()


def test_with_equalisation_factors_and_ones(dec8):
    c = dec8
    eng = c.engine()
    eng.set_gv(c.eta)
    c.check(c.decode(eng), c.sel_gv)
    assert all(a[2].tobytes() != b[2].tobytes() for a, b in zip(c.sel, c.sel_gv))
    eng.set_gv(np.ones(2 * c.D, np.float32))                               # ones: the bits of no vector
    c.check(c.decode(eng), c.sel)
    eng.set_gv(None)
    c.check(c.decode(eng), c.sel)
    eng.close()


def test_a_relu_mask_engine(dec8):
    c = dec8
    whole = c.engine(cap=0, activation="relu")
    want = [c.compose(whole, w, "select", None) for w in c.waves]
    whole.close()
    assert want[3][2].tobytes() != c.sel[3][2].tobytes()
    relu = c.engine(activation="relu")
    c.check(c.decode(relu), want)
    relu.close()


# ---- 8: scores ------------------------------------------------------------------------------------------------

def test_the_scores_are_those_of_the_post_filtered_rows(pkg, dec8):
    c = dec8
    cleans = [frames_wave(F, c.fs, seed=60 + k, extra=3 * k) for k, F in enumerate(FRAMES)]
    eng = c.engine()
    out, rows, segsnr, lsd, stoi = eng.enhance_waves(c.waves, c.mean, c.inv, fs_khz=c.fs, fea_context=CTX,
                                                     return_lps=True, cleans=cleans, stoi=True)
    for u in range(len(FRAMES)):
        same(out[u], c.sel[u][0]), same(rows[u], c.sel[u][2])
    want_snr, want_lsd = pkg.score_waves(cleans, c.waves, rows, fs_khz=c.fs)
    assert segsnr.tobytes() == want_snr.tobytes() and lsd.tobytes() == want_lsd.tobytes()
    want_stoi = pkg.stoi_waves(cleans, out, fs_khz=c.fs)
    assert np.array_equal(stoi, want_stoi, equal_nan=True)
    eng.set_mask("off", LO, HI, float(c.s))
    lsd_off = eng.enhance_waves(c.waves, c.mean, c.inv, fs_khz=c.fs, fea_context=CTX, cleans=cleans)[2]
    assert (lsd_off != lsd).all()                                          # the post-filter reaches the scores
    eng.close()


# ---- 9: refusals and neutrality -------------------------------------------------------------------------------

def test_refusals(pkg, dec8, dec16):
    c = dec8
    eng = c.engine()
    with pytest.raises(pkg.MlggdError, match=r"error 4: mlggd_live_open: .*mask_bins = 129 is not built"):
        eng.live(c.mean, c.inv, 2, fs_khz=8, fea_context=CTX)
    with pytest.raises(pkg.MlggdError, match=r"error 1: .*257 bins at 16 kHz"):   # D != mask_bins at this rate
        eng.enhance_wave(dec16.waves[2], dec16.mean, dec16.inv, fea_context=CTX, fs_khz=16)
    for bad in (("select", 0.75, 0.25, 1.0), ("select", float("nan"), 0.75, 1.0), ("select", 0.25, float("inf"), 1.0),
                ("select", 0.25, 0.75, 0.0), ("select", 0.25, 0.75, -2.0), ("off", 0.25, 0.75, float("nan"))):
        with pytest.raises(pkg.MlggdError, match="error 1: mask lo"):
            eng.set_mask(*bad)
    with pytest.raises(ValueError):
        eng.set_mask("both")
    assert pkg.load().mlggd_set_mask(eng._h, 7, 0.25, 0.75, 1.0) == 1
    assert eng.mask() == ("select", LO, HI, float(c.s))                   # unchanged by all of them
    c.check(c.decode(eng), c.sel)
    eng.close()
    plain = pkg.BPGpu(1, 0, [CTX * c.D, HID, c.D], B, 0.1, 0.9, 1e-5, [c.ws[0], c.ws[1][:, :c.D]],
                      [c.bs[0], c.bs[1][:c.D]], 2.0, 0)
    assert plain.mask_bins == 0
    with pytest.raises(pkg.MlggdError, match="error 4: mlggd_set_mask: the engine was created without mask_bins"):
        plain.set_mask()
    with pytest.raises(pkg.MlggdError, match="error 4: mlggd_get_mask"):
        plain.mask()
    plain.close()
    wide = pkg.BPGpu(1, 0, c.ls, B, 0.1, 0.9, 1e-5, c.ws, c.bs, 2.0, 0)   # 2 D wide without mask_bins: as before
    with pytest.raises(pkg.MlggdError, match="error 1: output dimension 258 != 129 bins"):
        wide.enhance_wave(c.waves[2], c.mean, c.inv, fea_context=CTX, fs_khz=8)
    wide.close()
    with pytest.raises(pkg.MlggdError, match="mask_bins 128"):
        pkg.BPGpu(1, 0, c.ls, B, 0.1, 0.9, 1e-5, c.ws, c.bs, 2.0, 0, mask_bins=128)


def test_a_plain_engine_is_unchanged_by_a_mask_engine_in_the_process(pkg, synth, dec8, train8):
    c, t = dec8, train8
    ls = [CTX * c.D, HID, c.D]
    ws, bs = [c.ws[0], np.ascontiguousarray(c.ws[1][:, :c.D])], [c.bs[0], np.ascontiguousarray(c.bs[1][:c.D])]

    def plain_run():
        e = pkg.BPGpu(1, 0, ls, B, 0.01, 0.9, 1e-5, ws, bs, 1.2, 1, max_cache_frames=CAP)
        dec = e.enhance_waves(c.waves, c.mean, c.inv, fs_khz=8, fea_context=CTX, return_f32=True, return_lps=True)
        e.close()
        e = pkg.BPGpu(1, 0, ls, B, 0.01, 0.9, 1e-5, ws, bs, 1.2, 1)
        e.set_noise(t.noise)
        e.train_waves(t.cleans, t.snr, t.start, t.mean, t.inv, t.first, t.toff, noise_seg=t.seg, fea_context=CTX, fs_khz=8)
        st = state(e)
        e.close()
        return dec, st

    dec0, st0 = plain_run()
    m = c.engine()
    c.check(c.decode(m), c.sel)
    m.close()
    m = c.engine(cap=0)                                                    # ... and one that trains the whole table
    m.set_noise(t.noise)
    m.train_waves(t.cleans, t.snr, t.start, t.mean, t.inv, t.first, t.toff, noise_seg=t.seg, fea_context=CTX, fs_khz=8)
    m.close()
    dec1, st1 = plain_run()
    same_bits(st1, st0)
    for k in range(3):
        same_bits(dec1[k], dec0[k])


# ---- 10: the tool ---------------------------------------------------------------------------------------------

def write_wav(path, w, rate):
    w = np.asarray(w, "<i2")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + 2 * w.size) + b"WAVEfmt " +
                struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16) + b"data" + struct.pack("<I", 2 * w.size) +
                w.tobytes())


def read_wav(path):
    d = open(path, "rb").read()
    assert d[:4] == b"RIFF" and d[8:16] == b"WAVEfmt " and d[36:40] == b"data"
    return np.frombuffer(d[44:], "<i2").astype(np.int16)


def test_enhance_wav_with_a_mask_net(pkg, dec8, tmp_path):
    c = dec8
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    wts, norm = str(tmp_path / "mask.wts"), str(tmp_path / "n.norm")
    hostlib.write_wts(wts, c.ws, c.bs)
    hostlib.write_norm(norm, c.mean, c.inv)
    mean, inv = (np.asarray(v, np.float32) for v in hostlib.HostNorm.read(norm, c.D))   # as the tool reads them
    ws, bs = hostlib.read_wts(wts, c.ls)
    waves = c.waves[1:]
    for i, w in enumerate(waves):
        write_wav(tmp_path / ("n%d.wav" % i), w, 8000)
    common = [os.path.join(hostlib.HOST, "enhance_wav"), "wts=" + wts, "norm_file=" + norm, "fea_context=%d" % CTX,
              "bunchsize=%d" % B]
    eng = pkg.BPGpu(1, 0, c.ls, B, 0.1, 0.9, 1e-5, ws, bs, 2.0, 0, mask_bins=c.D)
    eng.set_mask("select", LO, HI, float(c.s))
    sel = [eng.enhance_wave(w, mean, inv, fea_context=CTX, fs_khz=8) for w in waves]
    eng.set_mask("off", LO, HI, float(c.s))
    off = [eng.enhance_wave(w, mean, inv, fea_context=CTX, fs_khz=8) for w in waves]
    eng.close()
    assert all(a.tobytes() != b.tobytes() for a, b in zip(sel, off))

    def tool(tag, extra, single=False, rc=0):
        os.makedirs(tmp_path / tag)
        if single:
            args = ["in=%s" % (tmp_path / "n0.wav"), "out=%s" % (tmp_path / tag / "e0.wav")]
        else:
            with open(tmp_path / tag / "list.scp", "w") as f:
                for i in range(len(waves)):
                    f.write("%s %s\n" % (tmp_path / ("n%d.wav" % i), tmp_path / tag / ("e%d.wav" % i)))
            args = ["scp=%s" % (tmp_path / tag / "list.scp")]
        r = subprocess.run(common + args + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == rc, r.stdout + r.stderr
        if rc:
            assert not os.path.exists(tmp_path / tag / "e0.wav")
            return r.stderr
        return [read_wav(tmp_path / tag / ("e%d.wav" % i)) for i in range(1 if single else len(waves))]

    m = ["mask_lo=%g" % LO, "mask_hi=%g" % HI, "mask_scale=%g" % c.s]
    match = lambda got, want: all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    assert match(tool("single", ["mask=select"] + m, single=True), sel)
    assert match(tool("scp", ["mask=select"] + m), sel)
    assert match(tool("off", ["mask=off"] + m), off)
    assert "live= and mask= do not go together" in tool("live", ["mask=select", "live=200"] + m, rc=1)
    assert "layersizes[0] is not fea_context x the output dimension" in tool("nomask", [], single=True, rc=1)
    assert "mask=both: must be select or off" in tool("both", ["mask=both"], single=True, rc=1)
    assert "mlggd_set_mask" in tool("order", ["mask=select", "mask_lo=0.8", "mask_hi=0.2"], single=True, rc=1)
