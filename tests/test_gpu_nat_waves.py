"""GPU: noise-aware training from waves -- train_waves / load_waves / cv_all_waves on a NAT engine against
train_frames_nat / cv_all_frames_nat on rows built on the host: mix_waves, wave_to_lps per utterance, (lps - mean) *
inv_std in numpy float32 as two operations, and the noise rows of tests/nat_model.py.  Every bit of every weight and
bias, of scalefactor() and of the three CV sums; with a chunk capacity of exactly n_samples the same bits, with one
sample more an argument error that moves nothing."""
import numpy as np
import pytest

import nat_model
import spec64

pytestmark = pytest.mark.gpu
B, T = 32, 6
# frames per utterance: 2 < ctx = 3 (no sample, but a noise row), 4 and 5 < T, T, T + 1 and longer ones
FRAMES = [3, 40, 2, 5, 1, 12, T, T + 1, 4, 33, 9, 17, 25, 10, 14, 38]
CASES = {"8k_ml": (8, 3, 1), "8k_betanorm": (8, 3, 0)}


class Case:
    def __init__(self, pkg, synth, fs, ctx, ml):
        self.pkg, self.fs, self.ctx, self.ml = pkg, fs, ctx, ml
        L, S, N = spec64.params(fs)
        D = self.D = N // 2 + 1
        rng = np.random.default_rng(7 * fs + ctx)
        self.cleans = [spec64.synth_speech(F * S + L - S + i, fs, seed=3 * fs + i) for i, F in enumerate(FRAMES)]
        self.cleans.insert(4, spec64.synth_speech(L - 1, fs, seed=1))          # shorter than one frame: no row at all
        frames = FRAMES[:4] + [0] + FRAMES[4:]
        n = len(self.cleans)
        self.noise = rng.integers(-2500, 2501, 9000).astype(np.int16)
        self.snr = [(-5.0, 0.0, 5.0, 10.0, 20.0)[u % 5] for u in range(n)]
        self.seg = [(int(rng.integers(0, 4000)), int(rng.integers(1, 5000))) for _ in range(n)]
        self.start = [int(rng.integers(0, s[1])) for s in self.seg]
        self.noisys = pkg.mix_waves(self.cleans, self.noise, self.snr, self.start, noise_seg=self.seg)
        rowsN = np.concatenate([pkg.wave_to_lps(w, fs_khz=fs) for w in self.noisys])
        rowsC = np.concatenate([pkg.wave_to_lps(w, fs_khz=fs) for w in self.cleans])
        self.mean = rowsN.mean(0).astype(np.float32)
        self.inv = (1.0 / rowsN.std(0)).astype(np.float32)
        self.feat = nat_model.normalise(rowsN, self.mean, self.inv)
        self.targ = nat_model.normalise(rowsC, self.mean, self.inv)
        self.fo = np.concatenate([[0], np.cumsum(frames)]).astype(np.int32)
        assert self.fo[-1] == rowsN.shape[0]
        table = pkg.wave_samples([w.size for w in self.cleans], ctx, fs)
        self.first = table[np.random.default_rng(5).permutation(table.size)]
        self.n = self.first.size
        assert self.n % B != 0 and self.n // B >= 3
        self.nat = nat_model.noise_rows(self.feat, self.fo, T)                  # one row per utterance, zeros without frames
        self.nat_row = nat_model.utt_of_frames(self.fo, self.first)
        short = [u for u, F in enumerate(frames) if 0 < F < ctx]
        assert short and not set(short) & set(self.nat_row.tolist())            # fewer than ctx frames: no samples
        assert any(ctx <= frames[u] < T for u in set(self.nat_row.tolist()))    # fewer than T frames, with samples
        self.toff = ctx // 2
        self.ls = [(ctx + 1) * D, 64, D]
        self.ws, self.bs = synth.make_weights(self.ls, seed=11)
        ref = self.engine()
        assert ref.train_frames_nat(self.feat, self.targ, self.first, ctx, self.toff, self.nat, self.nat_row) == self.n // B
        self.ref = state(ref)
        args = (self.feat, self.targ, self.first, ctx, self.toff, self.nat, self.nat_row)
        self.ref_cv = ref.cv_all_frames_nat(*args)
        ref.set_cv_device_reduce(True)
        self.ref_cv_dev = ref.cv_all_frames_nat(*args)
        ref.close()
        assert all(np.isfinite(a).all() for a in self.ref) and any(
            not np.array_equal(a, b) for a, b in zip(self.ref, self.ws))

    def engine(self, cap=0, nat=T):
        return self.pkg.BPGpu(1, 0, self.ls, B, 0.01, 0.9, 1e-5, self.ws, self.bs, 0.9, self.ml, max_cache_frames=cap,
                              nat_frames=nat)


def state(eng):
    ws, bs = eng.returnWeights()
    return ws + bs + [eng.scalefactor()]


def same_bits(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), "tensor %d" % i


@pytest.fixture(scope="module", params=list(CASES))
def case(pkg, synth, request):
    return Case(pkg, synth, *CASES[request.param])


def test_train_waves_equals_train_frames_nat_on_host_rows(case):
    eng = case.engine()
    eng.set_noise(case.noise)
    trained, noisys, _, _ = eng.train_waves(case.cleans, case.snr, case.start, case.mean, case.inv, case.first, case.toff,
                                            noise_seg=case.seg, fea_context=case.ctx, fs_khz=case.fs, return_noisy=True)
    assert trained == case.n // B
    same_bits(noisys, case.noisys)
    same_bits(state(eng), case.ref)
    eng.set_weights(case.ws, case.bs)                     # fea_context from the shape: (ctx + 1) * D on a NAT engine
    assert eng.train_waves(case.cleans, case.snr, case.start, case.mean, case.inv, case.first, case.toff,
                           noise_seg=case.seg, fs_khz=case.fs) == case.n // B
    eng.close()


def test_load_waves_then_train_resident(case):
    eng = case.engine()
    eng.load_waves(case.noisys, case.cleans, case.mean, case.inv, case.first, case.toff, case.ctx, case.fs)
    assert eng.train_resident(0, case.n) == case.n // B
    eng.sync()
    same_bits(state(eng), case.ref)
    eng.close()


def test_cv_all_waves_equals_cv_all_frames_nat(case):
    """all three sums, formed on the host (the default) and on the device, after the same training"""
    eng = case.engine()
    eng.load_waves(case.noisys, case.cleans, case.mean, case.inv, case.first, case.toff, case.ctx, case.fs)
    eng.train_resident(0, case.n)
    eng.sync()
    args = (case.noisys, case.cleans, case.mean, case.inv, case.first, case.toff, case.ctx, case.fs)
    got = eng.cv_all_waves(*args)
    print("cv (host order)", got, case.ref_cv)
    assert np.array(got, np.float32).tobytes() == np.array(case.ref_cv, np.float32).tobytes()
    eng.set_cv_device_reduce(True)
    got = eng.cv_all_waves(*args)
    print("cv (device)", got, case.ref_cv_dev)
    assert np.array(got, np.float32).tobytes() == np.array(case.ref_cv_dev, np.float32).tobytes()
    eng.close()


def test_the_context_must_fill_layer_0_with_the_noise_row(case):
    pkg = case.pkg
    eng = case.engine()
    with pytest.raises(pkg.MlggdError, match=r"error 1: \(fea_context %d \+ 1\) x %d bins != layersizes\[0\]" %
                       (case.ctx + 1, case.D)):
        eng.load_waves(case.noisys, case.cleans, case.mean, case.inv, case.first, case.toff, case.ctx + 1, case.fs)
    eng.load_waves(case.noisys, case.cleans, case.mean, case.inv, case.first, case.toff, case.ctx, case.fs)
    assert eng.train_resident(0, case.n) == case.n // B
    eng.sync()
    same_bits(state(eng), case.ref)
    eng.close()


def test_the_chunk_capacity_admits_n_samples(case):
    """max_cache_frames == n_samples: train_waves, load_waves and cv_all_waves give the uncapped bits"""
    eng = case.engine(cap=case.n)
    eng.set_noise(case.noise)
    assert eng.train_waves(case.cleans, case.snr, case.start, case.mean, case.inv, case.first, case.toff,
                           noise_seg=case.seg, fea_context=case.ctx, fs_khz=case.fs) == case.n // B
    same_bits(state(eng), case.ref)
    eng.close()
    eng = case.engine(cap=case.n)
    args = (case.noisys, case.cleans, case.mean, case.inv, case.first, case.toff, case.ctx, case.fs)
    eng.load_waves(*args)
    assert eng.train_resident(0, case.n) == case.n // B
    eng.sync()
    same_bits(state(eng), case.ref)
    got = eng.cv_all_waves(*args)
    assert np.array(got, np.float32).tobytes() == np.array(case.ref_cv, np.float32).tobytes()
    eng.set_cv_device_reduce(True)
    got = eng.cv_all_waves(*args)
    assert np.array(got, np.float32).tobytes() == np.array(case.ref_cv_dev, np.float32).tobytes()
    eng.close()


def test_one_sample_beyond_the_chunk_capacity_is_refused(case):
    """max_cache_frames == n_samples - 1: an argument error from each of the three that moves nothing; the engine then
    trains the table without its last sample -- part of the trailing bunch that is skipped either way -- to the bits"""
    pkg = case.pkg
    eng = case.engine(cap=case.n - 1)
    eng.set_noise(case.noise)
    start = state(eng)
    pair = (case.noisys, case.cleans, case.mean, case.inv, case.first, case.toff, case.ctx, case.fs)
    refusal = r"error 1: n_frames %d exceeds the chunk capacity %d" % (case.n, case.n - 1)
    with pytest.raises(pkg.MlggdError, match=refusal):
        eng.train_waves(case.cleans, case.snr, case.start, case.mean, case.inv, case.first, case.toff,
                        noise_seg=case.seg, fea_context=case.ctx, fs_khz=case.fs)
    with pytest.raises(pkg.MlggdError, match=refusal):
        eng.load_waves(*pair)
    with pytest.raises(pkg.MlggdError, match=refusal):
        eng.cv_all_waves(*pair)
    same_bits(state(eng), start)
    assert case.n % B >= 1
    assert eng.train_waves(case.cleans, case.snr, case.start, case.mean, case.inv, case.first[:-1], case.toff,
                           noise_seg=case.seg, fea_context=case.ctx, fs_khz=case.fs) == case.n // B
    same_bits(state(eng), case.ref)
    eng.close()
