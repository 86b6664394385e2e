"""GPU: training from waves -- load_waves / cv_all_waves / set_noise + train_waves -- against train_frames / cv_all_frames
on rows built on the host (wave_to_lps per utterance, then (lps - mean) * inv_std in numpy float32 as two operations):
every bit of every weight and bias and of scalefactor(), whatever the chunk capacity and whatever ran on the engine
before; and the state and argument errors, after which the engine still gives those bits."""
import numpy as np
import pytest

import spec64

pytestmark = pytest.mark.gpu
B = 32
CASES = {"8k_ml": (8, 3, 1), "8k_betanorm": (8, 3, 0), "16k_ml": (16, 7, 1)}
FRAMES = [3, 40, 5, 1, 12, 2, 6, 7, 8, 33, 4, 9, 17, 3, 25, 10, 6, 14, 38, 5]


class Case:
    def __init__(self, pkg, synth, fs, ctx, ml):
        self.fs, self.ctx, self.ml = fs, ctx, ml
        L, S, N = spec64.params(fs)
        D = self.D = N // 2 + 1
        rng = np.random.default_rng(7 * fs + ctx)
        self.cleans = [spec64.synth_speech(F * S + L - S + i, fs, seed=3 * fs + i) for i, F in enumerate(FRAMES)]
        self.cleans.insert(4, spec64.synth_speech(L - 1, fs, seed=1))          # shorter than one frame
        n = len(self.cleans)
        self.noise = rng.integers(-2500, 2501, 9000).astype(np.int16)
        self.snr = [(-5.0, 0.0, 5.0, 10.0, 20.0)[u % 5] for u in range(n)]
        self.seg = [(int(rng.integers(0, 4000)), int(rng.integers(1, 5000))) for _ in range(n)]
        self.start = [int(rng.integers(0, s[1])) for s in self.seg]
        self.noisys, self.gain, self.clipped = pkg.mix_waves(self.cleans, self.noise, self.snr, self.start,
                                                              noise_seg=self.seg, return_info=True)
        rowsN = np.concatenate([pkg.wave_to_lps(w, fs_khz=fs) for w in self.noisys])
        rowsC = np.concatenate([pkg.wave_to_lps(w, fs_khz=fs) for w in self.cleans])
        self.mean = rowsN.mean(0).astype(np.float32)
        self.inv = (1.0 / rowsN.std(0)).astype(np.float32)
        self.feat = (rowsN - self.mean) * self.inv                              # float32: a subtraction, then a product
        self.targ = (rowsC - self.mean) * self.inv
        assert self.feat.dtype == np.float32 and self.targ.dtype == np.float32
        table = pkg.wave_samples([w.size for w in self.cleans], ctx, fs)
        self.first = table[np.random.default_rng(5).permutation(table.size)]
        self.n = self.first.size
        assert self.n % B != 0 and self.n // B >= 3                             # a trailing partial bunch is skipped
        assert sum(1 for F in FRAMES if F < ctx) >= 1 and table.size == sum(max(0, F - ctx + 1) for F in FRAMES)
        self.toff = ctx // 2
        self.ls = [ctx * D, 64, D]
        self.ws, self.bs = synth.make_weights(self.ls, seed=11)
        self.pkg = pkg
        ref = self.engine()
        assert ref.train_frames(self.feat, self.targ, self.first, ctx, self.toff) == self.n // B
        self.ref = state(ref)
        self.ref_cv = ref.cv_all_frames(self.feat, self.targ, self.first, ctx, self.toff)
        ref.set_cv_device_reduce(True)
        self.ref_cv_dev = ref.cv_all_frames(self.feat, self.targ, self.first, ctx, self.toff)
        ref.close()
        assert all(np.isfinite(a).all() for a in self.ref) and any(
            not np.array_equal(a, b) for a, b in zip(self.ref, self.ws))       # the steps moved the weights

    def engine(self, cap=0):
        return self.pkg.BPGpu(1, 0, self.ls, B, 0.01, 0.9, 1e-5, self.ws, self.bs, 0.9, self.ml, max_cache_frames=cap)

    def load_and_train(self, eng):
        eng.load_waves(self.noisys, self.cleans, self.mean, self.inv, self.first, self.toff, self.ctx, self.fs)
        trained = eng.train_resident(0, self.n)
        eng.sync()
        return trained

    def train_waves(self, eng, **kw):
        return eng.train_waves(self.cleans, self.snr, self.start, self.mean, self.inv, self.first, self.toff,
                               noise_seg=self.seg, fea_context=self.ctx, fs_khz=self.fs, **kw)


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


def test_load_waves_then_train_resident_equals_train_frames(case):
    """check 1"""
    eng = case.engine()
    assert case.load_and_train(eng) == case.n // B
    same_bits(state(eng), case.ref)
    eng.close()


def test_train_waves_equals_mix_waves_then_load_waves(case):
    """check 2: the noisy waves, gains and counts that come back are mix_waves' own"""
    eng = case.engine()
    eng.set_noise(case.noise)
    trained, noisys, gain, clipped = case.train_waves(eng, return_noisy=True)
    assert trained == case.n // B
    same_bits(state(eng), case.ref)
    same_bits(noisys, case.noisys)
    assert gain.tobytes() == case.gain.tobytes() and clipped.tobytes() == case.clipped.tobytes()
    eng.set_weights(case.ws, case.bs)                     # ... and without asking for them: a second epoch from the bank
    assert case.train_waves(eng) == case.n // B
    eng.close()


def test_cv_all_waves_equals_cv_all_frames(case):
    """check 3, with the sums formed on the host (the default) and on the device"""
    eng = case.engine()
    case.load_and_train(eng)
    args = (case.noisys, case.cleans, case.mean, case.inv, case.first, case.toff, case.ctx, case.fs)
    got = eng.cv_all_waves(*args)
    print("cv (host order)", got, case.ref_cv)
    assert np.array(got, np.float32).tobytes() == np.array(case.ref_cv, np.float32).tobytes()
    eng.set_cv_device_reduce(True)
    got = eng.cv_all_waves(*args)
    assert np.array(got, np.float32).tobytes() == np.array(case.ref_cv_dev, np.float32).tobytes()
    eng.close()


@pytest.mark.parametrize("cap", ["just above", 150000])
def test_the_chunk_capacity_changes_no_bit(case, cap):
    """check 4"""
    cap = case.n + 1 if cap == "just above" else cap
    eng = case.engine(cap)
    case.load_and_train(eng)
    same_bits(state(eng), case.ref)
    eng.close()
    eng = case.engine(cap)
    eng.set_noise(case.noise)
    case.train_waves(eng)
    same_bits(state(eng), case.ref)
    eng.close()


def test_train_waves_between_two_enhance_waves_calls(case):
    """checks 5 and 6: the decoder and the loader share workspaces and the raw buffer sets"""
    eng = case.engine()
    eng.set_noise(case.noise)
    dec = [w for w in case.noisys if w.size >= spec64.params(case.fs)[0]]
    first = eng.enhance_waves(dec, case.mean, case.inv, fs_khz=case.fs, fea_context=case.ctx, return_f32=True)
    case.train_waves(eng)
    same_bits(state(eng), case.ref)
    eng.set_weights(case.ws, case.bs)
    second = eng.enhance_waves(dec, case.mean, case.inv, fs_khz=case.fs, fea_context=case.ctx, return_f32=True)
    same_bits(second[0], first[0])
    same_bits(second[1], first[1])
    eng.close()


def test_interleaved_with_train_frames_async(case):
    """the loader takes the idle raw buffer set while the steps of an asynchronous chunk may still run on the other"""
    eng = case.engine()
    eng.train_frames(case.feat, case.targ, case.first, case.ctx, case.toff, wait=False)
    case.load_and_train(eng)
    twice = state(eng)
    eng.close()
    eng = case.engine()
    eng.train_frames(case.feat, case.targ, case.first, case.ctx, case.toff)
    eng.train_frames(case.feat, case.targ, case.first, case.ctx, case.toff)
    same_bits(twice, state(eng))
    eng.close()


def test_state_and_argument_errors_leave_the_engine_usable(case):
    pkg = case.pkg
    eng = case.engine()
    with pytest.raises(pkg.MlggdError, match="error 4: .*noise bank"):
        case.train_waves(eng)                                           # no set_noise yet
    eng.set_noise(case.noise)
    eng.set_noise(None)
    with pytest.raises(pkg.MlggdError, match="error 4: .*noise bank"):
        case.train_waves(eng)                                           # ... and after it was freed
    eng.set_noise(case.noise)
    # a window that starts on the last frame of the second utterance crosses into the third
    F = [max(0, (w.size - (spec64.params(case.fs)[0] - spec64.params(case.fs)[1])) // spec64.params(case.fs)[1])
         if w.size >= spec64.params(case.fs)[0] else 0 for w in case.cleans]
    bad = case.first.copy()
    bad[5] = F[0] + F[1] - 1
    with pytest.raises(pkg.MlggdError, match=r"error 1: sample 5: window .* crosses the end of utterance 1"):
        eng.train_waves(case.cleans, case.snr, case.start, case.mean, case.inv, bad, case.toff, noise_seg=case.seg,
                        fea_context=case.ctx, fs_khz=case.fs)
    bad[5] = sum(F) - case.ctx + 1
    with pytest.raises(pkg.MlggdError, match=r"error 1: sample 5: window .* outside the %d packed frames" % sum(F)):
        eng.load_waves(case.noisys, case.cleans, case.mean, case.inv, bad, case.toff, case.ctx, case.fs)
    with pytest.raises(pkg.MlggdError, match=r"error 1: targ_offset %d" % case.ctx):
        eng.load_waves(case.noisys, case.cleans, case.mean, case.inv, case.first, case.ctx, case.ctx, case.fs)
    with pytest.raises(pkg.MlggdError, match=r"error 1: utterance 2: snr_db nan"):
        eng.train_waves(case.cleans, [0.0, 0.0, float("nan")] + case.snr[3:], case.start, case.mean, case.inv, case.first,
                        case.toff, noise_seg=case.seg, fea_context=case.ctx, fs_khz=case.fs)
    small = case.engine(case.n - 1)
    with pytest.raises(pkg.MlggdError, match="error 1: .*exceeds the chunk capacity"):
        case.load_and_train(small)
    small.close()
    assert case.train_waves(eng) == case.n // B                        # after all of them: the bits of check 1
    same_bits(state(eng), case.ref)
    eng.close()


def test_an_emulated_world_is_a_state_error(case):
    """... after which the engine trains its frame chunks as a twin that never saw the call"""
    pkg = case.pkg
    eng, twin = case.engine(), case.engine()
    for e in (eng, twin):
        e.fake_world(2)
    eng.set_noise(case.noise)
    with pytest.raises(pkg.MlggdError, match="error 4: mlggd_train_waves runs on a single-device engine"):
        case.train_waves(eng)
    with pytest.raises(pkg.MlggdError, match="error 4: mlggd_load_waves runs on a single-device engine"):
        eng.load_waves(case.noisys, case.cleans, case.mean, case.inv, case.first, case.toff, case.ctx, case.fs)
    for e in (eng, twin):
        assert e.train_frames(case.feat, case.targ, case.first, case.ctx, case.toff) == case.n // (2 * B)
    same_bits(state(eng), state(twin))
    eng.close()
    twin.close()


def test_nothing_to_train(case):
    eng = case.engine()
    eng.set_noise(case.noise)
    none = np.zeros(0, np.int32)
    assert eng.train_waves(case.cleans, case.snr, case.start, case.mean, case.inv, none, case.toff, noise_seg=case.seg,
                           fea_context=case.ctx, fs_khz=case.fs) == 0
    assert eng.train_waves([], [], [], case.mean, case.inv, none, case.toff, noise_seg=[], fea_context=case.ctx,
                           fs_khz=case.fs) == 0
    same_bits(state(eng)[:-1], case.ws + case.bs)
    eng.close()


def test_the_chunk_capacity_admits_n_samples(case):
    """max_cache_frames == n_samples: train_waves, load_waves and cv_all_waves give the uncapped bits"""
    eng = case.engine(case.n)
    eng.set_noise(case.noise)
    assert case.train_waves(eng) == case.n // B
    same_bits(state(eng), case.ref)
    eng.close()
    eng = case.engine(case.n)
    assert case.load_and_train(eng) == case.n // B
    same_bits(state(eng), case.ref)
    args = (case.noisys, case.cleans, case.mean, case.inv, case.first, case.toff, case.ctx, case.fs)
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
    eng = case.engine(case.n - 1)
    eng.set_noise(case.noise)
    start = state(eng)
    pair = (case.noisys, case.cleans, case.mean, case.inv, case.first, case.toff, case.ctx, case.fs)
    refusal = r"error 1: n_frames %d exceeds the chunk capacity %d" % (case.n, case.n - 1)
    with pytest.raises(pkg.MlggdError, match=refusal):
        case.train_waves(eng)
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
