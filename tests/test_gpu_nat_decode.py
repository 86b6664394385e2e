"""GPU: decoding with a noise-aware net -- enhance_waves / enhance_wave / the scored call / the enhance_wav tool on a
NAT engine against the chain through the public pieces, per utterance: wave_to_lps, (lps - mean) * inv_std, edge
replication, the numpy noise row of tests/nat_model.py, forward on the expanded rows, y / inv_std + mean, lps_to_wave.
Bit for bit on the int16 wave, the float32 wave and the de-normalised rows, whatever the chunk capacity."""
import os
import struct
import subprocess

import numpy as np
import pytest

import hostlib
import nat_model
import spec64

pytestmark = pytest.mark.gpu
T, CTX, FS, B = 6, 7, 16, 16
FRAMES = [1, T - 1, T, T + 7, 3, 20]


def frames_wave(F, seed, extra=7):
    L, S, _ = spec64.params(FS)
    return spec64.synth_speech(F * S + L - S + extra, FS, seed=seed)


class Case:
    def __init__(self, pkg):
        self.pkg = pkg
        D = self.D = spec64.params(FS)[2] // 2 + 1
        rng = np.random.default_rng(77)
        self.ls = [(CTX + 1) * D, 40, 24, D]
        self.ws = [rng.normal(0, 0.05, (self.ls[i], self.ls[i + 1])).astype(np.float32) for i in range(3)]
        self.bs = [rng.normal(0, 0.1, self.ls[i + 1]).astype(np.float32) for i in range(3)]
        self.mean = rng.normal(10, 2, D).astype(np.float32)
        self.inv = (1.0 / rng.uniform(2, 4, D)).astype(np.float32)
        self.waves = [frames_wave(F, seed=20 + i, extra=3 * i) for i, F in enumerate(FRAMES)]
        assert pkg.enhance_waves_layout([w.size for w in self.waves], FS)[0].tolist() == FRAMES
        # the reference: every utterance alone, through the expanded entry
        eng = self.engine()
        self.out, self.outf, self.lps = [], [], []
        for w in self.waves:
            x = nat_model.normalise(pkg.wave_to_lps(w, fs_khz=FS), self.mean, self.inv)
            F = x.shape[0]
            z = nat_model.noise_rows(x, [0, F], T)
            rows = nat_model.expand(nat_model.edge_stream(x, CTX), np.arange(F), CTX, z, np.zeros(F, np.int32))
            y = eng.forward(rows)
            den = (y / self.inv + self.mean).astype(np.float32)
            o, f = pkg.lps_to_wave(w, den, fs_khz=FS, return_float=True)
            self.out.append(o), self.outf.append(f), self.lps.append(den)
        eng.close()

    def engine(self, cap=0, nat=T, bunch=B):
        return self.pkg.BPGpu(1, 0, self.ls, bunch, 0.1, 0.9, 1e-5, self.ws, self.bs, 2.0, 0, max_cache_frames=cap,
                              nat_frames=nat)

    def run(self, eng, waves=None, **kw):
        return eng.enhance_waves(self.waves if waves is None else waves, self.mean, self.inv, fs_khz=FS, fea_context=CTX,
                                 return_f32=True, return_lps=True, **kw)


def same(got, want):
    assert len(got) == len(want)
    for u, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), "utterance %d" % u


@pytest.fixture(scope="module")
def case(pkg):
    return Case(pkg)


def test_enhance_waves_equals_the_chain_through_the_public_pieces(case):
    """F_u = 1, T - 1, T, T + 7 among them: out, out_f32 and lps_out"""
    eng = case.engine()
    out, outf, lps = case.run(eng)
    same(lps, case.lps)
    same(outf, case.outf)
    same(out, case.out)
    same(eng.enhance_waves(case.waves, case.mean, case.inv, fs_khz=FS), case.out)   # fea_context from the shape
    eng.close()
    # the noise row is in the result: T = 1 gives the same rows for the one-frame utterance and other rows for a long one
    other = case.engine(nat=1)
    lps1 = case.run(other)[2]
    other.close()
    assert lps1[0].tobytes() == case.lps[0].tobytes() and lps1[3].tobytes() != case.lps[3].tobytes()


@pytest.mark.parametrize("cap", [5, 7, 19])
def test_the_chunk_capacity_changes_no_bit(case, cap):
    """chunks begin inside the longer utterances, one of them beyond the first T frames of its utterance (cap 5: packed
    frame 20 is frame 8 of the 13-frame utterance): the noise rows are those of the whole utterance all the same"""
    fo = np.concatenate([[0], np.cumsum(FRAMES)])
    starts = np.arange(0, fo[-1], cap)
    assert any(fo[u] + T < a < fo[u + 1] for a in starts for u in range(len(FRAMES)))   # a chunk starts past T frames
    eng = case.engine(cap=cap)
    out, outf, lps = case.run(eng)
    same(lps, case.lps)
    same(outf, case.outf)
    same(out, case.out)
    eng.close()


def test_enhance_wave_equals_its_slot_of_the_batch_wherever_it_stands(case):
    eng = case.engine(cap=9)
    for u, w in enumerate(case.waves):
        o, f = eng.enhance_wave(w, case.mean, case.inv, fea_context=CTX, fs_khz=FS, return_float=True)
        assert o.tobytes() == case.out[u].tobytes() and f.tobytes() == case.outf[u].tobytes(), u
    perm = [3, 0, 5, 2, 4, 1]
    out, outf, lps = case.run(eng, [case.waves[i] for i in perm])
    same(out, [case.out[i] for i in perm])
    same(lps, [case.lps[i] for i in perm])
    eng.close()


def test_the_scored_calls_return_the_same_waves(case):
    eng = case.engine()
    cleans = [frames_wave(F, seed=90 + i, extra=3 * i) for i, F in enumerate(FRAMES)]
    res = case.run(eng, cleans=cleans)
    same(res[0], case.out)
    same(res[1], case.outf)
    same(res[2], case.lps)
    assert res[3].shape == res[4].shape == (len(FRAMES),) and np.isfinite(res[3]).all() and np.isfinite(res[4]).all()
    res = case.run(eng, cleans=cleans, stoi=True)
    same(res[0], case.out)
    eng.close()


def test_live_sessions_of_a_nat_engine_are_refused(case):
    eng = case.engine()
    with pytest.raises(case.pkg.MlggdError, match="error 4: mlggd_live_open"):
        eng.live(case.mean, case.inv, 2, fs_khz=FS, fea_context=CTX)
    same(case.run(eng)[0], case.out)                                            # the engine decodes as before
    eng.close()


def test_a_plain_engine_still_wants_the_plain_width(case):
    eng = case.engine(nat=0)
    with pytest.raises(case.pkg.MlggdError, match=r"error 1: fea_context 7 x 257 bins != layersizes\[0\]"):
        case.run(eng)
    eng.close()


def write_wav(path, w, rate=16000):
    w = np.asarray(w, "<i2")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + 2 * w.size) + b"WAVEfmt " +
                struct.pack("<IHHIIHH", 16, 1, 1, rate, 2 * rate, 2, 16) + b"data" + struct.pack("<I", 2 * w.size) +
                w.tobytes())


def read_wav_data(path):
    raw = open(path, "rb").read()
    at = raw.index(b"data")
    n = struct.unpack("<I", raw[at + 4:at + 8])[0]
    return np.frombuffer(raw[at + 8:at + 8 + n], "<i2")


def test_the_tool_with_nat_writes_the_bytes_of_the_python_call(case, tmp_path):
    """enhance_wav nat=T: a list in one batch, one line at a time, and a single pair with a report; live= with nat= and a
    nat= that does not fit the net exit with an error"""
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s"])
    hostlib.write_wts(str(tmp_path / "mlp.wts"), case.ws, case.bs)
    hostlib.write_norm(str(tmp_path / "n.norm"), case.mean, case.inv)
    common = [os.path.join(hostlib.HOST, "enhance_wav"), "wts=%s" % (tmp_path / "mlp.wts"),
              "norm_file=%s" % (tmp_path / "n.norm"), "fea_context=%d" % CTX, "bunchsize=%d" % B]
    with open(tmp_path / "list.scp", "w") as scp:
        for u, w in enumerate(case.waves):
            write_wav(tmp_path / ("n%d.wav" % u), w)
            scp.write("%s %s\n" % (tmp_path / ("n%d.wav" % u), tmp_path / ("e%d.wav" % u)))
    for extra in ([], ["batch_s=0"]):
        r = subprocess.run(common + ["nat=%d" % T, "scp=%s" % (tmp_path / "list.scp"), *extra], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        for u in range(len(FRAMES)):
            assert read_wav_data(tmp_path / ("e%d.wav" % u)).tobytes() == case.out[u].tobytes(), (extra, u)
            os.remove(tmp_path / ("e%d.wav" % u))
    write_wav(tmp_path / "clean.wav", frames_wave(FRAMES[3], seed=93))
    r = subprocess.run(common + ["nat=%d" % T, "in=%s" % (tmp_path / "n3.wav"), "out=%s" % (tmp_path / "single.wav"),
                                 "clean=%s" % (tmp_path / "clean.wav"), "info=%s" % (tmp_path / "info.txt")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert read_wav_data(tmp_path / "single.wav").tobytes() == case.out[3].tobytes()
    assert open(tmp_path / "info.txt").read().startswith("Segmental SNR:\n")
    r = subprocess.run(common + ["nat=%d" % T, "scp=%s" % (tmp_path / "list.scp"), "live=4000"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 1 and "live= and nat= do not go together" in r.stderr
    r = subprocess.run(common + ["scp=%s" % (tmp_path / "list.scp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and "layersizes[0] is not fea_context x" in r.stderr
    assert not any((tmp_path / ("e%d.wav" % u)).exists() for u in range(len(FRAMES)))
