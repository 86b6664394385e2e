"""GPU: the mix_wav tool -- RIFF files in, mixed RIFF files and the norm file out -- against mix_waves, lps_stats and
norm_from_stats on the same samples."""
import os
import re
import subprocess

import numpy as np
import pytest

import hostlib
import spec64

pytestmark = pytest.mark.gpu


def write_wav(path, w, hz):
    import wave
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(hz)
        f.writeframes(w.astype("<i2").tobytes())


def read_wav(path):
    import wave
    with wave.open(str(path), "rb") as f:
        assert f.getnchannels() == 1 and f.getsampwidth() == 2
        return np.frombuffer(f.readframes(f.getnframes()), "<i2").astype(np.int16), f.getframerate()


@pytest.mark.parametrize("batch_s", [300, 0.001])
def test_mix_wav_writes_mix_waves_samples_and_the_norm_file(pkg, tmp_path, batch_s):
    """four tiny files over two noise files; batch_s = 0.001 makes every line a batch of its own: the same files"""
    subprocess.check_call(["make", "-C", hostlib.HOST, "-s", "mix_wav"])
    fs, hz = 8, 8000
    L, S, N = spec64.params(fs)
    rng = np.random.default_rng(3)
    cleans = [spec64.synth_speech(F * S + L - S + 5 * i, fs, seed=40 + i) for i, F in enumerate([4, 9, 1, 6])]
    noises = [rng.integers(-1500, 1501, 700).astype(np.int16), rng.integers(-900, 901, 3100).astype(np.int16)]
    which, snr, start = [0, 1, 0, 1], [5.0, 0.0, float("inf"), -5.0], [0, 3099, 699, 17]
    for i, c in enumerate(cleans):
        write_wav(tmp_path / ("c%d.wav" % i), c, hz)
    for i, z in enumerate(noises):
        write_wav(tmp_path / ("n%d.wav" % i), z, hz)
    scp = tmp_path / "list.scp"
    scp.write_text("".join("%s %s %s %d %s\n" % (tmp_path / ("c%d.wav" % i), tmp_path / ("n%d.wav" % which[i]),
                                                  "inf" if snr[i] == float("inf") else repr(snr[i]), start[i],
                                                  tmp_path / ("out%d.wav" % i)) for i in range(4)))
    norm = tmp_path / "noisy.norm"
    r = subprocess.run([os.path.join(hostlib.HOST, "mix_wav"), "scp=%s" % scp, "norm_out=%s" % norm, "fs=%d" % fs,
                        "batch_s=%r" % batch_s], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    noise = np.concatenate(noises)
    seg = [(0, 700) if w == 0 else (700, 3100) for w in which]
    want, gain, clipped = pkg.mix_waves(cleans, noise, snr, start, noise_seg=seg, return_info=True)
    report = r.stdout.strip().split("\n")
    assert len(report) == 4
    for i in range(4):
        got, rate = read_wav(tmp_path / ("out%d.wav" % i))
        assert rate == hz and np.array_equal(got, want[i]), "file %d" % i
        m = re.fullmatch(r"(\S+) gain (\S+) clipped (\d+)", report[i])
        assert m and m.group(1).endswith("out%d.wav" % i) and float(m.group(2)) == gain[i] and int(m.group(3)) == clipped[i]
    assert np.array_equal(want[2], cleans[2])                       # snr_db inf
    D = N // 2 + 1
    mean, inv = hostlib.HostNorm.read(str(norm), D)
    wmean, winv = pkg.norm_from_stats(*pkg.lps_stats(want, fs_khz=fs))
    lines = norm.read_text().split("\n")
    assert lines[0] == "vec %d" % D and lines[D + 1] == "vec %d" % D
    # %g keeps six significant digits: half a unit of the sixth is 5e-6 relative
    assert np.allclose(mean, wmean, rtol=5e-6, atol=0) and np.allclose(inv, winv, rtol=5e-6, atol=0)
