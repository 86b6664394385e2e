"""Writes tests/golden/ref_lps_sx289.npz and ref_lps_sx379.npz (CPU only, run by hand; the tests never read the
original project's tree).

Each fixture holds, for one of the two TIMIT utterances the original project ships with the output of its own front end
(Feature_prepare/data/TEST_DR8_MPAM0_SX289 / SX379: a RIFF PCM16 .wav and the .lps that Wav2LPS_be wrote from it):
  samples      int16, the samples that frames 0..FRAMES-1 cover (FRAMES*256 + 256 of them)
  lps          float32 [FRAMES][257], the recorded LPS rows of those frames
  n_samples    the whole file's sample count
  n_frames     the whole file's frame count as the .lps header records it
  header       the .lps file's 12-byte HTK header, as bytes

    python tools/make_spec_golden.py ORIGINAL_PROJECT_ROOT
"""
import os
import struct
import sys

import numpy as np

FRAMES = 56
L, S = 512, 256
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def read_riff_pcm16(path):
    d = open(path, "rb").read()
    if d[:4] != b"RIFF" or d[8:12] != b"WAVE":
        raise ValueError(path + ": not a RIFF WAVE file")
    pos, fmt = 12, None
    while pos + 8 <= len(d):
        cid, size = d[pos:pos + 4], struct.unpack("<I", d[pos + 4:pos + 8])[0]
        body = d[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            fmt = struct.unpack("<HHIIHH", body[:16])
        elif cid == b"data":
            if fmt is None or fmt[0] != 1 or fmt[1] != 1 or fmt[5] != 16:
                raise ValueError(path + ": not mono PCM16")
            return np.frombuffer(body, "<i2").astype(np.int16), fmt[2]
        pos += 8 + size + (size & 1)
    raise ValueError(path + ": no data chunk")


def main(root):
    data = os.path.join(root, "Feature_prepare", "data")
    for tag in ("SX289", "SX379"):
        base = os.path.join(data, "TEST_DR8_MPAM0_" + tag)
        wave, fs = read_riff_pcm16(base + ".wav")
        assert fs == 16000
        raw = open(base + ".lps", "rb").read()
        n, period, size, kind = struct.unpack(">iihh", raw[:12])
        lps = np.frombuffer(raw[12:], ">f4").reshape(n, size // 4)
        np.savez_compressed(os.path.join(OUT, "ref_lps_%s.npz" % tag.lower()),
                            samples=wave[:FRAMES * S + L - S], lps=lps[:FRAMES].astype(np.float32),
                            n_samples=np.int64(wave.size), n_frames=np.int64(n),
                            header=np.frombuffer(raw[:12], np.uint8))
        print(tag, wave.size, n, (period, size, kind))


if __name__ == "__main__":
    main(sys.argv[1])
