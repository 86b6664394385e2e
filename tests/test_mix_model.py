"""CPU: the model of the mixing rule (tests/mix64.py) itself -- the yardstick of the GPU tests has to be right first."""
import math

import numpy as np
import pytest

import mix64


def rand16(n, seed, amp=8000):
    return np.random.default_rng(seed).integers(-amp, amp + 1, n).astype(np.int16)


@pytest.mark.parametrize("snr_db", [-40.0, -5.0, 0.0, 20.0])
def test_the_unrounded_mix_has_the_requested_snr(snr_db):
    clean, noise = rand16(3001, 1), rand16(977, 2, amp=300)
    nz = mix64.paired(noise, 5, 900, 899, clean.size)
    Ec, En = mix64.energies(clean, nz)
    g = mix64.gain(Ec, En, mix64.ratio(snr_db))
    e_noise = math.fsum((g * float(z)) ** 2 for z in nz.tolist())
    assert abs(10.0 * math.log10(Ec / e_noise) - snr_db) <= 1e-12


@pytest.mark.parametrize("ln_of", [lambda n: 1, lambda n: n - 1, lambda n: n + 13])
def test_wrap_around_indexing(ln_of):
    n = 57
    ln = ln_of(n)
    noise = rand16(200, 3)
    lo, start = 11, ln - 1
    want = np.array([noise[lo + (start + i) % ln] for i in range(n)], np.int16)
    got = mix64.paired(noise, lo, ln, start, n)
    assert np.array_equal(got, want)
    assert got[0] == noise[lo + ln - 1] and (ln == 1 or got[1] == noise[lo])    # the start at the segment's last sample wraps at once


def test_zero_energy_and_infinite_snr_leave_the_clean_wave():
    clean, noise = rand16(100, 4), rand16(100, 5)
    silent = np.zeros(100, np.int16)
    for c, z, snr in ((silent, noise, 0.0), (clean, silent, 0.0), (clean, noise, math.inf)):
        out, g, clipped = mix64.mix_utt(c, z, 0, 100, 0, snr)
        assert g == 0.0 and clipped == 0 and np.array_equal(out, c)
    assert mix64.ratio(math.inf) == 0.0 and mix64.ratio(0.0) == 1.0 and mix64.ratio(20.0) == 0.1


def test_ties_go_to_even_and_the_clamp_counts_what_it_changed():
    clean = np.array([0, 1, 2, -1, -2, 32767, 32767, -32768, -32768, -32768, 100], np.int16)
    nz = np.array([1, 1, 1, 1, -1, 1, 3, -1, -3, 1, 0], np.int16)
    out, clipped = mix64.mix(clean, nz, 0.5)
    #                 0.5 1.5 2.5 -0.5 -2.5  32767.5->32768 32768.5->32768 -32768.5->-32768 -32769.5->-32770 -32767.5  100
    assert out.tolist() == [0, 2, 2, 0, -2, 32767, 32767, -32768, -32768, -32768, 100]
    assert clipped == 3                       # the two above 32767 and -32770; -32768.5 rounds to -32768 and is not clipped
    out, clipped = mix64.mix(np.array([30000, -30000], np.int16), np.array([30000, -30000], np.int16), 1.0)
    assert out.tolist() == [32767, -32768] and clipped == 2


def test_the_energies_are_exact_integers_beyond_2_to_the_53():
    c = np.full(5, -32768, np.int16)
    Ec, En = mix64.energies(c, c[:3])
    assert Ec == 5 * 2 ** 30 and En == 3 * 2 ** 30
    assert mix64.gain(2 ** 62 + 1, 2 ** 62 + 1, 1.0) == 1.0
