"""CPU: the learned scale's state file (host/scalefile.h behind pkg.read_scale_state / pkg.write_scale_state): the round
trip keeps every bit, and every malformed file is MLGGD_ERR_ARG with "PATH line N: ..." as the message."""
import re

import numpy as np
import pytest

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def awkward(D, seed):
    """values whose shortest decimal form is long: random mantissas over the whole exponent range, subnormals, the
    largest float, a seed (0) and both zeros of the velocity"""
    rng = np.random.default_rng(seed)
    a = (rng.integers(1, 2 ** 31 - 2 ** 23, D, dtype=np.int64).astype(np.uint32)).view(F).copy()   # positive, finite
    v = (rng.integers(0, 2 ** 32, D, dtype=np.int64).astype(np.uint32)).view(F).copy()
    v[~np.isfinite(v)] = F(-1.5)
    a[0], a[1], a[2], a[3] = 0.0, np.finfo(F).max, np.finfo(F).tiny, 1e-45
    v[0], v[1], v[2] = 0.0, -0.0, -np.finfo(F).max
    return a, v


@pytest.mark.parametrize("D", [1, 19, 257])
def test_the_round_trip_keeps_every_bit(pkg, tmp_path, D):
    a, v = awkward(max(D, 4), D)
    a, v = a[:D], v[:D]
    path = str(tmp_path / "scale.txt")
    pkg.write_scale_state(path, a, v, lrate=0.05, momentum=0.5, vmax=1.0, steps=1234)
    ra, rv = pkg.read_scale_state(path, D)
    assert np.array_equal(bits(ra), bits(a)) and np.array_equal(bits(rv), bits(v))
    text = open(path).read().split("\n")
    head = [l for l in text if l.startswith("#")]
    assert "# D %d" % D in head and "# steps 1234" in head and "# lrate 0.0500000007" in head
    assert "# momentum 0.5" in head and "# vmax 1" in head and head[-1] == "# d alpha velocity"
    rows = [l for l in text if l and not l.startswith("#")]
    assert len(rows) == D and all(r.split()[0] == str(d) and len(r.split()) == 3 for d, r in enumerate(rows))
    # velocity None: zeros
    pkg.write_scale_state(path, a)
    ra, rv = pkg.read_scale_state(path, D)
    assert np.array_equal(bits(ra), bits(a)) and np.array_equal(bits(rv), bits(np.zeros(D, F)))


def write(tmp_path, text):
    p = tmp_path / "bad.txt"
    p.write_text(text)
    return str(p)


def rows(D, alpha="1.5", velocity="0.25"):
    return ["%d %s %s" % (d, alpha, velocity) for d in range(D)]


CASES = [
    ("too_few_rows", ["# D 4"] + rows(3), 4, r"3 rows, the output layer has 4"),
    ("too_many_rows", ["# D 4"] + rows(5), 6, r"more than the 4 rows"),
    ("empty", [], 1, r"0 rows, the output layer has 4"),
    ("out_of_order", ["# h", "0 1 0", "2 1 0", "1 1 0", "3 1 0"], 3, r"row 2 where row 1 belongs"),
    ("negative_alpha", rows(2) + ["2 -0.5 0", "3 1 0"], 3, r"alpha -0.5 of bin 2 is negative or not finite"),
    ("nan_alpha", rows(1) + ["1 nan 0"] + ["2 1 0", "3 1 0"], 2, r"alpha nan of bin 1"),
    ("inf_alpha", rows(3) + ["3 inf 0"], 4, r"alpha inf of bin 3"),
    ("overflowing_alpha", ["0 1e39 0"] + rows(4)[1:], 1, r"alpha 1e39 of bin 0"),
    ("nan_velocity", ["# a", "# b"] + rows(3) + ["3 1 nan"], 6, r"velocity nan of bin 3 is not finite"),
    ("not_a_number", rows(2) + ["2 1.0x 0", "3 1 0"], 3, r"field 2 '1.0x' is not a number"),
    ("two_fields", rows(3) + ["3 1"], 4, r"a row has the fields d alpha velocity, this one has 2"),
]


@pytest.mark.parametrize("name,lines,line,what", CASES, ids=[c[0] for c in CASES])
def test_a_malformed_file_is_refused_with_its_line(pkg, tmp_path, name, lines, line, what):
    path = write(tmp_path, "".join(l + "\n" for l in lines))
    with pytest.raises(pkg.MlggdError, match=r"mlggd error 1: %s line %d: .*%s" % (re.escape(path), line, what)):
        pkg.read_scale_state(path, 4)


def test_an_unreadable_file_and_bad_arguments(pkg, tmp_path):
    missing = str(tmp_path / "no" / "such.txt")
    with pytest.raises(pkg.MlggdError, match=r"mlggd error 1: %s line 1: cannot read the file" % re.escape(missing)):
        pkg.read_scale_state(missing, 4)
    with pytest.raises(pkg.MlggdError, match=r"mlggd error 1: %s line 1: cannot write the file" % re.escape(missing)):
        pkg.write_scale_state(missing, np.ones(4, F))
    with pytest.raises(pkg.MlggdError, match="mlggd error 1: D 0 < 1"):
        pkg.read_scale_state(write(tmp_path, "0 1 0\n"), 0)
    with pytest.raises(pkg.MlggdError, match="mlggd error 1: NULL"):
        pkg.read_scale_state(None, 4)
    # a zero alpha ("seed") and a file without a header are fine; '#' lines and blank lines anywhere are skipped
    a, v = pkg.read_scale_state(write(tmp_path, "0 0 0\n\n# note\n1 2 -3\n"), 2)
    assert a.tolist() == [0.0, 2.0] and v.tolist() == [0.0, -3.0]
    assert "mlggd_read_scale_state" in pkg.EXPORTS and "mlggd_write_scale_state" in pkg.EXPORTS
