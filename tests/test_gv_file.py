"""CPU: pkg.read_gv (mlggd_read_gv, host/binfile.h) -- the reader of the decoders' gv=FILE: a plain list of D factors or
the file an epoch with MLGGD_GVFILE writes (written here by tests/gv64.write_gv_file in its documented format), the
shared factor, bins without a fit, and every malformed file with its path and line in the message."""
import numpy as np
import pytest

import gv64

D = 6


def fitted_file(tmp_path, name="gv.txt", unfit=(), shared_fitted=True):
    rng = np.random.default_rng(3)
    est, ref = rng.uniform(0.2, 0.9, D), rng.uniform(0.5, 1.5, D)
    eta = np.sqrt(ref / est).astype(np.float32)
    fitted = np.ones(D, bool)
    fitted[list(unfit)] = False
    shared = (0.4, 0.9, np.float32(np.sqrt(0.9 / 0.4)), shared_fitted)
    gv64.write_gv_file(str(tmp_path / name), 1234, est, ref, eta, fitted, shared)
    return tmp_path / name, eta, fitted, shared


def same32(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_a_plain_list(pkg, tmp_path):
    eta = gv64.draw_eta(D, 1)
    p = tmp_path / "list.txt"
    p.write_text(" ".join("%.9g" % v for v in eta[:4]) + "\n\n" + "\n".join("%.9g" % v for v in eta[4:]) + "\n")
    got = pkg.read_gv(str(p), D)
    assert got.dtype == np.float32 and same32(got, eta)
    p.write_text(" ".join("%.9g" % v for v in eta[:5]) + " nan\n")      # a bin written as nan takes 1
    assert same32(pkg.read_gv(str(p), D), np.append(eta[:5], np.float32(1)))
    with pytest.raises(pkg.MlggdError, match=r"list\.txt line 1: a plain list has no shared factor"):
        pkg.read_gv(str(p), D, shared=True)


def test_the_trainer_s_file(pkg, tmp_path):
    p, eta, _, shared = fitted_file(tmp_path)
    assert same32(pkg.read_gv(str(p), D), eta)                           # %.9g reads back to the bits
    assert same32(pkg.read_gv(str(p), D, shared=True), np.full(D, shared[2]))
    # without the header lines: the first data line starts with row 0 and has four fields
    q = tmp_path / "bare.txt"
    q.write_text("".join(l for l in open(p) if not l.startswith("#")))
    assert same32(pkg.read_gv(str(q), D), eta)


def test_bins_without_a_fit_take_one(pkg, tmp_path):
    p, eta, fitted, _ = fitted_file(tmp_path, unfit=(0, 4))
    want = np.where(fitted, eta, np.float32(1)).astype(np.float32)
    assert "\n4 " in open(p).read() and " nan\n" in open(p).read()
    assert same32(pkg.read_gv(str(p), D), want)
    p2, _, _, _ = fitted_file(tmp_path, "nofit.txt", unfit=range(D), shared_fitted=False)
    assert "# shared_eta nan" in open(p2).read()
    assert same32(pkg.read_gv(str(p2), D), np.ones(D)) and same32(pkg.read_gv(str(p2), D, shared=True), np.ones(D))


def edit(tmp_path, src, name, fn):
    lines = open(src).read().splitlines()
    fn(lines)
    (tmp_path / name).write_text("\n".join(lines) + "\n")
    return str(tmp_path / name)


def test_every_malformed_file_names_its_line(pkg, tmp_path):
    p, eta, _, _ = fitted_file(tmp_path)
    head = sum(1 for l in open(p) if l.startswith("#"))      # rows start at line head + 1
    cases = [
        ("short", lambda l: l.pop(), r"line %d: %d rows, the output layer has %d" % (head + D - 1, D - 1, D)),
        ("long", lambda l: l.append("%d 1 1 1" % D), r"line %d: more than the %d rows" % (head + D + 1, D)),
        ("order", lambda l: l.__setitem__(head + 2, "5 1 1 1"), r"line %d: row 5 where row 2 belongs" % (head + 3)),
        ("word", lambda l: l.__setitem__(head + 1, "1 0.5 0.5 abc"), r"line %d: field 4 'abc' is not a number" % (head + 2)),
        ("fields", lambda l: l.__setitem__(head + 1, "1 0.5 0.5"), r"line %d: a row has the fields d gv_ref gv_est eta" % (head + 2)),
        ("zero", lambda l: l.__setitem__(head, "0 0.5 0.5 0"), r"line %d: eta 0 of bin 0 is not positive and finite" % (head + 1)),
        ("neg", lambda l: l.__setitem__(head + 3, "3 0.5 0.5 -1.5"), r"line %d: eta -1.5 of bin 3" % (head + 4)),
        ("inf", lambda l: l.__setitem__(head + 3, "3 0.5 0.5 inf"), r"line %d: eta inf of bin 3" % (head + 4)),
        ("shared", lambda l: l.__setitem__(3, "# shared_eta -2"), r"line 4: shared_eta -2 is not positive and finite"),
        ("sharedword", lambda l: l.__setitem__(3, "# shared_eta x"), r"line 4: shared_eta 'x' is not a number"),
    ]
    assert open(p).read().splitlines()[3].startswith("# shared_eta")
    for name, fn, msg in cases:
        path = edit(tmp_path, p, name + ".txt", fn)
        with pytest.raises(pkg.MlggdError, match=r"error 1: .*%s\.txt %s" % (name, msg)):
            pkg.read_gv(path, D)
    # plain lists
    lists = [
        ("few", "1 1.5 2\n0.5\n", r"line 2: 4 factors, the output layer has %d" % D),
        ("many", "1 1 1\n1 1 1 1\n", r"line 2: more than the %d factors" % D),
        ("nonum", "1 1 1\n1 x 1\n", r"line 2: 'x' is not a number"),
        ("nonpos", "1 1 1\n1 1 0\n", r"line 2: factor 0 of bin 5 is not positive and finite"),
        ("empty", "", r"line 1: 0 factors"),
    ]
    for name, text, msg in lists:
        (tmp_path / (name + ".txt")).write_text(text)
        with pytest.raises(pkg.MlggdError, match=r"error 1: .*%s\.txt %s" % (name, msg)):
            pkg.read_gv(str(tmp_path / (name + ".txt")), D)
    # a header-less trainer file without its shared line has no shared factor
    bare = edit(tmp_path, p, "bare.txt", lambda l: l.__delitem__(slice(0, head)))
    with pytest.raises(pkg.MlggdError, match=r"bare\.txt line %d: the file has no '# shared_eta' line" % D):
        pkg.read_gv(bare, D, shared=True)
    # an unreadable path, and the arguments
    with pytest.raises(pkg.MlggdError, match=r"error 1: .*missing\.txt line 1: cannot read the file"):
        pkg.read_gv(str(tmp_path / "missing.txt"), D)
    with pytest.raises(pkg.MlggdError, match="error 1: D 0 < 1"):
        pkg.read_gv(str(p), 0)
    with pytest.raises(pkg.MlggdError, match="error 1: NULL"):
        pkg.read_gv(None, D)
    assert same32(pkg.read_gv(str(p), D), eta)
