"""CPU, no device: pkg.read_asymmetry (mlggd_read_asymmetry) on the two file forms it accepts -- a plain list of D
numbers, and the file MLGGD_ASYMMODEL writes (host/asymfile.h), written here in its documented format -- the same file
through pkg.read_shapefactors as it is, and the argument checks of the entry points that need no engine."""
import ctypes

import numpy as np
import pytest

D = 7
BEST_BETA = [0.5, 1.2, float("nan"), 2.5, 0.7, float("nan"), 1.0]
BEST_KAPPA = [0.8, 1.25, float("nan"), 1.0, 2.0, float("nan"), 0.5]


def g9(x):
    return "%.9g" % x


def model_text(betas, kappas, shared="1.10000002", rows=None, header=True):
    """'#' header lines, then `d p_plus p_minus alpha_at_best best_beta best_kappa alpha_at_shared kappa_at_shared`"""
    rng = np.random.default_rng(3)
    lines = []
    if header:
        lines += ["# asymmetric GGD error model of the CV set: beta/(alpha (kappa + 1/kappa) Gamma(1/beta)) exp(-(s(e)/alpha)^beta),",
                  "# e = out - targ, s(e) = kappa e for e > 0, -e / kappa for e < 0",
                  "# n 1234", "# D %d" % len(betas), "# betas 0.5 0.600000024 0.699999988"]
        if shared is not None:
            lines.append("# shared_beta %s" % shared)
        lines += ["# loglik_per_frame -1.5 -1.25 -1.125",
                  "# d p_plus p_minus alpha_at_best best_beta best_kappa alpha_at_shared kappa_at_shared"]
    for d, b, k in (zip(range(len(betas)), betas, kappas) if rows is None else rows):
        f = lambda v: g9(v) if isinstance(v, float) else str(v)
        lines.append(" ".join([str(d)] + [g9(v) for v in rng.uniform(0.1, 1, 3)] + [f(b), f(k), g9(0.9), g9(1.1)]))
    return "\n".join(lines) + "\n"


def test_a_plain_list_reads_back_exactly(pkg, tmp_path):
    want = np.random.default_rng(1).uniform(0.4, 2.5, D).astype(np.float32)
    p = tmp_path / "list.txt"
    p.write_text("\n".join(g9(v) for v in want) + "\n")
    assert np.array_equal(pkg.read_asymmetry(str(p), D), want)
    p.write_text("  ".join(g9(v) for v in want[:4]) + "\n\t" + " ".join(g9(v) for v in want[4:]))   # any layout
    assert np.array_equal(pkg.read_asymmetry(p, D, 1.0), want)


def test_a_model_file_gives_column_6_and_reads_as_a_shape_file(pkg, tmp_path):
    p = tmp_path / "cv.asymmodel"
    p.write_text(model_text(BEST_BETA, BEST_KAPPA))
    got = pkg.read_asymmetry(str(p), D)
    assert np.array_equal(got, np.where(np.isnan(BEST_KAPPA), np.float32(1.0), np.array(BEST_KAPPA, np.float32)))
    assert np.array_equal(pkg.read_asymmetry(str(p), D, 1.5)[[2, 5]], np.float32([1.5, 1.5]))      # nan rows: the fallback
    # the existing shape reader, unchanged, takes field 5 and the shared beta of the same file
    shapes = pkg.read_shapefactors(str(p), D, 1.7)
    want = np.array([np.float32(1.10000002) if np.isnan(b) else np.float32(g9(b)) for b in BEST_BETA], np.float32)
    assert np.array_equal(shapes, want)
    p.write_text(model_text(BEST_BETA, BEST_KAPPA, header=False))      # the rows alone: recognised by row 0 and its fields
    assert pkg.read_asymmetry(str(p), D)[4] == np.float32(2.0) and pkg.read_shapefactors(str(p), D, 1.7)[3] == np.float32(2.5)


def line_of(text, needle):
    return 1 + [i for i, l in enumerate(text.splitlines()) if l.startswith(needle)][0]


@pytest.mark.parametrize("case", ["D-1 rows", "D+1 rows", "out of order", "zero", "negative", "inf", "word", "five fields"])
def test_a_malformed_model_file_names_the_line(pkg, tmp_path, case):
    kap = [1.0 if np.isnan(k) else k for k in BEST_KAPPA]
    bet = [1.0 if np.isnan(b) else b for b in BEST_BETA]
    rows = list(zip(range(D), bet, kap))
    if case == "D-1 rows":
        rows = rows[:-1]
    elif case == "D+1 rows":
        rows = rows + [(D, 1.0, 1.0)]
    elif case == "out of order":
        rows[3], rows[4] = rows[4], rows[3]
    elif case != "five fields":
        rows[4] = (4, bet[4], {"zero": "0", "negative": "-1.5", "inf": "inf", "word": "kappa"}[case])
    text = model_text(bet, kap, rows=rows)
    if case == "five fields":
        lines = text.splitlines()
        i = line_of(text, "4 ") - 1
        lines[i] = " ".join(lines[i].split()[:5])
        text = "\n".join(lines) + "\n"
    p = tmp_path / "bad.asymmodel"
    p.write_text(text)
    n_lines = len(text.splitlines())
    want_line = {"D-1 rows": n_lines, "D+1 rows": n_lines}.get(case, line_of(text, "4 "))
    with pytest.raises(pkg.MlggdError, match=r"line %d\b" % want_line) as ei:
        pkg.read_asymmetry(str(p), D)
    assert str(p) in str(ei.value) and "mlggd error 1:" in str(ei.value)        # MLGGD_ERR_ARG


@pytest.mark.parametrize("bad,line", [("0", 2), ("-0.5", 2), ("inf", 2), ("nan", 2), ("kappa", 2), ("1.5x", 2), (None, 3), ("+", 4)])
def test_a_malformed_list_names_the_line(pkg, tmp_path, bad, line):
    vals = [["1", "1.5", "0.5"], ["2", "0.75"], ["1.25", "1"]]       # 7 numbers on three lines
    if bad is None:
        vals[2] = vals[2][:1]                                          # D-1 numbers: found at the end of the file
    elif bad == "+":
        vals.append(["1.5"])                                           # D+1: the line of the extra one
    else:
        vals[1][1] = bad
    p = tmp_path / "list.txt"
    p.write_text("\n".join(" ".join(v) for v in vals) + "\n")
    with pytest.raises(pkg.MlggdError, match=r"line %d\b" % line):
        pkg.read_asymmetry(str(p), D)


def test_null_arguments_are_err_arg(pkg, tmp_path):
    L = pkg.load()
    k = (ctypes.c_float * D)(*([1.0] * D))
    assert L.mlggd_set_asymmetry(None, k) == 1 and b"NULL" in L.mlggd_last_error()
    assert L.mlggd_get_asymmetry(None, k) == 1
    assert L.mlggd_read_asymmetry(None, D, 1.0, k) == 1 and b"NULL" in L.mlggd_last_error()
    assert L.mlggd_read_asymmetry(b"x", D, 1.0, None) == 1
    assert L.mlggd_read_asymmetry(b"x", 0, 1.0, k) == 1
    with pytest.raises(pkg.MlggdError):
        pkg.read_asymmetry(None, D)
    with pytest.raises(pkg.MlggdError, match="cannot read"):
        pkg.read_asymmetry(str(tmp_path / "missing.txt"), D)
