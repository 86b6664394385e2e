"""CPU, no device: pkg.read_shapefactors (mlggd_read_shapefactors) on the two file forms it accepts -- a plain list
of D numbers, and the file MLGGD_ERRMODEL writes (host/errmodel.h), written here in its documented format -- and the
argument checks of the new entry points that need no engine."""
import ctypes

import numpy as np
import pytest

D = 7
BEST = [0.5, 1.2, float("nan"), 2.5, 0.7, float("nan"), 1.0]


def g9(x):
    return "%.9g" % x


def model_text(best, shared="1.10000002", rows=None, header=True):
    """'#' header lines, then `d mean var kurt best_beta alpha_at_best alpha_at_shared` per bin, all %.9g"""
    rng = np.random.default_rng(3)
    lines = []
    if header:
        lines += ["# GGD error model of the CV set: beta/(2 alpha Gamma(1/beta)) exp(-(|e|/alpha)^beta), e = out - targ",
                  "# n 1234", "# D %d" % len(best), "# betas 0.5 0.600000024 0.699999988"]
        if shared is not None:
            lines.append("# shared_beta %s" % shared)
        lines += ["# loglik_per_frame -1.5 -1.25 -1.125", "# d mean var kurt best_beta alpha_at_best alpha_at_shared"]
    for d, b in (enumerate(best) if rows is None else rows):
        fit = not (isinstance(b, float) and np.isnan(b))
        lines.append(" ".join([str(d)] + [g9(v) for v in rng.normal(0, 1, 3)] +
                              [g9(b) if isinstance(b, float) else str(b), g9(0.8 if fit else 0.0), g9(0.9)]))
    return "\n".join(lines) + "\n"


def test_a_plain_list_reads_back_exactly(pkg, tmp_path):
    want = np.random.default_rng(1).uniform(0.5, 2.5, D).astype(np.float32)
    p = tmp_path / "list.txt"
    p.write_text("\n".join(g9(v) for v in want) + "\n")
    assert np.array_equal(pkg.read_shapefactors(str(p), D, 1.0), want)
    p.write_text("  ".join(g9(v) for v in want[:4]) + "\n\t" + " ".join(g9(v) for v in want[4:]))   # any layout
    assert np.array_equal(pkg.read_shapefactors(p, D, 1.0), want)


def test_an_error_model_file_gives_column_5(pkg, tmp_path):
    p = tmp_path / "cv.errmodel"
    p.write_text(model_text(BEST))
    got = pkg.read_shapefactors(str(p), D, 1.7)
    want = np.array([np.float32(1.10000002) if np.isnan(b) else np.float32(g9(b)) for b in BEST], np.float32)
    assert np.array_equal(got, want)                       # nan rows: the file's shared beta
    p.write_text(model_text(BEST, shared=None))
    got = pkg.read_shapefactors(str(p), D, 1.7)
    assert np.array_equal(got, np.where(np.isnan(BEST), np.float32(1.7), np.array(BEST, np.float32)))   # ... else fallback
    p.write_text(model_text(BEST, shared="nan"))           # no bin had a fit when the header was written
    assert np.array_equal(pkg.read_shapefactors(str(p), D, 1.7)[[2, 5]], np.float32([1.7, 1.7]))
    p.write_text(model_text(BEST, header=False))           # the rows alone: still recognised by row 0 and its 7 fields
    assert pkg.read_shapefactors(str(p), D, 1.7)[3] == np.float32(2.5)


def line_of(text, needle):
    return 1 + [i for i, l in enumerate(text.splitlines()) if l.startswith(needle)][0]


@pytest.mark.parametrize("case", ["D-1 rows", "D+1 rows", "out of order", "zero", "negative", "inf", "word"])
def test_a_malformed_error_model_names_the_line(pkg, tmp_path, case):
    full = [1.0 if np.isnan(b) else b for b in BEST]
    rows = list(enumerate(full))
    if case == "D-1 rows":
        rows = rows[:-1]
    elif case == "D+1 rows":
        rows = rows + [(D, 1.0)]
    elif case == "out of order":
        rows[3], rows[4] = rows[4], rows[3]
    else:
        rows[4] = (4, {"zero": "0", "negative": "-1.5", "inf": "inf", "word": "beta"}[case])
    text = model_text(full, rows=rows)
    p = tmp_path / "bad.errmodel"
    p.write_text(text)
    n_lines = len(text.splitlines())
    want_line = {"D-1 rows": n_lines, "D+1 rows": n_lines, "out of order": line_of(text, "4 ")}.get(case, line_of(text, "4 "))
    with pytest.raises(pkg.MlggdError, match=r"line %d\b" % want_line) as ei:
        pkg.read_shapefactors(str(p), D, 1.0)
    assert str(p) in str(ei.value) and "mlggd error 1:" in str(ei.value)        # MLGGD_ERR_ARG


@pytest.mark.parametrize("bad,line", [("0", 2), ("-0.5", 2), ("inf", 2), ("nan", 2), ("beta", 2), ("1.5x", 2), (None, 3), ("+", 4)])
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
        pkg.read_shapefactors(str(p), D, 1.0)


def test_null_arguments_are_err_arg(pkg, tmp_path):
    L = pkg.load()
    b = (ctypes.c_float * D)(*([1.0] * D))
    assert L.mlggd_set_shapefactors(None, b) == 1 and b"NULL" in L.mlggd_last_error()
    assert L.mlggd_get_shapefactors(None, b) == 1
    assert L.mlggd_read_shapefactors(None, D, 1.0, b) == 1 and b"NULL" in L.mlggd_last_error()
    assert L.mlggd_read_shapefactors(b"x", D, 1.0, None) == 1
    assert L.mlggd_read_shapefactors(b"x", 0, 1.0, b) == 1
    with pytest.raises(pkg.MlggdError):
        pkg.read_shapefactors(None, D, 1.0)
    with pytest.raises(pkg.MlggdError, match="cannot read"):
        pkg.read_shapefactors(str(tmp_path / "missing.txt"), D, 1.0)
