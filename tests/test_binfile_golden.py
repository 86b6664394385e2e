"""CPU, no device: the three per-bin model-file readers of the host tools (parse_shapefactors, parse_asymmetry, parse_gv;
host/binfile.h) against their recorded behaviour.  tests/binfile_main.cc, a stand-alone program built with the host
compiler under AddressSanitizer + UBSan (plain, and saying so, where g++ has no sanitizer runtime), runs every case of
the corpus below -- plain lists, the three model files in their documented formats with every malformed variant,
degenerate files -- through the readers and prints the return
value, the whole error text and the bits of the D floats.  tests/golden/binfile_cases.json is that output as recorded
before the three readers were folded into one; the test asks for the same lines, byte for byte, and for no sanitizer
report.  `python tests/test_binfile_golden.py DIR` writes the corpus and its case list into DIR."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "speech-enhancement-based-on-a-maximum-likelihood-criterion_amd", "host")
GOLDEN = os.path.join(ROOT, "tests", "golden", "binfile_cases.json")

D = 5
VALUE = {"shape": "1.7", "asym": "1.5", "gv": "0"}     # the fallbacks of the first two; gv: per-bin factors
LIST = ["0.5", "1.25", "2", "0.75", "1"]

HEAD = {
    "err": ["# GGD error model of the CV set: beta/(2 alpha Gamma(1/beta)) exp(-(|e|/alpha)^beta), e = out - targ",
            "# n 1234", "# D 5", "# betas 0.5 0.600000024 0.699999988", "# shared_beta 1.10000002",
            "# loglik_per_frame -1.5 -1.25 -1.125", "# d mean var kurt best_beta alpha_at_best alpha_at_shared"],
    "asym": ["# asymmetric GGD error model of the CV set: beta/(alpha (kappa + 1/kappa) Gamma(1/beta)) exp(-(s(e)/alpha)^beta),",
             "# e = out - targ, s(e) = kappa e for e > 0, -e / kappa for e < 0",
             "# n 1234", "# D 5", "# betas 0.5 0.600000024 0.699999988", "# shared_beta 1.10000002",
             "# loglik_per_frame -1.5 -1.25 -1.125",
             "# d p_plus p_minus alpha_at_best best_beta best_kappa alpha_at_shared kappa_at_shared"],
    "gv": ["# global variance equalisation of the CV set: eta = sqrt(gv_ref / gv_est), normalised outputs and targets",
           "# n 1234", "# D 5", "# shared_eta 1.08000004", "# gv_ref_shared 0.81000000000000005",
           "# gv_est_shared 0.69444444444444442", "# d gv_ref gv_est eta"],
}
# the fields after the row number; COL is the index, in the whole row, of the field the kind's own reader takes
ROW = {
    "err": [["0.01", "0.5", "3.5", "0.5", "0.8", "0.9"], ["-0.02", "0.25", "4", "1.20000005", "0.7", "0.9"],
            ["0.03", "1.5", "2.5", "2.5", "0.6", "0.9"], ["0", "0.75", "3", "0.699999988", "0.5", "0.9"],
            ["0.04", "1", "6", "1", "0.4", "0.9"]],
    "asym": [["0.3", "0.2", "0.8", "0.5", "0.800000012", "0.9", "1.1"], ["0.25", "0.35", "0.7", "1.20000005", "1.25", "0.9", "1.1"],
             ["0.4", "0.1", "0.6", "2.5", "1", "0.9", "1.1"], ["0.15", "0.45", "0.5", "0.699999988", "2", "0.9", "1.1"],
             ["0.2", "0.2", "0.4", "1", "0.5", "0.9", "1.1"]],
    "gv": [["0.81000000000000005", "0.64000000000000001", "1.125"], ["1", "1", "1"], ["0.25", "1", "0.5"],
           ["2.25", "1", "1.5"], ["0.5", "0.5", "1"]],
}
COL = {"err": 4, "asym": 5, "gv": 3}
SHARED = {"err": "shared_beta", "asym": "shared_beta", "gv": "shared_eta"}


def model(kind, head=True, shared_line="", rows=None, edit=None):
    """the text of a model file of `kind`: its header (shared_line None drops the shared line, a string replaces it),
    then `rows` (default 0..D-1) with edit = {row: {field index: text}} or {row: fields to keep}"""
    lines = []
    if head:
        for l in HEAD[kind]:
            if l.startswith("# shared_"):
                if shared_line is None:
                    continue
                l = shared_line or l
            lines.append(l)
    for d in (range(D) if rows is None else rows):
        f = [str(d)] + list(ROW[kind][d % D])
        e = (edit or {}).get(d)
        if isinstance(e, dict):
            for i, t in e.items():
                f[i] = t
        elif e is not None:
            f = f[:e]
        lines.append(" ".join(f))
    return "\n".join(lines) + "\n"


def corpus():
    """({file name: text}, [(reader, file, value)]); a name absent from the files is a missing file"""
    files, cases = {}, []

    def put(name, text, readers=("shape", "asym", "gv")):
        files[name] = text
        cases.extend((r, name, VALUE[r]) for r in readers)

    def lst(name, vals):
        put(name, "\n".join(vals) + "\n")

    lst("list_exact.txt", LIST)
    put("list_tabs.txt", "0.5\t1.25 2\n\t0.75\t1")                      # two lines, tabs, no final newline
    lst("list_comment.txt", LIST[:2] + ["# a remark"] + LIST[2:])
    lst("list_short.txt", LIST[:-1])
    lst("list_long.txt", LIST + ["1.5"])
    for name, bad in (("token", "1.5x"), ("zero", "0"), ("neg", "-1"), ("inf", "inf"), ("nan", "nan")):
        lst("list_%s.txt" % name, LIST[:2] + [bad] + LIST[3:])
    for k in ("err", "asym", "gv"):
        c, key = COL[k], SHARED[k]
        put(k + ".model", model(k))
        put(k + "_nohdr.model", model(k, head=False))
        put(k + "_nospace.model", model(k, shared_line="#%s 1.10000002" % key))
        for name, v in (("nan", "nan"), ("abc", "abc"), ("neg", "-1"), ("inf", "inf")):
            put("%s_shared_%s.model" % (k, name), model(k, shared_line="# %s %s" % (key, v)))
        put(k + "_shared_twice.model", model(k, shared_line="# %s 1.5\n# %s nan" % (key, key)))
        put(k + "_shared_bare.model", model(k, shared_line="# %s" % key))          # the key without a value
        put(k + "_noshared.model", model(k, shared_line=None))
        nan2 = {1: {c: "nan"}, 3: {c: "nan"}}
        if k == "asym":                                                            # a bin without a fit has both nan
            nan2 = {1: {4: "nan", 5: "nan"}, 3: {4: "nan", 5: "nan"}}
        put(k + "_nan2.model", model(k, edit=nan2))
        put(k + "_nan2_noshared.model", model(k, shared_line=None, edit=nan2))
        put(k + "_nan2_shared_twice.model", model(k, shared_line="# %s 1.5\n# %s nan" % (key, key), edit=nan2))
        put(k + "_neg.model", model(k, edit={2: {c: "-1"}}))
        put(k + "_word2.model", model(k, edit={2: {1: "mean"}}))
        put(k + "_fewfields.model", model(k, edit={3: c}))                        # one field too few for its own reader
        put(k + "_rows013.model", model(k, rows=[0, 1, 3]))
        put(k + "_short.model", model(k, rows=range(D - 1)))
        put(k + "_long.model", model(k, rows=range(D + 1)))
    put("empty.txt", "")
    put("blank.txt", "\n  \n\t\n")
    cases.extend((r, "missing.txt", VALUE[r]) for r in ("shape", "asym", "gv"))
    for name in ("list_exact.txt", "gv_noshared.model", "gv_shared_nan.model", "gv.model", "gv_nospace.model",
                 "gv_shared_twice.model", "err.model"):
        cases.append(("gv", name, "1"))                                            # shared: every bin takes shared_eta
    return files, cases


def write_corpus(where):
    files, cases = corpus()
    for name, text in files.items():
        with open(os.path.join(where, name), "w", newline="") as f:
            f.write(text)
    with open(os.path.join(where, "cases.list"), "w") as f:
        f.write("".join("%s %s %d %s\n" % (r, name, D, v) for r, name, v in cases))
    return os.path.join(where, "cases.list")


def test_the_readers_give_the_recorded_results_and_are_clean_under_asan_ubsan(tmp_path):
    exe = tmp_path / "binfile_main"
    probe = tmp_path / "probe.cc"
    probe.write_text("int main() { return 0; }\n")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(["g++", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        print("g++ cannot link the sanitizer runtimes here: binfile_main is built without them")
        san = []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I", HOST, *san,
                           os.path.join(ROOT, "tests", "binfile_main.cc"), "-o", str(exe)])
    where = tmp_path / "corpus"
    where.mkdir()
    cases = write_corpus(str(where))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe), str(where), cases], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    for bad in ("AddressSanitizer", "LeakSanitizer", "runtime error:"):
        assert bad not in r.stderr, r.stderr[-4000:]
    got, want = r.stdout.splitlines(), open(GOLDEN).read().splitlines()
    assert len(want) == len(corpus()[1]) and len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


if __name__ == "__main__":
    print(write_corpus(sys.argv[1]))
