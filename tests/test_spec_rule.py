"""CPU: the host-only layout rule of the spectral front end (csrc/spec_rule.h: the rate table, the frame count, the
tables of a packed batch, the window / score-frame checks, the compaction and the span of a decode chunk) under
AddressSanitizer + UBSan, as a stand-alone program: tests/spec_rule_main.cc, in the manner of
tests/test_live_sanitizers.py.  Any report fails.  Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "speech-enhancement-based-on-a-maximum-likelihood-criterion_amd", "csrc")


def test_spec_rule_is_right_and_clean_under_asan_ubsan(tmp_path):
    exe = tmp_path / "spec_rule_main"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Werror", "-I", CSRC,
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "spec_rule_main.cc"), "-o", str(exe)])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "spec_rule_main OK" in r.stdout
    for bad in ("AddressSanitizer", "LeakSanitizer", "runtime error:"):
        assert bad not in r.stderr, r.stderr[-4000:]
