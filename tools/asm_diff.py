"""Which kernels of two `make asm` outputs (csrc/engine.gfx950.s of two commits) compile to the same code.

    python tools/asm_diff.py PARENT.s THIS.s

Per kernel (every .amdhsa_kernel symbol) the text between its label and its end label is compared line by line after
comments are dropped and the function-numbered local labels (.LBB<n>_k, .Ltmp<n>, ...) lose the number <n>, which only
counts the functions in front of it in the file.  Prints the counts and the demangled names of what differs, what is
gone and what is new.  Host only."""
import re
import subprocess
import sys


def kernels(path):
    txt = open(path).read()
    out = {}
    for n in set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", txt, re.M)):
        i = txt.index("\n" + n + ":")
        body = txt[i:txt.index(".Lfunc_end", i)]
        lines = [re.sub(r"\.L(BB|tmp|JTI|func_begin|func_end)\d+", r".L\1", l.split(";")[0].rstrip()) for l in body.splitlines()]
        out[n] = "\n".join(l for l in lines if l.strip())
    return out


def demangled(names):
    if not names:
        return []
    return subprocess.run(["c++filt"] + sorted(names), capture_output=True, text=True).stdout.split("\n")[:-1]


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    diff = [n for n in a if n in b and a[n] != b[n]]
    print("kernels: parent %d, this build %d" % (len(a), len(b)))
    print("identical instruction text: %d" % sum(1 for n in a if n in b and a[n] == b[n]))
    for title, names in (("different", diff), ("missing", [n for n in a if n not in b]), ("new", [n for n in b if n not in a])):
        print("%s: %d" % (title, len(names)))
        for n in demangled(names):
            print("    " + n)
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
