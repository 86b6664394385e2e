"""Which kernels of two `make asm` outputs (csrc/engine.gfx950.s of two commits) compile to the same code.

    python tools/asm_diff.py PARENT.s THIS.s

Per kernel (every .amdhsa_kernel symbol) the text between its label and its end label is compared line by line after
comments are dropped and the function-numbered local labels (.LBB<n>_k, .Ltmp<n>, ...) lose the number <n>, which only
counts the functions in front of it in the file.  Prints the counts and the demangled names of what differs, what is
gone and what is new.  For every kernel that differs it then prints what a mere reordering leaves alone: the instruction
total, the opcode multiset (with the opcodes whose counts moved), and the kernel's metadata -- spills, register counts,
LDS and scratch sizes.  Host only."""
import collections
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


META = ("sgpr_spill_count", "vgpr_spill_count", "sgpr_count", "vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def metadata(path):
    """{mangled name: {key of META: int}} from the .amdgpu_metadata note (LDS = group, scratch = private segment)"""
    out = {}
    txt = open(path).read()
    for entry in re.split(r"^  - ", txt[txt.index("amdhsa.kernels:"):], flags=re.M)[1:]:  # one list item per kernel
        name = re.search(r"^    \.name:\s+(\S+)", entry, re.M)
        if name:  # the note's other lists (printf formats) have no such key
            out[name.group(1)] = dict((k, int(v)) for k, v in re.findall(r"^\s*\.(%s):\s+(\d+)" % "|".join(META), entry, re.M))
    return out


def opcodes(text):
    """Counter of the opcodes of a kernel's text as kernels() returns it (labels and directives dropped)"""
    ins = [l.split()[0] for l in text.splitlines() if not l.rstrip().endswith(":") and not l.strip().startswith(".")]
    return collections.Counter(ins)


def compare(shown, pa, pb, ma, mb):
    """what a reordering leaves alone: instruction total, opcode multiset, registers, spills, LDS and scratch"""
    ca, cb = opcodes(pa), opcodes(pb)
    la, lb = pa.splitlines(), pb.splitlines()
    moved = sum(1 for x, y in zip(la, lb) if x != y) + abs(len(la) - len(lb))
    print("    " + shown)
    print("        instructions %d -> %d, opcode multiset %s, lines that differ in place: %d"
          % (sum(ca.values()), sum(cb.values()), "same" if ca == cb else "DIFFERENT", moved))
    for op in sorted(set(ca) | set(cb)):
        if ca[op] != cb[op]:
            print("            %-28s %d -> %d" % (op, ca[op], cb[op]))
    print("        metadata %s: %s" % ("same" if ma == mb else "DIFFERENT",
                                      ", ".join("%s %s" % (k, ma.get(k) if ma.get(k) == mb.get(k) else "%s -> %s" % (ma.get(k), mb.get(k)))
                                                for k in META)))
    return ca == cb and ma == mb


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    diff = sorted(n for n in a if n in b and a[n] != b[n])
    print("kernels: parent %d, this build %d" % (len(a), len(b)))
    print("identical instruction text: %d" % sum(1 for n in a if n in b and a[n] == b[n]))
    for title, names in (("different", diff), ("missing", [n for n in a if n not in b]), ("new", [n for n in b if n not in a])):
        print("%s: %d" % (title, len(names)))
        for n in demangled(names):
            print("    " + n)
    if diff:
        ma, mb = metadata(sys.argv[1]), metadata(sys.argv[2])
        print("the different kernels, parent -> this build:")
        same = [compare(s, a[n], b[n], ma.get(n, {}), mb.get(n, {})) for n, s in zip(diff, demangled(diff))]
        print("reordered only (same opcode multiset and metadata): %d of %d" % (sum(same), len(diff)))
    return 1 if diff else 0


if __name__ == "__main__":
    sys.exit(main())
