#!/usr/bin/env python3
"""Instruction histogram of compiled kernels, from the `make asm` output (csrc/engine.gfx950.s).  CPU only.

    python tools/isa_count.py [ASM] [PATTERN]

ASM defaults to <package>/csrc/engine.gfx950.s; PATTERN is a regular expression matched against the demangled
kernel name (the mangled one when no demangler is on the PATH) and defaults to the hot kernels of a training step.
Per kernel it prints
  * the instructions in front of the first buffer_load (text order) and how many of them are `s_waitcnt lgkmcnt(0)`
    -- the kernel-argument round trips a wave pays before its first memory access;
  * the SGPR / VGPR spill counts of the kernel's metadata;
  * for the largest loop (the backward branch that spans the most instructions) the instruction counts by class.
Classes are recognised by prefix only: v_mfma, other v_, s_waitcnt, other s_, ds_, buffer_ / global_; lane
moves (v_readlane / v_writelane) are listed as a part of "other v_".  A histogram, nothing more.
"""
import os
import re
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "speech-enhancement-based-on-a-maximum-likelihood-criterion_amd"
DEFAULT_ASM = os.path.join(ROOT, PKG, "csrc", "engine.gfx950.s")
DEFAULT_PATTERN = r"^void k_(fwd|dx|dwp|dwp_bias|fwd64|dx64)<"
CLASSES = ("v_mfma", "v_other", "s_waitcnt", "s_other", "ds_", "buffer_/global_", "other")


def classify(op):
    if op.startswith("v_mfma"):
        return "v_mfma"
    if op.startswith("v_"):
        return "v_other"
    if op.startswith("s_waitcnt"):
        return "s_waitcnt"
    if op.startswith("s_"):
        return "s_other"
    if op.startswith("ds_"):
        return "ds_"
    if op.startswith("buffer_") or op.startswith("global_"):
        return "buffer_/global_"
    return "other"


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return dict((n, n) for n in names)
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.splitlines()))


def kernels(path):
    """-> ({mangled name: [(label or None, instruction text)]}, {mangled name: {metadata key: int}})"""
    with open(path) as f:
        lines = f.read().splitlines()
    names = set(m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m)
    body, cur = {}, None
    for ln in lines:
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", ln)
        if m and m.group(1) in names:
            cur = body.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", ln):
            cur = None
            continue
        if m:
            cur.append((m.group(1), None))
            continue
        text = ln.split(";", 1)[0].strip()
        if text and not text.startswith("."):
            cur.append((None, text))
    meta, name = {}, None
    for ln in lines:
        m = re.match(r"\s*\.name:\s+(\S+)", ln)
        if m:
            name = m.group(1)
        m = re.match(r"\s*\.(sgpr_spill_count|vgpr_spill_count|sgpr_count|vgpr_count|agpr_count):\s+(\d+)", ln)
        if m and name in names:
            meta.setdefault(name, {})[m.group(1)] = int(m.group(2))
    return body, meta


def report(name, shown, items, meta, out):
    ins = [(i, t) for i, (lab, t) in enumerate(items) if t is not None]
    first = next((k for k, (_, t) in enumerate(ins) if t.startswith("buffer_load")), len(ins))
    waits = sum(1 for _, t in ins[:first] if t.startswith("s_waitcnt") and "lgkmcnt(0)" in t)
    out.write("%s\n" % shown)
    out.write("  before the first buffer_load: %d instructions, %d lgkmcnt(0) waits\n" % (first, waits))
    out.write("  spills: sgpr %d, vgpr %d   registers: sgpr %d, vgpr %d, agpr %d\n" % tuple(
        meta.get(k, -1) for k in ("sgpr_spill_count", "vgpr_spill_count", "sgpr_count", "vgpr_count", "agpr_count")))
    label_at = dict((lab, i) for i, (lab, t) in enumerate(items) if lab is not None)
    best = None  # (instructions, first item, last item)
    for i, t in ins:
        op = t.split()[0]
        if op.startswith("s_cbranch") or op == "s_branch":
            tgt = label_at.get(t.split()[-1])
            if tgt is not None and tgt < i:
                n = sum(1 for j, _ in ins if tgt < j <= i)
                if best is None or n > best[0]:
                    best = (n, tgt, i)
    if best is None:
        out.write("  no loop\n\n")
        return
    counts = dict((c, 0) for c in CLASSES)
    lanes = 0
    for j, t in ins:
        if best[1] < j <= best[2]:
            op = t.split()[0]
            counts[classify(op)] += 1
            lanes += op.startswith("v_readlane") or op.startswith("v_writelane")
    out.write("  largest loop (%s): %d instructions\n" % (items[best[1]][0], best[0]))
    for c in CLASSES:
        if counts[c] or c != "other":
            out.write("    %-16s %5d%s\n" % (c, counts[c], "   (v_readlane / v_writelane: %d)" % lanes if c == "v_other" else ""))
    out.write("\n")


def main(argv):
    path = argv[1] if len(argv) > 1 else DEFAULT_ASM
    pattern = re.compile(argv[2] if len(argv) > 2 else DEFAULT_PATTERN)
    if not os.path.exists(path):
        sys.exit("%s is missing: run `make asm` in the package's csrc/ first" % path)
    body, meta = kernels(path)
    shown = demangle(sorted(body))
    hits = sorted((shown[n], n) for n in body if pattern.search(shown[n]))
    if not hits:
        sys.exit("no kernel matches %r" % pattern.pattern)
    for s, n in hits:
        report(n, s, body[n], meta.get(n, {}), sys.stdout)


if __name__ == "__main__":
    main(sys.argv)
