#!/usr/bin/env python3
"""Compare the functions of two sets of `hipcc --cuda-device-only -S` outputs, symbol by symbol.

    kernel_isa_diff.py OLD.s[,OLD2.s...] NEW.s[,NEW2.s...]

(the .s files: sigtk_amd/build.py's HIPCC_FLAGS without -shared, plus --cuda-device-only -S, one per .hip unit)

A function = the text from its `<sym>:` label to `.Lfunc_endN:` (kernels and out-of-line device functions alike) plus,
for a kernel, its .amdhsa_kernel block; local labels are renumbered by order of appearance, comments dropped.
Class A: same text and block.  B: same block, same multiset of mnemonics (reordered / registers renamed).
C: same block, other instructions (the differing mnemonic counts are printed).  X: the block differs."""
import collections
import re
import sys


def functions(paths):
    out = {}
    for path in paths.split(","):
        txt = open(path).read()
        for m in re.finditer(r"^\t\.type\t(\S+),@function\n\1:.*\n((?:.*\n)*?)^\.Lfunc_end\d+:", txt, re.M):
            name, body = m.group(1), m.group(2)
            ids = {}
            body = re.sub(r"\.L(BB|JTI|tmp)\d+_?\d*", lambda k: ids.setdefault(k.group(0), ".L%d" % len(ids)), body)
            lines = [l.split(";")[0].rstrip() for l in body.split("\n")]
            k = re.search(r"^\t\.amdhsa_kernel %s\n((?:.*\n)*?)^\t\.end_amdhsa_kernel" % re.escape(name), txt, re.M)
            out[name] = ([l for l in lines if l.strip()], k.group(1) if k else "")
    return out


def mnemonics(lines):
    return collections.Counter(l.split()[0] for l in lines if l.startswith("\t") and not l.lstrip().startswith("."))


a, b = functions(sys.argv[1]), functions(sys.argv[2])
print(len(a), "functions in", sys.argv[1], ";", len(b), "in", sys.argv[2])
for n in sorted(set(a) | set(b)):
    if n not in a or n not in b:
        print("ONLY IN %s  %s" % ("OLD" if n in a else "NEW", n))
        continue
    ma, mb = mnemonics(a[n][0]), mnemonics(b[n][0])
    cls = "X" if a[n][1] != b[n][1] else "A" if a[n][0] == b[n][0] else "B" if ma == mb else "C"
    changed = sum(1 for x, y in zip(a[n][0], b[n][0]) if x != y) + abs(len(a[n][0]) - len(b[n][0]))
    print("%s %6d instr %6d lines differ  %s" % (cls, sum(mb.values()), changed, n))
    if cls == "C":
        print("    ", {k: mb[k] - ma[k] for k in sorted(set(ma) | set(mb)) if ma[k] != mb[k]})
