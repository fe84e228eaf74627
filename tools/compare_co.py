#!/usr/bin/env python3
"""Compare two disassemblies written by tools/extract_co.py kernel by kernel: python tools/compare_co.py parent.s branch.s
A kernel is identical when its instruction text (addresses and encodings dropped, trailing s_nop / s_code_end padding ignored) is
the same in both.  Prints the kernels of the first file that differ or are missing in the second, and the kernels only the
second has with their instruction and v_fma_f64 counts; exits 1 when a kernel of the first file moved."""
import re
import sys


def load(path):
    out, name = {}, None
    for ln in open(path):
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln.strip())
        if m:
            name = m.group(1)
            out[name] = []
        elif name and ln.strip():
            out[name].append(ln.split("//")[0].strip())
    for body in out.values():      # the padding between functions depends on what follows
        while body and body[-1].split()[0] in ("s_nop", "s_code_end"):
            body.pop()
    return out


a, b = load(sys.argv[1]), load(sys.argv[2])
moved = [k for k in a if a[k] != b.get(k)]
for k in moved:
    print("MISSING" if k not in b else "DIFFERENT", k, len(a[k]), len(b.get(k, [])))
print(f"{len(a)} kernels in {sys.argv[1]}: {len(a) - len(moved)} identical in {sys.argv[2]}, {len(moved)} moved")
for k in sorted(set(b) - set(a)):
    print("NEW", k, len(b[k]), "instructions,", sum("v_fma_f64" in i for i in b[k]), "v_fma_f64")
sys.exit(1 if moved else 0)
