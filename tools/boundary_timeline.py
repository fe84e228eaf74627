#!/usr/bin/env python3
"""Per-dispatch timeline of the LayerNorm GEMM -> projection boundaries of the hidden-384 layer.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --steps 10 --warmup 2 --no-cpu-baseline
    python3 tools/boundary_timeline.py DIR [FIRST SECOND]

Reads the newest *kernel_trace.csv under DIR, orders the dispatches by their begin timestamp and, for every dispatch whose kernel
name contains FIRST (default ln_rows_gemm; ln_rows_xres2 for the fused form) with a later dispatch containing SECOND (default
gemm_xres2) before the next FIRST, prints: end of the first to begin of the second (the remainder launches of the LayerNorm GEMM
run in between), the time from the end of the last kernel in between to the begin of the second, and both durations.  One summary
line per (second kernel's template arguments), then the per-forward sum of every encoder kernel."""
import csv, glob, os, sys
from collections import defaultdict

d = sys.argv[1]
first = sys.argv[2] if len(sys.argv) > 2 else "ln_rows_gemm"
second = sys.argv[3] if len(sys.argv) > 3 else "gemm_xres2"
f = max(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
rows = []
with open(f, newline="") as fh:
    for r in csv.DictReader(fh):
        rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
rows.sort()


def short(n):
    n = n.replace("tsim::", "").replace("void ", "")
    return n.split("(")[0]


ENC = ("embed_ln", "gemm_xres2", "attention_kernel", "ln_rows", "ln_split", "ln_tail", "pool_packed")
pairs = defaultdict(list)   # (first, second) -> (gap_total, gap_last, dur_first, dur_between, dur_second)
i = 0
while i < len(rows):
    s0, e0, n0 = rows[i]
    if first in n0:
        j, between = i + 1, 0
        while j < len(rows) and any(k in rows[j][2] for k in ("ln_split", "ln_tail", "gemm_bf16")):
            between += rows[j][1] - rows[j][0]
            j += 1
        if j < len(rows) and second in rows[j][2] and first not in rows[j][2]:
            s1, e1, n1 = rows[j]
            pairs[(short(n0), short(n1))].append((s1 - e0, s1 - rows[j - 1][1], e0 - s0, between, e1 - s1))
    i += 1
print(f"# {os.path.basename(f)}: {len(rows)} dispatches; times in us, mean [min .. max] over the pairs")
for (a, b), v in sorted(pairs.items()):
    def col(k):
        x = [t[k] / 1e3 for t in v]
        return f"{sum(x) / len(x):7.2f} [{min(x):6.2f} .. {max(x):6.2f}]"
    print(f"{a} -> {b}: {len(v)} pairs")
    print(f"    first kernel            {col(2)}")
    print(f"    kernels in between      {col(3)}   (remainder launches of the LayerNorm GEMM)")
    print(f"    end first -> begin second {col(0)}")
    print(f"    end last  -> begin second {col(1)}")
    print(f"    second kernel           {col(4)}")
    x = [(t[2] + t[0] + t[4]) / 1e3 for t in v]
    print(f"    begin first -> end second {sum(x) / len(x):7.2f} [{min(x):6.2f} .. {max(x):6.2f}]")
# the encoder's kernels per forward: sums between consecutive embed_ln dispatches
fw, cur = [], None
for s, e, n in rows:
    if "embed_ln" in n:
        if cur:
            fw.append(cur)
        cur = defaultdict(float)
        t_begin = s
    if cur is not None and any(k in n for k in ENC):
        cur[short(n)] += (e - s) / 1e3
        cur["~span"] = (e - t_begin) / 1e3
if cur:
    fw.append(cur)
if fw:
    names = sorted({k for c in fw for k in c})
    print(f"# encoder kernels per forward, us (mean over {len(fw)} forwards); ~span = begin of embed_ln to end of the last encoder kernel")
    tot = 0.0
    for k in names:
        m = sum(c.get(k, 0.0) for c in fw) / len(fw)
        if k != "~span":
            tot += m
        print(f"    {m:9.2f}  {k}")
    print(f"    {tot:9.2f}  sum of kernel durations")
