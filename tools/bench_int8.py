#!/usr/bin/env python3
"""Timing of the int8-embedding ops on the GPU box: python tools/bench_int8.py [N] [d] [Q ...] [--k K ...] [--rescore M]
[--quantize] [--codes-only]

One line per (Q, k): ms per ops.int8_ip_topk call on int8 codes of N x d Gaussian rows, pairs per second and the rate at which
the code rows stream (one pass over the N x int8_bytes(d) bytes per group of queries: at most 16 while k <= 64, else 8).
--rescore M: also time ops.int8_rescore_topk of the k * M (<= 1024) candidates per query down to k, and the two calls together.
--quantize: time ops.quantize_int8_rows on the float32 corpus first.  --codes-only: draw the codes at random instead of
quantising float rows (a corpus whose float32 rows would not fit beside everything else; no --quantize, no --rescore)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from text_similarity_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("N", nargs="?", type=int, default=1_000_000)
ap.add_argument("d", nargs="?", type=int, default=384)
ap.add_argument("Q", nargs="*", type=int, default=[1, 16, 256, 4096])
ap.add_argument("--k", nargs="+", type=int, default=[10])
ap.add_argument("--rescore", type=int, default=0, metavar="M")
ap.add_argument("--quantize", action="store_true")
ap.add_argument("--codes-only", action="store_true")
a = ap.parse_args()
N, d = a.N, a.d
dev = "cuda:0"
g = torch.Generator(device=dev).manual_seed(4321)
cb = ops.int8_bytes(d)


def timed(run, iters, warm=2):
    for _ in range(warm):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


ranges = torch.tensor([[-4.0] * d, [4.0] * d], device=dev)      # Gaussian rows: +-4 sigma, the tails saturate
if a.codes_only:
    codes = torch.zeros((N, cb), dtype=torch.int8, device=dev)
    codes[:, :d] = torch.randint(-128, 128, (N, d), generator=g, device=dev, dtype=torch.int8)
else:
    step = 1 << 20      # (quantised in slices: the float32 rows of a large corpus never exist all at once)
    codes = torch.empty((N, cb), dtype=torch.int8, device=dev)
    for r0 in range(0, N, step):
        cf = torch.randn((min(step, N - r0), d), generator=g, device=dev)
        ops.quantize_int8_rows(cf, ranges, out=codes[r0:r0 + cf.shape[0]])
    if a.quantize:
        ms = timed(lambda: ops.quantize_int8_rows(cf, ranges), 5)
        print(json.dumps({"quantize": True, "rows": cf.shape[0], "d": d, "ms": round(ms, 4),
                          "read_GBs": round(cf.shape[0] * d * 4 / ms / 1e6, 1)}), flush=True)
    del cf
for Q, k in [(Q, k) for Q in a.Q for k in a.k]:
    qf = torch.randn((Q, d), generator=g, device=dev)
    qc = ops.quantize_int8_rows(qf, ranges)
    iters = 5 if Q <= 4096 else 2
    ms = timed(lambda: ops.int8_ip_topk(qc, codes, d, k), iters)
    G = max(1, min(16 if k <= 64 else 8, -(-Q // (2 if cb > 512 else 4))))      # csrc/int8_search.h i8_group
    rec = {"score": "int8_ip", "Q": Q, "N": N, "d": d, "k": k, "ms": round(ms, 4), "Gpairs_s": round(Q * N / ms / 1e6, 1),
           "stream_GBs": round(-(-Q // G) * N * cb / ms / 1e6, 1)}
    if a.rescore and not a.codes_only:
        m = min(k * a.rescore, ops.MAX_K, N)
        cand = ops.int8_ip_topk(qc, codes, d, m)[1]
        rec["m"] = m
        rec["ms_rescore"] = round(timed(lambda: ops.int8_rescore_topk(qf, codes, d, cand, k), iters), 4)
        rec["ms_both"] = round(timed(lambda: ops.int8_rescore_topk(qf, codes, d, ops.int8_ip_topk(qc, codes, d, m)[1], k), iters), 4)
    print(json.dumps(rec), flush=True)
