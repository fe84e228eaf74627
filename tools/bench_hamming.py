#!/usr/bin/env python3
"""Timing of the binary-embedding ops on the GPU box: python tools/bench_hamming.py [N] [d] [Q ...] [--k K ...] [--rescore M]
[--pack] [--codes-only]

One line per (Q, k): ms per ops.hamming_topk call on sign-bit codes of N x d Gaussian rows, pairs per second and the rate at which
the code rows stream (one pass over the N x code_bytes(d) bytes per group of min(8, ceil(Q / 4)) queries).  --rescore M: also time
ops.sign_rescore_topk of the k * M (<= 1024) Hamming candidates per query down to k, and the two calls together.  --pack: time
ops.pack_sign_rows on the N x d float32 corpus first.  --codes-only: draw the codes at random instead of packing float rows (a
corpus whose float32 rows would not fit beside everything else; no --pack, no --rescore)."""
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
ap.add_argument("--pack", action="store_true")
ap.add_argument("--codes-only", action="store_true")
a = ap.parse_args()
N, d = a.N, a.d
dev = "cuda:0"
g = torch.Generator(device=dev).manual_seed(4321)
cb = ops.code_bytes(d)


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


def random_codes(rows):
    c = torch.randint(0, 256, (rows, cb), generator=g, device=dev, dtype=torch.uint8)
    return ops.codes_from_packbits(c[:, :(d + 7) // 8].contiguous(), d)


if a.codes_only:
    codes = random_codes(N)
else:
    step = 1 << 20      # (packed in slices: the float32 rows of a large corpus never exist all at once)
    codes = torch.empty((N, cb), dtype=torch.uint8, device=dev)
    for r0 in range(0, N, step):
        cf = torch.randn((min(step, N - r0), d), generator=g, device=dev)
        codes[r0:r0 + cf.shape[0]] = ops.pack_sign_rows(cf)
    if a.pack:
        ms = timed(lambda: ops.pack_sign_rows(cf), 5)
        print(json.dumps({"pack": True, "rows": cf.shape[0], "d": d, "ms": round(ms, 4),
                          "read_GBs": round(cf.shape[0] * d * 4 / ms / 1e6, 1)}), flush=True)
    del cf
for Q, k in [(Q, k) for Q in a.Q for k in a.k]:
    qf = torch.randn((Q, d), generator=g, device=dev)
    qc = ops.pack_sign_rows(qf)
    iters = 5 if Q <= 4096 else 2
    ms = timed(lambda: ops.hamming_topk(qc, codes, d, k), iters)
    rec = {"score": "hamming", "Q": Q, "N": N, "d": d, "k": k, "ms": round(ms, 4), "Gpairs_s": round(Q * N / ms / 1e6, 1),
           "stream_GBs": round(-(-Q // min(8, -(-Q // 4))) * N * cb / ms / 1e6, 1)}
    if a.rescore and not a.codes_only:
        m = min(k * a.rescore, ops.MAX_K, N)
        cand = ops.hamming_topk(qc, codes, d, m)[1]
        rec["m"] = m
        rec["ms_rescore"] = round(timed(lambda: ops.sign_rescore_topk(qf, codes, d, cand, k), iters), 4)
        rec["ms_both"] = round(timed(lambda: ops.sign_rescore_topk(qf, codes, d, ops.hamming_topk(qc, codes, d, m)[1], k), iters), 4)
    print(json.dumps(rec), flush=True)
