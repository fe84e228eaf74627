#!/usr/bin/env python3
"""Randomised parity sweep of the product-quantisation ops (ops.pq_encode_rows / pq_tables / pq_adc_topk_tables / pq_adc_topk)
against the numpy restatement of tests/pq_cases.py: codes, tables, exponents, int32 values, float32 bits and indices must be
identical.  Every case draws (d, M), N, Q, k, a space and a row stride; encodes rows that sit on (duplicated) centroids, midway
between two, or hold NaN and infinities; builds the tables of queries scaled by 1e-20 .. 1e20 with a zero and a NaN query among
them; and searches uniform or tie-heavy codes with copied rows and junk in the bytes beyond M and beyond the code row.
Usage: python tools/fuzz_pq.py [cases] [seed]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import pq_cases as pc
from text_similarity_amd import ops

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
SHAPES = [(1, 1), (8, 1), (64, 1), (12, 3), (15, 15), (32, 16), (34, 17), (66, 33), (96, 48), (384, 48), (768, 48), (1024, 64), (1024, 16)]
bad = 0
t0 = time.time()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


for case in range(cases):
    d, M = SHAPES[int(rng.integers(len(SHAPES)))]
    Q = int(rng.choice([1, 3, 8, 9, 17, 33, 256, 259]))
    N = int(rng.choice([0, 1, 9, 255, 256, 257, 1023, 1025, 5000, 20000]))
    k = int(rng.choice([1, 10, 64, 65, 100, 1024]))
    space = "ip" if rng.random() < 0.5 else "l2"
    cb = pc.tied_codebooks(rng, d, M)
    w = pc.code_bytes(M)
    x = pc.encoder_rows(rng, int(rng.choice([1, 5, 300])), cb)
    ok = np.array_equal(ops.pq_encode_rows(dev(x), dev(cb)).cpu().numpy(), pc.encode_ref(x, cb))
    q = rng.standard_normal((Q, d)).astype(np.float32) * np.float32(10.0 ** rng.integers(-20, 21, size=(Q, 1)))
    if Q >= 3:
        q[1] = 0
        q[2, rng.integers(d)] = np.nan
    want_t, want_e = pc.tables_ref(q, cb, space)
    t, e = ops.pq_tables(dev(q), dev(cb), space)
    ok = ok and np.array_equal(t.cpu().numpy(), want_t) and np.array_equal(e.cpu().numpy(), want_e)
    codes = (pc.uniform_codes if rng.random() < 0.5 else pc.binary_codes)(rng, N, M)
    if N:
        codes[rng.choice(N, min(N, 50), replace=False)] = codes[0]              # ties
    stride = w * int(rng.choice([1, 2, 3]))
    junk = pc.pad_codes(codes, stride, junk_rng=rng)                            # junk beyond M and beyond the code row
    jc = dev(junk)[:, :w] if N else torch.zeros((0, w), dtype=torch.uint8, device="cuda")
    wv, wi = pc.adc_topk_ref(want_t, junk, k, space, idx_offset=7)
    gv, gi = ops.pq_adc_topk_tables(t, jc, k, space, idx_offset=7)
    ok = ok and np.array_equal(gv.cpu().numpy(), wv) and np.array_equal(gi.cpu().numpy(), wi)
    gs, gi2 = ops.pq_adc_topk(dev(q), dev(cb), jc, k, space, idx_offset=7)
    torch.cuda.synchronize()
    ok = ok and np.array_equal(gs.cpu().numpy().view(np.uint32), pc.values_to_float(wv, want_e, space).view(np.uint32))
    ok = ok and np.array_equal(gi2.cpu().numpy(), wi)
    bad += not ok
    print(f"case {case:3d} d={d:4d} M={M:2d} Q={Q:3d} N={N:6d} k={k:4d} {space} stride={stride:3d} {'ok' if ok else 'MISMATCH'}"
          f"  ({time.time() - t0:.0f} s)", flush=True)
print(f"fuzz_pq: {cases - bad}/{cases} cases exact")
sys.exit(1 if bad else 0)
