#!/usr/bin/env python3
"""Randomised parity sweep of the int8-embedding ops (ops.quantize_int8_rows / int8_ip_topk / int8_rescore_topk) against the numpy
restatement of tests/int8_cases.py: codes, scores (int32, and float32 bits), indices and status words must be identical.
Every case draws a width, Q, N, k and a re-score list length, quantises rows seeded with out-of-range values, range ends, integer
boundaries, NaN, infinities and a constant column, searches uniform or tie-heavy codes with copied rows, junk in the bytes
beyond d and beyond the code row, and sprinkles padding, repeats and rows beyond the corpus into the candidate lists.
Usage: python tools/fuzz_int8.py [cases] [seed]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import int8_cases as ic
from text_similarity_amd import ops

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
bad = 0
t0 = time.time()
for case in range(cases):
    d = int(rng.choice([1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 300, 384, 768, 1000, 1023, 1024]))
    Q = int(rng.choice([1, 3, 8, 9, 17, 33, 70]))
    N = int(rng.choice([1, 9, 1023, 1024, 1025, 5000, 20000]))
    k = int(rng.choice([1, 10, 64, 65, 100, 1024]))
    m = int(rng.choice([1, k, 100, 1025, 2500]))
    x, ranges = ic.quantiser_rows(int(rng.choice([1, 5, 300])), d, seed=int(rng.integers(1 << 30)))
    got = ops.quantize_int8_rows(torch.from_numpy(x).cuda(), torch.from_numpy(ranges).cuda())
    ok = np.array_equal(got.cpu().numpy(), ic.quantize_ref(x, ranges))
    make = ic.uniform_codes if rng.random() < 0.5 else ic.ternary_codes
    qc, cc = make(rng, Q, d), make(rng, N, d)
    cc[rng.choice(N, min(N, 50), replace=False)] = cc[0]                     # ties
    cb = ic.int8_bytes(d)
    junk = np.full((N, cb + 32), 0x5A, np.int8)                              # wider rows, junk beyond d
    junk[:, :d] = cc[:, :d]
    jq = qc.copy()
    jq[:, d:] = -0x3D
    jc = torch.from_numpy(junk).cuda()[:, :cb]
    ws, wi = ic.ip_topk_ref(qc, cc, d, k, idx_offset=7)
    gs, gi = ops.int8_ip_topk(torch.from_numpy(jq).cuda(), jc, d, k, idx_offset=7)
    ok = ok and np.array_equal(gs.cpu().numpy(), ws) and np.array_equal(gi.cpu().numpy(), wi)
    q = ic.random_rows(rng, Q, d)
    cand = rng.integers(0, N, (Q, m)).astype(np.int64)
    cand[rng.random((Q, m)) < 0.05] = -1
    cand[rng.random((Q, m)) < 0.01] = N + 2
    wf, wfi, wst = ic.rescore_ref(q, cc, d, cand, k, idx_offset=7)
    gf, gfi, gst = ops.int8_rescore_topk(torch.from_numpy(q).cuda(), jc, d, torch.from_numpy(cand).cuda(), k, idx_offset=7,
                                         return_status=True)
    torch.cuda.synchronize()
    ok = ok and np.array_equal(gf.cpu().numpy().view(np.uint32), wf.view(np.uint32)) and np.array_equal(gfi.cpu().numpy(), wfi)
    ok = ok and np.array_equal(gst.cpu().numpy(), wst)
    bad += not ok
    print(f"case {case:3d} d={d:4d} Q={Q:3d} N={N:6d} k={k:4d} m={m:5d} {'ok' if ok else 'MISMATCH'}  ({time.time() - t0:.0f} s)", flush=True)
print(f"fuzz_int8: {cases - bad}/{cases} cases exact")
sys.exit(1 if bad else 0)
