#!/usr/bin/env python3
"""Randomised parity sweep of the binary-embedding ops (ops.pack_sign_rows / hamming_topk / sign_rescore_topk) against the numpy
restatement of tests/hamming_cases.py: codes, distances, scores (float32 bits), indices and status words must be identical.
Every case draws a width, Q, N, k and a re-score list length, seeds the rows with zeros, NaN, infinities and subnormals, copies
rows (ties), writes junk into the bits beyond d and the bytes beyond the code, and sprinkles padding, repeats and rows beyond
the corpus into the candidate lists.
Usage: python tools/fuzz_hamming.py [cases] [seed]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import hamming_cases as hc
from text_similarity_amd import ops

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
bad = 0
t0 = time.time()
for case in range(cases):
    d = int(rng.choice([1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 300, 384, 768, 1000, 1023, 1024]))
    Q = int(rng.choice([1, 3, 8, 9, 33]))
    N = int(rng.choice([1, 9, 1023, 1024, 1025, 5000, 20000]))
    k = int(rng.choice([1, 10, 64, 65, 100, 1024]))
    m = int(rng.choice([1, k, 100, 1025, 2500]))
    c = hc.special_rows(N, d, seed=int(rng.integers(1 << 30)))
    q = hc.random_rows(rng, Q, d)
    c[rng.choice(N, min(N, 50), replace=False)] = c[0]                       # ties
    cb = hc.code_bytes(d)
    want_c = hc.pack_ref(c)
    got_c = ops.pack_sign_rows(torch.from_numpy(c).cuda())
    qc = ops.pack_sign_rows(torch.from_numpy(q).cuda())
    ok = np.array_equal(got_c.cpu().numpy(), want_c) and np.array_equal(qc.cpu().numpy(), hc.pack_ref(q))
    junk = np.full((N, cb + 32), 0x5A, np.uint8)                             # wider rows, junk beyond d
    junk[:, :cb] = want_c
    if d % 8:
        junk[:, (d + 7) // 8 - 1] |= np.uint8(0xFF >> (d % 8))
    junk[:, (d + 7) // 8:cb] = 0xC3
    jc = torch.from_numpy(junk).cuda()[:, :cb]
    wd, wi = hc.hamming_topk_ref(hc.pack_ref(q), want_c, d, k, idx_offset=7)
    gd, gi = ops.hamming_topk(qc, jc, d, k, idx_offset=7)
    ok = ok and np.array_equal(gd.cpu().numpy(), wd) and np.array_equal(gi.cpu().numpy(), wi)
    cand = rng.integers(0, N, (Q, m)).astype(np.int64)
    cand[rng.random((Q, m)) < 0.05] = -1
    cand[rng.random((Q, m)) < 0.01] = N + 2
    ws, wsi, wst = hc.rescore_ref(q, want_c, d, cand, k, idx_offset=7)
    gs, gsi, gst = ops.sign_rescore_topk(torch.from_numpy(q).cuda(), jc, d, torch.from_numpy(cand).cuda(), k, idx_offset=7,
                                         return_status=True)
    torch.cuda.synchronize()
    ok = ok and np.array_equal(gs.cpu().numpy().view(np.uint32), ws.view(np.uint32)) and np.array_equal(gsi.cpu().numpy(), wsi)
    ok = ok and np.array_equal(gst.cpu().numpy(), wst)
    bad += not ok
    print(f"case {case:3d} d={d:4d} Q={Q:3d} N={N:6d} k={k:4d} m={m:5d} {'ok' if ok else 'MISMATCH'}  ({time.time() - t0:.0f} s)", flush=True)
print(f"fuzz_hamming: {cases - bad}/{cases} cases exact")
sys.exit(1 if bad else 0)
