#!/usr/bin/env python3
"""Randomised parity sweep of the IVF-PQ ops against the restatement in tests/ivfpq_cases.py: everything must be identical.
A scan case draws a space, M, Q, nlist, nprobe, k, the list lengths (around the 256-row step and TSIM_IVFPQ_SEG), ids with
tombstones, probes with padding, repeats and list numbers beyond nlist, one table a query or a pair, a bias or none, a sizing
hint that may be far too small, a row stride with junk pad bytes and now and then list offsets that are out of order
(ops.ivfpq_scan_topk: values, ids and status words).  A tables case draws a space, (d, M), magnitudes from 1e-15 to 1e15,
centroids up to 100 times the codebook entries, padding probes and zero, NaN, infinite and overflowing queries
(ops.ivfpq_tables: tables of the valid pairs, biases and exponents).
Usage: python tools/fuzz_ivfpq.py [cases] [seed]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import ivfpq_cases as ic
import pq_cases as pc
from text_similarity_amd import ops

SEG = ic.header_seg()
cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
bad = 0
t0 = time.time()
for case in range(cases):
    space = str(rng.choice(["ip", "l2"]))
    Q = int(rng.choice([1, 3, 17, 40]))
    nlist = int(rng.choice([1, 2, 7, 40]))
    nprobe = int(rng.choice([1, 2, 5, 12]))
    probes = rng.integers(0, nlist, (Q, nprobe))
    junk = rng.random((Q, nprobe))
    probes[junk < 0.1] = -1
    probes[junk > 0.95] = nlist + int(rng.integers(0, 3))
    probes = probes.astype(np.int64)
    if case % 2 == 0:      # ------------------------------------------------------------------ the scan
        M = int(rng.choice([1, 7, 16, 17, 32, 33, 48, 64]))
        k = int(rng.choice([1, 10, 64, 65, 100, 1024]))
        lens = rng.choice([0, 1, 255, 256, 257, 700, SEG - 1, SEG, SEG + 1, 2 * SEG + 1], nlist, p=[.15, .1, .1, .1, .1, .2, .07, .06, .06, .06])
        if lens.sum() == 0:
            lens[0] = 5
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        N = int(off[-1])
        kind = str(rng.choice(["random", "small", "one_hot", "badoff"]))
        if kind == "badoff" and nlist > 1:
            j = rng.choice(nlist + 1, 2)
            off[j[0]], off[j[1]] = int(rng.choice([-3, N + 9, off[j[1]]])), off[j[0]]
        raw = pc.binary_codes(rng, N, M) if kind == "small" else pc.uniform_codes(rng, N, M)
        stride = pc.code_bytes(M) + 16 * int(rng.integers(0, 3))
        codes = pc.pad_codes(raw, stride=stride, junk_rng=rng)
        ids = rng.permutation(N).astype(np.int32)
        ids[rng.random(N) < 0.1] *= -1          # tombstones (id 0 stays live)
        per_pair = bool(rng.integers(0, 2))
        n = Q * nprobe if per_pair else Q
        t = {"small": pc.small_tables(rng, n, M, space), "one_hot": pc.one_hot_tables(n, M, space)}.get(kind)
        if t is None:
            t = pc.random_tables(rng, n, M, space) // 2
        t = t.reshape(Q, nprobe, M, 256) if per_pair else t
        hi = 3 if kind in ("small", "one_hot") else 1 << 22
        b = rng.integers(-hi, hi + 1, size=(Q, nprobe))
        b = None if rng.random() < 0.3 else (-np.abs(b) if space == "l2" else b).astype(np.int32)
        hint = None if rng.random() < 0.3 else int(rng.choice([0, 1, SEG, int(lens.max()), 10 ** 7]))
        wv, wi, wst = ic.scan_ref(t, b, codes, off, ids, probes, k, space, idx_offset=11)
        v, i, st = ops.ivfpq_scan_topk(space, dev(t), None if b is None else dev(b), dev(codes)[:, :pc.code_bytes(M)], dev(off), dev(ids),
                                       dev(probes), k, idx_offset=11, return_status=True, max_list_len=hint)
        torch.cuda.synchronize()
        ok = np.array_equal(v.cpu().numpy(), wv) and np.array_equal(i.cpu().numpy(), wi) and np.array_equal(st.cpu().numpy(), wst)
        what = f"scan   {space} M={M:2d} Q={Q:2d} nlist={nlist:2d} nprobe={nprobe:2d} k={k:4d} N={N:6d} hint={hint!s:8s} {kind:7s} pair={int(per_pair)}"
    else:                  # ------------------------------------------------------------------ the tables
        d, M = pc.SHAPES[int(rng.integers(0, len(pc.SHAPES)))]
        scale = float(rng.choice([1e-15, 1e-3, 1.0, 1e6, 1e15]))
        cscale = float(rng.choice([0.01, 1.0, 3.0, 100.0]))
        cb = pc.random_codebooks(rng, d, M, scale)
        cent = (rng.standard_normal((nlist, d)) * cscale * scale).astype(np.float32)
        q = (rng.standard_normal((Q, d)) * scale).astype(np.float32)
        for a in range(Q):
            kind = rng.random()
            if kind < 0.08:
                q[a] = 0
            elif kind < 0.16:
                q[a, rng.integers(0, d)] = rng.choice([np.nan, np.inf, -np.inf])
            elif kind < 0.24:                   # finite, but the residual to one centroid overflows
                i = int(rng.integers(0, d))
                q[a, i], cent[int(rng.integers(0, nlist)), i] = 3e38, -3e38
        t, b, e = ops.ivfpq_tables(dev(q), dev(cent), dev(probes), dev(cb), space)
        torch.cuda.synchronize()
        if space == "ip":
            wt, wb, we = ic.tables_ip_ref(q, cent, probes, cb)
            ok = np.array_equal(t.cpu().numpy(), wt) and np.array_equal(b.cpu().numpy(), wb)
            ok = ok and bool((ic.score_bound(wt, wb) < 2 ** 24).all())
        else:
            wt, we = ic.tables_l2_ref(q, cent, probes, cb)
            valid = ic.valid_probes(probes, nlist)
            ok = np.array_equal(t.cpu().numpy()[valid], wt[valid]) and bool((ic.score_bound(wt) < 2 ** 24).all())
        ok = ok and np.array_equal(e.cpu().numpy(), we)
        what = f"tables {space} d={d:4d} M={M:2d} Q={Q:2d} nlist={nlist:2d} nprobe={nprobe:2d} scale={scale:g} cscale={cscale:g}"
    bad += not ok
    print(f"case {case:3d} {what} {'ok' if ok else 'MISMATCH'}  ({time.time() - t0:.0f} s)", flush=True)
print(f"fuzz_ivfpq: {cases - bad}/{cases} cases exact")
sys.exit(1 if bad else 0)
