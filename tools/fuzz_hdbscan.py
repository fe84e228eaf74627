#!/usr/bin/env python3
"""Randomised parity sweep of HDBSCAN (ops.mst_prim, ops.hdbscan) against the restatement of tests/hdbscan_cases.py: the edges
(from, to, and the float32 bits of w2), the core distances and the labels must be identical.  Every case draws a size (around
the wave's 64 and the workgroup's 256 rows), a width, a row stride, min_cluster_size and min_samples, a metric, and a kind of
data: blobs with noise, plain Gaussian rows, an integer grid, groups of identical rows, rows of large norm.
Usage: python tools/fuzz_hdbscan.py [cases] [seed]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import hdbscan_cases as hc
from list_cases import same_bits
from text_similarity_amd import ops

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
bad = 0
t0 = time.time()
for case in range(cases):
    n = int(rng.choice([1, 2, 5, 63, 64, 65, 200, 255, 256, 257, 400, 700]))
    d = int(rng.choice([1, 2, 16, 63, 64, 65, 300, 384, 385, 767]))
    pad = int(rng.choice([0, 0, 1, 5]))
    kind = str(rng.choice(["blobs", "gauss", "grid", "dups", "large"]))
    metric = str(rng.choice(["euclidean", "euclidean", "cosine"]))
    mcs = int(rng.choice([2, 3, 5, 15, 40]))
    ms = int(min(n, rng.choice([1, 2, 5, 15, 70])))
    if kind == "blobs":
        x = hc.blobs(n, d, int(rng.integers(1, 6)), int(rng.integers(1 << 30)), centre_scale=float(rng.choice([1.2, 4.0])))
    elif kind == "grid":
        x = rng.integers(0, 4, size=(n, d)).astype(np.float32)
    elif kind == "dups":
        x = np.repeat(rng.standard_normal((-(-n // 9), d)), 9, axis=0)[rng.permutation(-(-n // 9) * 9)[:n]].astype(np.float32)
    else:
        x = (rng.standard_normal((n, d)) * (1e4 if kind == "large" else 1.0)).astype(np.float32)
    buf = torch.full((n, d + pad), float("nan"), dtype=torch.float32, device="cuda:0")
    buf[:, :d] = torch.from_numpy(x).cuda()
    view = buf[:, :d]
    # the tree alone, on the strided view, with and without core distances
    core2 = hc.core2_ref(x, ms)
    ok = True
    for c in (None, core2):
        got = ops.mst_prim(view, None if c is None else torch.from_numpy(c).cuda())
        want = hc.mst_ref(x, c)
        ok &= all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(got[:2], want[:2])) and same_bits(got[2].cpu().numpy(), want[2])
    # the whole pipeline (cosine: the restatement runs on the unit rows the device made; a zero row is its own unit row)
    rows = ops.hdbscan_unit_rows(view.contiguous()).cpu().numpy() if metric == "cosine" else x
    want, want_k, _, want_core = hc.hdbscan_ref(rows, mcs, ms)
    labels, info = ops.hdbscan(view, mcs, ms, metric=metric, return_info=True)
    ok &= np.array_equal(labels.cpu().numpy(), want) and info["n_clusters"] == want_k and same_bits(info["core2"].cpu().numpy(), want_core)
    bad += not ok
    print(f"case {case:3d} {kind:6s} {metric:9s} n={n:3d} d={d:3d} pad={pad} min_cluster_size={mcs:2d} min_samples={ms:2d} "
          f"clusters={want_k:2d} {'ok' if ok else 'MISMATCH'}  ({time.time() - t0:.0f} s)", flush=True)
print(f"fuzz_hdbscan: {cases - bad}/{cases} cases exact")
sys.exit(1 if bad else 0)
