#!/usr/bin/env python3
"""Randomised parity sweep of the graph search (ops.graph_search) and of the pruning (ops.graph_prune, ops.graph_merge_reverse)
against the restatement of tests/graph_cases.py: scores (float32 bits), ids, status words, detour counts and graph rows must be
identical.  A search case draws a space, a width of the rows, N, R, E, Q, k, ef, the expansion width, a cap on the iterations
that may or may not cut the search, a crafted graph (ring, repeats, self-loops, padding, ids >= N, an unreachable island), entry
points with padding and repeats, and now and then tombstones, NaN rows, duplicate rows or an id offset.  A prune case draws N, K0,
R and a kNN graph with repeats, padding and ids >= N.  Every fourth case from the second on is a SEEDED search
(ops.graph_search_seeded against tests/graph_seed_cases.py): the same draws with per-query entry points instead — a seed table
[T, S] and probes [Q, P] with padding, repeats and ids past their tables, or no seed table (probes as rows), or centroids, some of
them NaN or duplicates, for the kernel's own coarse phase (then the probes are compared too).
Usage: python tools/fuzz_graph.py [cases] [seed]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
from graph_cases import detours, forward_lists, graph_search_ref, merge_reverse, random_graph, random_rows
from graph_seed_cases import graph_search_seeded_ref
from list_cases import same_bits
from text_similarity_amd import ops

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
dev = lambda x, t=None: torch.from_numpy(np.ascontiguousarray(x, dtype=t)).cuda()
bad = 0
t0 = time.time()
for case in range(cases):
    if case % 4 == 3:
        N = int(rng.choice([1, 2, 65, 300, 1000]))
        K0 = int(rng.choice([1, 2, 8, 33, 64, 128]))
        R = int(rng.integers(1, min(K0, 64) + 1))
        G0 = rng.integers(-1, N + 2, size=(N, K0))
        near = (np.arange(N)[:, None] + rng.integers(1, 2 * K0 + 2, size=(N, K0))) % N
        G0 = np.where(rng.random((N, K0)) < rng.choice([0.0, 0.5, 0.95]), near, G0).astype(np.int32)
        fwd, det = ops.graph_prune(dev(G0), R, return_detours=True)
        merged = ops.graph_merge_reverse(fwd)
        torch.cuda.synchronize()
        D = detours(G0)
        F = forward_lists(G0, D, R)
        ok = np.array_equal(det.cpu().numpy(), D) and np.array_equal(fwd.cpu().numpy(), F) and \
            np.array_equal(merged.cpu().numpy(), merge_reverse(F))
        bad += not ok
        print(f"case {case:3d} prune  N={N:5d} K0={K0:3d} R={R:2d} {'ok' if ok else 'MISMATCH'}  ({time.time() - t0:.0f} s)", flush=True)
        continue
    d = int(rng.choice([1, 63, 64, 65, 128, 300, 384, 385, 767, 768]))
    space = str(rng.choice(["cosine", "dot", "l2"] if d <= ops.L2_MAX_DIM else ["cosine", "dot"]))
    N = int(rng.choice([1, 2, 65, 500, 3000]))
    R = int(rng.choice([1, 2, 8, 33, 64]))
    E = int(rng.choice([1, 4, 64, 256]))
    Q = int(rng.choice([1, 3, 20]))
    k = int(rng.choice([1, 10, 64, 65, 200]))
    ef = int(rng.choice([k, k + 1, 63, 64, 65, 300, 1024]))
    ef = max(ef, k)
    width = int(rng.integers(1, 5))
    iters = int(rng.choice([1, 3, 20, 100, 10 ** 6]))
    iters = max(1, min(iters, ops.graph_max_iters(E, R, width)))
    kind = str(rng.choice(["normal", "tombs", "nan", "offset"]))
    c = random_rows(rng, N, d, dup=rng.random() < 0.5)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    if kind == "nan":
        c[rng.choice(N, max(1, N // 20), replace=False), 0] = np.nan
        q[0, 0] = np.nan
    g, lost = random_graph(rng, N, R, beyond=rng.random() < 0.5, island=int(rng.choice([0, 3])) if N > 10 else 0)
    e = rng.choice(np.setdiff1d(np.arange(N), lost), size=E, replace=True)
    if E >= 4:
        e[1], e[3] = -1, N + 2
    ids = None
    if kind == "tombs":
        ids = rng.permutation(N).astype(np.int32)
        ids[rng.random(N) < 0.3] = -1
    off = 11 if kind == "offset" else 0
    if case % 4 == 1:
        how = str(rng.choice(["probes", "rows", "centroids"]))
        T = N if how == "rows" else int(rng.choice([1, 7, 256, 257, 1000]))
        S = 1 if how == "rows" else int(rng.choice([s for s in (1, 2, 4, 64, 256) if s <= E]))
        P = E // S
        iters = max(1, min(iters, ops.graph_max_iters(P * S, R, width)))
        seeds = None if how == "rows" else rng.integers(-1, N + 1, size=(T, S))
        kw = {}
        if how == "centroids":
            cent = random_rows(rng, T, d, dup=True)
            cent[rng.random(T) < 0.1, 0] = np.nan
            kw = dict(centroids=cent, n_probe=P)
        else:
            kw = dict(probes=rng.integers(-1, T + 2, size=(Q, P)))
        rs, ri, rst, rp = graph_search_seeded_ref(space, q, c, g, ef, width, iters, k, seeds=seeds, row_ids=ids, idx_offset=off, **kw)
        dkw = {name: (dev(v, np.float32 if name == "centroids" else np.int32) if isinstance(v, np.ndarray) else v) for name, v in kw.items()}
        s, i, st, pr = ops.graph_search_seeded(space, dev(q), dev(c), dev(g), k, ef, seeds=None if seeds is None else dev(seeds, np.int32),
                                               width=width, max_iters=iters, row_ids=None if ids is None else dev(ids), idx_offset=off,
                                               return_status=True, return_probes=True, **dkw)
        torch.cuda.synchronize()
        ok = same_bits(s.cpu().numpy(), rs) and np.array_equal(i.cpu().numpy(), ri) and np.array_equal(st.cpu().numpy(), rst) and \
            np.array_equal(pr.cpu().numpy(), rp)
        bad += not ok
        print(f"case {case:3d} seeded {space:6s} {how:9s} d={d:3d} N={N:5d} R={R:2d} T={T:4d} S={S:3d} P={P:3d} Q={Q:2d} k={k:4d} ef={ef:4d} "
              f"w={width} iters={iters:5d} {kind:6s} {'ok' if ok else 'MISMATCH'}  ({time.time() - t0:.0f} s)", flush=True)
        continue
    rs, ri, rst = graph_search_ref(space, q, c, g, e, ef, width, iters, k, row_ids=ids, idx_offset=off)
    s, i, st = ops.graph_search(space, dev(q), dev(c), dev(g), dev(e, np.int32), k, ef, width=width, max_iters=iters,
                                row_ids=None if ids is None else dev(ids), idx_offset=off, return_status=True)
    torch.cuda.synchronize()
    ok = same_bits(s.cpu().numpy(), rs) and np.array_equal(i.cpu().numpy(), ri) and np.array_equal(st.cpu().numpy(), rst)
    bad += not ok
    print(f"case {case:3d} {space:6s} d={d:3d} N={N:5d} R={R:2d} E={E:3d} Q={Q:2d} k={k:4d} ef={ef:4d} w={width} iters={iters:5d} {kind:6s} "
          f"{'ok' if ok else 'MISMATCH'}  ({time.time() - t0:.0f} s)", flush=True)
print(f"fuzz_graph: {cases - bad}/{cases} cases exact")
sys.exit(1 if bad else 0)
