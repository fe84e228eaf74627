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
Behind them come cases // 4 (at least one) INSERTION cases against tests/graph_insert_cases.py, drawn from a generator of their own
so that the cases above keep their draws: in turn a prune case (ops.graph_insert_prune: N, B, K0, R, candidates with padding,
repeats, batch rows and ids >= n + B), a link case (ops.graph_link_reverse: a space, a width, a crafted graph, targets and
incoming lists with padding, repeats, ids >= N, NaN and duplicate rows, now and then a pool beyond 256 entries) and a whole
insertion (ops.graph_insert, sub-batch after sub-batch, against insert_ref: the graph rows must be identical).
Usage: python tools/fuzz_graph.py [cases] [seed]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
import graph_insert_cases as gic
from graph_cases import build_graph_ref, detours, forward_lists, graph_search_ref, merge_reverse, random_graph, random_rows
from graph_seed_cases import graph_search_seeded_ref
from list_cases import same_bits
from text_similarity_amd import ops

cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
rng = np.random.default_rng(seed)
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
rng = np.random.default_rng([seed, 1])
inserts = max(1, cases // 4)
for case in range(inserts):
    same = lambda t, a: np.array_equal(t.cpu().numpy(), a)
    if case % 3 == 0:
        n, B = int(rng.choice([1, 2, 65, 500])), int(rng.choice([1, 7, 300]))
        K0 = int(rng.choice([1, 2, 8, 33, 64, 128]))
        R = int(rng.integers(1, min(K0, 64) + 1))
        graph = rng.integers(-1, n + B + 2, size=(n, R))
        near = (rng.integers(0, n + B, size=(B, 1)) + rng.integers(0, 2 * K0 + 2, size=(B, K0))) % (n + B)
        cand = np.where(rng.random((B, K0)) < rng.choice([0.0, 0.5, 0.95]), near, rng.integers(-1, n + B + 2, size=(B, K0)))
        fwd, det, st = ops.graph_insert_prune(dev(cand, np.int32), dev(graph, np.int32), return_detours=True)
        torch.cuda.synchronize()
        F, D, rst = gic.insert_prune(cand, graph)
        ok = same(fwd, F) and same(det, D) and same(st, rst)
        what = f"insert-prune n={n:4d} B={B:3d} K0={K0:3d} R={R:2d}"
    elif case % 3 == 1:
        d = int(rng.choice([1, 63, 64, 65, 300, 384, 385, 767, 768]))
        space = str(rng.choice(["cosine", "dot", "l2"] if d <= ops.L2_MAX_DIM else ["cosine", "dot"]))
        N, R = int(rng.choice([2, 65, 400])), int(rng.choice([1, 2, 8, 33, 64]))
        c = random_rows(rng, N, d, dup=True)
        c[rng.choice(N, max(1, N // 20), replace=False), 0] = np.nan
        graph = np.where(rng.random((N, R)) < 0.2, -1, rng.integers(0, N, size=(N, R)))
        T = int(rng.integers(1, N + 1))
        targets = np.sort(rng.choice(N, size=T, replace=False))
        lens = rng.integers(0, int(rng.choice([4, 40, 700])), size=T)
        lims = np.concatenate([[0], np.cumsum(lens)])
        ids = rng.integers(-1, N + 2, size=int(lims[-1]))
        g = dev(graph, np.int32)
        st = ops.graph_link_reverse(space, dev(c), g, dev(targets, np.int32), dev(lims, np.int64), dev(ids, np.int32))
        torch.cuda.synchronize()
        G, rst = gic.link_reverse(space, c, graph, targets, lims, ids)
        ok = same(g, G) and same(st, rst)
        what = f"insert-link  {space:6s} d={d:3d} N={N:4d} R={R:2d} T={T:4d} in={int(lims[-1]):6d} cut={int((rst & gic.LINK_ST_CUT).any())}"
    else:
        d = int(rng.choice([8, 65, 384]))
        space = str(rng.choice(["cosine", "dot", "l2"]))
        n, B, batch = int(rng.choice([40, 300])), int(rng.choice([1, 30, 130])), int(rng.choice([1, 16, 64]))
        R = int(rng.choice([2, 8, 16]))
        K0 = int(rng.choice([R, 2 * R]))
        width, E = int(rng.integers(1, 5)), int(rng.choice([1, 8]))
        iters = int(rng.choice([2, 20]))
        c = random_rows(rng, n + B, d, dup=True)
        base = build_graph_ref(space, c[:n], min(K0, n - 1), R)
        e = rng.choice(n, size=E, replace=False)
        dead = rng.random(n) < 0.1
        want = gic.insert_ref(space, c[:n], base, c[n:], K0, R, batch, width, iters, entries=e, dead=dead)
        rows, graph = dev(c), torch.empty((n + B, R), dtype=torch.int32, device="cuda")
        graph[:n] = dev(base, np.int32)
        for a in range(n, n + B, batch):
            b = min(batch, n + B - a)
            row_ids = np.arange(a, dtype=np.int32)
            row_ids[:n][dead] = -1
            ops.graph_insert(space, rows[:a + b], graph[:a + b], a, K0, entries=dev(e, np.int32), width=width, max_iters=iters,
                             row_ids=dev(row_ids) if dead.any() else None)
        torch.cuda.synchronize()
        ok = same(graph, want)
        what = f"insert       {space:6s} d={d:3d} n={n:4d} B={B:3d} batch={batch:2d} R={R:2d} K0={K0:2d} w={width} iters={iters:2d}"
    bad += not ok
    print(f"case {cases + case:3d} {what} {'ok' if ok else 'MISMATCH'}  ({time.time() - t0:.0f} s)", flush=True)
cases += inserts
print(f"fuzz_graph: {cases - bad}/{cases} cases exact")
sys.exit(1 if bad else 0)
