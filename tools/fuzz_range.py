#!/usr/bin/env python3
"""Randomised parity sweep of the exact range search (ops.cosine_range / ops.dot_range / ops.l2_range) against the oracle: per
query the rows whose exact score is >= tau, ordered (score desc, index asc); lims, indices and float32 score bits must be
identical.  The Euclidean space (widths <= 767) is checked as score = -(squared distance) of tests/l2_cases.py, tau = -radius:
negation is exact, so the same mask and order apply; the distances that come back must be the negated scores' bits.
Usage: python tools/fuzz_range.py [cases] [seed]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
from l2_cases import l2_dists
from oracle.search_ref import _lane_sum, exact_cosine
from text_similarity_amd import ops


def dot_scores(q, c):
    out = np.empty((q.shape[0], c.shape[0]), dtype=np.float32)
    for b in range(0, c.shape[0], 4096):
        out[:, b:b + 4096] = _lane_sum(q[:, None, :], c[None, b:b + 4096, :]).astype(np.float32)
    return out


cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
bad = 0
t0 = time.time()
for case in range(cases):
    d = int(rng.choice([64, 128, 300, 384, 768]))
    Q = int(rng.choice([1, 7, 33, 200]))
    N = int(rng.choice([5, 100, 3000, 20000, 70001]))
    space = str(rng.choice(["cosine", "dot", "l2"] if d <= ops.L2_MAX_DIM else ["cosine", "dot"]))
    kind = str(rng.choice(["normal", "dups", "spread", "zeros", "cluster"]))
    c = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    if kind == "dups":                       # a block of copies that may or may not overflow a query's collect buffer
        n = int(rng.choice([10, ops.RANGE_SLOT_CAP - 3, ops.RANGE_SLOT_CAP + 300]))
        c[rng.choice(N, min(n, N), replace=False)] = q[0]
    elif kind == "spread":
        c *= (10.0 ** rng.uniform(-3, 3, (N, 1))).astype(np.float32)
    elif kind == "zeros":
        c[rng.choice(N, max(1, N // 10), replace=False)] = 0.0
        q[0] = 0.0
    elif kind == "cluster":
        c[:min(40, N)] = q[0] + 1e-7 * rng.standard_normal((min(40, N), d)).astype(np.float32)
    sel = np.unique(np.concatenate([[0], rng.choice(Q, min(Q, 6), replace=False)]))
    exact = exact_cosine(q[sel], c) if space == "cosine" else -l2_dists(q[sel], c) if space == "l2" else dot_scores(q[sel], c)
    pick = str(rng.choice(["rank", "rank", "none", "all", "zero"]))
    row = np.sort(exact[0])[::-1]
    tau = {"rank": float(row[min(int(rng.choice([0, 5, 50, 500])), N - 1)]), "none": float(exact.max()) * 2.0 + 1.0,
           "all": float("-inf"), "zero": 0.0}[pick]
    qf, cf = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    if space == "l2":
        cn, rho, scale = ops.l2_rows(cf)
        lims, s, i, st = ops.l2_range(ops.l2_query_rows(qf, scale), cn, d, -tau, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale,
                                      return_status=True)
        s = -s
    elif space == "cosine":
        cn, rho = ops.l2norm_rows(cf, return_rho=True)
        lims, s, i, st = ops.cosine_range(ops.l2norm_rows(qf), cn, d, tau, eq_f32=qf, ec_f32=cf, rho_c=rho, return_status=True)
    else:
        cn, rho, scale = ops.dot_scaled_rows(cf)
        lims, s, i, st = ops.dot_range(ops.l2norm_rows(qf), cn, d, tau, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale,
                                       return_status=True)
    torch.cuda.synchronize()
    lims, s, i, st = lims.cpu().numpy(), s.cpu().numpy(), i.cpu().numpy(), st.cpu().numpy()
    ok = lims[0] == 0 and lims[-1] == s.size == i.size and bool((np.diff(lims) >= 0).all()) and bool(np.isin(st, (1, 2)).all())
    for r, qi in enumerate(sel):
        hit = np.nonzero(exact[r] >= np.float32(tau))[0]
        hit = hit[np.lexsort((hit, -exact[r, hit].astype(np.float64)))]
        a, b = int(lims[qi]), int(lims[qi + 1])
        ok = ok and np.array_equal(i[a:b], hit) and np.array_equal(s[a:b].view(np.uint32), exact[r, hit].view(np.uint32))
    bad += not ok
    print(f"case {case:3d} {space:6s} d={d:3d} Q={Q:3d} N={N:6d} {kind:7s} tau={pick:4s} hits={int(lims[-1]):8d} "
          f"status={np.bincount(st, minlength=3).tolist()} {'ok' if ok else 'MISMATCH'}  ({time.time() - t0:.0f} s)", flush=True)
print(f"fuzz_range: {cases - bad}/{cases} cases exact")
sys.exit(1 if bad else 0)
