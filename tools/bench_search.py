#!/usr/bin/env python3
"""Quick timing of the search on the GPU box: python tools/bench_search.py [N] [d] [Q ...] [--score cosine|dot|l2] [--spread]
[--k K ...] [--range TAU ... | --range-hits H ...] [--tau-array] [--range-merge R Q HITS]

--score cosine (default): tsim_cosine_topk on unit rows.  --score dot: tsim_dot_topk_ex on the float32 rows (corpus scaled by
one power of two, dot_scaled_rows), which also reports the per-pass status counts.  --score l2: tsim_l2_topk_ex (squared
Euclidean distance; half rows one element wider, l2_rows / l2_query_rows).  --prep: also time the corpus row
preparation (dot_scaled_rows / l2_rows) and print it.  --spread: corpus row norms spread
log-uniformly over two decades (dot and l2; the default rows are Gaussian).  --k: the k values to time (default 10; up to 1024,
k > 64 runs the _large entries); one line per (Q, k).
--range TAU ...: time the exact range search (ops.cosine_range / ops.dot_range / ops.l2_range on the float32 rows) at these
thresholds (l2: squared radii) instead of top-k: ms per call (scan + the host read of the total + fill), mean hits per query and the status counts; one line per (Q, tau).
--range-hits H ...: the same with tau derived from the normal tail so that about H of the N Gaussian rows pass per query (a cosine
of Gaussian rows is ~ N(0, 1/d), an inner product ~ N(0, d)); the achieved mean is printed.  --score l2: the radius is the
median over a sample of 64 queries of their H-th smallest squared distance (ops.l2_topk over the whole corpus).
--tau-array: pass the threshold of a range run as a per-query tensor [Q] holding that one value (the _tau entries) instead of a float.
With --score l2 --range-hits the tensor holds every query's OWN H-th smallest squared distance instead (one radius hits very
different numbers of rows for queries of different norm: dist^2 ~ |q|^2 + |c|^2), so every query has H hits.
--range-merge R Q HITS: time ops.range_merge alone on R synthetic lists of Q queries x HITS sorted entries each (no corpus is made)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from text_similarity_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("N", nargs="?", type=int, default=1_000_000)
ap.add_argument("d", nargs="?", type=int, default=384)
ap.add_argument("Q", nargs="*", type=int, default=[256, 1024, 4096, 16384])
ap.add_argument("--score", choices=("cosine", "dot", "l2"), default="cosine")
ap.add_argument("--prep", action="store_true")
ap.add_argument("--spread", action="store_true")
ap.add_argument("--k", nargs="+", type=int, default=[10])
ap.add_argument("--range", nargs="+", type=float, default=[], dest="taus")
ap.add_argument("--range-hits", nargs="+", type=float, default=[])
ap.add_argument("--tau-array", action="store_true")
ap.add_argument("--range-merge", nargs=3, type=int, default=None, metavar=("R", "Q", "HITS"))
a = ap.parse_args()
N, d, Qs = a.N, a.d, a.Q
dev = "cuda:0"
g = torch.Generator(device=dev).manual_seed(4321)


def timed(run, iters):
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


if a.range_merge:
    R, Q, H = a.range_merge
    lims = torch.arange(Q + 1, device=dev, dtype=torch.int64) * H
    lists = []
    for r in range(R):      # list r holds the indices = r mod R; scores sorted descending within each query
        sc = torch.rand((Q, H), generator=g, device=dev).sort(dim=1, descending=True).values.reshape(-1)
        ix = torch.arange(H, device=dev, dtype=torch.int64).repeat(Q) * R + r
        lists.append((lims, sc, ix))
    ms = timed(lambda: ops.range_merge(lists, total=R * Q * H), 5)
    ms_read = timed(lambda: ops.range_merge(lists), 5)
    ml, msc, mi = ops.range_merge(lists)
    srt = msc.view(Q, R * H)
    assert int(ml[-1]) == R * Q * H and bool((srt[:, 1:] <= srt[:, :-1]).all())
    print(json.dumps({"range_merge": True, "R": R, "Q": Q, "hits_per_list": H, "entries": R * Q * H, "ms_total_given": round(ms, 4),
                      "ms_total_read_back": round(ms_read, 4)}), flush=True)
    sys.exit(0)
cf = torch.randn((N, d), generator=g, device=dev)
if a.spread:
    cf *= 10.0 ** (2.0 * torch.rand((N, 1), generator=g, device=dev) - 1.0)
if a.score in ("dot", "l2"):
    rows_fn = ops.dot_scaled_rows if a.score == "dot" else ops.l2_rows
    corpus, rho, scale = rows_fn(cf)
    if a.prep:
        print(json.dumps({"score": a.score, "prep": rows_fn.__name__, "N": N, "d": d,
                          "ms": round(timed(lambda: rows_fn(cf, scale), 5), 4)}), flush=True)
else:
    corpus, rho = ops.l2norm_rows(cf, return_rho=True)
    if not (a.taus or a.range_hits):
        del cf
own_k = {}     # l2 --range-hits: the H behind a derived radius
if a.score == "l2":
    taus = list(a.taus)
    if a.range_hits:
        sf = torch.randn((64, d), generator=torch.Generator(device=dev).manual_seed(99), device=dev)
        for h in a.range_hits:
            kh = max(1, min(int(round(h)), ops.MAX_K, N))
            kth = ops.l2_topk(ops.l2_query_rows(sf, scale), corpus, d, kh, eq_f32=sf, ec_f32=cf, rho_c=rho, scale_c=scale)[0][:, kh - 1]
            taus.append(float(kth.median()))
            own_k[taus[-1]] = kh
else:
    taus = list(a.taus) + [statistics.NormalDist().inv_cdf(1.0 - h / N) * (d ** 0.5 if a.score == "dot" else d ** -0.5) for h in a.range_hits]


for Q, tau in [(Q, tau) for Q in (Qs if taus else []) for tau in taus]:
    qf = torch.randn((Q, d), generator=g, device=dev)
    q = ops.l2_query_rows(qf, scale) if a.score == "l2" else ops.l2norm_rows(qf)
    thr = torch.full((Q,), tau, dtype=torch.float32, device=dev) if a.tau_array else tau
    if a.tau_array and tau in own_k:
        thr = ops.l2_topk(q, corpus, d, own_k[tau], eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale)[0][:, own_k[tau] - 1].contiguous()

    def run():
        if a.score == "l2":
            return ops.l2_range(q, corpus, d, thr, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale, return_status=True)
        if a.score == "dot":
            return ops.dot_range(q, corpus, d, thr, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale, return_status=True)
        return ops.cosine_range(q, corpus, d, thr, eq_f32=qf, ec_f32=cf, rho_c=rho, return_status=True)
    ms = timed(run, 5 if Q <= 4096 else 2)
    lims, _, _, st = run()
    print(json.dumps({"score": a.score, "range": True, "tau_array": a.tau_array, "Q": Q, "N": N, "d": d, "tau": round(tau, 6), "ms": round(ms, 4),
                      "mean_hits": round(int(lims[-1]) / Q, 2), "status_counts": torch.bincount(st.long(), minlength=3).tolist()}),
          flush=True)
if taus:
    sys.exit(0)
for Q, k in [(Q, k) for Q in Qs for k in a.k]:
    qf = torch.randn((Q, d), generator=g, device=dev)
    q = ops.l2_query_rows(qf, scale) if a.score == "l2" else ops.l2norm_rows(qf)
    if a.score == "l2":
        def run(status=False):
            return ops.l2_topk(q, corpus, d, k, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale, return_status=status)
    elif a.score == "dot":
        def run(status=False):
            return ops.dot_topk(q, corpus, d, k, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale, return_status=status)
    else:
        def run(status=False):
            return ops.cosine_topk(q, corpus, d, k, return_status=status)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    iters = 5 if Q <= 4096 else 2
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    pairs = Q * N
    rec = {"score": a.score, "spread": a.spread, "Q": Q, "N": N, "d": d, "k": k, "ms": round(ms, 4),
           "Gpairs_s": round(pairs / ms / 1e6, 1), "TFLOPs": round(2 * pairs * d / ms / 1e9, 1),
           "stream_GBs": round(-(-Q // 256) * N * d * 2 / ms / 1e6, 1)}
    rec["status_counts"] = torch.bincount(run(True)[2].long(), minlength=3).tolist()
    print(json.dumps(rec), flush=True)
