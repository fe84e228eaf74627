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
--range-merge R Q HITS: time ops.range_merge alone on R synthetic lists of Q queries x HITS sorted entries each (no corpus is made).
--list-len L ...: time the exact search WITHIN LISTS (ops.cosine_list_topk / dot_list_topk / l2_list_topk on the float32 rows) instead:
every query gets its own list of L random rows (CSR), or with --shared all queries share ONE list of L rows; --list-order
sorted|shuffled|arange orders the shared list (arange: rows 0 .. L-1).  ms per call and GB/s of (sum of list lengths) x d x 4; one
line per (Q, L, k).
--filter-frac F ...: GpuFlatIndex.search(filter=a shared allow-list of F x N labels) in both regimes, ms per call each and what
filter_plan would choose; one line per (Q, F, k)."""
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
ap.add_argument("--list-len", nargs="+", type=int, default=[])
ap.add_argument("--shared", action="store_true")
ap.add_argument("--list-order", choices=("sorted", "shuffled", "arange"), default="sorted")
ap.add_argument("--filter-frac", nargs="+", type=float, default=[])
a = ap.parse_args()
N, d, Qs = a.N, a.d, a.Q
dev = "cuda:0"
g = torch.Generator(device=dev).manual_seed(4321)


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
if a.list_len:
    fn = {"cosine": ops.cosine_list_topk, "dot": ops.dot_list_topk, "l2": ops.l2_list_topk}[a.score]
    for Q, L, k in [(Q, L, k) for Q in Qs for L in a.list_len for k in a.k]:
        qf = torch.randn((Q, d), generator=g, device=dev)
        if a.shared:
            cand = torch.arange(L, device=dev) if a.list_order == "arange" else torch.randperm(N, generator=g, device=dev)[:L]
            cand = cand.sort().values if a.list_order == "sorted" else cand
            lims = None
        else:      # (random rows, a repeat now and then: the lists go to the kernel as they are)
            cand = torch.randint(0, N, (Q * L,), generator=g, device=dev)
            cand = cand.view(Q, L).sort(dim=1).values.reshape(-1) if a.list_order == "sorted" else cand
            lims = torch.arange(Q + 1, device=dev, dtype=torch.int64) * L
        ms = timed(lambda: fn(qf, cf, cand, lims, k=k, assume_unique=True), 5 if Q * L <= 1 << 26 else 2)
        print(json.dumps({"score": a.score, "list": True, "shared": a.shared, "order": a.list_order, "Q": Q, "N": N, "d": d, "L": L,
                          "k": k, "ms": round(ms, 4), "gather_GBs": round(Q * L * d * 4 / ms / 1e6, 1)}), flush=True)
    sys.exit(0)
if a.filter_frac:
    from text_similarity_amd.index import GpuFlatIndex
    ix = GpuFlatIndex(space={"cosine": "cosine", "dot": "ip", "l2": "euclidean"}[a.score], dim=d, device=dev)
    ix.add_items(cf, range(N))
    del cf
    for Q, F, k in [(Q, F, k) for Q in Qs for F in a.filter_frac for k in a.k]:
        qf = torch.randn((Q, d), generator=g, device=dev)
        allowed = torch.randperm(N, generator=g, device=dev)[:max(1, int(F * N))]
        rec = {"score": a.score, "filter": True, "Q": Q, "N": N, "d": d, "frac": F, "n_allowed": allowed.numel(), "k": k,
               "plan": ix.filter_plan(Q, allowed.numel())}
        gathered = Q * allowed.numel() * d * 4      # what the list regime reads; beyond 7e13 B it is not run (minutes per call)
        for plan in ("list", "compact"):
            if plan == "list" and gathered > 7e13:
                rec["ms_list"] = None
                continue
            long = plan == "list" and gathered > 5e12
            rec["ms_" + plan] = round(timed(lambda: ix.search(qf, k, filter=allowed, filter_plan=plan), 1 if long else 3, 1 if long else 2), 4)
        print(json.dumps(rec), flush=True)
    sys.exit(0)
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
