#!/usr/bin/env python3
"""Timing of the product-quantisation ops on the GPU box: python tools/bench_pq.py [N] [d] [M] [Q ...] [--k K ...] [--space ip|l2]
[--niter I] [--no-recall] [--refine float32 float16] [--rescore-multiplier 1 4 10 32 100]

The corpus is N rows around 4 096 Gaussian centres (the data of tools/bench_ivf.py); the codebooks are trained on 65 536 of them
(GpuPQIndex.train from a sample of rows as initial centroids, --niter Lloyd iterations).  First line: ms of ops.pq_encode_rows on
a slice of 2^20 rows.  Then one line per (Q, k): ms of ops.pq_tables, of the scan alone (ops.pq_adc_topk_tables on those tables),
of the whole ops.pq_adc_topk call; the scan's share of the HBM floor — one pass over the N x pq_code_bytes(M) code bytes at
6.3 TB/s, the achievable rate csrc/hamming_search.h reckons with — and recall@10 of the PQ search against GpuFlatIndex on 256
queries (d <= 768: the flat search goes no wider).
--refine (one or both stores) with --rescore-multiplier (several): the rows are kept in a row store as well, and every (Q, k) line
gains ``refine``: per store and multiplier the ms of GpuPQIndex.search(q, k, rescore_multiplier=) — the ADC search for
min(k * multiplier, 1 024) candidates and their exact re-score — and its recall@10 on the same 256 queries.  Without the flags
the output is what it was."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from text_similarity_amd import _refine, ops
from text_similarity_amd.index import GpuFlatIndex
from text_similarity_amd.pq_index import GpuPQIndex

HBM_ACHIEVABLE = 6.3e12      # bytes per second
ap = argparse.ArgumentParser()
ap.add_argument("N", nargs="?", type=int, default=1_000_000)
ap.add_argument("d", nargs="?", type=int, default=384)
ap.add_argument("M", nargs="?", type=int, default=48)
ap.add_argument("Q", nargs="*", type=int, default=[1, 16, 256, 4096])
ap.add_argument("--k", nargs="+", type=int, default=[10])
ap.add_argument("--space", default="ip", choices=("ip", "l2"))
ap.add_argument("--niter", type=int, default=4)
ap.add_argument("--no-recall", action="store_true")
ap.add_argument("--refine", nargs="+", default=[], choices=_refine.KINDS)
ap.add_argument("--rescore-multiplier", nargs="+", type=int, default=[4])
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_pq.py measures on the GPU: no device found")
N, d, M = a.N, a.d, a.M
dev = "cuda:0"
g = torch.Generator(device=dev).manual_seed(97)
centres = torch.randn((4096, d), generator=g, device=dev)


def draw(n):
    return centres[torch.randint(0, 4096, (n,), generator=g, device=dev)] + torch.randn((n, d), generator=g, device=dev)


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


index = GpuPQIndex(a.space, d, M, device=dev, seed=1)
sample = draw(65536)
index.train(sample, niter=a.niter, init_codebooks=sample[:256].reshape(256, M, d // M).permute(1, 0, 2))
del sample
cbk, cb = index.codebooks, ops.pq_code_bytes(M)
recall = not a.no_recall and d <= 768
flat = GpuFlatIndex("ip" if a.space == "ip" else "euclidean", d, device=dev) if recall else None
if recall:
    flat.init_index(N)
codes = torch.empty((N, cb), dtype=torch.uint8, device=dev)
stores = {kind: _refine.RowStore(kind, a.space, d, torch.device(dev)) for kind in a.refine}
for st in stores.values():
    st.reserve(N, 0)
step = 1 << 20      # (encoded in slices: the float32 rows of a large corpus never exist all at once)
for r0 in range(0, N, step):
    x = draw(min(step, N - r0))
    ops.pq_encode_rows(x, cbk, out=codes[r0:r0 + x.shape[0]])
    for st in stores.values():
        st.put(r0, st.convert(x))
    if recall:
        flat.add_items(x, torch.arange(r0, r0 + x.shape[0]).numpy())
ms = timed(lambda: ops.pq_encode_rows(x, cbk), 3, warm=1)
print(json.dumps({"encode": True, "rows": x.shape[0], "d": d, "M": M, "ms": round(ms, 3),
                  "Mrows_s": round(x.shape[0] / ms / 1e3, 2)}), flush=True)
del x
q_all = draw(max(256, max(a.Q)))
r10 = None
refine_r10 = {}
if stores:      # the index over the codes made above (labels = rows), one store attached at a time
    index._codes, index._labels, index._n = codes, torch.arange(N, device=dev), N


def attach(kind):
    index._store, index.refine = stores[kind], kind


if recall:
    truth = flat.search(q_all[:256], 10)[0]
    for kind in stores:
        attach(kind)
        for mult in a.rescore_multiplier:
            got = index.search(q_all[:256], 10, rescore_multiplier=mult)[1]
            refine_r10[f"{kind}_x{mult}"] = round(float((got[:, :, None] == truth[:, None, :]).any(2).float().sum(1).mean()) / 10.0, 4)
    got = ops.pq_adc_topk(q_all[:256].contiguous(), cbk, codes, 10, a.space)[1]
    r10 = round(float((got[:, :, None] == truth[:, None, :]).any(2).float().sum(1).mean()) / 10.0, 4)
    del flat, truth
    torch.cuda.empty_cache()
floor_ms = N * cb / HBM_ACHIEVABLE * 1e3
for Q, k in [(Q, k) for Q in a.Q for k in a.k]:
    q = q_all[:Q].contiguous()
    iters = 5 if Q <= 256 else 2
    t_tab = timed(lambda: ops.pq_tables(q, cbk, a.space, _trusted=True), iters)
    tables = ops.pq_tables(q, cbk, a.space, _trusted=True)[0]
    t_scan = timed(lambda: ops.pq_adc_topk_tables(tables, codes, k, a.space), iters)
    del tables
    t_all = timed(lambda: ops.pq_adc_topk(q, cbk, codes, k, a.space, _trusted=True), iters)
    extra = {}
    if stores:
        extra["refine"] = {}
        for kind in stores:
            attach(kind)
            for mult in a.rescore_multiplier:
                ms = timed(lambda: index.search(q, k, rescore_multiplier=mult), iters)
                extra["refine"][f"{kind}_x{mult}"] = {"ms": round(ms, 4), "recall10": refine_r10.get(f"{kind}_x{mult}")}
    print(json.dumps({"score": "pq_adc", "space": a.space, "Q": Q, "N": N, "d": d, "M": M, "k": k, "row_bytes": cb,
                      "ms_tables": round(t_tab, 4), "ms_scan": round(t_scan, 4), "ms_call": round(t_all, 4),
                      "Glookups_s": round(Q * N * M / t_scan / 1e6, 1), "hbm_floor_ms": round(floor_ms, 4),
                      "floor_share": round(floor_ms / t_scan, 4), "recall10": r10, **extra}), flush=True)
