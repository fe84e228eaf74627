#!/usr/bin/env python3
"""GpuIVFPQIndex beside GpuPQIndex, GpuIVFIndex and GpuFlatIndex on the GPU box: python tools/bench_ivfpq.py [--N ...] [--d D]
[--M M] [--Q ...] [--nlist ...] [--nprobe ...] [--k K] [--rounds R] [--iters I] [--space cosine|ip|l2] [--scan-only] [--refine float32 float16] [--rescore-multiplier 1 4 10 32 100]

Data and method are those of tools/bench_ivf.py: the rows are a seeded Gaussian mixture generated here (--components centres,
rows = centre + sigma * noise), the queries fresh draws from it; per N one flat index and one PQ index, per (N, nlist) one IVF
index and two IVF-PQ indexes (residual codes and codes of the rows themselves) on the IVF index's centroids.  One JSON line per
cell (nlist, nprobe, Q):
  *_ms          ms per ``search`` call: ivfpq (residuals), ivfpq_rows (by_residual=False), pq, ivf, flat — median [min, max] over
                R rounds, the indexes ALTERNATING inside every round (the order reversed every other round), I calls per round
                timed between device events;
  coarse_ms / tables_ms / scan_ms
                the three parts of the residual search on their own: the probes, ops.ivfpq_tables, ops.ivfpq_scan_topk; and
                scan_GBs, the code bytes of the probed lists (summed over the (query, probe) pairs) over scan_ms;
  recall10_*    recall@10 against the flat result on a fixed set of 256 queries.
--refine (one or both stores) with --rescore-multiplier (several): the rows are kept once per store (the three code indexes hold
the same rows in the same order, so they share it), and every line gains ``refine``: per store, multiplier and index (ivfpq,
ivfpq_rows, pq) the ms of search(q, k, rescore_multiplier=), timed inside the same alternating rounds, and its recall@10 on the
same 256 queries.  Without the flags the output is what it was.
--scan-only builds the residual IVF-PQ index alone and reports coarse / tables / scan: the form the segment-length variants
(libraries built with -DTSIM_IVFPQ_SEG=..., chosen with TSIM_LIB) are compared in; ``lib`` names the library.  Not part of
bench.py."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from text_similarity_amd import _lib, _refine, ops
from text_similarity_amd.index import GpuFlatIndex
from text_similarity_amd.ivf_index import GpuIVFIndex
from text_similarity_amd.ivfpq_index import _COARSE_SPACE, GpuIVFPQIndex
from text_similarity_amd.pq_index import GpuPQIndex

ap = argparse.ArgumentParser()
ap.add_argument("--N", nargs="+", type=int, default=[1_000_000, 16_000_000])
ap.add_argument("--d", type=int, default=384)
ap.add_argument("--M", type=int, default=48)
ap.add_argument("--Q", nargs="+", type=int, default=[1, 16, 256])
ap.add_argument("--nlist", nargs="+", type=int, default=[1024, 4096])
ap.add_argument("--nprobe", nargs="+", type=int, default=[1, 8, 32])
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--space", default="cosine", choices=GpuIVFPQIndex.SPACES)
ap.add_argument("--components", type=int, default=4096)
ap.add_argument("--sigma", type=float, default=1.0)
ap.add_argument("--points-per-list", type=int, default=64)
ap.add_argument("--niter", type=int, default=10)
ap.add_argument("--scan-only", action="store_true")
ap.add_argument("--refine", nargs="+", default=[], choices=_refine.KINDS)
ap.add_argument("--rescore-multiplier", nargs="+", type=int, default=[4])
a = ap.parse_args()
if a.refine and a.scan_only:
    sys.exit("--refine needs the full run, not --scan-only")
if not torch.cuda.is_available():
    sys.exit("bench_ivfpq.py measures on the GPU: no device found")
dev = "cuda:0"
d = a.d
g = torch.Generator(device=dev).manual_seed(97)
centres = torch.randn((a.components, d), generator=g, device=dev)
lib_name = os.path.basename(_lib.LIB_PATH)


def draw(n):
    return centres[torch.randint(0, a.components, (n,), generator=g, device=dev)] + a.sigma * torch.randn((n, d), generator=g, device=dev)


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


def spread(v):
    return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]


def attach(index, store):
    index._store, index.refine = store, None if store is None else store.kind


def recall(labels, truth):
    return round(float((labels[:, :, None] == truth[:, None, :]).any(2).float().sum(1).mean()) / 10.0, 4)


for N in a.N:
    sample = draw(min(N, max(a.points_per_list * max(a.nlist), 256 * 64)))
    flat = pq = None
    if not a.scan_only:
        flat = GpuFlatIndex(_COARSE_SPACE[a.space], d, device=dev)
        flat.init_index(N)
        pq = GpuPQIndex(a.space, d, a.M, device=dev, seed=1)
        pq.train(sample, niter=a.niter, max_points_per_centroid=64)
    for nl in a.nlist:
        ivf = GpuIVFIndex(_COARSE_SPACE[a.space], d, nl, device=dev, seed=1)
        ivf.train(sample, niter=a.niter, max_points_per_list=a.points_per_list)
        res = GpuIVFPQIndex(a.space, d, nl, 1, a.M, by_residual=True, device=dev, seed=1)
        res.train(sample, niter=a.niter, max_points_per_centroid=64, centroids=ivf.centroids)
        rows_ix = None
        if not a.scan_only:
            rows_ix = GpuIVFPQIndex(a.space, d, nl, 1, a.M, by_residual=False, device=dev, seed=1)
            rows_ix.train(centroids=ivf.centroids, codebooks=pq.codebooks)
            ivf.init_index(N)
        stores = {kind: _refine.RowStore(kind, a.space, d, torch.device(dev)) for kind in a.refine}
        for st in stores.values():
            st.reserve(N, 0)
        g.manual_seed(1000 + N % 997)      # the same rows for every index of this N
        for r0 in range(0, N, 1 << 20):
            x = draw(min(1 << 20, N - r0))
            ids = torch.arange(r0, r0 + x.shape[0]).numpy()
            res.add_items(x, ids)
            for st in stores.values():
                st.put(r0, st.convert(x))
            if not a.scan_only:
                rows_ix.add_items(x, ids)
                ivf.add_items(x, ids)
                if flat.get_current_count() < N:
                    flat.add_items(x, ids)
                    pq.add_items(x, ids)
        del x
        q_all = draw(max(256, max(a.Q)))
        truth = None if a.scan_only else flat.search(q_all[:256], 10)[0]
        codes, list_off, row_ids, longest = res._pack()
        lens = list_off[1:] - list_off[:-1]
        adc = "l2" if a.space == "l2" else "ip"
        for nprobe in a.nprobe:
            if nprobe > nl:
                continue
            res.set_nprobe(nprobe)
            rec = {}
            if not a.scan_only:
                rows_ix.set_nprobe(nprobe)
                ivf.set_nprobe(nprobe)
                rec = {"recall10_ivfpq": recall(res.search(q_all[:256], 10)[1], truth),
                       "recall10_ivfpq_rows": recall(rows_ix.search(q_all[:256], 10)[1], truth),
                       "recall10_pq": recall(pq.search(q_all[:256], 10)[1], truth),
                       "recall10_ivf": recall(ivf.search(q_all[:256], 10)[0], truth)}
            coded = {"ivfpq": res, "ivfpq_rows": rows_ix, "pq": pq}
            refined = [(kind, mult, name) for kind in stores for mult in a.rescore_multiplier for name in coded]
            ref_rec = {}
            for kind, mult, name in refined:
                attach(coded[name], stores[kind])
                ref_rec[(kind, mult, name)] = recall(coded[name].search(q_all[:256], 10, rescore_multiplier=mult)[1], truth)
                attach(coded[name], None)
            for Q in a.Q:
                q = res._rows(q_all[:Q]).contiguous()
                probes = res._coarse(q, nprobe).contiguous()
                tables, bias, _ = ops.ivfpq_tables(q, res.centroids, probes, res.codebooks, adc, _trusted=True)
                scanned = int(lens[probes.clamp(min=0)].sum()) * a.M
                t = {name: [] for name in ("ivfpq", "ivfpq_rows", "pq", "ivf", "flat", "coarse", "tables", "scan")}
                runs = [("coarse", lambda: res._coarse(q, nprobe)),
                        ("tables", lambda: ops.ivfpq_tables(q, res.centroids, probes, res.codebooks, adc, _trusted=True)),
                        ("scan", lambda: ops.ivfpq_scan_topk(adc, tables, bias, codes, list_off, row_ids, probes, a.k, max_list_len=longest)),
                        ("ivfpq", lambda: res.search(q_all[:Q], a.k))]
                if not a.scan_only:
                    runs += [("ivfpq_rows", lambda: rows_ix.search(q_all[:Q], a.k)), ("pq", lambda: pq.search(q_all[:Q], a.k)),
                             ("ivf", lambda: ivf.search(q_all[:Q], a.k)), ("flat", lambda: flat.search(q_all[:Q], a.k))]
                def refined_run(kind, mult, name):
                    def run():
                        attach(coded[name], stores[kind])
                        coded[name].search(q_all[:Q], a.k, rescore_multiplier=mult)
                        attach(coded[name], None)
                    return run
                for key in refined:
                    t[key] = []
                    runs.append((key, refined_run(*key)))
                for r in range(a.rounds):
                    for name, run in (runs if r % 2 == 0 else runs[::-1]):
                        t[name].append(timed(run, a.iters))
                line = {"lib": lib_name, "space": a.space, "N": N, "d": d, "M": a.M, "k": a.k, "nlist": nl, "nprobe": nprobe, "Q": Q}
                line.update({name + "_ms": spread(v) for name, v in t.items() if v and isinstance(name, str)})
                if refined:
                    line["refine"] = {f"{kind}_x{mult}": {name: {"ms": spread(t[(kind, mult, name)]), "recall10": ref_rec[(kind, mult, name)]}
                                                          for name in coded} for kind in stores for mult in a.rescore_multiplier}
                line.update({"scan_GBs": round(scanned / statistics.median(t["scan"]) / 1e6, 1), **rec, "longest_list": longest,
                             "mean_list": round(N / nl, 1)})
                print(json.dumps(line), flush=True)
                del tables, bias
        del ivf, res, rows_ix, codes, list_off, row_ids, truth, stores
        torch.cuda.empty_cache()
    del flat, pq
    torch.cuda.empty_cache()
