#!/usr/bin/env python3
"""GpuGraphIndex against GpuFlatIndex and GpuIVFIndex on the GPU box: python tools/bench_graph.py [--N N] [--d D] [--Q ...]
[--ef ...] [--width ...] [--M M] [--ef-construction C] [--k K] [--nlist L] [--nprobe P] [--rounds R] [--iters I] [--data ...]
[--entry shared coarse] [--seeds-per-list S] [--coarse kernel flat]

Three corpora, all seeded: ``mixture``, the Gaussian mixture of tools/bench_ivf.py (--components centres of unit variance per
element, rows = centre + sigma * noise, queries fresh draws from it); ``gauss``, isotropic standard-normal rows and queries —
data without clusters, where an inverted file has nothing to hold on to; and ``manifold`` (not in the default set), rows on a
--latent-dimensional linear manifold (standard-normal latents through a fixed random [latent, d] map, plus 0.05 noise per
element): connected, of low intrinsic dimension, the shape a proximity graph is made for.  Per corpus one JSON line for the build (seconds of
the self-search, the pruning and the reverse merge) and one per cell (Q, ef, width):
  graph_ms / ivf_ms / flat_ms   ms per ``search`` call on the same queries: median [min, max] over R rounds, the three indexes
                                ALTERNATING inside every round, I calls timed per round between device events;
  recall10, ivf_recall10        recall@10 against the flat result on a fixed set of 256 queries;
  cut                           the share of those queries whose search the iteration cap ended (TSIM_GRAPH_ST_ITERS).
With ``--entry coarse`` a second graph index with entry='coarse' (the same rows and kNN graph; --nlist lists, --nprobe probes,
--seeds-per-list seeds) joins the alternation: the build line gains ``coarse_build_s`` (centroids and seed table) and ``nlist``,
every cell
  coarse_ms                     {route: ms} for each --coarse route of the probes (kernel: the search kernel's own coarse phase; flat:
                                the exact flat search of the queries against the centroids, then the kernel), and ``given``: the
                                search with the probes handed in ready — a route minus ``given`` is what its coarse phase costs;
  coarse_recall10, coarse_cut   as recall10 and cut.
--entry shared (the default) prints the lines this tool printed before the option existed.

``--insert B [--base M] [--insert-batch S]`` measures INSERTION instead (GpuGraphIndex(incremental=True)) and prints, per corpus,
two JSON lines.  ``add``: B rows added to an index built over the first N - B rows, the two ways ALTERNATING inside every
round and each timed to a synchronised search result —
  insert_s    ``add_items`` of an incremental index (the rows are linked in), then one search of 256 queries;
  rebuild_s   the behaviour without it: ``add_items`` marks the graph stale and that search rebuilds it over all N rows;
median [min, max] over R rounds, both starting from the same built graph of N - B rows every time.  ``build``: the graph over all N
rows the two ways, alternating — ``insert_build_s``, ``build(insert_from=M)`` (M default N / 2), and ``exact_build_s``,
``build()`` — with, for both graphs, recall@10 against GpuFlatIndex on 256 fresh queries at every --ef (the first --width), and
``orphans``: the share of the inserted rows that end with in-degree 0.
Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from text_similarity_amd import ops
from text_similarity_amd.graph_index import _OPS_SPACE, GpuGraphIndex
from text_similarity_amd.index import GpuFlatIndex
from text_similarity_amd.ivf_index import GpuIVFIndex

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=1_000_000)
ap.add_argument("--d", type=int, default=384)
ap.add_argument("--Q", nargs="+", type=int, default=[1, 16, 256])
ap.add_argument("--ef", nargs="+", type=int, default=[32, 64, 128])
ap.add_argument("--width", nargs="+", type=int, default=[1, 4])
ap.add_argument("--M", type=int, default=16)
ap.add_argument("--ef-construction", type=int, default=0)
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--nlist", type=int, default=1024)
ap.add_argument("--nprobe", type=int, default=8)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--space", default="cosine", choices=GpuGraphIndex.SPACES)
ap.add_argument("--components", type=int, default=4096)
ap.add_argument("--sigma", type=float, default=1.0)
ap.add_argument("--latent", type=int, default=16)
ap.add_argument("--data", nargs="+", default=["mixture", "gauss"], choices=["mixture", "gauss", "manifold"])
ap.add_argument("--entry", nargs="+", default=["shared"], choices=["shared", "coarse"])
ap.add_argument("--seeds-per-list", type=int, default=4)
ap.add_argument("--coarse", nargs="+", default=["kernel", "flat"], choices=["kernel", "flat"])
ap.add_argument("--insert", type=int, default=0)
ap.add_argument("--base", type=int, default=0)
ap.add_argument("--insert-batch", type=int, default=1024)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_graph.py measures on the GPU: no device found")
dev = "cuda:0"
d, N = a.d, a.N
g = torch.Generator(device=dev).manual_seed(97)
centres = torch.randn((a.components, d), generator=g, device=dev)
lift = torch.randn((a.latent, d), generator=g, device=dev)


def draw(kind, n):
    noise = torch.randn((n, d), generator=g, device=dev)
    if kind == "gauss":
        return noise
    if kind == "manifold":
        return torch.randn((n, a.latent), generator=g, device=dev) @ lift + 0.05 * noise
    return centres[torch.randint(0, a.components, (n,), generator=g, device=dev)] + a.sigma * noise


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


def wall(f):
    torch.cuda.synchronize()
    t = time.time()
    out = f()
    torch.cuda.synchronize()
    return out, round(time.time() - t, 3)


def recall(got, truth):
    return round(float((got[:, :, None] == truth[:, None, :]).any(2).float().sum(1).mean()) / truth.shape[1], 4)


def bench_insert(kind):
    B, M = a.insert, (a.base or N // 2)
    mode = dict(entry=a.entry[0], nlist=a.nlist, nprobe=a.nprobe, seeds_per_list=a.seeds_per_list)
    g.manual_seed(1000 + N % 997)
    x = draw(kind, N)
    q = draw(kind, 256)
    flat = GpuFlatIndex(a.space, d, device=dev)
    flat.add_items(x)
    truth = flat.search(q, 10)[0]
    del flat
    made = {}
    for inc in (True, False):       # two indexes over the first N - B rows, built alike
        ix = GpuGraphIndex(a.space, d, M=a.M, ef_construction=a.ef_construction, device=dev, width=a.width[0], incremental=inc,
                           insert_batch=a.insert_batch, **mode)
        ix.init_index(N)
        ix.add_items(x[:N - B])
        ix.build()
        made[inc] = (ix, ix.graph.clone())

    def add(inc):
        ix, graph = made[inc]
        ix._n, ix.graph, ix._row_ids = N - B, graph.clone(), None      # back to the built index of N - B rows
        torch.cuda.synchronize()
        t = time.time()
        ix.add_items(x[N - B:])
        ix.search(q, 10)
        torch.cuda.synchronize()
        return time.time() - t
    t_ins, t_reb = [], []
    for r in range(a.rounds):
        for into, inc in ((t_ins, True), (t_reb, False)) if r % 2 == 0 else ((t_reb, False), (t_ins, True)):
            into.append(add(inc))
    rec = {inc: recall(made[inc][0].search(q, 10)[0], truth) for inc in made}
    print(json.dumps({"data": kind, "what": "add", "space": a.space, "N": N, "d": d, "B": B, "R": made[True][0].R, "K0": made[True][0].K0,
                      "entry": a.entry[0], "insert_batch": a.insert_batch, "insert_s": spread(t_ins), "rebuild_s": spread(t_reb),
                      "insert_recall10": rec[True], "rebuild_recall10": rec[False], "ef": made[True][0].ef}), flush=True)
    ix = made[True][0]
    del made
    ix._n, ix.graph = N, None
    t_by, t_ex, graphs = [], [], {}
    for r in range(a.rounds):
        for name in ("insert", "exact") if r % 2 == 0 else ("exact", "insert"):
            _, t = wall((lambda: ix.build(insert_from=M)) if name == "insert" else ix.build)
            (t_by if name == "insert" else t_ex).append(t)
            graphs[name] = ix.graph
    seen = torch.zeros((N,), dtype=torch.bool, device=dev)
    seen[graphs["insert"][graphs["insert"] >= 0].long()] = True
    rec = {}
    for name, graph in graphs.items():
        ix.graph = graph
        for ef in a.ef:
            ix.set_ef(ef)
            rec[f"{name}_recall10_ef{ef}"] = recall(ix.search(q, 10)[0], truth)
    print(json.dumps({"data": kind, "what": "build", "space": a.space, "N": N, "d": d, "insert_from": M, "R": ix.R, "K0": ix.K0,
                      "entry": a.entry[0], "insert_batch": a.insert_batch, "width": ix.width, "insert_build_s": spread(t_by),
                      "exact_build_s": spread(t_ex), **rec, "orphans": round(float((~seen[M:]).float().mean()), 4),
                      "insert_mean_degree": round(float((graphs["insert"] >= 0).sum(1).float().mean()), 2),
                      "exact_mean_degree": round(float((graphs["exact"] >= 0).sum(1).float().mean()), 2)}), flush=True)


if a.insert:
    for kind in a.data:
        bench_insert(kind)
        torch.cuda.empty_cache()
    sys.exit(0)

for kind in a.data:
    flat = GpuFlatIndex(a.space, d, device=dev)
    flat.init_index(N)
    ivf = GpuIVFIndex(a.space, d, a.nlist, nprobe=min(a.nprobe, a.nlist), device=dev, seed=1)
    gr = GpuGraphIndex(a.space, d, M=a.M, ef_construction=a.ef_construction, device=dev)
    gc = None
    if "coarse" in a.entry:
        gc = GpuGraphIndex(a.space, d, M=a.M, ef_construction=a.ef_construction, device=dev, entry="coarse", nlist=a.nlist,
                           nprobe=a.nprobe, seeds_per_list=a.seeds_per_list)
    g.manual_seed(1000 + N % 997)
    ivf.train(draw(kind, min(N, 64 * a.nlist)), niter=10, max_points_per_list=64)
    for r0 in range(0, N, 1 << 20):
        x = draw(kind, min(1 << 20, N - r0))
        ids = torch.arange(r0, r0 + x.shape[0]).numpy()
        for ix in (flat, ivf, gr) + ((gc,) if gc is not None else ()):
            ix.add_items(x, ids)
    del x
    knn, t_knn = wall(gr.knn_graph)
    fwd, t_prune = wall(lambda: ops.graph_prune(knn, gr.R))
    _, t_merge = wall(lambda: ops.graph_merge_reverse(fwd))
    del fwd
    _, t_rest = wall(lambda: gr.build(knn))
    extra = {}
    if gc is not None:
        gc.build(knn)
        _, t_coarse = wall(gc.build_coarse)      # (again, alone: the centroids and the seed table)
        extra = {"coarse_build_s": t_coarse, "nlist": int(gc.centroids.shape[0]), "seeds_per_list": gc.seeds_per_list}
    del knn
    t_build = round(t_knn + t_rest, 3)
    deg = float((gr.graph >= 0).sum(1).float().mean())
    print(json.dumps({"data": kind, "space": a.space, "N": N, "d": d, "R": gr.R, "K0": gr.K0, "entries": int(gr.entries.numel()),
                      "build_s": t_build, "knn_s": t_knn, "prune_s": t_prune, "merge_s": t_merge, "mean_degree": round(deg, 2),
                      **extra}), flush=True)
    q_all = draw(kind, max(256, max(a.Q)))
    truth = flat.search(q_all[:256], 10)[0]
    ivf_recall = recall(ivf.search(q_all[:256], 10)[0], truth)
    for ef in a.ef:
        for width in a.width:
            gr.set_ef(ef)
            gr.width = width
            efu, iters = gr.search_params(10)
            rc = recall(gr.search(q_all[:256], 10)[0], truth)
            st = ops.graph_search(_OPS_SPACE[a.space], q_all[:256].contiguous(), gr._f32[:N], gr.graph, gr.entries, 10, efu, width=width,
                                  max_iters=iters, return_status=True)[2]
            cut = round(float((st & ops.GRAPH_ST_ITERS).bool().float().mean()), 4)
            lds = ops.graph_search_lds_bytes(int(gr.entries.numel()), gr.R, width, iters)
            if gc is not None:
                gc.set_ef(ef)
                gc.width = width
                _, c_iters = gc.search_params(10)
                c_rc = recall(gc.search(q_all[:256], 10)[0], truth)
                P = gc._n_probe()
                probes_all = gc._exact_search(q_all.contiguous(), gc.centroids, P, gc._coarse_ops).to(torch.int32)
                st = ops.graph_search_seeded(_OPS_SPACE[a.space], q_all[:256].contiguous(), gc._f32[:N], gc.graph, 10, efu, seeds=gc.seeds,
                                             probes=probes_all[:256], width=width, max_iters=c_iters, return_status=True)[2]
                c_cut = round(float((st & ops.GRAPH_ST_ITERS).bool().float().mean()), 4)
            for Q in a.Q:
                q = q_all[:Q].contiguous()
                t_gr, t_ivf, t_flat = [], [], []
                t_co = {route: [] for route in a.coarse + ["given"]} if gc is not None else {}

                def coarse_run(route):
                    if route == "given":
                        pr = probes_all[:Q]
                        return lambda: ops.graph_search_seeded(_OPS_SPACE[a.space], q, gc._f32[:N], gc.graph, a.k, max(ef, a.k),
                                                               seeds=gc.seeds, probes=pr, width=width, max_iters=c_iters)

                    def run():
                        gc.coarse = route
                        return gc.search(q, a.k)
                    return run
                for r in range(a.rounds):
                    runs = [(t_gr, lambda: gr.search(q, a.k)), (t_ivf, lambda: ivf.search(q, a.k)), (t_flat, lambda: flat.search(q, a.k))]
                    runs += [(t_co[route], coarse_run(route)) for route in t_co]
                    for into, run in (runs if r % 2 == 0 else runs[::-1]):
                        into.append(timed(run, a.iters))
                print(json.dumps({"data": kind, "N": N, "d": d, "k": a.k, "R": gr.R, "ef": ef, "width": width, "max_iters": iters,
                                  "lds_bytes": lds, "Q": Q, "graph_ms": spread(t_gr), "ivf_ms": spread(t_ivf), "flat_ms": spread(t_flat),
                                  "recall10": rc, "cut": cut, "ivf_recall10": ivf_recall, "nlist": a.nlist, "nprobe": ivf.nprobe,
                                  **({"coarse_ms": {route: spread(v) for route, v in t_co.items()}, "coarse_recall10": c_rc,
                                      "coarse_cut": c_cut, "coarse_max_iters": c_iters, "seeds_per_list": gc.seeds_per_list}
                                     if gc is not None else {})}), flush=True)
    del flat, ivf, gr, gc, truth
    torch.cuda.empty_cache()
