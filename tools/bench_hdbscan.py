#!/usr/bin/env python3
"""HDBSCAN on the GPU box, stage by stage: python tools/bench_hdbscan.py [--N N ...] [--d D] [--data mixture gauss]
[--min-cluster-size M] [--min-samples S] [--rounds R] [--sklearn-max-N N]

Two corpora, both seeded: ``mixture`` is the clustered generator of tools/bench_community.py (a Gaussian mixture of --components
centres, rows = centre + sigma * noise) and ``gauss`` plain Gaussian rows (no structure: every row is noise or one cluster).
Per (corpus, N) one JSON line, wall clock with a synchronise on either side, median [min, max] over --rounds runs after one
warm-up (one run, no warm-up, from N = 50 000 up):
  core2_ms     the half operands and ops.l2_topk of the rows against themselves at k = min_samples, last column;
  mst_ms       ops.mst_prim: N - 1 steps of two launches, enqueued without a read in between;
  step_us      mst_ms / (N - 1);
  readback_ms  the three edge arrays to the host;
  tree_ms      ops.hdbscan_tree_labels on the host;
  total_ms     ops.hdbscan end to end (its own run, including the finiteness check and the copy of the labels);
  clusters, noise   of that run;
  sklearn_ms   sklearn.cluster.HDBSCAN(min_cluster_size, min_samples, algorithm="brute") on the same rows as float64 on the host,
               one run, where scikit-learn is importable and N <= --sklearn-max-N; sklearn_ari: adjusted Rand index of the two
               labelings (separated clusters: 1.0; elsewhere float32 against float64 distances and tie orders may move a label).
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

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, nargs="+", default=[5000, 20000, 100000])
ap.add_argument("--d", type=int, default=384)
ap.add_argument("--min-cluster-size", type=int, default=15)
ap.add_argument("--min-samples", type=int, default=None)
ap.add_argument("--components", type=int, default=2048)
ap.add_argument("--sigma", type=float, default=1.0)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--data", nargs="+", default=["mixture", "gauss"], choices=["mixture", "gauss"])
ap.add_argument("--sklearn-max-N", type=int, default=20000)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_hdbscan.py measures on the GPU: no device found")
dev = "cuda:0"
d, mcs = a.d, a.min_cluster_size
ms = mcs if a.min_samples is None else a.min_samples
g = torch.Generator(device=dev).manual_seed(97)
centres = torch.randn((a.components, d), generator=g, device=dev)


def draw(kind, n):
    noise = torch.randn((n, d), generator=g, device=dev)
    if kind == "gauss":
        return noise
    return centres[torch.randint(0, a.components, (n,), generator=g, device=dev)] + a.sigma * noise


def wall(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def spread(v):
    return [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]


def core2_of(x):
    ec, rho, maxnorm = ops.l2_rows(x)
    dist, _ = ops.l2_topk(ops.l2_query_rows(x, maxnorm), ec, d, ms, x, x, rho, maxnorm)
    return dist[:, ms - 1].contiguous()


try:
    from sklearn.cluster import HDBSCAN
    from sklearn.metrics import adjusted_rand_score
except ImportError:
    HDBSCAN = None

for kind in a.data:
    for n in a.N:
        g.manual_seed(1000 + n % 997)
        x = draw(kind, n).contiguous()
        rounds = a.rounds if n < 50000 else 1
        t = {k: [] for k in ("core2", "mst", "readback", "tree", "total")}
        for r in range(rounds + (1 if n < 50000 else 0)):
            core2, t_core = wall(lambda: core2_of(x))
            edges, t_mst = wall(lambda: ops.mst_prim(x, core2))
            host, t_read = wall(lambda: tuple(e.cpu().numpy() for e in edges))
            (labels, k), t_tree = wall(lambda: ops.hdbscan_tree_labels(*host, n, mcs))
            got, t_total = wall(lambda: ops.hdbscan(x, mcs, ms))
            if r or n >= 50000:
                for name, v in zip(t, (t_core, t_mst, t_read, t_tree, t_total)):
                    t[name].append(v)
        assert (got.cpu().numpy() == labels).all()
        line = {"data": kind, "N": n, "d": d, "min_cluster_size": mcs, "min_samples": ms, **{f"{k}_ms": spread(v) for k, v in t.items()},
                "step_us": round(statistics.median(t["mst"]) * 1e3 / max(n - 1, 1), 3), "clusters": k, "noise": int((labels < 0).sum())}
        if HDBSCAN is not None and n <= a.sklearn_max_N:
            x64 = x.cpu().numpy().astype("float64")
            t0 = time.perf_counter()
            sk = HDBSCAN(min_cluster_size=mcs, min_samples=ms, algorithm="brute").fit(x64).labels_
            line["sklearn_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            line["sklearn_ari"] = round(float(adjusted_rand_score(sk, labels)), 6)
            line["sklearn_clusters"] = int(sk.max()) + 1
        print(json.dumps(line), flush=True)
        del x, core2, edges, got
        torch.cuda.empty_cache()
