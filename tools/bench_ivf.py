#!/usr/bin/env python3
"""GpuIVFIndex against GpuFlatIndex on the GPU box: python tools/bench_ivf.py [--N ...] [--d D] [--Q ...] [--nlist ...]
[--nprobe ...] [--k K] [--rounds R] [--iters I] [--space cosine|ip|euclidean] [--points-per-list P]

The rows are a seeded Gaussian mixture generated here (--components centres of unit variance per element, rows = centre + sigma *
noise), the queries fresh draws from the same mixture.  For every N one flat index, for every (N, nlist) one IVF index trained on
a seeded sample of P * nlist rows; then one JSON line per cell (Q, nprobe):
  ivf_ms / flat_ms   ms per ``search`` call of the two indexes on the same queries: median [min, max] over R rounds, the two
                     indexes ALTERNATING inside every round, I calls timed per round between device events;
  scan_ms            the same for ops.ivf_scan_topk alone (no coarse search, no label gather), and scan_GBs, the float32 bytes of
                     the probed lists (summed over the (query, probe) pairs) over that time;
  recall10           recall@10 of the IVF result against the flat result, on a fixed set of 256 queries per (N, nlist, nprobe).
Not part of bench.py."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from text_similarity_amd import ops
from text_similarity_amd.index import GpuFlatIndex
from text_similarity_amd.ivf_index import _OPS_SPACE, GpuIVFIndex

ap = argparse.ArgumentParser()
ap.add_argument("--N", nargs="+", type=int, default=[1_000_000, 16_000_000])
ap.add_argument("--d", type=int, default=384)
ap.add_argument("--Q", nargs="+", type=int, default=[1, 16, 256])
ap.add_argument("--nlist", nargs="+", type=int, default=[1024, 4096])
ap.add_argument("--nprobe", nargs="+", type=int, default=[1, 8, 32])
ap.add_argument("--k", type=int, default=10)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--space", default="cosine", choices=GpuIVFIndex.SPACES)
ap.add_argument("--components", type=int, default=4096)
ap.add_argument("--sigma", type=float, default=1.0)
ap.add_argument("--points-per-list", type=int, default=64)
ap.add_argument("--niter", type=int, default=10)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_ivf.py measures on the GPU: no device found")
dev = "cuda:0"
d = a.d
g = torch.Generator(device=dev).manual_seed(97)
centres = torch.randn((a.components, d), generator=g, device=dev)


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


for N in a.N:
    flat = GpuFlatIndex(a.space, d, device=dev)
    flat.init_index(N)
    ivfs = {nl: GpuIVFIndex(a.space, d, nl, device=dev, seed=1) for nl in a.nlist}
    sample = draw(min(N, a.points_per_list * max(a.nlist)))
    for nl, ix in ivfs.items():
        ix.train(sample, niter=a.niter, max_points_per_list=a.points_per_list)
    del sample
    for nl in a.nlist:      # (one IVF index at a time beside the flat one: each holds the float32 rows twice)
        ix = ivfs.pop(nl)
        ix.init_index(N)
        g.manual_seed(1000 + N % 997)      # the same rows for every index of this N
        for r0 in range(0, N, 1 << 20):
            x = draw(min(1 << 20, N - r0))
            ids = torch.arange(r0, r0 + x.shape[0]).numpy()
            ix.add_items(x, ids)
            if flat.get_current_count() < N:
                flat.add_items(x, ids)
        del x
        q_all = draw(max(256, max(a.Q)))
        truth = flat.search(q_all[:256], 10)[0]
        rows, list_off, row_ids, longest = ix._pack()
        lens = list_off[1:] - list_off[:-1]
        for nprobe in a.nprobe:
            if nprobe > nl:
                continue
            ix.set_nprobe(nprobe)
            got = ix.search(q_all[:256], 10)[0]
            recall = float((got[:, :, None] == truth[:, None, :]).any(2).float().sum(1).mean()) / 10.0
            for Q in a.Q:
                q = q_all[:Q].contiguous()
                probes = ix._coarse(q, nprobe).contiguous()
                scanned = int(lens[probes.clamp(min=0)].sum()) * d * 4
                t_ivf, t_flat, t_scan = [], [], []
                for r in range(a.rounds):
                    runs = [(t_ivf, lambda: ix.search(q, a.k)), (t_flat, lambda: flat.search(q, a.k)),
                            (t_scan, lambda: ops.ivf_scan_topk(_OPS_SPACE[a.space], q, rows, list_off, row_ids, probes, a.k,
                                                               max_list_len=longest))]
                    for into, run in (runs if r % 2 == 0 else runs[::-1]):
                        into.append(timed(run, a.iters))
                print(json.dumps({"space": a.space, "N": N, "d": d, "k": a.k, "nlist": nl, "nprobe": nprobe, "Q": Q,
                                  "ivf_ms": spread(t_ivf), "flat_ms": spread(t_flat), "scan_ms": spread(t_scan),
                                  "scan_GBs": round(scanned / statistics.median(t_scan) / 1e6, 1), "recall10": round(recall, 4),
                                  "longest_list": longest, "mean_list": round(N / nl, 1)}), flush=True)
        del ix, rows, list_off, row_ids, truth
        torch.cuda.empty_cache()
    del flat
    torch.cuda.empty_cache()
