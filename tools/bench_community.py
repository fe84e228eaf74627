#!/usr/bin/env python3
"""Community detection on the GPU box, step by step: python tools/bench_community.py [--N N] [--d D] [--min-size M]
[--data mixture manifold chain] [--tau-mixture T] [--tau-manifold T] [--chain-N N] [--chain-width W] [--rounds R] [--no-host]

Three corpora, all seeded: ``mixture`` and ``manifold`` are the corpora of tools/bench_graph.py (a Gaussian mixture of
--components centres, rows = centre + sigma * noise; rows on a --latent-dimensional linear manifold plus 0.05 noise), and
``chain``, --chain-N equally spaced points of a line seen through d Gaussian bumps (cosine falls with the distance along the
line alone), the threshold set half-way between the scores of neighbour --chain-width and the next, so that a row hits its
--chain-width neighbours on either side: every interior candidate has the same size, so the priority order runs along the line
and each accepted community waits for the one before it — the corpus made to need many rounds.  Per corpus one JSON line:
  range_ms        steps 1 and 2 (ops.community_candidates: the range search of the rows against themselves, the centres' hits
                  only, and the priority sort), one call, wall clock;
  C, T            candidate communities and their members;
  rounds_needed   rounds of the parallel de-overlap when nothing caps them;
  rounds_ms / serial_ms / default_ms   ops.community_select with max_rounds = 2^20 / 0 / the default: median [min, max] over
                  --rounds calls, the three ALTERNATING, wall clock with a synchronise on either side (the call reads back);
  default_rounds  rounds the default budget used (the serial finish ran iff it is below rounds_needed);
  host_ms         the same loop in host Python over the same CSR (sets, as sentence-transformers does), including the copy of
                  the CSR to the host; one run; its accepted set is compared with the device's;
  K, covered      communities found and rows in one.
Not part of bench.py."""
import argparse
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from text_similarity_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--N", type=int, default=100_000)
ap.add_argument("--d", type=int, default=384)
ap.add_argument("--min-size", type=int, default=10)
ap.add_argument("--components", type=int, default=2048)
ap.add_argument("--sigma", type=float, default=1.0)
ap.add_argument("--latent", type=int, default=16)
ap.add_argument("--tau-mixture", type=float, default=0.35)
ap.add_argument("--tau-manifold", type=float, default=0.7)
ap.add_argument("--chain-N", type=int, default=20_000)
ap.add_argument("--chain-width", type=int, default=32)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--data", nargs="+", default=["mixture", "manifold", "chain"], choices=["mixture", "manifold", "chain"])
ap.add_argument("--no-host", action="store_true")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_community.py measures on the GPU: no device found")
dev = "cuda:0"
d = a.d
g = torch.Generator(device=dev).manual_seed(97)
centres = torch.randn((a.components, d), generator=g, device=dev)
lift = torch.randn((a.latent, d), generator=g, device=dev)


def draw(kind, n):
    if kind == "chain":     # element k of row i: exp(-(p_i - k)^2 / 2), p_i = 4 + i (d - 8) / n; cos(i, j) ~ exp(-(p_i - p_j)^2 / 4)
        p = 4.0 + torch.arange(n, device=dev, dtype=torch.float64) * ((d - 8) / n)
        return torch.exp(-0.5 * (p[:, None] - torch.arange(d, device=dev, dtype=torch.float64)[None, :]) ** 2).float()
    noise = torch.randn((n, d), generator=g, device=dev)
    if kind == "manifold":
        return torch.randn((n, a.latent), generator=g, device=dev) @ lift + 0.05 * noise
    return centres[torch.randint(0, a.components, (n,), generator=g, device=dev)] + a.sigma * noise


def wall(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t) * 1e3


def spread(v):
    return [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]


def host_loop(plims, pmem, min_size):
    L, M = plims.cpu().tolist(), pmem.cpu().tolist()
    taken, acc = set(), []
    for c in range(len(L) - 1):
        free = [j for j in M[L[c]:L[c + 1]] if j not in taken]
        if len(free) >= min_size:
            acc.append(c)
            taken.update(free)
    return acc


for kind in a.data:
    n = a.chain_N if kind == "chain" else a.N
    tau = {"mixture": a.tau_mixture, "manifold": a.tau_manifold,
           "chain": math.exp(-0.25 * ((a.chain_width + 0.5) * (d - 8) / n) ** 2)}[kind]
    g.manual_seed(1000 + n % 997)
    x = draw(kind, n).contiguous()
    unit, rho = ops.l2norm_rows(x, return_rho=True)
    ops.community_candidates(unit[:256].contiguous(), x[:256].contiguous(), d, tau, a.min_size, rho=rho)      # warm-up
    (centre, plims, pmem, _), t_range = wall(lambda: ops.community_candidates(unit, x, d, tau, a.min_size, rho=rho))
    pm32 = pmem.to(torch.int32)
    forms = {"rounds": 1 << 20, "serial": 0, "default": None}
    times = {k: [] for k in forms}
    got = {}
    for r in range(a.rounds + 1):                            # (round 0 warms up and is dropped)
        for k in (list(forms) if r % 2 == 0 else list(forms)[::-1]):
            got[k], t = wall(lambda: ops.community_select(plims, pm32, n, a.min_size, forms[k]))
            if r:
                times[k].append(t)
    same = all(torch.equal(got[k][0], got["serial"][0]) and torch.equal(got[k][1], got["serial"][1]) for k in forms)
    line = {"data": kind, "N": n, "d": d, "tau": tau, "min_size": a.min_size, "range_ms": round(t_range, 3), "C": int(centre.numel()),
            "T": int(pmem.numel()), "rounds_needed": got["rounds"][2], "rounds_ms": spread(times["rounds"]),
            "serial_ms": spread(times["serial"]), "default_ms": spread(times["default"]), "default_rounds": got["default"][2],
            "forms_equal": same, "K": int(got["serial"][0].sum()), "covered": int(got["serial"][1].sum())}
    if not a.no_host:
        acc, t_host = wall(lambda: host_loop(plims, pmem, a.min_size))
        line["host_ms"] = round(t_host, 3)
        line["host_equal"] = acc == torch.nonzero(got["serial"][0]).reshape(-1).tolist()
    print(json.dumps(line), flush=True)
    del x, unit, centre, plims, pmem, pm32, got
    torch.cuda.empty_cache()
