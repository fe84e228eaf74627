"""GpuGraphIndex — a proximity-graph index resident in HBM (the family of hnswlib's base layer and of CAGRA) with the
hnswlib-shaped surface of :class:`text_similarity_amd.index.GpuFlatIndex`: every row keeps ``R`` neighbours, and a query walks
the graph from shared entry points with a beam of ``ef`` rows instead of reading the corpus.  Every score is the exact float32
score of ``GpuFlatIndex`` (:func:`ops.graph_search`), so a result is a subset of the exact one with identical scores, ordered
by (score desc, arrival row asc); what the index may lose is recall, never precision of a score.

Parameters, with hnswlib's names:
  ``M``                the degree, ``R = min(2 M, 64)`` (hnswlib's base layer holds 2 M links); ``M <= 0`` means hnswlib's 16.
  ``ef_construction``  the width of the exact kNN graph the build prunes, ``K0 = clamp(ef_construction, R, 128)``; 0 means
                       ``K0 = min(2 R, 128)``.
  ``set_ef(ef)``       the beam; a search uses ``max(ef, k)``, at most 1024.
  ``width``            beam entries expanded per iteration (1..4, default 4): iterations come out near ``ef / width``.
  ``max_iters``        None (default): ``min(ceil(3 ef / (2 width)) + 8, ops.graph_max_iters(E, R, width))`` — half as many
                       iterations again as a beam of ``ef`` needs to expand each entry once, plus eight, and never more than the
                       visited table in LDS can account for (E + max_iters width R <= 16 384 rows).

Build (:meth:`build`, run lazily before the first search): the exact kNN graph ``G0`` — the index's own exact search of the
rows against themselves, ``k = K0 + 1``, the row itself dropped (or the last entry, when duplicates pushed it out) —
pruned by detour count (:func:`ops.graph_prune`) and merged with its reverse edges (:func:`ops.graph_merge_reverse`).  The
entry points are ``min(n_entries, n)`` rows drawn by a ``torch.Generator`` seeded with ``seed``, stored in the index and its file.
The build is a self-search of the corpus: about a second for 1 M rows at the flat search's rate, plus the pruning.

Entry points (``entry``).  ``'shared'`` (default): the ``n_entries`` drawn rows above, the same for every query.  On a clustered
corpus the kNN graph falls apart into islands and a query whose island holds no entry point finds nothing; ``'coarse'`` starts
every query inside its own neighbourhood instead: the build clusters the live rows into ``nlist`` lists (0: ``max(1, min(4096,
int(sqrt(n))))``, never more than ``n``) with :func:`ivf_index.kmeans_centroids` — ``GpuIVFIndex``'s quantiser, bit for bit — or takes
``build(centroids=...)`` as given, and keeps a seed table ``[nlist, seeds_per_list]``: the stored rows of best score to each
centroid by the index's exact search, rank order, -1 where it pads.  A query enters through the seeds of its ``nprobe`` best
centroids (``set_nprobe``; ``nprobe * seeds_per_list`` in 1..256), :func:`ops.graph_search_seeded`.  The probes come from the
search kernel's own coarse phase, or — past ``COARSE_KERNEL_MAX_LISTS`` centroids or ``COARSE_KERNEL_MAX_QUERIES`` queries a
call — from the exact flat search of the queries against the centroids; both give the same probes.  A seed may be a
tombstone: tombstones route.

Insertion (``incremental``).  ``False`` (default): ``add_items`` after a build marks the graph stale and the next search rebuilds
it whole.  ``True``: ``add_items`` on a built graph INSERTS the new rows, in sub-batches of at most ``insert_batch`` rows (default
1024), each seeing the graph with the earlier ones linked in (:func:`ops.graph_insert`; include/tsim_graph_insert.h states the
step): the candidates of a new row are the index's own beam search of it over the graph as it stands — ``ef = k = K0``, the index's
``width`` and entry mode, ``max_iters`` by the rule above for ``ef = K0`` (:meth:`insert_params`) — merged with its exact neighbours
inside the sub-batch; the build's detour rule picks its R forward edges; and every row it chose re-ranks the back half of its own
edges with the newcomers by exact score.  Nothing is rebuilt or compacted: labels, tombstones, entry points, centroids and seed
table stay as they are (old seeds remain valid entry points; tombstones route the candidate search and are never linked to).
``build()`` still rebuilds everything and compacts.  ``build(insert_from=m)`` is the sub-quadratic build: the exact build, entry
points and quantiser included, over the first m live rows, the rest inserted by the same code path — id for id what "build over
m rows, then incremental ``add_items`` of the rest" gives.
``mark_deleted`` sets a tombstone: the row is still traversed (it routes the search) and never returned; a rebuild compacts
tombstones away.

On disk (``index.bin``, a numpy ``.npz`` without pickling): rows, labels, tombstones, the graph, the entry points, the
parameters (``incremental`` and ``insert_batch`` only from an incremental index: a file without them loads as non-incremental) and
``kind = 'graph'``; with ``entry='coarse'`` also the centroids, the seed table, ``entry``, ``nlist``, ``nprobe`` and
``seeds_per_list`` (a file without them loads as ``'shared'``); a file of another space or kind raises ``ValueError``.

Not here (``NotImplementedError``; ``GpuFlatIndex`` has them): ``filter=``, range and radius search.
"""
from __future__ import annotations

import os
from typing import Iterable, Optional, Tuple

import numpy as np
import torch

from . import ops

_OPS_SPACE = {"cosine": "cosine", "ip": "dot", "euclidean": "l2"}
_BUILD_CHUNK = 16384        # queries of one self-search call
# entry='coarse': where the probes come from.  The kernel's coarse phase costs a query 0.04 ms at 256 centroids, 0.09 - 0.11 at
# 1 024 and 0.31 - 0.34 at 4 096 (it scores them with the exact kernel, a workgroup a query); the flat search of the queries against
# the centroids, in launches of its own, 0.09 - 0.16 ms whatever their number (DESIGN.md "Graph index", *Per-query entry points*:
# 1 M x 384, Q = 1 / 16 / 256).  So the kernel up to 1 024 lists.  COARSE_KERNEL_MAX_QUERIES is no measured crossover: no call of more
# than 256 queries was measured, and beyond what was measured the index takes the flat route, whose cost does not grow with nlist.
COARSE_KERNEL_MAX_LISTS = 1024
COARSE_KERNEL_MAX_QUERIES = 256


def degree_params(M: int, ef_construction: int) -> Tuple[int, int]:
    """(R, K0) for hnswlib's ``M`` and ``ef_construction``."""
    M = int(M) if int(M) > 0 else 16
    R = min(2 * M, ops.GRAPH_MAX_DEGREE)
    K0 = min(2 * R, ops.GRAPH_PRUNE_MAX_K0) if int(ef_construction) <= 0 else min(max(int(ef_construction), R), ops.GRAPH_PRUNE_MAX_K0)
    return R, K0


class GpuGraphIndex:
    SPACES = ("cosine", "ip", "euclidean")
    KIND = "graph"

    def __init__(self, space: str = "cosine", dim: int = 0, M: int = 16, ef_construction: int = 0, ef: int = 64, width: int = 4,
                 n_entries: int = 64, max_iters: Optional[int] = None, device: Optional[torch.device] = None, seed: int = 0,
                 entry: str = "shared", nlist: int = 0, nprobe: int = 8, seeds_per_list: int = 4, incremental: bool = False,
                 insert_batch: int = 1024):
        if space not in self.SPACES:
            raise ValueError(f"GpuGraphIndex implements the spaces {self.SPACES}, not {space!r}")
        self.space = space
        self.dim = int(dim)
        self._check_dim()
        self.R, self.K0 = degree_params(M, ef_construction)
        if not 1 <= int(width) <= ops.GRAPH_MAX_WIDTH:
            raise ValueError(f"width={width} outside 1..{ops.GRAPH_MAX_WIDTH}")
        if not 1 <= int(n_entries) <= ops.GRAPH_MAX_ENTRIES:
            raise ValueError(f"n_entries={n_entries} outside 1..{ops.GRAPH_MAX_ENTRIES}")
        self.width, self.n_entries, self.max_iters, self.seed = int(width), int(n_entries), max_iters, int(seed)
        if entry not in ("shared", "coarse"):
            raise ValueError(f"entry={entry!r}: 'shared' or 'coarse'")
        if int(nlist) < 0:
            raise ValueError(f"nlist={nlist} < 0")
        self.entry, self.nlist, self.seeds_per_list = entry, int(nlist), int(seeds_per_list)
        self.nprobe = int(nprobe)                      # (entry='shared' ignores it and seeds_per_list, whatever they are)
        self._check_entry_budget()
        if int(insert_batch) < 1:
            raise ValueError(f"insert_batch={insert_batch} < 1")
        self.incremental, self.insert_batch = bool(incremental), int(insert_batch)
        self.coarse = "auto"                           # 'kernel' | 'flat': force one route of the probes (tools/bench_graph.py)
        self.ef = 1
        self.set_ef(ef)
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self._f32: Optional[torch.Tensor] = None       # [capacity, d] float32 rows in arrival order
        self._labels: Optional[torch.Tensor] = None    # [capacity] int64
        self._dead: Optional[torch.Tensor] = None      # [capacity] bool
        self._n = 0
        self._n_dead = 0
        self.graph: Optional[torch.Tensor] = None      # [n, R] int32, or None: stale
        self.entries: Optional[torch.Tensor] = None    # [E] int32
        self._row_ids = None                           # int32 [n] with -1 at the tombstones, or None: rebuild it
        self.centroids: Optional[torch.Tensor] = None  # entry='coarse': [T, d] float32, stale with the graph
        self.seeds: Optional[torch.Tensor] = None      # [T, seeds_per_list] int32
        self._given_centroids = None                   # what build(centroids=...) installed: kept across rebuilds
        self._coarse_ops = None                        # the centroids as the operands of the space's exact search

    # ------------------------------------------------------------------ hnswlib-shaped surface
    def init_index(self, max_elements: int, ef_construction: int = 0, M: int = 0):
        """hnswlib's call.  ``M`` and ``ef_construction`` set the degree and the build width (module docstring); 0 keeps what the
        constructor set."""
        if int(M) > 0 or int(ef_construction) > 0:
            R, K0 = degree_params(M if int(M) > 0 else self.R // 2, ef_construction)
            if (R, K0) != (self.R, self.K0):
                self.R, self.K0 = R, K0
                self.graph = None
        self._reserve(int(max_elements))

    def set_ef(self, ef: int):
        ef = int(ef)
        if ef <= 0:      # (the pipeline passes 0 when its parameters have no ef)
            return
        if ef > ops.GRAPH_MAX_EF:
            raise ValueError(f"ef={ef} outside 1..{ops.GRAPH_MAX_EF}")
        self.ef = ef

    def _check_entry_budget(self, nprobe: Optional[int] = None):
        """entry='coarse': a query starts from nprobe * seeds_per_list rows, 1..256 of them."""
        n = self.nprobe if nprobe is None else int(nprobe)
        if self.entry == "coarse" and (n < 1 or self.seeds_per_list < 1 or n * self.seeds_per_list > ops.GRAPH_MAX_ENTRIES):
            raise ValueError(f"nprobe={n} * seeds_per_list={self.seeds_per_list} outside 1..{ops.GRAPH_MAX_ENTRIES}")

    def set_nprobe(self, n: int):
        self._check_entry_budget(n)
        self.nprobe = int(n)

    def resize_index(self, new_size: int):
        self._reserve(int(new_size))

    def get_current_count(self) -> int:
        return self._n

    def num_live(self) -> int:
        return self._n - self._n_dead

    def add_items(self, data, ids: Optional[Iterable[int]] = None, num_threads: int = -1):
        x = torch.as_tensor(np.asarray(data) if not isinstance(data, torch.Tensor) else data)
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if self.dim == 0:
            self.dim = int(x.shape[1])
            self._check_dim()
        if x.shape[1] != self.dim:
            raise ValueError(f"expected width {self.dim}, got {x.shape[1]}")
        n = x.shape[0]
        if ids is None:
            ids = np.arange(self._n, self._n + n)
        lab = torch.as_tensor(np.asarray(list(ids), dtype=np.int64))
        if lab.numel() != n:
            raise ValueError("ids and data disagree in length")
        n0 = self._n
        insert = bool(n) and self.incremental and self.graph is not None and n0 > 0 and self.graph.shape[0] == n0
        if insert and self.entry == "coarse" and self.centroids is None:      # (as search: a graph from before the entry mode was set)
            self.build_coarse()
        self._reserve(self._n + n)
        self._f32[self._n:self._n + n] = x.to(self.device, dtype=torch.float32)
        self._labels[self._n:self._n + n] = lab.to(self.device)
        self._dead[self._n:self._n + n] = False
        self._n += n
        if insert:
            self._insert(n0)
        elif n:
            self.graph = None      # stale: rebuilt, whole, before the next search

    def mark_deleted(self, label: int):
        if self._n == 0:
            raise RuntimeError("label not found")
        hit = (self._labels[:self._n] == int(label)) & ~self._dead[:self._n]
        k = int(hit.sum())
        if k == 0:
            raise RuntimeError("label not found")      # as GpuFlatIndex and hnswlib
        self._dead[:self._n] |= hit
        self._n_dead += k
        self._row_ids = None

    def knn_query(self, data, k: int = 1, filter=None) -> Tuple[np.ndarray, np.ndarray]:
        """(labels [Q,k] int64, distances [Q,k] float32) best first, in ``GpuFlatIndex.knn_query``'s conventions."""
        labels, scores = self.search(data, k, filter=filter)
        if self.space == "euclidean":
            return labels.cpu().numpy(), scores.cpu().numpy()
        return labels.cpu().numpy(), (1.0 - scores).cpu().numpy()

    # ------------------------------------------------------------------ build
    def _operands(self, x: torch.Tensor):
        """``x`` as the stored operand of the space's exact search."""
        if self.space == "cosine":
            return ops.l2norm_rows(x, return_rho=True)
        return ops.dot_scaled_rows(x) if self.space == "ip" else ops.l2_rows(x)

    def _exact_search(self, q: torch.Tensor, x: torch.Tensor, k: int, operands=None) -> torch.Tensor:
        """idx [Q, k] int64 of the exact search of the rows ``q`` against the rows ``x`` (``operands``: ``_operands(x)``), -1 where
        it pads: (score desc, row asc), so a tie goes to the lower row."""
        d = self.dim
        operands = self._operands(x) if operands is None else operands
        if self.space == "cosine":
            half, rho = operands
            qhalf = (lambda a, b: half[a:b]) if q is x else (lambda a, b: ops.l2norm_rows(q[a:b]))      # (the self-search of the build)
            run = lambda a, b: ops.cosine_topk(qhalf(a, b), half, d, k, eq_f32=q[a:b], ec_f32=x, rho_c=rho)[1]
        elif self.space == "ip":
            half, rho, scale = operands
            run = lambda a, b: ops.dot_topk(ops.l2norm_rows(q[a:b]), half, d, k, eq_f32=q[a:b], ec_f32=x, rho_c=rho, scale_c=scale)[1]
        else:
            half, rho, scale = operands
            run = lambda a, b: ops.l2_topk(ops.l2_query_rows(q[a:b], scale), half, d, k, eq_f32=q[a:b], ec_f32=x, rho_c=rho,
                                           scale_c=scale)[1]
        n = q.shape[0]
        return torch.cat([run(a, min(a + _BUILD_CHUNK, n)) for a in range(0, n, _BUILD_CHUNK)], dim=0)

    def build_coarse(self, centroids=None):
        """(Re)build the coarse quantiser of ``entry='coarse'`` for the stored rows: the centroids (``centroids`` [T, d]: installed
        as given, and again at every rebuild; else k-means) and the seed table."""
        self._check_entry_budget()
        n, S = self._n, self.seeds_per_list
        x = self._f32[:n]
        if centroids is not None:
            c = torch.as_tensor(np.asarray(centroids) if not isinstance(centroids, torch.Tensor) else centroids)
            c = c.to(self.device, dtype=torch.float32).contiguous()
            if c.dim() != 2 or c.shape[0] < 1 or c.shape[1] != self.dim:
                raise ValueError(f"centroids must have shape (nlist >= 1, {self.dim}), got {tuple(c.shape)}")
            self._given_centroids = c
        if self._given_centroids is not None:
            c = self._given_centroids
        else:
            from .ivf_index import kmeans_centroids
            nlist = self.nlist if self.nlist > 0 else max(1, min(ops.GRAPH_MAX_COARSE_LISTS, int(n ** 0.5)))
            c = kmeans_centroids(x, min(nlist, n), self.space, self.seed)
        self.centroids, self._coarse_ops = c, self._operands(c)
        ks = min(S, n)
        seeds = torch.full((c.shape[0], S), -1, dtype=torch.int32, device=self.device)
        seeds[:, :ks] = self._exact_search(c, x, ks).to(torch.int32)
        self.seeds = seeds

    def knn_graph(self) -> torch.Tensor:
        """G0 [n, K0] int32 of the stored rows (tombstones compacted away first): each row's K0 best other rows, best first."""
        self._compact()
        n, K0 = self._n, self.K0
        idx = self._exact_search(self._f32[:n], self._f32[:n], K0 + 1)
        own = idx == torch.arange(n, device=self.device)[:, None]
        drop = torch.where(own.any(1), own.to(torch.int8).argmax(1), torch.full((n,), K0, device=self.device))
        keep = torch.arange(K0 + 1, device=self.device)[None, :] != drop[:, None]
        return idx[keep].view(n, K0).to(torch.int32).contiguous()

    def build(self, knn: Optional[torch.Tensor] = None, centroids=None, insert_from: Optional[int] = None):
        """(Re)build the graph and the entry points from the stored live rows.  ``knn``: what :meth:`knn_graph` returned for them
        (tools/bench_graph.py times the stages apart).  ``centroids`` (``entry='coarse'``): :meth:`build_coarse`.  ``insert_from``
        = m: the exact build over the first m live rows only, the rest inserted (module docstring)."""
        if centroids is not None and self.entry != "coarse":
            raise ValueError("build(centroids=...) needs entry='coarse'")
        self._compact()
        if insert_from is not None and 0 < int(insert_from) < self._n:
            if knn is not None:
                raise ValueError("build(insert_from=...) makes its own kNN graph of the first rows")
            n, self._n = self._n, int(insert_from)
            try:
                self.build(centroids=centroids)
            finally:
                self._n = n
            self._insert(int(insert_from))
            return
        n = self._n
        self.centroids = self.seeds = self._coarse_ops = None
        if n == 0:
            self.graph = torch.zeros((0, self.R), dtype=torch.int32, device=self.device)
            self.entries = torch.zeros((0,), dtype=torch.int32, device=self.device)
            return
        self.graph = ops.graph_merge_reverse(ops.graph_prune(self.knn_graph() if knn is None else knn, self.R)).contiguous()
        g = torch.Generator(device="cpu").manual_seed(self.seed)
        E = min(self.n_entries, n)
        self.entries = torch.randperm(n, generator=g)[:E].sort()[0].to(torch.int32).to(self.device)
        self._row_ids = None
        if self.entry == "coarse":
            self.build_coarse(centroids)

    def insert_params(self) -> Tuple[int, int]:
        """(ef, max_iters) of the candidate search of an insertion: ``ef = K0`` and :meth:`search_params`' rule for it, over the
        entry points the graph has."""
        E = self._n_probe() * self.seeds_per_list if self.entry == "coarse" else max(1, int(self.entries.numel()))
        fit = ops.graph_max_iters(E, self.R, self.width)
        iters = (3 * self.K0 + 2 * self.width - 1) // (2 * self.width) + 8 if self.max_iters is None else int(self.max_iters)
        return self.K0, max(1, min(iters, fit))

    def _insert(self, n0: int):
        """Link the stored rows n0 .. _n - 1 into the graph over the rows before them, ``insert_batch`` rows at a time."""
        n1 = self._n
        graph = torch.empty((n1, self.R), dtype=torch.int32, device=self.device)
        graph[:n0] = self.graph
        ef, iters = self.insert_params()
        for a in range(n0, n1, self.insert_batch):
            b = min(self.insert_batch, n1 - a)
            new = self._f32[a:a + b]
            row_ids = None
            if self._n_dead:
                ids = torch.arange(a, dtype=torch.int32, device=self.device)
                row_ids = torch.where(self._dead[:a], torch.full_like(ids, -1), ids)
            if self.entry == "coarse":
                P = self._n_probe()
                if self._kernel_coarse(b):
                    how = dict(seeded=dict(centroids=self.centroids, n_probe=P, seeds=self.seeds))
                else:
                    probes = self._exact_search(new, self.centroids, P, self._coarse_ops).to(torch.int32)
                    how = dict(seeded=dict(probes=probes, seeds=self.seeds))
            else:
                how = dict(entries=self.entries)
            ops.graph_insert(_OPS_SPACE[self.space], self._f32[:a + b], graph[:a + b], a, self.K0, width=self.width, max_iters=iters,
                             row_ids=row_ids, ef=ef, **how)
        self.graph = graph
        self._row_ids = None

    def search_params(self, k: int) -> Tuple[int, int]:
        """(ef, max_iters) a search for ``k`` results uses (module docstring)."""
        ef = max(self.ef, int(k))
        E = max(1, min(self.n_entries, self._n))
        if self.entry == "coarse":
            E = self._n_probe() * self.seeds_per_list
        fit = ops.graph_max_iters(E, self.R, self.width)
        iters = (3 * ef + 2 * self.width - 1) // (2 * self.width) + 8 if self.max_iters is None else int(self.max_iters)
        return ef, max(1, min(iters, fit))

    def _n_probe(self) -> int:
        return self.nprobe if self.centroids is None else min(self.nprobe, int(self.centroids.shape[0]))

    def _kernel_coarse(self, Q: int) -> bool:
        """Whether the search kernel finds the probes itself (module docstring); the other route gives the same probes."""
        T = int(self.centroids.shape[0])
        if T > ops.GRAPH_MAX_COARSE_LISTS or self.coarse == "flat":
            return False
        return self.coarse == "kernel" or (T <= COARSE_KERNEL_MAX_LISTS and Q <= COARSE_KERNEL_MAX_QUERIES)

    # ------------------------------------------------------------------ device-level API
    def search(self, data, k: int, filter=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(labels [Q,k] int64, scores [Q,k] float32) on the device, as ``GpuFlatIndex.search`` returns them, among the rows the
        beam search reaches; -1 / -inf pad ('euclidean': squared distances ascending, +inf pad) when it holds fewer than k live
        rows."""
        if filter is not None:
            raise NotImplementedError("GpuGraphIndex has no filtered search: GpuFlatIndex.search(filter=...) does")
        q = torch.as_tensor(np.asarray(data) if not isinstance(data, torch.Tensor) else data)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        qf = q.to(self.device, dtype=torch.float32).contiguous()
        k = int(k)
        if self.num_live() == 0 or qf.shape[0] == 0:
            return (torch.full((qf.shape[0], k), -1, dtype=torch.int64, device=self.device),
                    torch.full((qf.shape[0], k), float("inf" if self.space == "euclidean" else "-inf"), device=self.device))
        if self.graph is None:
            self.build()
        n = self._n
        if self._n_dead and self._row_ids is None:
            ids = torch.arange(n, dtype=torch.int32, device=self.device)
            self._row_ids = torch.where(self._dead[:n], torch.full_like(ids, -1), ids)
        if self.entry == "coarse" and self.centroids is None:      # (a graph loaded or built before the entry mode was set)
            self.build_coarse()
        ef, iters = self.search_params(k)
        row_ids = self._row_ids if self._n_dead else None
        if self.entry == "coarse":
            P = self._n_probe()
            if self._kernel_coarse(qf.shape[0]):
                how = dict(centroids=self.centroids, n_probe=P)
            else:
                how = dict(probes=self._exact_search(qf, self.centroids, P, self._coarse_ops).to(torch.int32))
            s, i = ops.graph_search_seeded(_OPS_SPACE[self.space], qf, self._f32[:n], self.graph, k, ef, seeds=self.seeds,
                                           width=self.width, max_iters=iters, row_ids=row_ids, **how)
        else:
            s, i = ops.graph_search(_OPS_SPACE[self.space], qf, self._f32[:n], self.graph, self.entries, k, ef, width=self.width,
                                    max_iters=iters, row_ids=row_ids)
        lab = torch.where(i >= 0, self._labels[i.clamp(min=0)], torch.full_like(i, -1))
        return lab, s

    def _unsupported(self, what):
        raise NotImplementedError(f"GpuGraphIndex has no {what}: GpuFlatIndex does")

    def range_search(self, data, threshold):
        self._unsupported("range_search")

    def range_query(self, data, threshold):
        self._unsupported("range_query")

    def radius_search(self, data, radius):
        self._unsupported("radius_search")

    def radius_query(self, data, radius):
        self._unsupported("radius_query")

    # ------------------------------------------------------------------ persistence
    def save_index(self, path: str):
        if self.graph is None:
            self.build()
        if os.path.isdir(path):
            path = os.path.join(path, "index.bin")
        n = self._n
        rows = self._f32[:n].cpu().numpy() if n else np.zeros((0, self.dim), np.float32)
        labels = self._labels[:n].cpu().numpy() if n else np.zeros((0,), np.int64)
        dead = self._dead[:n].cpu().numpy() if n else np.zeros((0,), bool)
        coarse = {}
        if self.entry == "coarse":
            if self.centroids is None and n:
                self.build_coarse()
            coarse = dict(entry=np.array(self.entry), nlist=np.int64(self.nlist), nprobe=np.int64(self.nprobe),
                          seeds_per_list=np.int64(self.seeds_per_list), given_centroids=np.bool_(self._given_centroids is not None),
                          centroids=self.centroids.cpu().numpy() if n else np.zeros((0, self.dim), np.float32),
                          seeds=self.seeds.cpu().numpy() if n else np.zeros((0, self.seeds_per_list), np.int32))
        # (optional keys: a non-incremental index writes exactly the arrays of a file from before insertion existed)
        insertion = dict(incremental=np.bool_(True), insert_batch=np.int64(self.insert_batch)) if self.incremental else {}
        with open(path, "wb") as f:
            np.savez(f, rows_f32=rows, labels=labels, dead=dead, graph=self.graph.cpu().numpy(), entries=self.entries.cpu().numpy(),
                     dim=np.int64(self.dim), space=np.array(self.space), R=np.int64(self.R), K0=np.int64(self.K0), ef=np.int64(self.ef),
                     width=np.int64(self.width), n_entries=np.int64(self.n_entries), seed=np.int64(self.seed),
                     kind=np.array(self.KIND), **coarse, **insertion)

    def load_index(self, path: str, max_elements: int = 0):
        if os.path.isdir(path):
            path = os.path.join(path, "index.bin")
        z = np.load(path, allow_pickle=False)
        kind = str(z["kind"]) if "kind" in z.files else "flat"
        if kind != self.KIND:
            raise ValueError(f"{path} holds a {kind!r} index, not a {self.KIND!r} one")
        space = str(z["space"])
        if space != self.space:
            raise ValueError(f"{path} holds a {space!r} index; this index is {self.space!r}")
        self.dim = int(z["dim"])
        self.R, self.K0, self.width = int(z["R"]), int(z["K0"]), int(z["width"])
        self.n_entries, self.seed = int(z["n_entries"]), int(z["seed"])
        self.set_ef(int(z["ef"]))
        self.incremental = bool(z["incremental"]) if "incremental" in z.files else False
        self.insert_batch = int(z["insert_batch"]) if "insert_batch" in z.files else 1024
        self._f32 = self._labels = self._dead = self._row_ids = None
        self._n = self._n_dead = 0
        rows = z["rows_f32"]
        n = rows.shape[0]
        self._reserve(max(n, int(max_elements)))
        if n:
            self._f32[:n] = torch.from_numpy(np.ascontiguousarray(rows)).to(self.device)
            self._labels[:n] = torch.from_numpy(z["labels"]).to(self.device)
            self._dead[:n] = torch.from_numpy(z["dead"]).to(self.device)
            self._n, self._n_dead = n, int(z["dead"].sum())
        self.graph = torch.from_numpy(np.ascontiguousarray(z["graph"], dtype=np.int32)).to(self.device)
        self.entries = torch.from_numpy(np.ascontiguousarray(z["entries"], dtype=np.int32)).to(self.device)
        if self.graph.shape != (n, self.R):
            raise ValueError(f"{path}: the graph is {tuple(self.graph.shape)}, the rows want ({n}, {self.R})")
        self.entry = str(z["entry"]) if "entry" in z.files else "shared"
        self.centroids = self.seeds = self._coarse_ops = self._given_centroids = None
        if self.entry == "coarse":
            self.nlist = int(z["nlist"]) if "nlist" in z.files else 0
            self.seeds_per_list = int(z["seeds_per_list"])
            self.set_nprobe(int(z["nprobe"]))
        if self.entry == "coarse" and n:      # (an empty index holds no quantiser: the first build makes it)
            self.centroids = torch.from_numpy(np.ascontiguousarray(z["centroids"], dtype=np.float32)).to(self.device)
            self.seeds = torch.from_numpy(np.ascontiguousarray(z["seeds"], dtype=np.int32)).to(self.device)
            if self.centroids.dim() != 2 or self.centroids.shape[0] < 1 or self.centroids.shape[1] != self.dim or \
                    self.seeds.shape != (self.centroids.shape[0], self.seeds_per_list):
                raise ValueError(f"{path}: centroids {tuple(self.centroids.shape)} and seeds {tuple(self.seeds.shape)} do not fit")
            self._coarse_ops = self._operands(self.centroids)
            if "given_centroids" in z.files and bool(z["given_centroids"]):
                self._given_centroids = self.centroids

    # ------------------------------------------------------------------ internals
    def _check_dim(self):
        if self.dim > 768 or (self.space == "euclidean" and self.dim > ops.L2_MAX_DIM):
            raise ValueError(f"the {self.space!r} space takes rows of width <= {ops.L2_MAX_DIM if self.space == 'euclidean' else 768}, "
                             f"not {self.dim}")

    def _reserve(self, n: int):
        if self.dim == 0:
            return
        cap = 0 if self._f32 is None else self._f32.shape[0]
        if n <= cap:
            return
        new_cap = max(n, 2 * cap, 1024)
        f32 = torch.zeros((new_cap, self.dim), dtype=torch.float32, device=self.device)
        labels = torch.full((new_cap,), -1, dtype=torch.int64, device=self.device)
        dead = torch.zeros((new_cap,), dtype=torch.bool, device=self.device)
        if self._f32 is not None and self._n:
            f32[:self._n] = self._f32[:self._n]
            labels[:self._n] = self._labels[:self._n]
            dead[:self._n] = self._dead[:self._n]
        self._f32, self._labels, self._dead = f32, labels, dead

    def _compact(self):
        """Drop the tombstones (only a rebuild does: the graph's row numbers would no longer hold)."""
        if self._n_dead == 0:
            return
        keep = (~self._dead[:self._n]).nonzero(as_tuple=False).squeeze(1)
        m = keep.numel()
        self._f32[:m] = self._f32[keep]
        self._labels[:m] = self._labels[keep]
        self._dead[:self._n] = False
        self._n, self._n_dead = m, 0
        self.graph = None
        self._row_ids = None
