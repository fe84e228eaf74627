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

NOT incremental: ``add_items`` after a build marks the graph stale and the next search rebuilds it whole.  ``mark_deleted`` sets
a tombstone: the row is still traversed (it routes the search) and never returned; a rebuild compacts tombstones away.

On disk (``index.bin``, a numpy ``.npz`` without pickling): rows, labels, tombstones, the graph, the entry points, the
parameters and ``kind = 'graph'``; a file of another space or kind raises ``ValueError``.

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
                 n_entries: int = 64, max_iters: Optional[int] = None, device: Optional[torch.device] = None, seed: int = 0):
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
        self._reserve(self._n + n)
        self._f32[self._n:self._n + n] = x.to(self.device, dtype=torch.float32)
        self._labels[self._n:self._n + n] = lab.to(self.device)
        self._dead[self._n:self._n + n] = False
        self._n += n
        if n:
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
    def _self_search(self, x: torch.Tensor, k: int) -> torch.Tensor:
        """idx [n, k] int64 of the exact search of the rows against themselves, in the index's space."""
        d = self.dim
        if self.space == "cosine":
            half, rho = ops.l2norm_rows(x, return_rho=True)
            run = lambda a, b: ops.cosine_topk(half[a:b], half, d, k, eq_f32=x[a:b], ec_f32=x, rho_c=rho)[1]
        elif self.space == "ip":
            half, rho, scale = ops.dot_scaled_rows(x)
            run = lambda a, b: ops.dot_topk(ops.l2norm_rows(x[a:b]), half, d, k, eq_f32=x[a:b], ec_f32=x, rho_c=rho, scale_c=scale)[1]
        else:
            half, rho, scale = ops.l2_rows(x)
            run = lambda a, b: ops.l2_topk(ops.l2_query_rows(x[a:b], scale), half, d, k, eq_f32=x[a:b], ec_f32=x, rho_c=rho,
                                           scale_c=scale)[1]
        n = x.shape[0]
        return torch.cat([run(a, min(a + _BUILD_CHUNK, n)) for a in range(0, n, _BUILD_CHUNK)], dim=0)

    def knn_graph(self) -> torch.Tensor:
        """G0 [n, K0] int32 of the stored rows (tombstones compacted away first): each row's K0 best other rows, best first."""
        self._compact()
        n, K0 = self._n, self.K0
        idx = self._self_search(self._f32[:n], K0 + 1)
        own = idx == torch.arange(n, device=self.device)[:, None]
        drop = torch.where(own.any(1), own.to(torch.int8).argmax(1), torch.full((n,), K0, device=self.device))
        keep = torch.arange(K0 + 1, device=self.device)[None, :] != drop[:, None]
        return idx[keep].view(n, K0).to(torch.int32).contiguous()

    def build(self, knn: Optional[torch.Tensor] = None):
        """(Re)build the graph and the entry points from the stored live rows.  ``knn``: what :meth:`knn_graph` returned for them
        (tools/bench_graph.py times the stages apart)."""
        self._compact()
        n = self._n
        if n == 0:
            self.graph = torch.zeros((0, self.R), dtype=torch.int32, device=self.device)
            self.entries = torch.zeros((0,), dtype=torch.int32, device=self.device)
            return
        self.graph = ops.graph_merge_reverse(ops.graph_prune(self.knn_graph() if knn is None else knn, self.R)).contiguous()
        g = torch.Generator(device="cpu").manual_seed(self.seed)
        E = min(self.n_entries, n)
        self.entries = torch.randperm(n, generator=g)[:E].sort()[0].to(torch.int32).to(self.device)
        self._row_ids = None

    def search_params(self, k: int) -> Tuple[int, int]:
        """(ef, max_iters) a search for ``k`` results uses (module docstring)."""
        ef = max(self.ef, int(k))
        E = max(1, min(self.n_entries, self._n))
        fit = ops.graph_max_iters(E, self.R, self.width)
        iters = (3 * ef + 2 * self.width - 1) // (2 * self.width) + 8 if self.max_iters is None else int(self.max_iters)
        return ef, max(1, min(iters, fit))

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
        ef, iters = self.search_params(k)
        s, i = ops.graph_search(_OPS_SPACE[self.space], qf, self._f32[:n], self.graph, self.entries, k, ef, width=self.width,
                                max_iters=iters, row_ids=self._row_ids if self._n_dead else None)
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
        with open(path, "wb") as f:
            np.savez(f, rows_f32=rows, labels=labels, dead=dead, graph=self.graph.cpu().numpy(), entries=self.entries.cpu().numpy(),
                     dim=np.int64(self.dim), space=np.array(self.space), R=np.int64(self.R), K0=np.int64(self.K0), ef=np.int64(self.ef),
                     width=np.int64(self.width), n_entries=np.int64(self.n_entries), seed=np.int64(self.seed),
                     kind=np.array(self.KIND))

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
