"""GpuFlatIndex — an exact cosine index resident in HBM with the call surface the reference uses from
``hnswlib.Index(space='cosine')`` (/root/reference/src/pipeline/search_pipeline.py:105-169): ``init_index``,
``add_items``, ``knn_query``, ``range_query`` (every row within a threshold; not in hnswlib), ``mark_deleted``, ``resize_index``, ``save_index`` / ``load_index``, ``get_current_count``,
``set_ef``.  Every query is a brute-force pass of the fused MFMA cosine + top-k kernel, so results are exact (hnswlib's are
approximate) and ordered by (score desc, label-row asc).

Layout: float32 rows ``[capacity, d]`` as given (the reference's scores are cosines of these) + their unit float16 rows
``[capacity, pad_dim(d)]`` (what the MFMA kernel streams to select candidates) + int64 labels + a tombstone mask.
Deleting marks a tombstone; the matrices are compacted (one device gather) before the next query, so deleted rows cost
nothing afterwards and labels stay stable.  On disk (``index.bin``, a numpy ``.npz`` written without pickling): the
float32 live rows, their labels, ``d`` (unit rows are recomputed on load; a file written by the first version of this
index holds bf16 unit rows only, which then ARE the float32 rows).  k <= 1024, d <= 768.

``space='ip'`` ranks by inner product instead (hnswlib's space for dot-product models; ``knn_query`` distances are
``1 - q.c``): the half rows are the float32 rows divided by one power of two S >= the largest row norm
(:func:`ops.dot_scaled_rows`), and an ``add_items`` batch that raises S re-derives all of them.  Rows with a non-finite
element are refused there.  The file records the space; a file without it is a cosine index, and loading a file of the
other space raises ``ValueError``.

``space='euclidean'`` ranks by Euclidean distance (hnswlib's and faiss' default space; ``knn_query`` returns SQUARED distances,
ascending, hnswlib's l2 convention; ``search`` pads with -1 / +inf): the half rows are one element wider than the float32 rows
(:func:`ops.l2_rows`), so d <= 767, and they follow the 'ip' rules — one power of two from the largest row norm, re-derived
when a batch raises it, non-finite rows refused.  ``radius_search`` / ``radius_query`` return every row within a SQUARED radius
(faiss' ``range_search`` in this space); ``range_search`` means "score >= threshold" and stays undefined here.  The name
``'l2'`` stays refused, as it was before this space existed (callers test for that).
"""
from __future__ import annotations

import math
import os
from typing import Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops


class GpuFlatIndex:
    SPACES = ("cosine", "ip", "euclidean")

    def __init__(self, space: str = "cosine", dim: int = 0, device: Optional[torch.device] = None):
        if space not in self.SPACES:
            raise ValueError(f"GpuFlatIndex implements the spaces {self.SPACES}, not {space!r}")
        self.space = space
        self.dim = int(dim)
        self._check_dim()
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self._rows: Optional[torch.Tensor] = None      # [capacity, ld] float16 unit rows
        self._f32: Optional[torch.Tensor] = None       # [capacity, d] float32 rows as given
        self._labels: Optional[torch.Tensor] = None    # [capacity] int64
        self._dead: Optional[torch.Tensor] = None      # [capacity] bool
        self._rho: Optional[torch.Tensor] = None       # [1] float32: largest rounding residual of any unit row ever stored
        self._maxnorm: Optional[torch.Tensor] = None   # ip: [1] float32 max-norm word of every row ever stored (S derives from it)
        self._n = 0
        self._n_dead = 0

    # ------------------------------------------------------------------ hnswlib-shaped surface
    def init_index(self, max_elements: int, ef_construction: int = 0, M: int = 0):
        self._reserve(int(max_elements))

    def set_ef(self, ef: int):      # exact search: nothing to tune
        pass

    def resize_index(self, new_size: int):
        self._reserve(int(new_size))

    def get_current_count(self) -> int:
        """rows ever added and not yet compacted away + live rows == hnswlib's count of inserted elements"""
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
        xf = x.to(self.device, dtype=torch.float32).contiguous()
        if self._rho is None:
            self._rho = ops.new_rho(self.device)
        if self.space in ("ip", "euclidean"):
            unit = self._ip_rows(xf)
        else:
            unit = ops.l2norm_rows(xf, rho=self._rho)   # the word only grows: deleted rows leave the bound conservative
        self._reserve(self._n + n)
        self._rows[self._n:self._n + n] = unit
        self._f32[self._n:self._n + n] = xf
        self._labels[self._n:self._n + n] = lab.to(self.device)
        self._dead[self._n:self._n + n] = False
        self._n += n

    def mark_deleted(self, label: int):
        if self._n == 0:
            raise RuntimeError("label not found")
        hit = (self._labels[:self._n] == int(label)) & ~self._dead[:self._n]
        k = int(hit.sum())
        if k == 0:
            raise RuntimeError("label not found")      # hnswlib raises RuntimeError too (search_pipeline.py:167)
        self._dead[:self._n] |= hit
        self._n_dead += k

    def knn_query(self, data, k: int = 1, filter=None) -> Tuple[np.ndarray, np.ndarray]:
        """(labels [Q,k] int64, distances [Q,k] float32 = 1 - cosine, 1 - q.c for 'ip', or the squared distance for 'euclidean'),
        best first — hnswlib's return convention.  ``filter``: see :meth:`search` (hnswlib's ``filter=callable`` among its forms)."""
        labels, scores = self.search(data, k, filter=filter)
        if self.space == "euclidean":
            return labels.cpu().numpy(), scores.cpu().numpy()
        return labels.cpu().numpy(), (1.0 - scores).cpu().numpy()

    # ------------------------------------------------------------------ device-level API
    def search(self, data, k: int, filter=None, filter_plan: Optional[str] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(labels [Q,k] int64, scores [Q,k] float32) on the device; -1 / -inf pad when fewer than k live rows.  'euclidean': the
        scores are squared distances, ascending, padded with +inf.
        ``filter`` restricts the search to the rows it allows — exact, same scores and tie rule (row asc) as the unfiltered call:
        a 1-D int array / tensor of allowed labels (faiss ``IDSelectorBatch``); a callable ``label -> bool`` (hnswlib's form,
        evaluated on the host over the live labels); a ``list`` of Q label arrays, or a ``tuple`` ``(lims [Q+1], labels)``, for
        one allow-list per query.  Unknown labels are ignored, deleted rows never match, fewer than k matches pad.
        ``filter_plan``: ``"list"`` or ``"compact"`` forces the regime of a shared allow-list (:meth:`filter_plan` chooses)."""
        self._compact()
        q = torch.as_tensor(np.asarray(data) if not isinstance(data, torch.Tensor) else data)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        qf = q.to(self.device, dtype=torch.float32).contiguous()
        euclid = self.space == "euclidean"
        if filter is not None:
            return self._search_filtered(qf, int(k), filter, filter_plan)
        qn = None if euclid else ops.l2norm_rows(qf)     # (euclidean: the query rows need the corpus' word, below)
        if self._n == 0:
            Q = q.shape[0]
            return (torch.full((Q, k), -1, dtype=torch.int64, device=self.device),
                    torch.full((Q, k), float("inf" if euclid else "-inf"), device=self.device))
        if euclid:
            s, i = ops.l2_topk(ops.l2_query_rows(qf, self._maxnorm), self._rows[:self._n], self.dim, k, eq_f32=qf,
                               ec_f32=self._f32[:self._n], rho_c=self._rho, scale_c=self._maxnorm)
        elif self.space == "ip":
            s, i = ops.dot_topk(qn, self._rows[:self._n], self.dim, k, eq_f32=qf, ec_f32=self._f32[:self._n], rho_c=self._rho,
                                scale_c=self._maxnorm)
        else:
            s, i = ops.cosine_topk(qn, self._rows[:self._n], self.dim, k, eq_f32=qf, ec_f32=self._f32[:self._n],
                                   rho_c=self._rho)
        lab = torch.where(i >= 0, self._labels[i.clamp(min=0)], torch.full_like(i, -1))
        return lab, s

    # The byte model of :meth:`filter_plan`: what the compact regime costs before its search reads a row (two gathers, the
    # queries' unit rows, the launches of the ordinary search), in bytes of the list kernel's traffic.  Set from the table in
    # DESIGN.md §7 (MI355X, N = 1 M, d = 384, k = 10; ms per call list / compact): Q = 16: n = 10 k 0.93 / 0.91, 100 k 1.32 / 1.66,
    # 500 k 3.56 / 1.46; Q = 256: 10 k 1.34 / 0.88, 100 k 6.79 / 1.37; Q = 4 096: 10 k 9.44 / 0.96.  The list regime still wins
    # at Q n d 4 = 2.5e9 B and has lost at 3.9e9 B: the crossover lies between, about 0.6 ms of the list kernel's 5 TB/s.
    FILTER_COMPACT_FIXED_BYTES = 3 << 30

    def filter_plan(self, Q: int, n_allowed: int) -> str:
        """``"list"`` or ``"compact"``: the regime :meth:`search` takes for ONE allow-list of ``n_allowed`` rows shared by ``Q``
        queries.  Pure host arithmetic on a byte model: the list kernel (:func:`ops.cosine_list_topk`) reads Q n d 4 bytes — every
        query gathers every allowed float32 row; the compact regime reads and writes the allowed half and float32 rows once,
        2 n (2 ld + 4 d) bytes, runs the space's ordinary MFMA search on the temporary, whose traffic does not grow with Q, and
        pays a fixed cost.  Monotone: more queries or more rows never turn "compact" back into "list"."""
        d = self.dim or 384
        ld = ops.pad_dim(d + 1 if self.space == "euclidean" else d)
        Q, n = int(Q), int(n_allowed)
        return "list" if Q * n * d * 4 <= self.FILTER_COMPACT_FIXED_BYTES + 2 * n * (2 * ld + 4 * d) else "compact"

    def _filter_rows(self, filt, Q: int):
        """rows (device int64) and lims (None: one list for all queries) of a filter; per-query lists carry -1 for labels the
        index does not hold."""
        n = self._n
        labels = self._labels[:n]
        if callable(filt):
            lab = labels.cpu().numpy()
            keep = np.fromiter((bool(filt(int(x))) for x in lab), dtype=bool, count=lab.shape[0])
            return torch.from_numpy(np.flatnonzero(keep)).to(self.device), None
        lims = None
        if isinstance(filt, tuple):
            if len(filt) != 2:
                raise ValueError("filter: a tuple is (lims [Q+1], labels)")
            lims = torch.as_tensor(np.asarray(filt[0]) if not isinstance(filt[0], torch.Tensor) else filt[0])
            lims = lims.to(self.device, dtype=torch.int64)
            if lims.shape != (Q + 1,):
                raise ValueError(f"filter: lims must have {Q + 1} entries for {Q} queries")
            filt = filt[1]
        elif isinstance(filt, list) and len(filt) and np.ndim(filt[0]) > 0:
            if len(filt) != Q:
                raise ValueError(f"filter: {len(filt)} allow-lists for {Q} queries")
            parts = [np.asarray(p.cpu() if isinstance(p, torch.Tensor) else p, dtype=np.int64).reshape(-1) for p in filt]
            lims = torch.from_numpy(np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.int64)).to(self.device)
            filt = np.concatenate(parts) if parts else np.zeros((0,), np.int64)
        lab = torch.as_tensor(np.asarray(filt) if not isinstance(filt, torch.Tensor) else filt)
        if lab.dim() != 1 or lab.dtype.is_floating_point or lab.dtype == torch.bool:
            raise ValueError("filter: expected a 1-D integer array of labels, a callable, a list of Q label arrays or (lims, labels)")
        lab = lab.to(self.device, dtype=torch.int64)
        if lims is None:
            return torch.isin(labels, lab).nonzero(as_tuple=False).squeeze(1), None      # ascending rows
        if n == 0 or lab.numel() == 0:
            return torch.full_like(lab, -1), lims
        sl, order = torch.sort(labels)
        pos = torch.searchsorted(sl, lab).clamp(max=n - 1)
        return torch.where(sl[pos] == lab, order[pos], torch.full_like(lab, -1)), lims

    def _search_filtered(self, qf: torch.Tensor, k: int, filt, plan: Optional[str]):
        if plan not in (None, "list", "compact"):
            raise ValueError(f"filter_plan must be 'list' or 'compact', not {plan!r}")
        Q = qf.shape[0]
        euclid = self.space == "euclidean"
        pad = (torch.full((Q, k), -1, dtype=torch.int64, device=self.device),
               torch.full((Q, k), float("inf" if euclid else "-inf"), device=self.device))
        if self._n == 0 or Q == 0:
            return pad
        rows, lims = self._filter_rows(filt, Q)
        if lims is None and rows.numel() == 0:
            return pad
        n = self._n
        if lims is not None or (plan or self.filter_plan(Q, rows.numel())) == "list":
            fn = ops.l2_list_topk if euclid else ops.dot_list_topk if self.space == "ip" else ops.cosine_list_topk
            # (a shared list comes from nonzero(): distinct and ascending already)
            s, i = fn(qf, self._f32[:n], rows, lims, k=k, assume_unique=lims is None)
        else:
            # compact: the allowed rows, in row order, as a temporary index; positions in it map back through `rows`, and
            # because the gather keeps the order, (score, position) ranks exactly as (score, row) does
            half, f32 = self._rows[:n].index_select(0, rows), self._f32[:n].index_select(0, rows)
            if euclid:
                s, i = ops.l2_topk(ops.l2_query_rows(qf, self._maxnorm), half, self.dim, k, eq_f32=qf, ec_f32=f32, rho_c=self._rho,
                                   scale_c=self._maxnorm)
            elif self.space == "ip":
                s, i = ops.dot_topk(ops.l2norm_rows(qf), half, self.dim, k, eq_f32=qf, ec_f32=f32, rho_c=self._rho,
                                    scale_c=self._maxnorm)
            else:
                s, i = ops.cosine_topk(ops.l2norm_rows(qf), half, self.dim, k, eq_f32=qf, ec_f32=f32, rho_c=self._rho)
            i = torch.where(i >= 0, rows[i.clamp(min=0)], torch.full_like(i, -1))
        lab = torch.where(i >= 0, self._labels[i.clamp(min=0)], torch.full_like(i, -1))
        return lab, s

    def range_search(self, data, threshold) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Every live row whose score against a query is >= ``threshold`` (cosine, or q.c for 'ip'): ``(lims int64 [Q+1], scores
        float32 [T], labels int64 [T])`` on the device, faiss' ``range_search`` layout — the hits of query q are
        ``[lims[q], lims[q+1])``, ordered by (score desc, row asc).  Exact and complete (:func:`ops.cosine_range`).
        ``threshold``: a float, or an array / tensor [Q] with one threshold per query (a wrong length is a ValueError)."""
        if self.space == "euclidean":
            raise NotImplementedError("range_search (score >= threshold) is not defined in the 'euclidean' space: "
                                      "radius_search returns every row within a squared distance")
        self._compact()
        q = torch.as_tensor(np.asarray(data) if not isinstance(data, torch.Tensor) else data)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        qf = q.to(self.device, dtype=torch.float32).contiguous()
        if self._n == 0:
            ops._threshold_array("range_search", threshold, qf.shape[0], self.device)      # (the length check of the ops)
            return (torch.zeros((qf.shape[0] + 1,), dtype=torch.int64, device=self.device),
                    torch.empty((0,), dtype=torch.float32, device=self.device),
                    torch.empty((0,), dtype=torch.int64, device=self.device))
        qn = ops.l2norm_rows(qf)
        if self.space == "ip":
            lims, s, i = ops.dot_range(qn, self._rows[:self._n], self.dim, threshold, eq_f32=qf, ec_f32=self._f32[:self._n],
                                       rho_c=self._rho, scale_c=self._maxnorm)
        else:
            lims, s, i = ops.cosine_range(qn, self._rows[:self._n], self.dim, threshold, eq_f32=qf, ec_f32=self._f32[:self._n],
                                          rho_c=self._rho)
        return lims, s, self._labels[i]

    def range_query(self, data, threshold) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """numpy form of :meth:`range_search` with ``knn_query``'s distance convention: ``(lims [Q+1], labels [T], distances [T]
        = 1 - score)``, best first within each query."""
        lims, scores, labels = self.range_search(data, threshold)
        return lims.cpu().numpy(), labels.cpu().numpy(), (1.0 - scores).cpu().numpy()

    def radius_search(self, data, radius) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """'euclidean' only: every live row whose SQUARED distance to a query is <= ``radius`` (faiss' L2 ``range_search``, which
        compares with ``<``): ``(lims int64 [Q+1], dist2 float32 [T], labels int64 [T])`` on the device, the hits of query q in
        ``[lims[q], lims[q+1])`` ordered by (distance asc, row asc).  Exact and complete (:func:`ops.l2_range`).  ``radius``: a
        float, or an array / tensor [Q] with one radius per query (a wrong length is a ValueError)."""
        if self.space != "euclidean":
            raise ValueError(f"radius_search is defined in the 'euclidean' space, not {self.space!r} (range_search takes a score)")
        self._compact()
        q = torch.as_tensor(np.asarray(data) if not isinstance(data, torch.Tensor) else data)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        qf = q.to(self.device, dtype=torch.float32).contiguous()
        if self._n == 0:
            ops._threshold_array("radius_search", radius, qf.shape[0], self.device)      # (the length check of the ops)
            return (torch.zeros((qf.shape[0] + 1,), dtype=torch.int64, device=self.device),
                    torch.empty((0,), dtype=torch.float32, device=self.device),
                    torch.empty((0,), dtype=torch.int64, device=self.device))
        lims, s, i = ops.l2_range(ops.l2_query_rows(qf, self._maxnorm), self._rows[:self._n], self.dim, radius, eq_f32=qf,
                                  ec_f32=self._f32[:self._n], rho_c=self._rho, scale_c=self._maxnorm)
        return lims, s, self._labels[i]

    def radius_query(self, data, radius) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """numpy form of :meth:`radius_search` with ``knn_query``'s convention for this space: ``(lims [Q+1], labels [T],
        distances [T])``, the squared distances themselves, nearest first within each query."""
        lims, dist2, labels = self.radius_search(data, radius)
        return lims.cpu().numpy(), labels.cpu().numpy(), dist2.cpu().numpy()

    # ------------------------------------------------------------------ persistence
    def save_index(self, path: str):
        self._compact()
        if os.path.isdir(path):
            path = os.path.join(path, "index.bin")
        labels = self._labels[:self._n].cpu().numpy() if self._n else np.zeros((0,), np.int64)
        rows = self._f32[:self._n].cpu().numpy() if self._n else np.zeros((0, self.dim), np.float32)
        with open(path, "wb") as f:
            np.savez(f, rows_f32=rows, labels=labels, dim=np.int64(self.dim), space=np.array(self.space))

    def load_index(self, path: str, max_elements: int = 0):
        if os.path.isdir(path):
            path = os.path.join(path, "index.bin")
        z = np.load(path, allow_pickle=False)
        space = str(z["space"]) if "space" in z.files else "cosine"
        if space != self.space:
            raise ValueError(f"{path} holds a {space!r} index; this index is {self.space!r}")
        self.dim = int(z["dim"])
        labels = z["labels"]
        self._rows = self._f32 = self._labels = self._dead = None
        self._rho = ops.new_rho(self.device)
        self._maxnorm = None
        self._n = self._n_dead = 0
        if "rows_f32" in z.files:
            rows = z["rows_f32"]
        else:   # first-version file: bf16 bit patterns of unit rows
            rows = (z["rows_bf16"].astype(np.uint32) << np.uint32(16)).view(np.float32)
        n = rows.shape[0]
        self._reserve(max(n, int(max_elements)))
        if n:
            xf = torch.from_numpy(np.ascontiguousarray(rows)).to(self.device)
            self._f32[:n] = xf
            self._rows[:n] = self._ip_rows(xf) if self.space in ("ip", "euclidean") else ops.l2norm_rows(xf, rho=self._rho)
        if n:
            self._labels[:n] = torch.from_numpy(labels).to(self.device)
            self._n = n

    # ------------------------------------------------------------------ internals
    def _check_dim(self):
        if self.space == "euclidean" and self.dim > ops.L2_MAX_DIM:
            raise ValueError(f"the 'euclidean' space takes rows of width <= {ops.L2_MAX_DIM}, not {self.dim}")

    def _ip_rows(self, xf: torch.Tensor) -> torch.Tensor:
        """Half rows of a new batch for the 'ip' and 'euclidean' spaces.  The batch's max norm (read back: one synchronisation per
        batch) joins the index's word; when that raises S, every stored row is re-derived under the new S with a fresh residual
        word."""
        rows_fn = ops.l2_rows if self.space == "euclidean" else ops.dot_scaled_rows
        batch = float(ops.max_norm_rows(xf).item())
        if not math.isfinite(batch):
            raise ValueError("add_items: rows with non-finite elements (or norms beyond the float32 range) cannot be indexed "
                             f"in the {self.space!r} space")
        old = 0.0 if self._maxnorm is None else float(self._maxnorm.item())
        if self._maxnorm is None:
            self._maxnorm = ops.new_rho(self.device)
        if batch > old:
            self._maxnorm.fill_(batch)
            if self._n and ops.dot_scale(batch) != ops.dot_scale(old):
                self._rho.zero_()
                self._rows[:self._n] = rows_fn(self._f32[:self._n], self._maxnorm, self._rho)[0]
        return rows_fn(xf, self._maxnorm, self._rho)[0]

    def _reserve(self, n: int):
        if self.dim == 0:
            return
        cap = 0 if self._rows is None else self._rows.shape[0]
        if n <= cap:
            return
        new_cap = max(n, 2 * cap, 1024)
        ld = ops.pad_dim(self.dim + 1 if self.space == "euclidean" else self.dim)
        rows = torch.zeros((new_cap, ld), dtype=ops.UNIT_DTYPE, device=self.device)
        f32 = torch.zeros((new_cap, self.dim), dtype=torch.float32, device=self.device)
        if self._f32 is not None and self._n:
            f32[:self._n] = self._f32[:self._n]
        self._f32 = f32
        labels = torch.full((new_cap,), -1, dtype=torch.int64, device=self.device)
        dead = torch.zeros((new_cap,), dtype=torch.bool, device=self.device)
        if self._rows is not None and self._n:
            rows[:self._n] = self._rows[:self._n]
            labels[:self._n] = self._labels[:self._n]
            dead[:self._n] = self._dead[:self._n]
        self._rows, self._labels, self._dead = rows, labels, dead

    def _compact(self):
        if self._n_dead == 0:
            return
        keep = (~self._dead[:self._n]).nonzero(as_tuple=False).squeeze(1)
        m = keep.numel()
        self._rows[:m] = self._rows[keep]
        self._f32[:m] = self._f32[keep]
        self._labels[:m] = self._labels[keep]
        self._dead[:self._n] = False
        self._n, self._n_dead = m, 0
