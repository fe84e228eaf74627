"""GpuIVFPQIndex — inverted lists of product-quantisation codes resident in HBM (faiss' ``IndexIVFPQ`` with 8-bit codes, the
IVFADC of the PQ paper): the rows are clustered into ``nlist`` lists as in :class:`GpuIVFIndex`, each row is stored as the ``M``
bytes of the PQ code of its RESIDUAL to its list's centroid (``by_residual=True``, the default; else of the row itself), and a
query is scored by table lookups against the ``nprobe`` lists nearest to it only.  Without ``refine=`` it keeps no float rows:
that is its point.

``space``: ``"ip"``, ``"l2"`` (squared Euclidean distance, smaller is better) or ``"cosine"`` — ip with rows normalised before
they are assigned and encoded and queries before their tables (:meth:`GpuPQIndex.normalise`) — in :class:`GpuPQIndex`'s sense;
``dim`` in 1..1024, ``M`` in 1..64, ``dim % M == 0``, ``dim / M <= 64``.

It composes what the tree has.  The coarse quantiser is a row-less :class:`GpuIVFIndex` of the matching space (``train``,
``_coarse``: the exact search of rows or queries against the centroids, ties to the lower list); rows wider than the float
searches take (768, Euclidean 767) are assigned by :func:`_wide_coarse`, a float32 product with the centroids and ``torch.topk``
— the one step here that is not a kernel of ours, off the scan's path and stated, not a fallback.  The codebooks come from
:meth:`GpuPQIndex.train` on the residuals of the training sample to their assigned centroids (or on the rows).  ``train`` must
come before ``add_items`` (``RuntimeError`` otherwise, faiss' rule): without centroids and codebooks a row cannot be stored.

Layout: uint8 code rows, list numbers, int64 labels and a tombstone mask in arrival order, and the packed form the scan reads
(:func:`ivf_index.pack_lists`), rebuilt lazily.  ``mark_deleted`` sets a tombstone; the codes are compacted before the next
search.  ``search`` is exact for the integer scores of :func:`ops.ivfpq_search` over the probed lists under (score desc, arrival
row asc) — l2: (distance asc, row asc) — and returns ``(values, labels)`` as ``GpuPQIndex.search`` does.  On disk: one ``.npz``
without pickling with ``kind = 'ivfpq'`` and the codes under ``ivfpq_codes`` (so that ``GpuPQIndex.load_index`` refuses it); a file
of another kind, space, width or M raises ``ValueError``.

Refine stage (faiss' ``IndexRefineFlat`` over ``IndexIVFPQ``): ``refine="float32"`` or ``"float16"`` keeps the rows as given
(before the cosine normalisation) in arrival order beside the codes, compacted with them, exactly as :class:`GpuPQIndex`
describes; ``search(q, k, rescore_multiplier=mult)`` re-scores the ``min(k * mult, ops.MAX_K, live rows)`` best rows of the scan
exactly against them with the query as given.  The file gains ``refine`` and ``refine_rows``; loading adopts them.

Not here (``NotImplementedError``; ``GpuFlatIndex`` has them): ``filter=``, range and radius search.  No OPQ rotation and no
precomputed tables.
"""
from __future__ import annotations

import os
from typing import Iterable, Optional, Tuple

import numpy as np
import torch

from . import _refine, ops
from .ivf_index import GpuIVFIndex, pack_lists
from .pq_index import GpuPQIndex

_COARSE_SPACE = {"ip": "ip", "l2": "euclidean", "cosine": "cosine"}
_ENCODE_CHUNK = 1 << 18      # rows whose residuals are formed at a time in front of the encoder


def _wide_coarse(space: str, x: torch.Tensor, c: torch.Tensor, k: int) -> torch.Tensor:
    """List numbers [rows, k] of the k best centroids, best first, for rows wider than the exact searches take: float32 scores
    in torch (l2: 2 x.c - |c|^2, which ranks as minus the squared distance) and ``torch.topk``, in row chunks that keep the score
    matrix within 64 MiB.  Equal scores, and a row without a usable score (NaN), fall to whichever list ``topk`` names."""
    out = []
    step = max(1, (1 << 24) // c.shape[0])
    cn = c.norm(dim=1).clamp(min=1e-12) if space == "cosine" else None
    c2 = (c * c).sum(1) if space == "l2" else None
    for r0 in range(0, x.shape[0], step):
        s = x[r0:r0 + step] @ c.T
        if space == "l2":
            s = 2 * s - c2[None, :]
        elif space == "cosine":
            s = s / cn[None, :]
        s = torch.nan_to_num(s, nan=float("-inf"), posinf=float("inf"), neginf=float("-inf"))
        out.append(torch.topk(s, k, dim=1, largest=True, sorted=True)[1])
    return torch.cat(out) if out else torch.zeros((0, k), dtype=torch.int64, device=x.device)


class GpuIVFPQIndex:
    SPACES = ("ip", "l2", "cosine")
    KIND = "ivfpq"
    _FILE_NAME = "ivfpq_index.bin"

    def __init__(self, space: str = "ip", dim: int = 0, nlist: int = 1, nprobe: int = 1, M: int = 8, by_residual: bool = True,
                 device: Optional[torch.device] = None, seed: int = 0, refine: Optional[str] = None):
        if space not in self.SPACES:
            raise ValueError(f"GpuIVFPQIndex implements the spaces {self.SPACES}, not {space!r}")
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self.refine = _refine.check_refine("GpuIVFPQIndex", refine, space, int(dim))
        self._store = None if self.refine is None else _refine.RowStore(self.refine, space, int(dim), self.device)
        self._pq = GpuPQIndex(space=space, dim=dim, M=M, device=self.device, seed=seed)      # (checks dim and M)
        self.space, self.dim, self.M, self.seed = space, int(dim), int(M), int(seed)
        self.by_residual = bool(by_residual)
        self.nlist = int(nlist)
        if self.nlist < 1:
            raise ValueError(f"nlist={nlist} < 1")
        self._adc_space = "l2" if space == "l2" else "ip"
        self._wide = self.dim > (ops.L2_MAX_DIM if space == "l2" else 768)
        # the coarse quantiser: a GpuIVFIndex that never holds a row (wide rows: it only trains the centroids, at a width it takes)
        self._ivf = None if self._wide else GpuIVFIndex(space=_COARSE_SPACE[space], dim=self.dim, nlist=self.nlist, nprobe=1,
                                                        device=self.device, seed=seed)
        self.nprobe = 1
        self.set_nprobe(nprobe)
        self.centroids: Optional[torch.Tensor] = None    # [nlist, dim] float32
        self._cb = ops.pq_code_bytes(self.M)
        self._codes: Optional[torch.Tensor] = None       # [capacity, _cb] uint8 in arrival order
        self._list: Optional[torch.Tensor] = None        # [capacity] int64
        self._labels: Optional[torch.Tensor] = None      # [capacity] int64
        self._dead: Optional[torch.Tensor] = None        # [capacity] bool
        self._n = 0
        self._n_dead = 0
        self._packed = None                              # (codes in list order, list_off, row_ids, longest list) or None: rebuild

    # ------------------------------------------------------------------ surface
    @property
    def codebooks(self) -> Optional[torch.Tensor]:
        return self._pq.codebooks

    @property
    def is_trained(self) -> bool:
        return self.centroids is not None and self._pq.codebooks is not None

    def set_nprobe(self, n: int):
        n = int(n)
        if not 1 <= n <= min(self.nlist, ops.MAX_K):
            raise ValueError(f"nprobe={n} outside 1..{min(self.nlist, ops.MAX_K)} (nlist = {self.nlist})")
        self.nprobe = n

    def init_index(self, max_elements: int, ef_construction: int = 0, M: int = 0):
        self._reserve(int(max_elements))

    def resize_index(self, new_size: int):
        self._reserve(int(new_size))

    def set_ef(self, ef: int):      # accepted and ignored: nprobe is this index's knob
        pass

    def get_current_count(self) -> int:
        return self._n

    def num_live(self) -> int:
        return self._n - self._n_dead

    # ------------------------------------------------------------------ training
    def _rows(self, data) -> torch.Tensor:
        return self._pq._rows(data)     # float32 on the device, normalised under 'cosine'

    def _coarse(self, x: torch.Tensor, k: int) -> torch.Tensor:
        if self._wide:
            return _wide_coarse(self.space, x, self.centroids, k)
        return self._ivf._coarse(x.contiguous(), k)

    def _residuals(self, x: torch.Tensor, lists: torch.Tensor) -> torch.Tensor:
        return x - self.centroids[lists] if self.by_residual else x

    def train(self, data=None, niter: int = 20, max_points_per_list: int = 256, max_points_per_centroid: int = 256, centroids=None,
              codebooks=None):
        """Set the ``nlist`` centres and the codebooks.  ``centroids`` [nlist, dim] and ``codebooks`` [M, 256, dim / M] are
        installed as given; what is not given is learned from ``data``: the centres by ``GpuIVFIndex.train`` (seeded sample,
        ``niter`` Lloyd iterations at most), then the codebooks by ``GpuPQIndex.train`` on the residuals of (a seeded sample
        of) ``data`` to their assigned centres — or on the rows when ``by_residual`` is off.  Rows already stored keep their
        codes: train before adding."""
        x = None
        if centroids is None or codebooks is None:
            if data is None:
                raise ValueError("train needs data= unless centroids= and codebooks= are both given")
            x = self._rows(data)
            if x.shape[0] == 0 or not bool(torch.isfinite(x).all()):
                raise ValueError("train needs at least one row, all finite")
        if centroids is not None:
            c = torch.as_tensor(np.asarray(centroids) if not isinstance(centroids, torch.Tensor) else centroids)
            c = c.to(self.device, dtype=torch.float32).contiguous()
            if tuple(c.shape) != (self.nlist, self.dim):
                raise ValueError(f"centroids must have shape ({self.nlist}, {self.dim}), got {tuple(c.shape)}")
            if not bool(torch.isfinite(c).all()):
                raise ValueError("centroids must be finite")
            if not self._wide:
                self._ivf.train(centroids=c)
        elif self._wide:
            c = self._train_wide_centroids(x, niter, max_points_per_list)
        else:
            self._ivf.train(x, niter=niter, max_points_per_list=max_points_per_list)
            c = self._ivf.centroids
        self.centroids = c
        if codebooks is not None:
            self._pq.train(codebooks=codebooks)
        else:
            m = 256 * int(max_points_per_centroid)
            if x.shape[0] > m:       # (the sample GpuPQIndex.train would draw, drawn here so that only its residuals are formed)
                g = torch.Generator(device="cpu").manual_seed(self.seed)
                x = x[torch.randperm(x.shape[0], generator=g)[:m].sort()[0].to(self.device)]
            r = self._residuals(x, self._coarse(x, 1)[:, 0])
            pq = GpuPQIndex(space=self._adc_space, dim=self.dim, M=self.M, device=self.device, seed=self.seed)   # (rows as they are)
            pq.train(r, niter=niter, max_points_per_centroid=max_points_per_centroid)
            self._pq.train(codebooks=pq.codebooks)
        self._packed = None

    def _train_wide_centroids(self, x, niter, max_points_per_list):
        from .pipeline.clustering import ClusteringPipeline
        m = int(max_points_per_list) * self.nlist
        if x.shape[0] < self.nlist:
            raise ValueError(f"train: {x.shape[0]} rows cannot seed {self.nlist} lists")
        if x.shape[0] > m:
            g = torch.Generator(device="cpu").manual_seed(self.seed)
            x = x[torch.randperm(x.shape[0], generator=g)[:m].sort()[0].to(self.device)]
        km = ClusteringPipeline(self.nlist, params=None, model=None, max_iter=int(niter), seed=self.seed)
        was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
        torch.use_deterministic_algorithms(True, warn_only=True)
        try:
            return km.fit(x.contiguous()).cluster_centers_.contiguous()
        finally:
            torch.use_deterministic_algorithms(was, warn_only=warn)

    # ------------------------------------------------------------------ rows in
    def _need_trained(self):
        if not self.is_trained:
            raise RuntimeError("the index is not trained: call train(data) or train(centroids=..., codebooks=...) first")

    def add_items(self, data, ids: Optional[Iterable[int]] = None, num_threads: int = -1):
        self._need_trained()
        kept = None
        if self._store is not None:      # the rows as given; one that is not finite in the store's dtype raises before anything is added
            raw = _refine.raw_queries(data, self.dim, self.device)
            kept = self._store.convert(raw)
            x = self._pq._prepared(raw)
        else:
            x = self._rows(data)
        n = x.shape[0]
        if ids is None:
            ids = np.arange(self._n, self._n + n)
        lab = torch.as_tensor(np.asarray(list(ids), dtype=np.int64))
        if lab.numel() != n:
            raise ValueError("ids and data disagree in length")
        self._reserve(self._n + n)
        if kept is not None:
            self._store.put(self._n, kept)
        for r0 in range(0, n, _ENCODE_CHUNK):
            xs = x[r0:r0 + _ENCODE_CHUNK]
            lists = self._coarse(xs, 1)[:, 0]
            at = self._n + r0
            ops.pq_encode_rows(self._residuals(xs, lists), self._pq.codebooks, out=self._codes[at:at + xs.shape[0]], _trusted=True)
            self._list[at:at + xs.shape[0]] = lists
        self._labels[self._n:self._n + n] = lab.to(self.device)
        self._dead[self._n:self._n + n] = False
        self._n += n
        self._packed = None

    def mark_deleted(self, label: int):
        if self._n == 0:
            raise RuntimeError("label not found")
        hit = (self._labels[:self._n] == int(label)) & ~self._dead[:self._n]
        k = int(hit.sum())
        if k == 0:
            raise RuntimeError("label not found")      # as GpuFlatIndex and hnswlib
        self._dead[:self._n] |= hit
        self._n_dead += k

    # ------------------------------------------------------------------ results out
    def search(self, data, k: int, filter=None, rescore_multiplier: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(values [Q,k] float32, labels [Q,k] int64), best first, over the ``nprobe`` lists nearest to each query: ip and cosine by
        (score desc, arrival row asc), padded with (-inf, -1); l2 by (squared distance asc, row asc), padded with (+inf, -1).
        ``rescore_multiplier`` (an integer >= 1; needs ``refine=``): the ``min(k * rescore_multiplier, ops.MAX_K, live rows)`` best
        rows of the scan are re-scored exactly against the stored rows with the query as given; the values are then the exact
        float32 scores of the space (module docstring)."""
        if filter is not None:
            raise NotImplementedError("GpuIVFPQIndex has no filtered search: GpuFlatIndex.search(filter=...) does")
        self._need_trained()
        self._compact()
        k = int(k)
        q_raw = None
        if rescore_multiplier is not None:
            mult = _refine.check_multiplier(rescore_multiplier, self._store)
            if not 1 <= k <= ops.MAX_K:
                raise ValueError(f"k={k} outside 1..{ops.MAX_K}")
            q_raw = _refine.raw_queries(data, self.dim, self.device)
            q = self._pq._prepared(q_raw).contiguous()
        else:
            q = self._rows(data).contiguous()
        if self._n == 0 or q.shape[0] == 0:
            return (torch.full((q.shape[0], k), float("inf" if self.space == "l2" else "-inf"), device=self.device),
                    torch.full((q.shape[0], k), -1, dtype=torch.int64, device=self.device))
        codes, list_off, row_ids, longest = self._pack()
        probes = self._coarse(q, self.nprobe).contiguous()
        m = k if q_raw is None else min(k * mult, ops.MAX_K, self._n)
        val, idx = ops.ivfpq_search(q, self.centroids, self._pq.codebooks, codes, list_off, row_ids, probes, m, self._adc_space,
                                    by_residual=self.by_residual, max_list_len=longest, _trusted=True)
        if q_raw is not None:
            val, idx = self._store.rescore(q_raw, self._n, idx, k)
        return val, torch.where(idx >= 0, self._labels[idx.clamp(min=0)], torch.full_like(idx, -1))

    def knn_query(self, data, k: int = 1, filter=None, rescore_multiplier: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(labels [Q,k] int64, values [Q,k] float32) as numpy arrays, best first: ``GpuPQIndex.knn_query``'s conventions."""
        val, lab = self.search(data, k, filter=filter, rescore_multiplier=rescore_multiplier)
        return lab.cpu().numpy(), val.cpu().numpy()

    def reconstruct(self, labels) -> torch.Tensor:
        """float32 [n, dim]: the list centroid plus the decoded residual of the live rows with these labels (cosine: of the
        normalised row)"""
        self._need_trained()
        self._compact()
        lab = torch.as_tensor(np.ascontiguousarray(np.asarray(labels, dtype=np.int64).reshape(-1))).to(self.device)
        held = self._labels[:self._n] if self._n else torch.zeros((0,), dtype=torch.int64, device=self.device)
        order = torch.argsort(held, stable=True)
        pos = torch.searchsorted(held[order], lab).clamp(max=max(self._n - 1, 0))
        if self._n == 0 or not bool((held[order][pos] == lab).all()):
            raise RuntimeError("label not found")
        rows = order[pos]
        dec = ops.pq_decode_rows(self._codes[rows], self._pq.codebooks)
        return self.centroids[self._list[rows]] + dec if self.by_residual else dec

    def _unsupported(self, what):
        raise NotImplementedError(f"GpuIVFPQIndex has no {what}: GpuFlatIndex does")

    def range_search(self, data, threshold):
        self._unsupported("range_search")

    def range_query(self, data, threshold):
        self._unsupported("range_query")

    def radius_search(self, data, radius):
        self._unsupported("radius_search")

    def radius_query(self, data, radius):
        self._unsupported("radius_query")

    # ------------------------------------------------------------------ files
    def _file(self, path: str) -> str:
        return os.path.join(path, self._FILE_NAME) if os.path.isdir(path) else path

    def save_index(self, path: str):
        self._need_trained()
        self._compact()
        n = self._n
        codes = self._codes[:n, :self.M].cpu().numpy() if n else np.zeros((0, self.M), np.uint8)
        labels = self._labels[:n].cpu().numpy() if n else np.zeros((0,), np.int64)
        lists = self._list[:n].cpu().numpy() if n else np.zeros((0,), np.int64)
        with open(self._file(path), "wb") as f:
            np.savez(f, ivfpq_codes=np.ascontiguousarray(codes), labels=labels, lists=lists, centroids=self.centroids.cpu().numpy(),
                     codebooks=self._pq.codebooks.cpu().numpy(), space=np.array(self.space), dim=np.int64(self.dim), M=np.int64(self.M),
                     nlist=np.int64(self.nlist), nprobe=np.int64(self.nprobe), by_residual=np.int64(self.by_residual),
                     kind=np.array(self.KIND), **_refine.save_fields(self._store, n))

    def load_index(self, path: str, max_elements: int = 0):
        z = np.load(self._file(path), allow_pickle=False)
        kind = str(z["kind"]) if "kind" in z.files else ("pq" if "pq_codes" in z.files else "flat")
        if kind != self.KIND:
            raise ValueError(f"{path} holds a {kind!r} index, not an {self.KIND!r} one")
        have = (str(z["space"]), int(z["dim"]), int(z["M"]))
        if have != (self.space, self.dim, self.M):
            raise ValueError(f"{path} holds an IVF-PQ index of (space, dim, M) = {have}; this one has "
                             f"{(self.space, self.dim, self.M)}")
        codes, labels, lists = z["ivfpq_codes"], z["labels"].astype(np.int64), z["lists"].astype(np.int64)
        nlist, n = int(z["nlist"]), codes.shape[0]
        cent = z["centroids"]
        if (codes.dtype != np.uint8 or codes.ndim != 2 or codes.shape[1] != self.M or labels.shape != (n,) or lists.shape != (n,)
                or cent.shape != (nlist, self.dim) or (n and (lists.min() < 0 or lists.max() >= nlist))):
            raise ValueError(f"{path}: malformed IVF-PQ index")
        store, kept = _refine.load_store(z, path, n, self.space, self.dim, self.device)
        if nlist != self.nlist:
            self.nlist = nlist
            if not self._wide:
                self._ivf = GpuIVFIndex(space=_COARSE_SPACE[self.space], dim=self.dim, nlist=nlist, nprobe=1, device=self.device,
                                        seed=self.seed)
        self.by_residual = bool(int(z["by_residual"]))
        self.set_nprobe(int(z["nprobe"]))
        self.train(centroids=cent, codebooks=z["codebooks"])
        self._codes = self._list = self._labels = self._dead = None
        self._n = self._n_dead = 0
        self._store, self.refine = store, None if store is None else store.kind      # (the file decides, as for nlist)
        self._reserve(max(n, int(max_elements)))
        if n and store is not None:
            store.put(0, torch.from_numpy(kept).to(self.device))
        if n:
            self._codes[:n] = ops.pq_codes_from_numpy(codes, self.M, device=self.device)
            self._labels[:n] = torch.from_numpy(labels).to(self.device)
            self._list[:n] = torch.from_numpy(lists).to(self.device)
            self._n = n
        self._packed = None

    # ------------------------------------------------------------------ internals
    def _reserve(self, n: int):
        cap = 0 if self._codes is None else self._codes.shape[0]
        if n <= cap:
            return
        new_cap = max(n, 2 * cap, 1024)
        codes = torch.zeros((new_cap, self._cb), dtype=torch.uint8, device=self.device)
        lists = torch.zeros((new_cap,), dtype=torch.int64, device=self.device)
        labels = torch.full((new_cap,), -1, dtype=torch.int64, device=self.device)
        dead = torch.zeros((new_cap,), dtype=torch.bool, device=self.device)
        if self._codes is not None and self._n:
            codes[:self._n] = self._codes[:self._n]
            lists[:self._n] = self._list[:self._n]
            labels[:self._n] = self._labels[:self._n]
            dead[:self._n] = self._dead[:self._n]
        self._codes, self._list, self._labels, self._dead = codes, lists, labels, dead
        if self._store is not None:
            self._store.reserve(new_cap, self._n)

    def _compact(self):
        if self._n_dead == 0:
            return
        keep = (~self._dead[:self._n]).nonzero(as_tuple=False).squeeze(1)
        m = keep.numel()
        self._codes[:m] = self._codes[keep]
        self._list[:m] = self._list[keep]
        self._labels[:m] = self._labels[keep]
        if self._store is not None:
            self._store.compact(keep)
        self._dead[:self._n] = False
        self._n, self._n_dead = m, 0
        self._packed = None

    def _pack(self):
        """The packed form, rebuilt when rows came or went; the longest list's length is read back here, once per rebuild."""
        if self._packed is None:
            order, list_off, row_ids = pack_lists(self._list[:self._n], self.nlist)
            longest = int((list_off[1:] - list_off[:-1]).max())
            self._packed = (self._codes[:self._n].index_select(0, order), list_off, row_ids, longest)
        return self._packed
