"""GpuIVFIndex — an inverted-file index resident in HBM (faiss' ``IndexIVFFlat``) with the hnswlib-shaped surface of
:class:`text_similarity_amd.index.GpuFlatIndex`: the rows are clustered into ``nlist`` lists and a query is scored against the
``nprobe`` lists nearest to it only, so one online query no longer reads the whole corpus.  Within the probed lists the search
is exact: the scores, the order (score desc, arrival row asc) and the label mapping are those of ``GpuFlatIndex``, and at
``nprobe == nlist`` the two indexes return the same bits, ties and deletions included.

Training: Lloyd's iterations of :class:`pipeline.clustering.ClusteringPipeline` as it stands, on a seeded sample of at most
``max_points_per_list * nlist`` rows (faiss' rule; 256 is faiss' default, a convention), on the unit rows for ``'cosine'``.  A
cluster that ends empty keeps its centre and its list is empty.  An index with rows that was never trained trains itself at
the first search, on its stored rows with its seed — hnswlib's call sequence (``init_index``, ``add_items``, ``knn_query``)
works without a ``train`` call.  Fewer rows than ``nlist`` cannot seed the lists: ``ValueError``.

Assignment (k = 1) and probing (k = nprobe) are the index's own exact search of rows or queries against the centroids
(:func:`ops.cosine_topk` with float32 rows, :func:`ops.dot_topk`, :func:`ops.l2_topk`): deterministic, ties to the lower list.

Layout: float32 rows ``[capacity, d]`` in arrival order + their list number + int64 labels + a tombstone mask; and the packed
form the scan kernel reads (:func:`pack_lists`): the rows gathered into list order by ONE stable sort of the list numbers —
arrival order survives within a list — with ``list_off`` int64 [nlist+1] and ``row_ids`` int32 [n], the arrival row of each
position.  Deleting marks a tombstone; rows are compacted and the packed form rebuilt before the next search.  On disk
(``index.bin``, a numpy ``.npz`` without pickling): rows, labels, list numbers, centroids, space, nlist, nprobe and
``kind = 'ivf'``; a file of another space or kind raises ``ValueError``.

Not here (``NotImplementedError``; ``GpuFlatIndex`` has them): ``filter=``, range and radius search.
"""
from __future__ import annotations

import os
from typing import Iterable, Optional, Tuple

import numpy as np
import torch

from . import ops

_OPS_SPACE = {"cosine": "cosine", "ip": "dot", "euclidean": "l2"}


def kmeans_centroids(x: torch.Tensor, nlist: int, space: str, seed: int, niter: int = 20,
                     max_points_per_list: int = 256) -> torch.Tensor:
    """Centres [nlist, d] float32 of the device rows ``x`` [n >= nlist, d]: Lloyd's iterations of
    :class:`pipeline.clustering.ClusteringPipeline` on a sample of at most ``max_points_per_list * nlist`` rows drawn with
    ``seed``, on the unit rows for ``'cosine'``.  The coarse quantiser of :class:`GpuIVFIndex` and of
    :class:`graph_index.GpuGraphIndex` (``entry='coarse'``): the same rows, ``nlist`` and seed give the same bits in both."""
    m = int(max_points_per_list) * int(nlist)
    if x.shape[0] > m:
        g = torch.Generator(device="cpu").manual_seed(int(seed))
        x = x[torch.randperm(x.shape[0], generator=g)[:m].sort()[0].to(x.device)]
    if space == "cosine":
        x = x / x.norm(dim=1, keepdim=True).clamp(min=1e-12)
    from .pipeline.clustering import ClusteringPipeline
    km = ClusteringPipeline(int(nlist), params=None, model=None, max_iter=int(niter), seed=int(seed))
    # fit's update step is a scatter-add, which adds in whatever order its atomics land unless torch is asked for its
    # deterministic form: with it, the same rows and seed give the same centres bit for bit — and so the same lists
    was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        return km.fit(x.contiguous()).cluster_centers_.contiguous()
    finally:
        torch.use_deterministic_algorithms(was, warn_only=warn)


def pack_lists(list_numbers: torch.Tensor, nlist: int):
    """The packed layout of ``n`` rows with list numbers in [0, nlist): ``(order int64 [n], list_off int64 [nlist+1], row_ids int32
    [n])``.  ``order`` is the stable sort of the list numbers — position p of the packed form holds row ``order[p]``, the rows of
    a list keep their arrival order — ``list_off`` the exclusive cumulative count per list and ``row_ids = order`` as int32.  A
    pure function of its arguments; runs on CPU and device tensors alike."""
    ln = list_numbers.to(torch.int64)
    order = torch.sort(ln, stable=True)[1]
    list_off = torch.zeros((int(nlist) + 1,), dtype=torch.int64, device=ln.device)
    list_off[1:] = torch.cumsum(torch.bincount(ln, minlength=int(nlist)), 0)
    return order, list_off, order.to(torch.int32)


class GpuIVFIndex:
    SPACES = ("cosine", "ip", "euclidean")
    KIND = "ivf"

    def __init__(self, space: str = "cosine", dim: int = 0, nlist: int = 1, nprobe: int = 1,
                 device: Optional[torch.device] = None, seed: int = 0):
        if space not in self.SPACES:
            raise ValueError(f"GpuIVFIndex implements the spaces {self.SPACES}, not {space!r}")
        self.space = space
        self.dim = int(dim)
        self._check_dim()
        self.nlist = int(nlist)
        if self.nlist < 1:
            raise ValueError(f"nlist={nlist} < 1")
        self.nprobe = 1
        self.set_nprobe(nprobe)
        self.seed = int(seed)
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self._f32: Optional[torch.Tensor] = None       # [capacity, d] float32 rows in arrival order
        self._list: Optional[torch.Tensor] = None      # [capacity] int64 list number (undefined until trained)
        self._labels: Optional[torch.Tensor] = None    # [capacity] int64
        self._dead: Optional[torch.Tensor] = None      # [capacity] bool
        self._n = 0
        self._n_dead = 0
        self.centroids: Optional[torch.Tensor] = None  # [nlist, d] float32
        self._coarse_ops = None                        # the centroids as the operands of the space's exact search
        self._packed = None                            # (rows [n, d], list_off, row_ids, longest list) or None: rebuild

    # ------------------------------------------------------------------ hnswlib-shaped surface
    def init_index(self, max_elements: int, ef_construction: int = 0, M: int = 0):
        self._reserve(int(max_elements))

    def set_ef(self, ef: int):      # accepted and ignored, as in GpuFlatIndex: nprobe is this index's knob
        pass

    def set_nprobe(self, n: int):
        n = int(n)
        if not 1 <= n <= min(self.nlist, ops.MAX_K):
            raise ValueError(f"nprobe={n} outside 1..{min(self.nlist, ops.MAX_K)} (nlist = {self.nlist})")
        self.nprobe = n

    def resize_index(self, new_size: int):
        self._reserve(int(new_size))

    def get_current_count(self) -> int:
        return self._n

    def num_live(self) -> int:
        return self._n - self._n_dead

    @property
    def is_trained(self) -> bool:
        return self.centroids is not None

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
        self._reserve(self._n + n)
        self._f32[self._n:self._n + n] = xf
        self._labels[self._n:self._n + n] = lab.to(self.device)
        self._dead[self._n:self._n + n] = False
        if self.is_trained and n:
            self._list[self._n:self._n + n] = self._coarse(xf, 1)[:, 0]
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

    def knn_query(self, data, k: int = 1, filter=None) -> Tuple[np.ndarray, np.ndarray]:
        """(labels [Q,k] int64, distances [Q,k] float32) best first, in ``GpuFlatIndex.knn_query``'s conventions."""
        labels, scores = self.search(data, k, filter=filter)
        if self.space == "euclidean":
            return labels.cpu().numpy(), scores.cpu().numpy()
        return labels.cpu().numpy(), (1.0 - scores).cpu().numpy()

    # ------------------------------------------------------------------ training
    def train(self, data=None, niter: int = 20, max_points_per_list: int = 256, centroids=None):
        """Set the ``nlist`` centres and (re)assign every stored row.  ``centroids`` [nlist, d]: installed as given, no clustering.
        Else k-means (``niter`` Lloyd iterations at most) on ``data``, or on the stored live rows when None — on a seeded sample of
        at most ``max_points_per_list * nlist`` of them."""
        if centroids is not None:
            c = torch.as_tensor(np.asarray(centroids) if not isinstance(centroids, torch.Tensor) else centroids)
            c = c.to(self.device, dtype=torch.float32).contiguous()
            if self.dim == 0 and c.dim() == 2:
                self.dim = int(c.shape[1])
                self._check_dim()
            if c.shape != (self.nlist, self.dim):
                raise ValueError(f"centroids must have shape ({self.nlist}, {self.dim}), got {tuple(c.shape)}")
        else:
            if data is None:
                self._compact()
                x = self._f32[:self._n] if self._n else None
            else:
                x = torch.as_tensor(np.asarray(data) if not isinstance(data, torch.Tensor) else data)
                x = x.to(self.device, dtype=torch.float32)
            if x is None or x.dim() != 2 or x.shape[0] < self.nlist:
                raise ValueError(f"train: {0 if x is None else x.shape[0]} rows cannot seed {self.nlist} lists")
            if self.dim == 0:
                self.dim = int(x.shape[1])
                self._check_dim()
            if x.shape[1] != self.dim:
                raise ValueError(f"expected width {self.dim}, got {x.shape[1]}")
            c = kmeans_centroids(x, self.nlist, self.space, self.seed, niter=niter, max_points_per_list=max_points_per_list)
        self.centroids = c
        if self.space == "cosine":
            self._coarse_ops = ops.l2norm_rows(c, return_rho=True)
        elif self.space == "ip":
            self._coarse_ops = ops.dot_scaled_rows(c)
        else:
            self._coarse_ops = ops.l2_rows(c)
        if self._n:
            self._list[:self._n] = self._coarse(self._f32[:self._n], 1)[:, 0]
        self._packed = None

    def _coarse(self, xf: torch.Tensor, k: int) -> torch.Tensor:
        """List numbers [rows, k] int64 of the k centroids nearest to each row of ``xf`` in the index's space: the exact search,
        so ties go to the lower list.  A row without a usable score (a zero row under 'cosine') goes to list 0."""
        c, d = self.centroids, self.dim
        if self.space == "cosine":
            half, rho = self._coarse_ops
            i = ops.cosine_topk(ops.l2norm_rows(xf), half, d, k, eq_f32=xf, ec_f32=c, rho_c=rho)[1]
        elif self.space == "ip":
            half, rho, scale = self._coarse_ops
            i = ops.dot_topk(ops.l2norm_rows(xf), half, d, k, eq_f32=xf, ec_f32=c, rho_c=rho, scale_c=scale)[1]
        else:
            half, rho, scale = self._coarse_ops
            i = ops.l2_topk(ops.l2_query_rows(xf, scale), half, d, k, eq_f32=xf, ec_f32=c, rho_c=rho, scale_c=scale)[1]
        return i.clamp(min=0) if k == 1 else i      # (probing: -1 is padding to the scan)

    # ------------------------------------------------------------------ device-level API
    def search(self, data, k: int, filter=None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(labels [Q,k] int64, scores [Q,k] float32) on the device, as ``GpuFlatIndex.search`` returns them, over the ``nprobe``
        lists nearest to each query; -1 / -inf pad ('euclidean': squared distances ascending, +inf pad) when they hold fewer than
        k live rows."""
        if filter is not None:
            raise NotImplementedError("GpuIVFIndex has no filtered search: GpuFlatIndex.search(filter=...) does")
        self._compact()
        q = torch.as_tensor(np.asarray(data) if not isinstance(data, torch.Tensor) else data)
        if q.dim() == 1:
            q = q.unsqueeze(0)
        qf = q.to(self.device, dtype=torch.float32).contiguous()
        k = int(k)
        if self._n == 0 or qf.shape[0] == 0:
            return (torch.full((qf.shape[0], k), -1, dtype=torch.int64, device=self.device),
                    torch.full((qf.shape[0], k), float("inf" if self.space == "euclidean" else "-inf"), device=self.device))
        if not self.is_trained:
            self.train()
        rows, list_off, row_ids, longest = self._pack()
        probes = self._coarse(qf, self.nprobe).contiguous()
        s, i = ops.ivf_scan_topk(_OPS_SPACE[self.space], qf, rows, list_off, row_ids, probes, k, max_list_len=longest)
        lab = torch.where(i >= 0, self._labels[i.clamp(min=0)], torch.full_like(i, -1))
        return lab, s

    def _unsupported(self, what):
        raise NotImplementedError(f"GpuIVFIndex has no {what}: GpuFlatIndex does")

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
        self._compact()
        if self._n and not self.is_trained:
            self.train()
        if os.path.isdir(path):
            path = os.path.join(path, "index.bin")
        n = self._n
        rows = self._f32[:n].cpu().numpy() if n else np.zeros((0, self.dim), np.float32)
        labels = self._labels[:n].cpu().numpy() if n else np.zeros((0,), np.int64)
        lists = self._list[:n].cpu().numpy() if n and self.is_trained else np.zeros((0,), np.int64)
        cent = self.centroids.cpu().numpy() if self.is_trained else np.zeros((0, self.dim), np.float32)
        with open(path, "wb") as f:
            np.savez(f, rows_f32=rows, labels=labels, lists=lists, centroids=cent, dim=np.int64(self.dim), space=np.array(self.space),
                     nlist=np.int64(self.nlist), nprobe=np.int64(self.nprobe), kind=np.array(self.KIND))

    def load_index(self, path: str, max_elements: int = 0):
        if os.path.isdir(path):
            path = os.path.join(path, "index.bin")
        z = np.load(path, allow_pickle=False)
        kind = str(z["kind"]) if "kind" in z.files else "flat"
        if kind != self.KIND:
            raise ValueError(f"{path} holds a {kind!r} index, not an {self.KIND!r} one")
        space = str(z["space"])
        if space != self.space:
            raise ValueError(f"{path} holds a {space!r} index; this index is {self.space!r}")
        self.dim = int(z["dim"])
        self.nlist = int(z["nlist"])
        self.set_nprobe(int(z["nprobe"]))
        self._f32 = self._list = self._labels = self._dead = None
        self._n = self._n_dead = 0
        self.centroids = self._coarse_ops = self._packed = None
        rows, cent = z["rows_f32"], z["centroids"]
        n = rows.shape[0]
        self._reserve(max(n, int(max_elements)))
        if n:
            self._f32[:n] = torch.from_numpy(np.ascontiguousarray(rows)).to(self.device)
            self._labels[:n] = torch.from_numpy(z["labels"]).to(self.device)
            self._n = n
        if cent.shape[0]:
            lists = z["lists"]
            self.train(centroids=cent)       # (assigns the rows again: the same exact search gives the stored numbers)
            if n and lists.shape[0] == n:
                self._list[:n] = torch.from_numpy(lists).to(self.device)

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
        lists = torch.zeros((new_cap,), dtype=torch.int64, device=self.device)
        labels = torch.full((new_cap,), -1, dtype=torch.int64, device=self.device)
        dead = torch.zeros((new_cap,), dtype=torch.bool, device=self.device)
        if self._f32 is not None and self._n:
            f32[:self._n] = self._f32[:self._n]
            lists[:self._n] = self._list[:self._n]
            labels[:self._n] = self._labels[:self._n]
            dead[:self._n] = self._dead[:self._n]
        self._f32, self._list, self._labels, self._dead = f32, lists, labels, dead

    def _compact(self):
        if self._n_dead == 0:
            return
        keep = (~self._dead[:self._n]).nonzero(as_tuple=False).squeeze(1)
        m = keep.numel()
        self._f32[:m] = self._f32[keep]
        self._list[:m] = self._list[keep]
        self._labels[:m] = self._labels[keep]
        self._dead[:self._n] = False
        self._n, self._n_dead = m, 0
        self._packed = None

    def _pack(self):
        """The packed form, rebuilt when rows came or went.  The longest list's length is read back HERE, once per rebuild — the
        search path passes it to the scan as a host number."""
        if self._packed is None:
            order, list_off, row_ids = pack_lists(self._list[:self._n], self.nlist)
            longest = int((list_off[1:] - list_off[:-1]).max())
            self._packed = (self._f32[:self._n].index_select(0, order), list_off, row_ids, longest)
        return self._packed
