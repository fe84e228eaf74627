"""GpuPQIndex — a product-quantisation index resident in HBM (faiss' ``IndexPQ`` with 8-bit codes): a learned code of ``M``
bytes per row, searched with the FLOAT query by asymmetric distance computation (ADC).

Layout: uint8 code rows ``[capacity, ops.pq_code_bytes(M)]`` — byte m is the number of the centroid of sub-space m nearest to
the row's sub-vector m, zero-padded to a multiple of 16 bytes — int64 labels, and the codebooks ``[M, 256, dim / M]`` float32.
A 384-wide row takes 48 bytes at M = 48 and a 1024-wide one 64 bytes at M = 64, so the hidden-1024 encoders, which the float
searches (d <= 768) cannot serve, search here too.  ``dim`` in 1..1024, ``M`` in 1..64, ``dim % M == 0``, ``dim / M <= 64``.

``space``: ``"ip"`` (inner product with the row's reconstruction, larger is better), ``"l2"`` (squared Euclidean distance to
it, smaller is better) or ``"cosine"`` — ip with rows normalised before encoding and queries before their tables
(:meth:`GpuPQIndex.normalise`).

``train`` learns the codebooks: per sub-space, Lloyd's iterations of :class:`pipeline.clustering.ClusteringPipeline` with 256
centres on a seeded sample of the rows, as ``GpuIVFIndex.train`` does for its lists; or installs given ``codebooks``.  Adding or
searching before training raises.  ``search`` is exact for the integer ADC scores of :func:`ops.pq_adc_topk` under (score desc,
row asc) — l2: (distance asc, row asc) — and returns them as float32.

Refine stage (faiss' ``IndexRefineFlat`` / ``IndexRefine(SQfp16)``).  ``refine="float32"`` or ``"float16"`` keeps the rows as
they were given (before the cosine normalisation) beside the codes, as float32 or as the float16 of :func:`ops.f16_rows`
(``dim <= 768``, ``"l2"`` 767: the widths the list search takes).  ``search(q, k, rescore_multiplier=mult)`` then takes the
``min(k * mult, ops.MAX_K, rows held)`` best rows of the ADC search as candidates and re-scores them exactly against the
stored rows with the query as given — ``ops.cosine_list_topk`` / ``dot_list_topk`` / ``l2_list_topk`` on a float32 store,
``ops.f16_list_topk`` on a float16 one — and returns the exact float32 scores of the index's space.  Without
``rescore_multiplier`` a search is the ADC search, store or not.

No deletions, no filters, no sharding, no residual or IVF-PQ encoding and no OPQ rotation here.  On disk: one
numpy ``.npz`` written without pickling, holding the codebooks, the codes ``[n, M]`` uint8, the labels, ``space``, ``dim`` and
``M``, and with a store ``refine`` and ``refine_rows`` ``[n, dim]``; loading adopts the file's ``refine``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _refine, ops
from ._code_index import _CodeIndex

K_CENTROIDS = 256


class GpuPQIndex(_CodeIndex):
    SPACES = ("ip", "l2", "cosine")
    _CODE_DTYPE, _NP_DTYPE, _FILE_NAME = torch.uint8, np.uint8, "pq_index.bin"

    def __init__(self, space: str = "ip", dim: int = 0, M: int = 8, device: Optional[torch.device] = None, seed: int = 0,
                 refine: Optional[str] = None):
        if space not in self.SPACES:
            raise ValueError(f"GpuPQIndex implements the spaces {self.SPACES}, not {space!r}")
        dim, M = int(dim), int(M)
        if not (1 <= dim <= ops.MAX_CODE_DIM and 1 <= M <= ops.PQ_MAX_M and dim % M == 0 and dim // M <= ops.PQ_MAX_DSUB):
            raise ValueError(f"GpuPQIndex takes 1 <= dim <= {ops.MAX_CODE_DIM}, 1 <= M <= {ops.PQ_MAX_M}, dim % M == 0 and "
                             f"dim / M <= {ops.PQ_MAX_DSUB}; got dim={dim}, M={M}")
        super().__init__(dim, ops.pq_code_bytes(M), device)
        self.space, self.M, self.dsub, self.seed = space, M, dim // M, int(seed)
        self._adc_space = "l2" if space == "l2" else "ip"
        self.codebooks: Optional[torch.Tensor] = None    # [M, 256, dsub] float32 on the device, finite
        self.refine = _refine.check_refine("GpuPQIndex", refine, space, dim)
        self._store = None if self.refine is None else _refine.RowStore(self.refine, space, dim, self.device)

    @property
    def is_trained(self) -> bool:
        return self.codebooks is not None

    def num_live(self) -> int:
        """rows held (nothing is ever deleted here): what ``GpuFlatIndex.num_live`` reports"""
        return self._n

    @staticmethod
    def normalise(x: torch.Tensor) -> torch.Tensor:
        """what the cosine space does to rows before encoding and to queries before their tables (float32)"""
        return x / x.norm(dim=1, keepdim=True).clamp(min=1e-12)

    # ------------------------------------------------------------------ training
    def _set_codebooks(self, codebooks):
        c = codebooks if isinstance(codebooks, torch.Tensor) else torch.as_tensor(np.asarray(codebooks, dtype=np.float32))
        if tuple(c.shape) != (self.M, K_CENTROIDS, self.dsub) or not c.dtype.is_floating_point:
            raise ValueError(f"codebooks must be float [{self.M}, {K_CENTROIDS}, {self.dsub}], got {tuple(c.shape)}")
        c = c.to(self.device, dtype=torch.float32).contiguous()
        if not bool(torch.isfinite(c).all()):
            raise ValueError("codebooks must be finite")
        self.codebooks = c

    def _rows(self, data) -> torch.Tensor:
        x = data if isinstance(data, torch.Tensor) else torch.as_tensor(np.asarray(data))
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if x.dim() != 2 or x.shape[1] != self.dim:
            raise ValueError(f"expected rows of width {self.dim}, got {tuple(x.shape)}")
        if not x.dtype.is_floating_point:
            raise ValueError(f"expected float rows, got {x.dtype}")
        return self._prepared(x.to(self.device, dtype=torch.float32))

    def _prepared(self, x: torch.Tensor) -> torch.Tensor:
        return self.normalise(x) if self.space == "cosine" else x

    def train(self, data=None, niter: int = 20, max_points_per_centroid: int = 256, codebooks=None, init_codebooks=None):
        """Set the codebooks.  ``codebooks`` [M, 256, dim / M]: installed as given, no clustering.  Else, per sub-space, k-means
        with 256 centres (``niter`` Lloyd iterations at most; k-means++ seeding, or ``init_codebooks`` [M, 256, dim / M]) on a
        seeded sample of at most ``256 * max_points_per_centroid`` rows of ``data``.  With fewer than 256 training rows the
        missing centroids are copies of centroid 0, which the encoder never chooses (ties go to the lower number).  Any
        sub-space width trains, down to dim == M (one element: tests/test_pq_index_gpu.py trains at widths 1, 2 and 4).  Rows
        already stored keep their codes: train before adding."""
        if codebooks is not None:
            self._set_codebooks(codebooks)
            return
        if data is None:
            raise ValueError("train needs data= or codebooks=")
        x = self._rows(data)
        if x.shape[0] == 0 or not bool(torch.isfinite(x).all()):
            raise ValueError("train needs at least one row, all finite")
        m = K_CENTROIDS * int(max_points_per_centroid)
        if x.shape[0] > m:
            g = torch.Generator(device="cpu").manual_seed(self.seed)
            x = x[torch.randperm(x.shape[0], generator=g)[:m].sort()[0].to(self.device)]
        init = None
        if init_codebooks is not None:
            init = torch.as_tensor(np.asarray(init_codebooks) if not isinstance(init_codebooks, torch.Tensor) else init_codebooks)
            if tuple(init.shape) != (self.M, K_CENTROIDS, self.dsub):
                raise ValueError(f"init_codebooks must have shape ({self.M}, {K_CENTROIDS}, {self.dsub}), got {tuple(init.shape)}")
        from .pipeline.clustering import ClusteringPipeline
        k = min(K_CENTROIDS, x.shape[0])
        out = torch.empty((self.M, K_CENTROIDS, self.dsub), dtype=torch.float32, device=self.device)
        # (the deterministic form of fit's scatter-add: the same rows and seed give the same codebooks bit for bit)
        was, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
        torch.use_deterministic_algorithms(True, warn_only=True)
        try:
            for s in range(self.M):
                km = ClusteringPipeline(K_CENTROIDS, params=None, model=None, max_iter=int(niter), seed=self.seed + s)
                sub = x[:, s * self.dsub:(s + 1) * self.dsub].contiguous()
                c = km.fit(sub, init=None if init is None else init[s, :k]).cluster_centers_
                out[s, :k] = c
                out[s, k:] = c[0]
        finally:
            torch.use_deterministic_algorithms(was, warn_only=warn)
        self._set_codebooks(out)

    # ------------------------------------------------------------------ rows in, results out
    def _need_trained(self):
        if self.codebooks is None:
            raise RuntimeError("the index is not trained: call train(data) or train(codebooks=...) first")

    def _as_codes(self, data, adding: bool = False) -> torch.Tensor:
        """float rows [n, dim] are encoded on the device with the index's codebooks; uint8 rows [n, M] are codes"""
        self._need_trained()
        x = data if isinstance(data, torch.Tensor) else torch.as_tensor(np.asarray(data))
        if x.dtype == torch.uint8:
            if x.dim() != 2 or x.shape[1] != self.M:
                raise ValueError(f"expected uint8 codes [n, {self.M}], got {tuple(x.shape)}")
            return ops.pq_codes_from_numpy(x.to(self.device), self.M)
        return ops.pq_encode_rows(self._rows(x), self.codebooks, _trusted=True)

    def add_items(self, data, ids=None):
        """Rows in (float rows are encoded; uint8 rows [n, M] are codes).  With a row store the rows as given are kept too: codes
        alone raise ``ValueError`` then (there is no row to keep), and so does a row that is not finite in the store's dtype —
        before anything is added."""
        if self._store is None:
            return super().add_items(data, ids)
        x = data if isinstance(data, torch.Tensor) else torch.as_tensor(np.asarray(data))
        if x.dtype == torch.uint8:
            raise ValueError(f"refine={self.refine!r} keeps the rows: add float rows, not uint8 codes")
        self._need_trained()
        kept = self._store.convert(_refine.raw_queries(x, self.dim, self.device))
        at = self._n
        super().add_items(x, ids)
        self._store.put(at, kept)

    def _reserve(self, n: int):
        super()._reserve(n)
        if self._store is not None:
            self._store.reserve(self._codes.shape[0], self._n)

    def search(self, data, k: int, rescore_multiplier: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(values [Q,k] float32, labels [Q,k] int64) of float queries [Q, dim], best first: ip and cosine by (score desc, row
        asc), padded with (-inf, -1); l2 by (squared distance asc, row asc), padded with (+inf, -1).  The values are those of
        :func:`ops.pq_adc_topk` with the index's codebooks and codes.  ``rescore_multiplier`` (an integer >= 1; needs
        ``refine=``): the ``min(k * rescore_multiplier, ops.MAX_K, rows held)`` best of that search are re-scored exactly
        against the stored rows with the query as given, and the values are the exact float32 scores of the space (module
        docstring)."""
        self._need_trained()
        k = int(k)
        if rescore_multiplier is not None:
            mult = _refine.check_multiplier(rescore_multiplier, self._store)
            q_raw = _refine.raw_queries(data, self.dim, self.device)
            m = min(k * mult, ops.MAX_K, self._n)
            if not 1 <= k <= ops.MAX_K:
                raise ValueError(f"k={k} outside 1..{ops.MAX_K}")
            if m == 0 or q_raw.shape[0] == 0:
                return _refine.padded(q_raw.shape[0], k, self.space, self.device)
            _, cand = ops.pq_adc_topk(self._prepared(q_raw).contiguous(), self.codebooks, self._codes[:self._n], m, self._adc_space,
                                      _trusted=True)
            val, idx = self._store.rescore(q_raw, self._n, cand, k)
            return val, self._to_labels(idx)
        q = self._rows(data).contiguous()
        codes = self._codes[:self._n] if self._n else torch.zeros((0, self._cb), dtype=torch.uint8, device=self.device)
        val, idx = ops.pq_adc_topk(q, self.codebooks, codes, k, self._adc_space, _trusted=True)
        return val, self._to_labels(idx)

    def knn_query(self, data, k: int = 1, rescore_multiplier: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(labels [Q,k] int64, values [Q,k] float32) as numpy arrays, best first — the order of ``GpuFlatIndex.knn_query``;
        the values are :meth:`search`'s (scores for ip and cosine, squared distances for l2)."""
        val, lab = self.search(data, k, rescore_multiplier)
        return lab.cpu().numpy(), val.cpu().numpy()

    def reconstruct(self, labels) -> torch.Tensor:
        """float32 [n, dim]: the centroids the stored rows with these labels were replaced by (cosine: of the normalised row)"""
        self._need_trained()
        lab = torch.as_tensor(np.ascontiguousarray(np.asarray(labels, dtype=np.int64).reshape(-1))).to(self.device)
        held = self._labels[:self._n] if self._n else torch.zeros((0,), dtype=torch.int64, device=self.device)
        order = torch.argsort(held, stable=True)
        pos = torch.searchsorted(held[order], lab).clamp(max=max(self._n - 1, 0))
        if self._n == 0 or not bool((held[order][pos] == lab).all()):
            raise RuntimeError("label not found")
        return ops.pq_decode_rows(self._codes[order[pos]], self.codebooks)

    # ------------------------------------------------------------------ files
    def save_index(self, path: str):
        self._need_trained()
        codes, labels = self._stored(self.M)
        with open(self._file(path), "wb") as f:
            np.savez(f, pq_codes=np.ascontiguousarray(codes), labels=labels, codebooks=self.codebooks.cpu().numpy(),
                     space=np.array(self.space), dim=np.int64(self.dim), M=np.int64(self.M), **_refine.save_fields(self._store, self._n))

    def load_index(self, path: str, max_elements: int = 0):
        z = np.load(self._file(path), allow_pickle=False)
        if "pq_codes" not in z.files:
            raise ValueError(f"{path} does not hold a PQ index")
        if (int(z["dim"]), int(z["M"]), str(z["space"])) != (self.dim, self.M, self.space):
            raise ValueError(f"{path} holds a PQ index of (dim, M, space) = ({int(z['dim'])}, {int(z['M'])}, {str(z['space'])!r}); "
                             f"this one has ({self.dim}, {self.M}, {self.space!r})")
        codes, labels = z["pq_codes"], z["labels"].astype(np.int64)
        if codes.dtype != np.uint8 or codes.ndim != 2 or codes.shape[1] != self.M or labels.shape != (codes.shape[0],):
            raise ValueError(f"{path}: malformed PQ index")
        store, kept = _refine.load_store(z, path, codes.shape[0], self.space, self.dim, self.device)
        self._set_codebooks(z["codebooks"])
        self._store, self.refine = store, None if store is None else store.kind      # (the file decides)
        self._restore(codes, labels, max_elements)
        if store is not None and codes.shape[0]:
            store.put(0, torch.from_numpy(kept).to(self.device))

    @staticmethod
    def _pad_codes(codes, dim, device=None):   # (_CodeIndex._restore hands the index's dim; the row width is the codes' own)
        return ops.pq_codes_from_numpy(codes, codes.shape[1], device=device)
