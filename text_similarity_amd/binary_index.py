"""GpuBinaryIndex — an exact Hamming index over sign-bit codes resident in HBM (faiss' ``IndexBinaryFlat``; the corpus side of
sentence-transformers' ``quantize_embeddings(precision="ubinary")`` + ``semantic_search_faiss(..., rescore=True)``).

Layout: uint8 code rows ``[capacity, ops.code_bytes(dim)]`` — ``np.packbits(x > 0, axis=1)`` of every row, zero-padded to a
multiple of 16 bytes — and int64 labels.  A 384-wide row takes 48 bytes, a 1024-wide one 128; ``dim`` may be anything in
1..1024, so the hidden-1024 encoders, which the float searches (d <= 768) cannot serve, search here.

``search`` is exact under (Hamming distance asc, row asc).  With ``rescore_multiplier`` the k * multiplier nearest codes are
re-scored with the FLOAT32 query against the +-1 expansion of the codes (:func:`ops.sign_rescore_topk`) and the best k by
(score desc, row asc) are returned — the usual second stage; the float32 corpus is never needed.

No deletions, no filters and no sharding here.  On disk: a numpy ``.npz`` written without pickling, holding the
packbits codes ``[n, ceil(dim / 8)]``, the labels and ``dim``.
"""
from __future__ import annotations

import os
from typing import Iterable, Optional, Tuple

import numpy as np
import torch

from . import ops


class GpuBinaryIndex:
    def __init__(self, dim: int, device: Optional[torch.device] = None):
        self.dim = int(dim)
        self._cb = ops.code_bytes(self.dim)           # raises outside 1..1024
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self._codes: Optional[torch.Tensor] = None     # [capacity, code_bytes(dim)] uint8
        self._labels: Optional[torch.Tensor] = None    # [capacity] int64
        self._n = 0

    def get_current_count(self) -> int:
        return self._n

    def _as_codes(self, data) -> torch.Tensor:
        """float rows [n, dim] are packed on the device; uint8 rows [n, ceil(dim / 8)] are packbits codes"""
        x = data if isinstance(data, torch.Tensor) else torch.as_tensor(np.asarray(data))
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if x.dim() != 2:
            raise ValueError("expected a 2-D array of rows")
        if x.dtype == torch.uint8:
            if x.shape[1] != (self.dim + 7) // 8:
                raise ValueError(f"uint8 codes of width {self.dim} have {(self.dim + 7) // 8} bytes a row, got {x.shape[1]}")
            return ops.codes_from_packbits(x.to(self.device), self.dim)
        if not x.dtype.is_floating_point:
            raise ValueError(f"expected float rows or uint8 packbits codes, got {x.dtype}")
        if x.shape[1] != self.dim:
            raise ValueError(f"expected width {self.dim}, got {x.shape[1]}")
        if x.dtype != torch.bfloat16:
            x = x.to(torch.float32)
        return ops.pack_sign_rows(x.to(self.device))

    def add_items(self, data, ids: Optional[Iterable[int]] = None):
        codes = self._as_codes(data)
        n = codes.shape[0]
        if ids is None:
            ids = np.arange(self._n, self._n + n)
        lab = torch.as_tensor(np.asarray(list(ids), dtype=np.int64))
        if lab.numel() != n:
            raise ValueError("ids and data disagree in length")
        self._reserve(self._n + n)
        self._codes[self._n:self._n + n] = codes
        self._labels[self._n:self._n + n] = lab.to(self.device)
        self._n += n

    def search(self, data, k: int, rescore_multiplier: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Without ``rescore_multiplier``: (dist [Q,k] int32, labels [Q,k] int64) by (Hamming distance asc, row asc), padded with
        (2**31 - 1, -1) when the index holds fewer than k rows.  With it (float queries only): the min(k * multiplier, 1024, count)
        nearest codes are re-scored with the float32 queries; returns (scores [Q,k] float32, labels) by (score desc, row asc),
        padded with (-inf, -1)."""
        k = int(k)
        q = data if isinstance(data, torch.Tensor) else torch.as_tensor(np.asarray(data))
        if q.dim() == 1:
            q = q.unsqueeze(0)
        qc = self._as_codes(q)
        Q = qc.shape[0]
        codes = self._codes[:self._n] if self._n else torch.zeros((0, self._cb), dtype=torch.uint8, device=self.device)
        if rescore_multiplier is None:
            dist, idx = ops.hamming_topk(qc, codes, self.dim, k)
            return dist, self._to_labels(idx)
        if q.dtype == torch.uint8:
            raise ValueError("re-scoring needs the float queries, not their codes")
        mult = int(rescore_multiplier)
        if mult < 1:
            raise ValueError(f"rescore_multiplier={rescore_multiplier} must be >= 1")
        qf = q.to(self.device, dtype=torch.float32).contiguous()
        m = min(k * mult, ops.MAX_K, self._n)
        if m == 0 or Q == 0:
            return (torch.full((Q, k), float("-inf"), dtype=torch.float32, device=self.device),
                    torch.full((Q, k), -1, dtype=torch.int64, device=self.device))
        _, cand = ops.hamming_topk(qc, codes, self.dim, m)
        scores, idx = ops.sign_rescore_topk(qf, codes, self.dim, cand, k)
        return scores, self._to_labels(idx)

    def knn_query(self, data, k: int = 1, rescore_multiplier: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(labels [Q,k] int64, distances [Q,k]) as numpy arrays, best first — the order of ``GpuFlatIndex.knn_query``.  Distances
        are int32 Hamming distances, or with ``rescore_multiplier`` the float32 re-scores (larger is better)."""
        d, lab = self.search(data, k, rescore_multiplier)
        return lab.cpu().numpy(), d.cpu().numpy()

    def save_index(self, path: str):
        if os.path.isdir(path):
            path = os.path.join(path, "binary_index.bin")
        nb = (self.dim + 7) // 8
        codes = self._codes[:self._n, :nb].cpu().numpy() if self._n else np.zeros((0, nb), np.uint8)
        labels = self._labels[:self._n].cpu().numpy() if self._n else np.zeros((0,), np.int64)
        with open(path, "wb") as f:
            np.savez(f, codes=np.ascontiguousarray(codes), labels=labels, dim=np.int64(self.dim))

    def load_index(self, path: str, max_elements: int = 0):
        if os.path.isdir(path):
            path = os.path.join(path, "binary_index.bin")
        z = np.load(path, allow_pickle=False)
        if "codes" not in z.files:
            raise ValueError(f"{path} does not hold a binary index")
        if int(z["dim"]) != self.dim:
            raise ValueError(f"{path} holds codes of width {int(z['dim'])}; this index has width {self.dim}")
        codes, labels = z["codes"], z["labels"]
        self._codes = self._labels = None
        self._n = 0
        n = codes.shape[0]
        self._reserve(max(n, int(max_elements)))
        if n:
            self._codes[:n] = ops.codes_from_packbits(codes, self.dim, device=self.device)
            self._labels[:n] = torch.from_numpy(labels.astype(np.int64)).to(self.device)
            self._n = n

    # ------------------------------------------------------------------ internals
    def _to_labels(self, idx: torch.Tensor) -> torch.Tensor:
        if self._n == 0:
            return torch.full_like(idx, -1)
        return torch.where(idx >= 0, self._labels[idx.clamp(min=0)], torch.full_like(idx, -1))

    def _reserve(self, n: int):
        cap = 0 if self._codes is None else self._codes.shape[0]
        if n <= cap:
            return
        new_cap = max(n, 2 * cap, 1024)
        codes = torch.zeros((new_cap, self._cb), dtype=torch.uint8, device=self.device)
        labels = torch.full((new_cap,), -1, dtype=torch.int64, device=self.device)
        if self._codes is not None and self._n:
            codes[:self._n] = self._codes[:self._n]
            labels[:self._n] = self._labels[:self._n]
        self._codes, self._labels = codes, labels
