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

from typing import Optional, Tuple

import numpy as np
import torch

from . import ops
from ._code_index import _CodeIndex


class GpuBinaryIndex(_CodeIndex):
    _CODE_DTYPE, _NP_DTYPE, _FILE_NAME = torch.uint8, np.uint8, "binary_index.bin"
    _first_stage = staticmethod(ops.hamming_topk)
    _rescore = staticmethod(ops.sign_rescore_topk)
    _pad_codes = staticmethod(ops.codes_from_packbits)

    def __init__(self, dim: int, device: Optional[torch.device] = None):
        super().__init__(dim, ops.code_bytes(int(dim)), device)   # raises outside 1..1024

    def _as_codes(self, data, adding: bool = False) -> torch.Tensor:
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

    def search(self, data, k: int, rescore_multiplier: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Without ``rescore_multiplier``: (dist [Q,k] int32, labels [Q,k] int64) by (Hamming distance asc, row asc), padded with
        (2**31 - 1, -1) when the index holds fewer than k rows.  With it (float queries only): the min(k * multiplier, 1024, count)
        nearest codes are re-scored with the float32 queries; returns (scores [Q,k] float32, labels) by (score desc, row asc),
        padded with (-inf, -1)."""
        return super().search(data, k, rescore_multiplier)

    def knn_query(self, data, k: int = 1, rescore_multiplier: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(labels [Q,k] int64, distances [Q,k]) as numpy arrays, best first — the order of ``GpuFlatIndex.knn_query``.  Distances
        are int32 Hamming distances, or with ``rescore_multiplier`` the float32 re-scores (larger is better)."""
        return super().knn_query(data, k, rescore_multiplier)

    def save_index(self, path: str):
        codes, labels = self._stored((self.dim + 7) // 8)
        with open(self._file(path), "wb") as f:
            np.savez(f, codes=np.ascontiguousarray(codes), labels=labels, dim=np.int64(self.dim))

    def load_index(self, path: str, max_elements: int = 0):
        path = self._file(path)
        z = np.load(path, allow_pickle=False)
        if "codes" not in z.files:
            raise ValueError(f"{path} does not hold a binary index")
        if int(z["dim"]) != self.dim:
            raise ValueError(f"{path} holds codes of width {int(z['dim'])}; this index has width {self.dim}")
        self._restore(z["codes"], z["labels"], max_elements)
