"""GpuInt8Index — an exact inner-product index over int8 codes resident in HBM (usearch's ``Index(dtype="i8", metric="ip")``;
the corpus side of sentence-transformers' ``quantize_embeddings(precision="int8")`` + ``semantic_search_usearch(...,
rescore=True)``).

Layout: int8 code rows ``[capacity, ops.int8_bytes(dim)]`` — each float row quantised column by column with the index's
calibration ``ranges`` [2, dim] (per-column minimum and maximum), zero-padded to a multiple of 16 bytes — and int64 labels.  One
byte per element; ``dim`` may be anything in 1..1024, so the hidden-1024 encoders, which the float searches (d <= 768) cannot
serve, search here too, much closer to their float ranking than the sign codes of ``GpuBinaryIndex``.

``ranges=None``: the first float batch given to ``add_items`` calibrates the index (``ops.int8_ranges``) and fixes the ranges;
int8 codes can be added without ranges, float queries cannot be searched without them.

``search`` is exact under (int32 score desc, row asc); float queries are quantised with the index's ranges for this stage, as
sentence-transformers does.  With ``rescore_multiplier`` the k * multiplier best codes are re-scored with the FLOAT32 query
against the code values (:func:`ops.int8_rescore_topk`) and the best k by (score desc, row asc) are returned.

No deletions, no filters and no sharding here.  On disk: a numpy ``.npz`` written without pickling, holding the
codes ``[n, dim]`` int8, the labels, ``dim`` and the ranges (shape [0, dim] while the index is uncalibrated).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import ops
from ._code_index import _CodeIndex


def pack_index_file(path, codes: np.ndarray, labels: np.ndarray, dim: int, ranges: Optional[np.ndarray]):
    """the file format of ``save_index`` on numpy data: needs no device"""
    codes = np.ascontiguousarray(codes, dtype=np.int8).reshape(-1, dim)
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    if labels.shape[0] != codes.shape[0]:
        raise ValueError("labels and codes disagree in length")
    r = np.zeros((0, dim), np.float32) if ranges is None else np.asarray(ranges, dtype=np.float32)
    if r.shape not in ((0, dim), (2, dim)):
        raise ValueError(f"ranges must be [2, {dim}], got {r.shape}")
    with open(path, "wb") as f:
        np.savez(f, int8_codes=codes, labels=labels, dim=np.int64(dim), ranges=r)


def unpack_index_file(path, dim: int):
    """(codes int8 [n, dim], labels int64 [n], ranges float32 [2, dim] or None) of a file written by ``pack_index_file``"""
    z = np.load(path, allow_pickle=False)
    if "int8_codes" not in z.files:
        raise ValueError(f"{path} does not hold an int8 index")
    if int(z["dim"]) != dim:
        raise ValueError(f"{path} holds codes of width {int(z['dim'])}; this index has width {dim}")
    codes, labels, r = z["int8_codes"], z["labels"].astype(np.int64), z["ranges"].astype(np.float32)
    if codes.dtype != np.int8 or codes.ndim != 2 or codes.shape[1] != dim or labels.shape != (codes.shape[0],):
        raise ValueError(f"{path}: malformed int8 index")
    return codes, labels, (r if r.shape == (2, dim) else None)


class GpuInt8Index(_CodeIndex):
    _CODE_DTYPE, _NP_DTYPE, _FILE_NAME = torch.int8, np.int8, "int8_index.bin"
    _first_stage = staticmethod(ops.int8_ip_topk)
    _rescore = staticmethod(ops.int8_rescore_topk)
    _pad_codes = staticmethod(ops.int8_codes_from_numpy)

    def __init__(self, dim: int, ranges=None, device: Optional[torch.device] = None):
        super().__init__(dim, ops.int8_bytes(int(dim)), device)   # raises outside 1..1024
        self._ranges: Optional[torch.Tensor] = None    # [2, dim] float32 on the device
        if ranges is not None:
            self._set_ranges(ranges)

    @property
    def ranges(self) -> Optional[torch.Tensor]:
        return self._ranges

    def _set_ranges(self, ranges):
        r = ranges if isinstance(ranges, torch.Tensor) else torch.as_tensor(np.asarray(ranges, dtype=np.float32))
        if tuple(r.shape) != (2, self.dim) or not r.dtype.is_floating_point:
            raise ValueError(f"ranges must be float [2, {self.dim}] (per-column minimum and maximum), got {tuple(r.shape)}")
        self._ranges = r.to(self.device, dtype=torch.float32).contiguous()

    def _as_codes(self, data, adding: bool = False) -> torch.Tensor:
        """float rows [n, dim] are quantised on the device with the index's ranges (rows being added calibrate an index that has
        none); int8 rows [n, dim] are codes"""
        x = data if isinstance(data, torch.Tensor) else torch.as_tensor(np.asarray(data))
        if x.dim() == 1:
            x = x.unsqueeze(0)
        if x.dim() != 2:
            raise ValueError("expected a 2-D array of rows")
        if x.shape[1] != self.dim:
            raise ValueError(f"expected width {self.dim}, got {x.shape[1]}")
        if x.dtype == torch.int8:
            return ops.int8_codes_from_numpy(x.to(self.device), self.dim)
        if not x.dtype.is_floating_point:
            raise ValueError(f"expected float rows or int8 codes, got {x.dtype}")
        x = x.to(self.device, dtype=torch.float32)
        if self._ranges is None:
            if not adding or x.shape[0] == 0:
                raise ValueError("the index has no calibration ranges yet: pass ranges=, or add float rows first")
            self._ranges = ops.int8_ranges(x)
        return ops.quantize_int8_rows(x, self._ranges)

    def search(self, data, k: int, rescore_multiplier: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Without ``rescore_multiplier``: (score [Q,k] int32, labels [Q,k] int64) by (score desc, row asc), padded with
        (-2**31, -1) when the index holds fewer than k rows.  With it (float queries only): the min(k * multiplier, 1024, count)
        best codes are re-scored with the float32 queries; returns (scores [Q,k] float32, labels) by (score desc, row asc),
        padded with (-inf, -1)."""
        return super().search(data, k, rescore_multiplier)

    def knn_query(self, data, k: int = 1, rescore_multiplier: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(labels [Q,k] int64, scores [Q,k]) as numpy arrays, best first — the order of ``GpuFlatIndex.knn_query``.  Scores are
        the int32 code products, or with ``rescore_multiplier`` the float32 re-scores (larger is better either way)."""
        return super().knn_query(data, k, rescore_multiplier)

    def save_index(self, path: str):
        codes, labels = self._stored(self.dim)
        pack_index_file(self._file(path), codes, labels, self.dim, None if self._ranges is None else self._ranges.cpu().numpy())

    def load_index(self, path: str, max_elements: int = 0):
        codes, labels, ranges = unpack_index_file(self._file(path), self.dim)
        self._ranges = None
        if ranges is not None:
            self._set_ranges(ranges)
        self._restore(codes, labels, max_elements)
