"""The row store behind the refine stage of GpuPQIndex and GpuIVFPQIndex (faiss' ``IndexRefineFlat`` / ``IndexRefine(SQfp16)``):
the rows as they were given, in arrival order beside the codes, as float32 or as float16 made by :func:`ops.f16_rows`, and the
exact re-score of a first stage's candidates against them (``ops.*_list_topk`` / ``ops.f16_list_topk``)."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import ops

KINDS = ("float32", "float16")
_CONVERT_CHUNK = 1 << 18      # rows converted at a time (ivfpq_index._ENCODE_CHUNK: the encoder's input is cut the same way)
_LIST_SPACE = {"ip": "dot", "l2": "l2", "cosine": "cosine"}
_F32_OPS = {"ip": ops.dot_list_topk, "l2": ops.l2_list_topk, "cosine": ops.cosine_list_topk}


def check_refine(who: str, refine, space: str, dim: int):
    """``refine`` of a constructor: None or one of KINDS, and with a store a width the list search takes"""
    if refine is None:
        return None
    if refine not in KINDS:
        raise ValueError(f"{who}: refine must be None, 'float32' or 'float16', not {refine!r}")
    limit = ops.L2_MAX_DIM if space == "l2" else 768
    if dim > limit:
        raise ValueError(f"{who}: refine={refine!r} re-scores with the exact list search, which takes dim <= {limit} under "
                         f"{space!r}; got dim={dim}")
    return refine


def raw_queries(data, dim: int, device) -> torch.Tensor:
    """rows or queries as given (NOT normalised): float32 [Q, dim] on the device, contiguous"""
    q = data if isinstance(data, torch.Tensor) else torch.as_tensor(np.asarray(data))
    if q.dim() == 1:
        q = q.unsqueeze(0)
    if q.dim() != 2 or q.shape[1] != dim:
        raise ValueError(f"expected rows of width {dim}, got {tuple(q.shape)}")
    if not q.dtype.is_floating_point:
        raise ValueError(f"expected float rows, got {q.dtype}")
    return q.to(device, dtype=torch.float32).contiguous()


def check_multiplier(rescore_multiplier, store) -> int:
    if store is None:
        raise ValueError("rescore_multiplier needs a row store: build the index with refine='float32' or refine='float16'")
    if isinstance(rescore_multiplier, bool) or int(rescore_multiplier) != rescore_multiplier or int(rescore_multiplier) < 1:
        raise ValueError(f"rescore_multiplier={rescore_multiplier!r} must be an integer >= 1")
    return int(rescore_multiplier)


def padded(Q: int, k: int, space: str, device) -> Tuple[torch.Tensor, torch.Tensor]:
    return (torch.full((Q, k), float("inf" if space == "l2" else "-inf"), dtype=torch.float32, device=device),
            torch.full((Q, k), -1, dtype=torch.int64, device=device))


class RowStore:
    def __init__(self, kind: str, space: str, dim: int, device):
        self.kind, self.space, self.dim, self.device = kind, space, int(dim), device
        self.dtype = torch.float32 if kind == "float32" else torch.float16
        self.np_dtype = np.float32 if kind == "float32" else np.float16
        self.rows: Optional[torch.Tensor] = None     # [capacity, dim]

    def convert(self, x: torch.Tensor) -> torch.Tensor:
        """float32 rows [n, dim] on the device -> the store's dtype; a row that is not finite there raises ``ValueError``"""
        out = torch.empty((x.shape[0], self.dim), dtype=self.dtype, device=self.device)
        for r0 in range(0, x.shape[0], _CONVERT_CHUNK):
            xs = x[r0:r0 + _CONVERT_CHUNK]
            if self.kind == "float16":
                try:
                    out[r0:r0 + xs.shape[0]] = ops.f16_rows(xs)
                except ValueError as e:
                    raise ValueError(f"refine='float16': a row among rows {r0}..{r0 + xs.shape[0] - 1} cannot be stored ({e})") from None
            else:
                if not bool(torch.isfinite(xs).all()):
                    raise ValueError(f"refine='float32': a row among rows {r0}..{r0 + xs.shape[0] - 1} is not finite")
                out[r0:r0 + xs.shape[0]] = xs
        return out

    def reserve(self, capacity: int, n: int):
        """at least ``capacity`` rows, the first ``n`` kept"""
        if self.rows is not None and self.rows.shape[0] >= capacity:
            return
        rows = torch.zeros((capacity, self.dim), dtype=self.dtype, device=self.device)
        if self.rows is not None and n:
            rows[:n] = self.rows[:n]
        self.rows = rows

    def put(self, at: int, rows: torch.Tensor):
        self.rows[at:at + rows.shape[0]] = rows

    def compact(self, keep: torch.Tensor):
        self.rows[:keep.numel()] = self.rows[keep]

    def rescore(self, q_raw: torch.Tensor, n: int, cand: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """exact (scores, store rows) [Q, k] of the raw queries among the candidates ``cand`` [Q, m] (arrival rows, -1 padding)"""
        rows = self.rows[:n]
        if self.kind == "float16":
            return ops.f16_list_topk(_LIST_SPACE[self.space], q_raw, rows, cand, k=k, assume_unique=True)
        return _F32_OPS[self.space](q_raw, rows, cand, k=k, assume_unique=True)

    def to_numpy(self, n: int) -> np.ndarray:
        return self.rows[:n].cpu().numpy() if n else np.zeros((0, self.dim), self.np_dtype)


def save_fields(store: Optional[RowStore], n: int) -> dict:
    """what a ``.npz`` gains when a store is held"""
    if store is None:
        return {}
    return {"refine": np.array(store.kind), "refine_rows": np.ascontiguousarray(store.to_numpy(n))}


def load_store(z, path: str, n: int, space: str, dim: int, device) -> Tuple[Optional[RowStore], Optional[np.ndarray]]:
    """(store, rows) of a file, (None, None) when it holds none; a ``refine_rows`` of the wrong shape or dtype is malformed"""
    if "refine" not in z.files and "refine_rows" not in z.files:
        return None, None
    if "refine" not in z.files or "refine_rows" not in z.files:
        raise ValueError(f"{path}: malformed index: refine and refine_rows come together")
    kind = str(z["refine"])
    if kind not in KINDS:
        raise ValueError(f"{path}: malformed index: refine={kind!r}")
    check_refine(path, kind, space, dim)
    store = RowStore(kind, space, dim, device)
    rows = z["refine_rows"]
    if rows.dtype != store.np_dtype or rows.shape != (n, dim):
        raise ValueError(f"{path}: malformed index: refine_rows is {rows.dtype} {tuple(rows.shape)}, expected "
                         f"{np.dtype(store.np_dtype)} {(n, dim)}")
    return store, rows
