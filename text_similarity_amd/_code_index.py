"""What GpuBinaryIndex and GpuInt8Index share: code rows and int64 labels resident in HBM, appended in place, searched in one
stage or two (first stage over the codes, re-score of its candidates with the float32 queries), saved as one ``.npz``.

A subclass sets ``_CODE_DTYPE``, ``_NP_DTYPE`` and ``_FILE_NAME``, gives the padded row width to the constructor and supplies
``_as_codes(data, adding=False)``, the ops ``_first_stage``, ``_rescore`` and ``_pad_codes`` (unpadded codes -> the device
layout), ``save_index`` and ``load_index``."""
from __future__ import annotations

import os
from typing import Iterable, Optional, Tuple

import numpy as np
import torch

from . import ops


class _CodeIndex:
    _CODE_DTYPE: torch.dtype
    _NP_DTYPE: type
    _FILE_NAME: str                                        # what save_index / load_index use inside a directory

    def __init__(self, dim: int, cb: int, device: Optional[torch.device]):
        self.dim = int(dim)
        self._cb = cb
        self.device = torch.device(device) if device is not None else torch.device("cuda")
        self._codes: Optional[torch.Tensor] = None     # [capacity, _cb] _CODE_DTYPE
        self._labels: Optional[torch.Tensor] = None    # [capacity] int64
        self._n = 0

    def get_current_count(self) -> int:
        return self._n

    def add_items(self, data, ids: Optional[Iterable[int]] = None):
        codes = self._as_codes(data, adding=True)
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
        k = int(k)
        q = data if isinstance(data, torch.Tensor) else torch.as_tensor(np.asarray(data))
        if q.dim() == 1:
            q = q.unsqueeze(0)
        qc = self._as_codes(q)
        Q = qc.shape[0]
        codes = self._codes[:self._n] if self._n else torch.zeros((0, self._cb), dtype=self._CODE_DTYPE, device=self.device)
        if rescore_multiplier is None:
            val, idx = self._first_stage(qc, codes, self.dim, k)
            return val, self._to_labels(idx)
        if q.dtype == self._CODE_DTYPE:
            raise ValueError("re-scoring needs the float queries, not their codes")
        mult = int(rescore_multiplier)
        if mult < 1:
            raise ValueError(f"rescore_multiplier={rescore_multiplier} must be >= 1")
        qf = q.to(self.device, dtype=torch.float32).contiguous()
        m = min(k * mult, ops.MAX_K, self._n)
        if m == 0 or Q == 0:
            return (torch.full((Q, k), float("-inf"), dtype=torch.float32, device=self.device),
                    torch.full((Q, k), -1, dtype=torch.int64, device=self.device))
        _, cand = self._first_stage(qc, codes, self.dim, m)
        scores, idx = self._rescore(qf, codes, self.dim, cand, k)
        return scores, self._to_labels(idx)

    def knn_query(self, data, k: int = 1, rescore_multiplier: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        val, lab = self.search(data, k, rescore_multiplier)
        return lab.cpu().numpy(), val.cpu().numpy()

    # ------------------------------------------------------------------ internals
    def _file(self, path: str) -> str:
        return os.path.join(path, self._FILE_NAME) if os.path.isdir(path) else path

    def _stored(self, width: int):
        """(codes [n, width], labels [n]) of the rows held, as numpy arrays"""
        codes = self._codes[:self._n, :width].cpu().numpy() if self._n else np.zeros((0, width), self._NP_DTYPE)
        labels = self._labels[:self._n].cpu().numpy() if self._n else np.zeros((0,), np.int64)
        return codes, labels

    def _restore(self, codes: np.ndarray, labels: np.ndarray, max_elements: int):
        """replace what the index holds by the unpadded numpy ``codes`` and ``labels`` of a file"""
        self._codes = self._labels = None
        self._n = 0
        n = codes.shape[0]
        self._reserve(max(n, int(max_elements)))
        if n:
            self._codes[:n] = self._pad_codes(codes, self.dim, device=self.device)
            self._labels[:n] = torch.from_numpy(labels.astype(np.int64)).to(self.device)
            self._n = n

    def _to_labels(self, idx: torch.Tensor) -> torch.Tensor:
        if self._n == 0:
            return torch.full_like(idx, -1)
        return torch.where(idx >= 0, self._labels[idx.clamp(min=0)], torch.full_like(idx, -1))

    def _reserve(self, n: int):
        cap = 0 if self._codes is None else self._codes.shape[0]
        if n <= cap:
            return
        new_cap = max(n, 2 * cap, 1024)
        codes = torch.zeros((new_cap, self._cb), dtype=self._CODE_DTYPE, device=self.device)
        labels = torch.full((new_cap,), -1, dtype=torch.int64, device=self.device)
        if self._codes is not None and self._n:
            codes[:self._n] = self._codes[:self._n]
            labels[:self._n] = self._labels[:self._n]
        self._codes, self._labels = codes, labels
