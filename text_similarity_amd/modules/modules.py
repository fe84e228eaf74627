"""Pooling modules on the hot path (/root/reference/src/modules/modules.py:154-195): ``AvgPoolingStrategy``, the masked
mean of the HIP kernel ``mean_pool_kernel`` through ``tsim_mean_pool``; ``CLSPoolingStrategy`` and ``BertPoolingStrategy``;
and ``SentenceEmbeddingHead``, the Pooling -> Dense -> Normalize chain of a sentence-transformers checkpoint.  The last three
run ``tsim_pool`` / ``tsim_dense_rows`` on padded input, and hand the native encoder a ``SentenceHead`` (``native_head``)
that its packed forward runs in place of the mean pool (include/tsim.h tsim_encoder_forward_head)."""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .. import ops
from ..dataset.dataset import EmbeddingsFeatures


class PoolingStrategy(nn.Module):
    """Base class (modules.py:44-55).  ``params`` is optional here: the reference's own ``from_pretrained`` calls
    ``AvgPoolingStrategy()`` without it (sentence_encoder.py:201), which its constructor rejects."""

    def __init__(self, params=None, *args, **kwargs):
        super().__init__()
        self.params = params

    def forward(self, embeddings: torch.Tensor, features: EmbeddingsFeatures = None):
        raise NotImplementedError()


class AvgPoolingStrategy(PoolingStrategy):
    def forward(self, embeddings: torch.Tensor, features: EmbeddingsFeatures):
        assert len(embeddings.shape) == 3  # batch, seq_len, embed_size
        mask = features.to_dict()["attention_mask"]
        return ops.mean_pool(embeddings, mask)


class _NativeHead(PoolingStrategy):
    """A pooling mode, an optional Dense (``_linear()``: an nn.Linear or None) with activation, an optional Normalize."""
    pooling_mode = "mean"
    activation_name = "identity"
    normalize = False

    def _linear(self) -> Optional[nn.Linear]:
        return None

    def output_width(self, hidden: int) -> int:
        lin = self._linear()
        return int(lin.out_features) if lin is not None else int(hidden)

    def _device_dense(self, device):
        """(W, b) of the Dense as contiguous float32 tensors on ``device``; copies are kept while the parameters are unchanged."""
        lin = self._linear()
        if lin is None:
            return None, None
        b = lin.bias
        key = (str(torch.device(device)), lin.weight.data_ptr(), lin.weight._version,
               None if b is None else (b.data_ptr(), b._version))
        cached = self.__dict__.get("_dense_cache")
        if cached is None or cached[0] != key:
            w_d = lin.weight.detach().to(device=device, dtype=torch.float32).contiguous()
            b_d = None if b is None else b.detach().to(device=device, dtype=torch.float32).contiguous()
            cached = (key, w_d, b_d)
            self.__dict__["_dense_cache"] = cached
        return cached[1], cached[2]

    def native_head(self, device):
        """The :class:`~text_similarity_amd.native_encoder.SentenceHead` the packed forward runs for this module."""
        from ..native_encoder import SentenceHead
        w, b = self._device_dense(device)
        return SentenceHead(self.pooling_mode, w, b, self.activation_name, self.normalize)

    def forward(self, embeddings: torch.Tensor, features: EmbeddingsFeatures):
        assert len(embeddings.shape) == 3  # batch, seq_len, embed_size
        mask = features.to_dict()["attention_mask"]
        x = ops.pool(embeddings, mask, self.pooling_mode)
        lin = self._linear()
        if lin is None and not self.normalize:
            return x
        w, b = self._device_dense(x.device)
        return ops.dense_rows(x, w, b, self.activation_name, self.normalize)


class CLSPoolingStrategy(_NativeHead):
    """modules.py:174-181.  The reference returns ``embeddings[:0:]``, an empty slice of the batch; its evident meaning, the
    CLS (first) token's row of every sequence, is what runs here."""
    pooling_mode = "cls"


class BertPoolingStrategy(_NativeHead):
    """modules.py:184-195: tanh(Linear(CLS row)).  Holds ``linear`` (nn.Linear(H, H)) and ``activation`` (nn.Tanh) as the
    reference does, so its state_dict loads; both run natively (CLS pooling, then ``tsim_dense_rows`` with tanh).
    ``hidden_size`` overrides ``params.model_parameters.hidden_size``."""
    pooling_mode = "cls"
    activation_name = "tanh"

    def __init__(self, params=None, *args, hidden_size: Optional[int] = None, **kwargs):
        super().__init__(params, *args, **kwargs)
        if hidden_size is None:
            hidden_size = self.params.model_parameters.hidden_size
        self.linear = nn.Linear(hidden_size, hidden_size)
        self.activation = nn.Tanh()

    def _linear(self):
        return self.linear


class SentenceEmbeddingHead(_NativeHead):
    """The sentence-transformers chain Pooling -> optional Dense -> optional Normalize as one pooling strategy.
    ``pooling_mode``: 'mean' | 'cls' | 'max' | 'mean_sqrt_len'; ``dense``: an nn.Linear (float32, widths multiples of 8 up to
    1024) or None; ``activation``: 'identity' | 'tanh' (the Dense's); ``normalize``: F.normalize of the final rows."""

    def __init__(self, params=None, pooling_mode: str = "mean", dense: Optional[nn.Linear] = None,
                 activation: str = "identity", normalize: bool = False):
        super().__init__(params)
        ops.pool_mode_id(pooling_mode)
        ops.activation_id(activation)
        if dense is None and activation != "identity":
            raise ValueError("an activation needs a Dense")
        self.pooling_mode = pooling_mode
        self.activation_name = activation
        self.normalize = bool(normalize)
        self.dense = dense

    def _linear(self):
        return self.dense

    @classmethod
    def from_spec(cls, spec, params=None) -> "SentenceEmbeddingHead":
        """From a parsed sentence-transformers directory (models/st_format.HeadSpec)."""
        dense = None
        if spec.dense is not None:
            d = spec.dense
            dense = nn.Linear(d.in_features, d.out_features, bias=d.bias is not None)
            with torch.no_grad():
                dense.weight.copy_(torch.from_numpy(d.weight))
                if d.bias is not None:
                    dense.bias.copy_(torch.from_numpy(d.bias))
        return cls(params, spec.pooling, dense, spec.dense.activation if spec.dense is not None else "identity", spec.normalize)


def st_modules(pooler):
    """The sentence-transformers description (pooling, DenseSpec or None, normalize) of a native head module."""
    from ..models.st_format import DenseSpec
    lin = pooler._linear()
    dense = None
    if lin is not None:
        dense = DenseSpec(int(lin.in_features), int(lin.out_features), pooler.activation_name,
                          lin.weight.detach().float().cpu().numpy(),
                          None if lin.bias is None else lin.bias.detach().float().cpu().numpy())
    return pooler.pooling_mode, dense, bool(pooler.normalize)
