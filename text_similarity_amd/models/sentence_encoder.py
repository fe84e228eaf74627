"""SBERT-style bi-encoder wrappers with the reference's names and signatures
(/root/reference/src/models/sentence_encoder.py): ``OnnxSentenceTransformerWrapper`` (:17-39) and
``SentenceTransformerWrapper`` (:71-217), running on the native MI355X encoder.

What is reproduced is the *intended* behaviour: ``encode_text`` in the reference calls
``self.encode(features, parallel_mode=False)`` (:161) although ``encode`` is ``encode(documents, output_np)``
(:133) — a TypeError as shipped; its evident meaning, encoder forward + pooler on the batch, is what runs here.
"""
from __future__ import annotations

import os
import warnings
from typing import List, Optional, Union

import numpy as np
import torch
from torch import nn

from ..dataset.dataset import EmbeddingsFeatures
from ..modules.modules import AvgPoolingStrategy, PoolingStrategy, SentenceEmbeddingHead, st_modules
from ..native_encoder import NativeEncoder
from .modeling import BaseEncoderModel, _native_from_dir
from .st_format import (read_sentence_transformers_dir, similarity_fn, write_sentence_transformers_modules,
                        write_similarity_fn_name)

_RESOLVE = object()   # encode_packed(head=...): look the head up from the wrapper's pooler


def _tokenizer_signature(tokenizer):
    """What a NativeWordPiece was built from, as far as a caller can change it on a live tokenizer: its size, its added tokens
    (id, content, ``normalized``), its truncation side, and the TSIM_NATIVE_TOKENIZER switch.  A few microseconds: the added
    tokens are a handful of entries, the vocabulary itself is not read."""
    try:
        size = len(tokenizer)
    except Exception:
        size = None
    try:
        added = tuple((int(i), str(getattr(t, "content", t)), bool(getattr(t, "normalized", False)))
                      for i, t in tokenizer.added_tokens_decoder.items())
    except Exception:
        added = None
    return (size, added, getattr(tokenizer, "truncation_side", "right"), os.environ.get("TSIM_NATIVE_TOKENIZER", "1") != "0")


def _native_wordpiece(tokenizer):
    """The tokenizer's NativeWordPiece, or None when its pipeline is not BERT's, the library is not built, or
    TSIM_NATIVE_TOKENIZER=0.  Kept on the tokenizer object together with the signature it was built from
    (``_tokenizer_signature``) and rebuilt when that changes: after ``add_tokens`` / ``add_special_tokens`` the new contents
    must send their sentences to the library, and after ``truncation_side = "left"`` the native path steps aside."""
    sig = _tokenizer_signature(tokenizer)
    wp = getattr(tokenizer, "_tsim_native_wordpiece", None)
    if wp is None or getattr(tokenizer, "_tsim_native_signature", None) != sig:
        wp = False
        if sig[-1]:
            from ..wordpiece import NativeWordPiece
            wp = NativeWordPiece.from_tokenizer(tokenizer) or False
        try:
            tokenizer._tsim_native_wordpiece = wp
            tokenizer._tsim_native_signature = sig
        except Exception:
            pass
    return wp or None


def _tokenize_packed(tokenizer, docs: List[str], max_len: int, batch_size: int):
    """Tokenise without padding -> (flat ids int32, lengths): the native WordPiece path for the sentences it handles (pure
    ASCII, no added-token content in the raw or the normalised text; csrc/wordpiece.cpp — same ids,
    tests/test_wordpiece_cpu.py), the library for the rest."""
    wp = _native_wordpiece(tokenizer)
    if wp is not None:
        return wp.tokenize_packed(docs, int(max_len), lambda rest: _tokenize_library(tokenizer, rest, max_len, batch_size))
    return _tokenize_library(tokenizer, docs, max_len, batch_size)


def _tokenize_library(tokenizer, docs: List[str], max_len: int, batch_size: int):
    """Tokenise without padding -> (flat ids int32, lengths).  Same tokenizer kwargs as
    sentence_encoder.py:144-153 except padding: the packed layout has no pad tokens, which is equivalent
    because padded positions are masked out of attention and pooling.

    Fast (Rust-backed) tokenizers are driven through their backend ``encode_batch`` on the whole chunk: the same code the
    ``tokenizer(text=...)`` call ends in — identical ids, and the backend's truncation and padding settings put back
    (tests/test_wordpiece_cpu.py::test_tokenize_library_equals_the_tokenizer_call) — without the per-call Python wrapping
    (BatchEncoding construction, per-batch option handling), which is single-threaded and was about half of the tokenizer
    time; the backend itself spreads a batch over the host cores (rayon), so one call per chunk uses all of them."""
    bt = getattr(tokenizer, "backend_tokenizer", None) if getattr(tokenizer, "is_fast", False) else None
    if bt is not None and hasattr(bt, "encode_batch"):
        prev_trunc, prev_pad = bt.truncation, bt.padding
        try:
            bt.enable_truncation(max_length=int(max_len), stride=0, strategy="longest_first",
                                 direction=getattr(tokenizer, "truncation_side", "right"))
            bt.no_padding()
            encs = bt.encode_batch(docs, add_special_tokens=True)
        finally:
            if prev_trunc is None:
                bt.no_truncation()
            else:
                bt.enable_truncation(**prev_trunc)
            if prev_pad is not None:
                bt.enable_padding(**prev_pad)
        lens = np.fromiter((len(e) for e in encs), dtype=np.int64, count=len(encs))
        flat = np.empty(int(lens.sum()), dtype=np.int32)
        o = 0
        for e, n in zip(encs, lens):
            flat[o:o + n] = e.ids
            o += n
        return flat, lens
    flat, lens = [], []
    for s in range(0, len(docs), batch_size):
        enc = tokenizer(text=docs[s:s + batch_size], add_special_tokens=True, padding=False, truncation=True,
                        max_length=max_len, return_attention_mask=False, return_token_type_ids=False)
        for ids in enc["input_ids"]:
            flat.extend(ids)
            lens.append(len(ids))
    return np.asarray(flat, dtype=np.int32), np.asarray(lens, dtype=np.int64)


def _capacity_slices(enc: NativeEncoder, cu_h: np.ndarray):
    """(s, e) ranges of the sequences of one packed chunk such that each range fits one forward of ``enc`` (max_seqs sequences,
    max_tokens tokens); ``cu_h``: the chunk's offsets on the host."""
    B = len(cu_h) - 1
    s = 0
    while s < B:
        e = s + 1
        while e < B and e - s < enc.max_seqs and cu_h[e + 1] - cu_h[s] <= enc.max_tokens:
            e += 1
        if cu_h[e] - cu_h[s] > enc.max_tokens:
            raise ValueError("a single sequence exceeds the encoder token capacity")
        yield s, e
        s = e


class _EncodeMixin:
    """encode / encode_text shared by both wrappers."""

    def encode(self, documents, output_np: bool = False):
        # evaluators call model.encode(EmbeddingsFeatures) (src/evaluation/evaluators.py:75): dispatch on type
        if isinstance(documents, EmbeddingsFeatures):
            return self._encode_features(documents)
        return self.encode_text(documents, output_np)

    def _encode_features(self, features: EmbeddingsFeatures) -> torch.Tensor:
        d = features.to_dict()
        hidden = self.context_embedder(input_ids=d["input_ids"], attention_mask=d["attention_mask"])[0]
        pooler = getattr(self, "pooler", None) or AvgPoolingStrategy(self.params)
        return self.projection(pooler(hidden, features))

    def _native_head(self, device):
        """The SentenceHead of the wrapper's pooler for the native forward: None (the mean pool) for AvgPoolingStrategy or no
        pooler; a pooler of another class without a native form keeps the mean pool and raises a UserWarning naming it."""
        pooler = getattr(self, "pooler", None)
        if pooler is None or isinstance(pooler, AvgPoolingStrategy):
            return None
        if callable(getattr(pooler, "native_head", None)):
            return pooler.native_head(device)
        warnings.warn(f"pooler {type(pooler).__name__} has no native form: the native forward returns mean-pooled embeddings "
                      "(use AvgPoolingStrategy, CLSPoolingStrategy, BertPoolingStrategy or SentenceEmbeddingHead)", UserWarning,
                      stacklevel=3)
        return None

    def encode_packed(self, flat_ids: torch.Tensor, cu: torch.Tensor, unit: bool = False, cu_host: np.ndarray = None,
                      head=_RESOLVE):
        """Device-resident pre-tokenised input (the benchmark path): the embeddings f32 [B, width] (+ their unit float16
        rows), pooled by the wrapper's pooler when it has a native form (``head``: a NativeEncoder SentenceHead or None to
        override it).  ``cu_host``: the same offsets on the host, when the caller has them (saves a device->host copy and its
        sync)."""
        enc: NativeEncoder = self.context_embedder
        if head is _RESOLVE:
            head = self._native_head(cu.device)
        outs, units = [], []
        cu_h = (cu.cpu().numpy() if cu_host is None else np.asarray(cu_host)).astype(np.int64)
        for s, e in _capacity_slices(enc, cu_h):
            r = enc.forward_packed(flat_ids[cu_h[s]:cu_h[e]], cu[s:e + 1] - cu[s], pooled=True, unit=unit,
                                   max_len=int(np.diff(cu_h[s:e + 1]).max()), head=head)
            outs.append(r["pooled"])
            if unit:
                units.append(r["unit"])
        width = head.width(enc.cfg.hidden) if head is not None else enc.cfg.hidden
        pooled = torch.cat(outs) if outs else torch.empty((0, width), device=cu.device)
        return (pooled, torch.cat(units)) if unit else pooled

    def _sorted_chunks(self, documents: List[str], order: np.ndarray, t_tok: list):
        """The batching of encode_text (sentence_encoder.py:136-173), shared by every text entry point: the documents in
        ``order`` (ascending character length), cut into chunks, each tokenised without padding.  Yields (lo, flat ids int32,
        lengths int64) per chunk; chunk i+1 is tokenised on a host thread while the caller works on chunk i.  ``t_tok[0]``
        accumulates the tokenizer time."""
        import time
        from concurrent.futures import ThreadPoolExecutor
        n = len(documents)
        docs = [documents[i] for i in order]
        tok_batch = max(int(self.params.batch_size), 1) * 64
        chunk = max(tok_batch, int(getattr(self.params, "encode_chunk_sentences", 8192)))

        def tokenize(lo):
            t0 = time.perf_counter()
            r = _tokenize_packed(self.params.tokenizer, docs[lo:lo + chunk], self.params.sequence_max_len, tok_batch)
            t_tok[0] += time.perf_counter() - t0
            return r

        with ThreadPoolExecutor(max_workers=1) as pool:
            fut = pool.submit(tokenize, 0)
            for lo in range(0, n, chunk):
                flat, lens = fut.result()
                if lo + chunk < n:
                    fut = pool.submit(tokenize, lo + chunk)
                yield lo, flat, lens

    def _token_embeddings(self, documents: List[str], output_np: bool):
        """encode_text(output_value="token_embeddings"): the final hidden states of each sentence, [len_i, H] float32."""
        enc: NativeEncoder = self.context_embedder
        dev = enc.device
        if len(documents) == 0:
            return []
        order = np.argsort([len(s) for s in documents], kind="stable")
        out = [None] * len(documents)
        with torch.no_grad():
            for lo, flat, lens in self._sorted_chunks(documents, order, [0.0]):
                cu = np.zeros(len(lens) + 1, dtype=np.int64)
                np.cumsum(lens, out=cu[1:])
                flat_d = torch.from_numpy(flat).to(dev, non_blocking=True)
                cu_d = torch.from_numpy(cu.astype(np.int32)).to(dev, non_blocking=True)
                for s, e in _capacity_slices(enc, cu):
                    h = enc.forward_packed(flat_d[cu[s]:cu[e]], cu_d[s:e + 1] - cu_d[s], pooled=False, hidden=True,
                                           max_len=int(lens[s:e].max()))["hidden"].float()
                    for j, piece in enumerate(torch.split(h, [int(v) for v in lens[s:e]])):   # one slice per sentence
                        out[order[lo + s + j]] = piece
        enc.check()
        return [t.cpu().numpy() for t in out] if output_np else out

    def encode_text(self, documents: List[str], output_np: bool = False,
                    output_value: str = "sentence_embedding", precision: str = "float32",
                    ranges=None) -> Union[torch.Tensor, np.ndarray, list]:
        """sentence_encoder.py:136-173: sort by character length, encode in batches, un-sort, stack.
        Returns float32 [N, H] on params.device (or numpy when ``output_np``), un-normalised.
        ``output_value="token_embeddings"`` (the sentence-transformers name) returns instead a list of [len_i, H] float32
        tensors in input order: the final hidden states of each sentence's tokens, special tokens included, no padding.
        The host tokenizer is the end-to-end bottleneck of this path, so it runs one chunk AHEAD on a
        host thread: chunk i+1 is tokenised while the GPU encodes chunk i (kernel launches are asynchronous; fast
        tokenizers release the GIL).  ``self.last_encode_stats`` holds the split of the wall time.
        ``precision="ubinary"`` (sentence-transformers' keyword and layout) returns instead uint8 [N, ceil(H / 8)]:
        ``np.packbits(embeddings > 0, axis=1)`` of the same pooled rows, packed on the device (``ops.pack_sign_rows``) — what
        ``GpuBinaryIndex.add_items`` and ``ops.codes_from_packbits`` take.  Any width up to 1024.
        ``precision="int8"`` with ``ranges=R`` (float [2, H]: per-column minimum and maximum, ``ops.int8_ranges`` of a
        calibration set) returns int8 [N, H]: sentence-transformers' ``quantize_embeddings(embeddings, "int8", ranges=R)`` of the
        same pooled rows, quantised on the device (``ops.quantize_int8_rows``) — what ``GpuInt8Index.add_items`` and
        ``ops.int8_codes_from_numpy`` take.  Without ``ranges`` it raises: calibrating on the call's own rows would give every
        call its own code."""
        import time
        if output_value not in ("sentence_embedding", "token_embeddings"):
            raise ValueError(f"output_value must be 'sentence_embedding' or 'token_embeddings', got {output_value!r}")
        if precision not in ("float32", "ubinary", "int8"):
            raise ValueError(f"precision must be 'float32', 'ubinary' or 'int8', got {precision!r}")
        if ranges is not None and precision != "int8":
            raise ValueError("ranges= belongs to precision='int8'")
        if precision == "int8":
            if output_value != "sentence_embedding":
                raise ValueError("precision='int8' quantises sentence embeddings, not token embeddings")
            if ranges is None:
                raise ValueError("precision='int8' needs calibration ranges: pass ranges=R, float [2, H] with the per-column "
                                 "minimum and maximum of a calibration set (ops.int8_ranges)")
            from .. import ops
            rows = self.encode_text(documents, output_np=False)
            codes = ops.quantize_int8_rows(rows, ranges)[:, :rows.shape[1]].contiguous()
            return codes.cpu().numpy() if output_np else codes
        if precision == "ubinary":
            if output_value != "sentence_embedding":
                raise ValueError("precision='ubinary' quantises sentence embeddings, not token embeddings")
            from .. import ops
            rows = self.encode_text(documents, output_np=False)
            codes = ops.pack_sign_rows(rows)[:, :(rows.shape[1] + 7) // 8].contiguous()
            return codes.cpu().numpy() if output_np else codes
        enc: NativeEncoder = self.context_embedder
        dev = enc.device
        n = len(documents)
        if output_value == "token_embeddings":
            return self._token_embeddings(documents, output_np)
        head = self._native_head(dev)
        if n == 0:
            out = torch.empty((0, head.width(enc.cfg.hidden) if head is not None else enc.cfg.hidden), dtype=torch.float32,
                              device=dev)
            return out.cpu().numpy() if output_np else out
        t_start = time.perf_counter()
        order = np.argsort([len(s) for s in documents], kind="stable")
        t_tok = [0.0]
        parts = []
        with torch.no_grad():
            for _, flat, lens in self._sorted_chunks(documents, order, t_tok):
                cu = np.zeros(len(lens) + 1, dtype=np.int64)
                np.cumsum(lens, out=cu[1:])
                flat_d = torch.from_numpy(flat).to(dev, non_blocking=True)
                cu_d = torch.from_numpy(cu.astype(np.int32)).to(dev, non_blocking=True)
                parts.append(self.projection(self.encode_packed(flat_d, cu_d, cu_host=cu, head=head)))
        pooled = torch.cat(parts) if len(parts) > 1 else parts[0]
        out = torch.empty_like(pooled)
        out[torch.from_numpy(order).to(dev)] = pooled      # un-sort (sentence_encoder.py:168)
        enc.check()      # out-of-range ids / positions: HF would have raised IndexError (synchronises, as the return would)
        self.last_encode_stats = {"sentences": n, "wall_s": time.perf_counter() - t_start, "tokenizer_s": t_tok[0]}
        return out.cpu().numpy() if output_np else out

    def get_sentence_embedding_dimension(self):
        hidden = self.context_embedder.config.hidden_size
        pooler = getattr(self, "pooler", None)
        if pooler is not None and callable(getattr(pooler, "output_width", None)):
            return pooler.output_width(hidden)
        return hidden


class OnnxSentenceTransformerWrapper(_EncodeMixin, BaseEncoderModel):
    """Inference wrapper with fixed average pooling (sentence_encoder.py:17-39)."""

    def __init__(self, *args, projection: nn.Module = None, **kwargs):
        super().__init__(*args, **kwargs)
        self.projection = projection if projection is not None else nn.Identity()

    def forward(self, input_ids, attention_mask, **kwargs):
        token_embeddings = self.context_embedder(input_ids=input_ids, attention_mask=attention_mask, **kwargs)[0]
        token_embeddings = self.projection(token_embeddings)
        from .. import ops
        return ops.mean_pool(token_embeddings, attention_mask)

    @classmethod
    def from_pretrained(cls, path, projection: nn.Module = None, params=None):
        assert params is not None, "Parameters not found, need to pass model parameters for the model to work"
        return cls(params=params, context_embedder=_native_from_dir(path, params), projection=projection)


class SentenceTransformerWrapper(_EncodeMixin, BaseEncoderModel):
    """sentence_encoder.py:71-217.  ``merge_strategy`` and ``loss`` are training-time modules: accepted and kept,
    unused on the embed-and-search path."""

    def __init__(self, pooler: PoolingStrategy = None, merge_strategy=None, loss=None, *args,
                 parallel_mode: bool = True, projection: nn.Module = None, similarity_fn_name: Optional[str] = None, **kwargs):
        super().__init__(*args, **kwargs)
        # the score function the checkpoint was trained for ('cosine' | 'dot'; None: not declared): the search pipelines'
        # default score_function
        self.similarity_fn_name = None if similarity_fn_name is None else similarity_fn(similarity_fn_name)
        self.pooler = pooler if pooler is not None else AvgPoolingStrategy(self.params)
        self.merge_strategy = merge_strategy
        self.loss = loss
        self.parallel_mode = parallel_mode
        self.projection = projection if projection is not None else nn.Identity()

    def forward(self, features, return_output=False, head_mask=None):
        if head_mask is not None:
            raise NotImplementedError("head_mask is a pruning-time feature outside the embed-and-search path")
        if self.parallel_mode:
            e1 = self._encode_features(features.sentence_1_features)
            e2 = self._encode_features(features.sentence_2_features)
            merged = torch.cat((e1, e2, torch.abs(e1 - e2)), dim=-1)
        else:
            merged = self._encode_features(features)
        if self.loss is None:
            return merged
        return self.loss(merged, features)

    @classmethod
    def from_pretrained(cls, path, pooler=None, merge_strategy=None, loss=None, params=None, parallel_mode=True):
        assert params is not None, "Parameters not found, need to pass model parameters for the model to work"
        return cls(pooler=pooler, merge_strategy=merge_strategy, loss=loss, params=params,
                   context_embedder=_native_from_dir(path, params), parallel_mode=parallel_mode)

    @classmethod
    def from_sentence_transformers(cls, path, params=None, merge_strategy=None, loss=None, parallel_mode=True):
        """A local sentence-transformers directory: modules.json naming the Transformer (at "" or "0_Transformer", read by
        NativeEncoder.from_pretrained), its Pooling, at most one Dense and an optional trailing Normalize, which become a
        :class:`SentenceEmbeddingHead` pooler run by the native forward.  Anything else is refused with a ValueError that
        names the file and field (models/st_format.py).  The truncation length stays ``params.sequence_max_len``."""
        assert params is not None, "Parameters not found, need to pass model parameters for the model to work"
        spec = read_sentence_transformers_dir(path)
        enc = _native_from_dir(os.path.join(path, spec.transformer_path) if spec.transformer_path else path, params)
        return cls(pooler=SentenceEmbeddingHead.from_spec(spec, params), merge_strategy=merge_strategy, loss=loss,
                   params=params, context_embedder=enc, parallel_mode=parallel_mode, similarity_fn_name=spec.similarity_fn_name)

    def save_pretrained(self, path):
        """BaseEncoderModel.save_pretrained, plus, for a pooler other than the default mean pool, the sentence-transformers
        module files (modules.json, 1_Pooling/, 2_Dense/, N_Normalize/) that from_sentence_transformers reads back."""
        super().save_pretrained(path)
        if callable(getattr(self.pooler, "native_head", None)):
            pooling, dense, normalize = st_modules(self.pooler)
            write_sentence_transformers_modules(path, self.context_embedder.config.hidden_size, pooling, dense, normalize)
        if self.similarity_fn_name is not None:
            write_similarity_fn_name(path, self.similarity_fn_name)

    @classmethod
    def from_preset(cls, preset: str, params, **kw):
        """Architecture preset with synthetic weights (offline stand-in for a hub checkpoint name)."""
        enc = NativeEncoder.from_preset(preset, max_tokens=params.max_tokens_per_batch,
                                        max_seqs=params.max_seqs_per_batch,
                                        device=params.device if torch.device(params.device).type == "cuda" else None)
        return cls(params=params, context_embedder=enc, **kw)
