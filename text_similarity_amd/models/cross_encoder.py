"""``CrossEncoder`` — the re-ranking stage of the reference's retrieve-then-rerank workflow
(/root/reference/src/pipeline/ranking_pipeline.py:27-33 calls ``cross_encoder.predict([[query, text], ...])`` on a
``sentence_transformers.CrossEncoder``), on the native encoder: a BERT ``BertForSequenceClassification`` (encoder with
token types, pooler, classifier) whose forward runs on packed pairs through ``tsim_encoder_forward_ex``.

Kept from ``sentence_transformers.CrossEncoder`` (2.x): the constructor's leading arguments and ``predict``'s signature and
results — [N] scores for one label, [N, num_labels] otherwise, a scalar for a single ``[a, b]`` pair; the default
activation is Sigmoid for one label and Identity otherwise, or the one a checkpoint names under
``sbert_ce_default_activation_function``.  That package is not a dependency: this convention is our contract.

Pairs are tokenised as the library would tokenise them (``tokenizer(list_a, list_b, truncation=True, max_length=L)``:
``[CLS] a [SEP] b [SEP]``, token types 0 then 1, ``longest_first`` truncation) without tokenising Q x k pairs: every
unique string goes once, untruncated, through the single-sentence path (``_tokenize_packed``: native WordPiece for ASCII, the
library for the rest), and the pairs are assembled from those ids in numpy (``PairTokenizer``).  BERT only: MPNet has no token types.

The BERT graph also carries ``DistilBertForSequenceClassification`` (``pre_classifier``, ReLU, ``classifier``) and
``RobertaForSequenceClassification`` / ``XLMRobertaForSequenceClassification`` / ``CamembertForSequenceClassification``
(``classifier.dense``, tanh, ``classifier.out_proj``): the same two-layer head on the first token's row.  These models have no
row for token type 1, so no type ids are sent; a tokenizer whose pair template is not BERT's (BPE and SentencePiece
tokenizers: ``<s> a </s></s> b </s>``) encodes the pairs itself (``LibraryPairTokenizer``).
"""
from __future__ import annotations

import json
import os
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ..native_encoder import NativeEncoder
from ..presets import PRESETS, synthetic_head_weights, synthetic_weights
from .sentence_encoder import _tokenize_packed

_ACTIVATIONS = {"Sigmoid": torch.nn.Sigmoid, "Identity": torch.nn.Identity}
_HEAD = ("pooler.dense.weight", "pooler.dense.bias", "classifier.weight", "classifier.bias")
_ROBERTA_HEAD = ("classifier.dense.weight", "classifier.dense.bias", "classifier.out_proj.weight", "classifier.out_proj.bias")
_DISTIL_HEAD = ("pre_classifier.weight", "pre_classifier.bias", "classifier.weight", "classifier.bias")
# HF model_type -> (the architecture a checkpoint must name, its head tensors [first layer w, b, second layer w, b], activation)
_SEQ_CLS = {"bert": ("BertForSequenceClassification", _HEAD, "tanh"),
            "distilbert": ("DistilBertForSequenceClassification", _DISTIL_HEAD, "relu"),
            "roberta": ("RobertaForSequenceClassification", _ROBERTA_HEAD, "tanh"),
            "xlm-roberta": ("XLMRobertaForSequenceClassification", _ROBERTA_HEAD, "tanh"),
            "camembert": ("CamembertForSequenceClassification", _ROBERTA_HEAD, "tanh")}


def longest_first(la: np.ndarray, lb: np.ndarray, budget: int) -> Tuple[np.ndarray, np.ndarray]:
    """Tokens kept of each segment when ``la + lb`` exceeds ``budget`` (= max_length - 3): the `tokenizers` library's
    ``longest_first`` rule for a pair.  The shorter segment (the first on a tie) keeps min(its length, budget // 2), the
    other what is left of the budget; e.g. 10 + 10 tokens into 5 -> (2, 3), into 13 -> (6, 7).
    tests/test_cross_tokenize_cpu.py pins this against the library over a grid of lengths and budgets."""
    la, lb = np.asarray(la, np.int64), np.asarray(lb, np.int64)
    swap = la > lb
    short, long_ = np.where(swap, lb, la), np.where(swap, la, lb)
    ks = np.minimum(short, budget // 2)
    kl = np.minimum(long_, budget - ks)
    over = la + lb > budget
    return np.where(over, np.where(swap, kl, ks), la), np.where(over, np.where(swap, ks, kl), lb)


def _spans(starts: np.ndarray, counts: np.ndarray) -> np.ndarray:
    """Concatenation of arange(s, s + c) over (starts, counts)."""
    counts = np.asarray(counts, np.int64)
    n = int(counts.sum())
    if n == 0:
        return np.empty(0, np.int64)
    excl = np.cumsum(counts) - counts
    return np.repeat(np.asarray(starts, np.int64) - excl, counts) + np.arange(n, dtype=np.int64)


class PairTemplateError(ValueError):
    """The tokenizer's single-sentence or pair template is not BERT's (no [CLS] / [SEP], or another arrangement)."""


class PairTokenizer:
    """(query, text) pairs -> packed ids, token types and lengths, equal to the library's pair encoding.
    Built from a BERT tokenizer; raises ValueError when the tokenizer's single / pair templates are not BERT's
    (``[CLS] x [SEP]`` / ``[CLS] a [SEP] b [SEP]`` with types 0..0 1..1)."""

    NO_TRUNCATION = 1 << 30
    PROBE = ("the first segment of a probe pair", "and the second, somewhat longer, segment of the same probe pair")

    def __init__(self, tokenizer, max_length: int, batch_size: int = 2048, typed: bool = True):
        """``typed`` False: the model has no row for token type 1 (DistilBERT), so the library's type ids are not compared."""
        self.tokenizer = tokenizer
        self.max_length = int(max_length)
        self.batch_size = int(batch_size)
        if self.max_length < 4:
            raise ValueError(f"max_length={max_length}: a pair needs 3 special tokens and at least one text token")
        self.cls_id, self.sep_id = tokenizer.cls_token_id, tokenizer.sep_token_id
        if self.cls_id is None or self.sep_id is None:
            raise PairTemplateError("the tokenizer has no [CLS] / [SEP] tokens: not a BERT tokenizer")
        for L in (self.max_length, 9):   # once without truncation (for short probes), once through longest_first
            ref = tokenizer([self.PROBE[0]], [self.PROBE[1]], truncation=True, max_length=L)
            ids, types, lens = self(([self.PROBE[0], self.PROBE[1]],), max_length=L)
            if list(ids) != list(ref["input_ids"][0]) or (typed and list(types) != list(ref.get("token_type_ids", [[None]])[0])):
                raise PairTemplateError("the tokenizer's pair template is not BERT's [CLS] a [SEP] b [SEP] with token types 0 / 1 "
                                        f"(library: {ref['input_ids'][0]} types {ref.get('token_type_ids')}; assembled: "
                                        f"{list(ids)} types {list(types)})")

    def _segments(self, docs: List[str]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Each string once through the single-sentence path, specials stripped -> (flat ids, start, length).  Not
        truncated: which segment of a pair is the longer one decides where ``longest_first`` puts an odd token, and two
        strings cut to the same length would tie (the library, too, tokenises a whole string before it truncates)."""
        flat, lens = _tokenize_packed(self.tokenizer, docs, self.NO_TRUNCATION, self.batch_size)
        cu = np.zeros(len(docs) + 1, np.int64)
        np.cumsum(lens, out=cu[1:])
        if len(docs) and not ((flat[cu[:-1]] == self.cls_id).all() and (flat[cu[1:] - 1] == self.sep_id).all()
                              and (lens >= 2).all()):
            raise PairTemplateError("the tokenizer's single-sentence template is not BERT's [CLS] x [SEP]")
        return flat, cu[:-1] + 1, lens - 2

    def __call__(self, pairs: Sequence[Sequence[str]], max_length: Optional[int] = None
                 ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """-> (ids int32 [T], token types int32 [T], lengths int64 [N]) of the pairs, back to back in input order."""
        L = self.max_length if max_length is None else int(max_length)
        index: Dict[str, int] = {}
        ia = np.empty(len(pairs), np.int64)
        ib = np.empty(len(pairs), np.int64)
        for i, p in enumerate(pairs):
            if len(p) != 2:
                raise ValueError(f"pair {i} has {len(p)} texts; a cross-encoder scores [query, text] pairs")
            ia[i] = index.setdefault(p[0], len(index))
            ib[i] = index.setdefault(p[1], len(index))
        flat, start, n = self._segments(list(index))
        ka, kb = longest_first(n[ia], n[ib], L - 3)
        lens = ka + kb + 3
        cu = np.zeros(len(pairs) + 1, np.int64)
        np.cumsum(lens, out=cu[1:])
        s = cu[:-1]
        ids = np.empty(int(cu[-1]), np.int32)
        types = np.zeros(int(cu[-1]), np.int32)
        ids[s] = self.cls_id
        ids[s + 1 + ka] = self.sep_id
        ids[cu[1:] - 1] = self.sep_id
        ids[_spans(s + 1, ka)] = flat[_spans(start[ia], ka)]
        db = _spans(s + 2 + ka, kb)
        ids[db] = flat[_spans(start[ib], kb)]
        types[db] = 1
        types[cu[1:] - 1] = 1
        return ids, types, lens


class LibraryPairTokenizer:
    """Pairs through the library tokenizer's own pair template, for tokenizers that are not BERT's (BPE, SentencePiece):
    ``tokenizer(list_a, list_b, truncation=True, max_length=L)``.  Same result layout as :class:`PairTokenizer`; the token types
    are all 0 (the models served have one token-type row or none)."""

    def __init__(self, tokenizer, max_length: int, batch_size: int = 2048):
        self.tokenizer, self.max_length, self.batch_size = tokenizer, int(max_length), int(batch_size)

    def __call__(self, pairs: Sequence[Sequence[str]], max_length: Optional[int] = None
                 ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        L = self.max_length if max_length is None else int(max_length)
        flat: List[int] = []
        lens: List[int] = []
        for i, p in enumerate(pairs):
            if len(p) != 2:
                raise ValueError(f"pair {i} has {len(p)} texts; a cross-encoder scores [query, text] pairs")
        for s in range(0, len(pairs), self.batch_size):
            chunk = pairs[s:s + self.batch_size]
            enc = self.tokenizer([p[0] for p in chunk], [p[1] for p in chunk], truncation=True, max_length=L, padding=False,
                                 return_attention_mask=False, return_token_type_ids=False)
            for ids in enc["input_ids"]:
                flat.extend(ids)
                lens.append(len(ids))
        ids = np.asarray(flat, np.int32)
        return ids, np.zeros(len(ids), np.int32), np.asarray(lens, np.int64)


def _read_hf_config(path: str) -> dict:
    with open(os.path.join(path, "config.json")) as f:
        return json.load(f)


class CrossEncoder:
    def __init__(self, path_or_preset: str, num_labels: Optional[int] = None, max_length: Optional[int] = None,
                 device=None, default_activation_function=None, *, tokenizer=None, max_tokens: int = 65536,
                 max_seqs: int = 8192):
        """``path_or_preset``: a LOCAL HF directory of a ``BertForSequenceClassification`` or of its DistilBERT / RoBERTa /
        XLM-R / CamemBERT counterpart (config.json, model.safetensors
        or pytorch_model.bin, tokenizer files), or a preset name of ``presets.PRESETS`` (BERT graph) with ``tokenizer=``
        and synthetic weights (``synthetic_weights`` + ``synthetic_head_weights``; ``num_labels`` default 1).
        ``max_length`` defaults to the tokenizer's ``model_max_length`` and is capped at what the position table holds.
        ``max_tokens`` / ``max_seqs``: capacity of one encoder forward; ``predict`` splits larger inputs."""
        act_name = None
        if os.path.isdir(path_or_preset):
            from ..weights import load_hf_dir
            d = _read_hf_config(path_or_preset)
            if d.get("model_type", "bert") not in _SEQ_CLS:
                raise ValueError(f"model_type {d.get('model_type')!r}: the cross-encoder supports BERT only "
                                 "(MPNet has no token types and a different pair template)")
            want, head, head_act = _SEQ_CLS[d.get("model_type", "bert")]
            if want not in (d.get("architectures") or []):
                raise ValueError(f"architectures {d.get('architectures')}: a cross-encoder checkpoint is a "
                                 + ("BertForSequenceClassification" if want == _SEQ_CLS["bert"][0] else
                                    f"{want} (the BertForSequenceClassification of {d['model_type']})"))
            n_ckpt = len(d["id2label"]) if d.get("id2label") else int(d.get("num_labels", 2))
            if num_labels is not None and int(num_labels) != n_ckpt:
                raise ValueError(f"num_labels={num_labels}, the checkpoint has {n_ckpt}")
            num_labels = n_ckpt
            act_name = d.get("sbert_ce_default_activation_function")
            cfg, w = load_hf_dir(path_or_preset)
            missing = [k for k in head if k not in w]
            if missing:
                raise KeyError(f"{path_or_preset}: missing head weights {missing}")
            if tokenizer is None:
                from transformers import AutoTokenizer
                tokenizer = AutoTokenizer.from_pretrained(path_or_preset)
        elif path_or_preset in PRESETS:
            cfg = PRESETS[path_or_preset]
            if cfg.arch != "bert":
                raise ValueError(f"preset {path_or_preset!r} is {cfg.arch}: the cross-encoder supports BERT only")
            if tokenizer is None:
                raise ValueError("a preset needs tokenizer=: presets carry no vocabulary")
            num_labels = 1 if num_labels is None else int(num_labels)
            want, head, head_act = _SEQ_CLS[cfg.source_type]
            w = synthetic_weights(path_or_preset)
            w.update(zip(head, synthetic_head_weights(path_or_preset, num_labels).values()))   # (drawn under BERT's names)
        else:
            raise ValueError(f"{path_or_preset!r} is neither a local directory nor a preset ({', '.join(PRESETS)})")
        self.config = cfg
        self.num_labels = int(num_labels)
        self.tokenizer = tokenizer
        if max_length is None:
            max_length = int(getattr(tokenizer, "model_max_length", cfg.max_pos) or cfg.max_pos)
        self.max_length = min(int(max_length), cfg.max_pos - cfg.first_pos)   # (a 514-row RoBERTa table holds 512 tokens)
        if default_activation_function is not None:
            self.default_activation_function = default_activation_function
        elif act_name is not None:
            cls_name = str(act_name).rsplit(".", 1)[-1]
            if cls_name not in _ACTIVATIONS:
                raise ValueError(f"sbert_ce_default_activation_function {act_name!r}: only Sigmoid and Identity are supported")
            self.default_activation_function = _ACTIVATIONS[cls_name]()
        else:
            self.default_activation_function = torch.nn.Sigmoid() if self.num_labels == 1 else torch.nn.Identity()
        typed = cfg.source_type == "bert"   # the others have no row for token type 1: no type ids are sent
        try:
            self.pair_tokenizer = PairTokenizer(tokenizer, self.max_length, typed=typed)
        except PairTemplateError:
            if typed:
                raise
            self.pair_tokenizer = LibraryPairTokenizer(tokenizer, self.max_length)
        enc_dev = torch.device(device) if device is not None else None
        if enc_dev is not None and enc_dev.type != "cuda":
            enc_dev = None
        self.model = NativeEncoder(cfg, w, max_tokens=max_tokens, max_seqs=max_seqs, device=enc_dev)
        self.model.set_cls_head(*(w[k] for k in head), act=head_act)
        self.device = self.model.device
        self.last_predict_stats: dict = {}

    @classmethod
    def from_pretrained(cls, path: str, **kw) -> "CrossEncoder":
        return cls(path, **kw)

    # ------------------------------------------------------------------ packed forward
    def logits_packed(self, flat: torch.Tensor, types: torch.Tensor, cu: torch.Tensor, cu_host: np.ndarray) -> torch.Tensor:
        """Device-resident tokenised pairs -> float32 logits [N, num_labels], over as many encoder forwards as the
        encoder's capacity (max_tokens / max_seqs) requires.  ``cu_host``: the same offsets on the host."""
        enc = self.model
        cu_h = np.asarray(cu_host, np.int64)
        B = len(cu_h) - 1
        outs = []
        s = 0
        while s < B:
            e = s + 1
            while e < B and e - s < enc.max_seqs and cu_h[e + 1] - cu_h[s] <= enc.max_tokens:
                e += 1
            if cu_h[e] - cu_h[s] > enc.max_tokens:
                raise ValueError("a single pair exceeds the encoder token capacity")
            t0, t1 = int(cu_h[s]), int(cu_h[e])
            r = enc.forward_packed(flat[t0:t1], cu[s:e + 1] - cu[s], types=types[t0:t1] if enc.n_types else None, pooled=False, logits=True,
                                   max_len=int(np.diff(cu_h[s:e + 1]).max()))
            outs.append(r["logits"])
            s = e
        return torch.cat(outs) if len(outs) > 1 else (outs[0] if outs else
                                                        torch.empty((0, self.num_labels), device=self.device))

    def predict(self, sentences, batch_size: int = 32, show_progress_bar=None, activation_fct=None,
                apply_softmax: bool = False, convert_to_numpy: bool = True, convert_to_tensor: bool = False):
        """Scores of ``[[a, b], ...]`` pairs: [N] (one label) or [N, num_labels], in input order; a single ``[a, b]`` pair
        gives one score (a scalar for one label).  ``activation_fct`` overrides the default activation; ``apply_softmax``
        normalises multi-label scores.  ``batch_size`` and ``show_progress_bar`` are accepted for compatibility: pairs are
        packed (no padding) into forwards sized by the encoder's capacity, sorted by length so that each forward's
        attention grid fits its longest pair."""
        t_start = time.perf_counter()
        single = len(sentences) > 0 and isinstance(sentences[0], str)
        pairs = [sentences] if single else list(sentences)
        n = len(pairs)
        act = activation_fct if activation_fct is not None else self.default_activation_function
        dev = self.device
        t_tok = 0.0
        if n == 0:
            logits = torch.empty((0, self.num_labels), dtype=torch.float32, device=dev)
        else:
            t0 = time.perf_counter()
            flat, types, lens = self.pair_tokenizer(pairs)
            order = np.argsort(lens, kind="stable")
            cu_unsorted = np.zeros(n + 1, np.int64)
            np.cumsum(lens, out=cu_unsorted[1:])
            idx = _spans(cu_unsorted[:-1][order], lens[order])
            flat, types, lens = flat[idx], types[idx], lens[order]
            cu = np.zeros(n + 1, np.int64)
            np.cumsum(lens, out=cu[1:])
            t_tok = time.perf_counter() - t0
            with torch.no_grad():
                flat_d = torch.from_numpy(flat).to(dev, non_blocking=True)
                types_d = torch.from_numpy(types).to(dev, non_blocking=True)
                cu_d = torch.from_numpy(cu.astype(np.int32)).to(dev, non_blocking=True)
                sorted_logits = self.logits_packed(flat_d, types_d, cu_d, cu)
                logits = torch.empty_like(sorted_logits)
                logits[torch.from_numpy(order).to(dev)] = sorted_logits      # un-sort
        with torch.no_grad():
            scores = act(logits)
            if apply_softmax and scores.shape[1] > 1:
                scores = torch.softmax(scores, dim=1)
            if self.num_labels == 1:
                scores = scores[:, 0]
        self.model.check()   # out-of-range ids / types / positions: HF would have raised IndexError (synchronises)
        self.last_predict_stats = {"pairs": n, "wall_s": time.perf_counter() - t_start, "tokenizer_s": t_tok}
        if convert_to_tensor:
            return scores[0] if single else scores
        if convert_to_numpy:
            out = scores.cpu().numpy()
            return out[0] if single else out
        return scores[0] if single else list(scores)
