"""Host tokenizer of encode_text, native for ASCII sentences (csrc/wordpiece.cpp, include/tsim.h "tokenizer").

The reference calls the HuggingFace tokenizer it is configured with (sentence_encoder.py:144-153).  ``NativeWordPiece`` is
built FROM that tokenizer — vocabulary, special ids, lower-casing and truncation side are read out of its `tokenizers`
backend — and produces the same ids for the sentences it handles (pure ASCII, no added-token content in the raw or in the
normalised text); every other sentence goes through the library itself, so the result is the library's for any input.  It is a
snapshot: tokens added to the tokenizer afterwards are unknown to it (``_native_wordpiece`` in models/sentence_encoder.py
rebuilds it when the tokenizer's signature changes).  A tokenizer whose backend is not
the BERT pipeline (BertNormalizer / BertPreTokenizer / WordPiece / CLS..SEP template) is not supported: ``from_tokenizer``
returns None and the caller keeps using the library for everything."""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import List, Optional, Tuple

import numpy as np

from . import _lib


def _blob(keys: List[str]) -> Tuple[bytes, np.ndarray]:
    enc = [k.encode("utf-8") for k in keys]
    off = np.zeros(len(enc) + 1, dtype=np.int64)
    np.cumsum([len(e) for e in enc], out=off[1:])
    return b"".join(enc), off


class NativeWordPiece:
    def __init__(self, handle, n_special: int, owner):
        self._h = handle
        self.n_special = n_special
        self._owner = owner          # the HF tokenizer this was built from (fallback for unhandled sentences)
        self.threads = int(os.environ.get("TSIM_TOKENIZER_THREADS", "0"))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().tsim_wordpiece_destroy(h)
            except Exception:
                pass

    # ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def create_args(tokenizer) -> Optional[dict]:
        """What ``tsim_wordpiece_create`` is called with for this tokenizer, as plain Python values (``from_tokenizer`` passes
        them on; tests/wordpiece_driver.cpp is fed the same); None when the tokenizer's pipeline is not the one
        csrc/wordpiece.cpp restates."""
        bt = getattr(tokenizer, "backend_tokenizer", None) if getattr(tokenizer, "is_fast", False) else None
        if bt is None:
            return None
        try:
            cfg = json.loads(bt.to_str())
        except Exception:
            return None
        norm, pre, model, post = cfg.get("normalizer"), cfg.get("pre_tokenizer"), cfg.get("model"), cfg.get("post_processor")
        if not (norm and norm.get("type") == "BertNormalizer" and norm.get("clean_text", True)):
            return None
        if not (pre and pre.get("type") == "BertPreTokenizer"):
            return None
        if not (model and model.get("type") == "WordPiece" and isinstance(model.get("vocab"), dict)):
            return None
        if getattr(tokenizer, "truncation_side", "right") != "right":
            return None
        vocab = model["vocab"]
        size = max(vocab.values()) + 1
        keys = [None] * size
        for k, i in vocab.items():
            keys[i] = k
        if any(k is None for k in keys):          # holes in the id range: keep the library
            return None
        unk = vocab.get(model.get("unk_token", "[UNK]"))
        if unk is None:
            return None
        prefix_ids, suffix_ids = [], []
        if post is None:
            pass
        elif post.get("type") == "TemplateProcessing":
            seen_seq = False
            for item in post.get("single", []):
                if "Sequence" in item:
                    if seen_seq:
                        return None
                    seen_seq = True
                elif "SpecialToken" in item:
                    ids = post["special_tokens"][item["SpecialToken"]["id"]]["ids"]
                    (suffix_ids if seen_seq else prefix_ids).extend(ids)
                else:
                    return None
            if not seen_seq:
                return None
        elif post.get("type") in ("BertProcessing", "RobertaProcessing"):
            prefix_ids, suffix_ids = [int(post["cls"][1])], [int(post["sep"][1])]
        else:
            return None
        # The library matches a normalized=False token on the raw text and a normalized=True one (the default of add_tokens)
        # on the normalised text, after normalising the token's content as well.  The native code gets every content as
        # written and, for the normalized=True ones, as the backend normaliser rewrites it, and searches each in both texts.
        added = []
        for a in cfg.get("added_tokens", []):
            added.append(a["content"])
            if a.get("normalized", False):
                try:
                    added.append(bt.normalizer.normalize_str(a["content"]))
                except Exception:
                    return None
        return {"vocab": keys, "continuing_prefix": model.get("continuing_subword_prefix", "##"), "unk_id": int(unk),
                "prefix_ids": [int(t) for t in prefix_ids], "suffix_ids": [int(t) for t in suffix_ids],
                "lowercase": bool(norm.get("lowercase", True)), "max_chars": int(model.get("max_input_chars_per_word", 100)),
                "added": list(dict.fromkeys(c for c in added if c))}

    @classmethod
    def from_tokenizer(cls, tokenizer) -> Optional["NativeWordPiece"]:
        """None when the tokenizer's pipeline is not the one csrc/wordpiece.cpp restates."""
        a = cls.create_args(tokenizer)
        if a is None:
            return None
        prefix_ids, suffix_ids = a["prefix_ids"], a["suffix_ids"]
        vtext, voff = _blob(a["vocab"])
        atext, aoff = _blob(a["added"])
        pre_a = np.asarray(prefix_ids, dtype=np.int32)
        suf_a = np.asarray(suffix_ids, dtype=np.int32)
        h = C.c_void_p()
        _lib.check(_lib.lib().tsim_wordpiece_create(
            vtext, voff.ctypes.data, len(a["vocab"]), a["continuing_prefix"].encode(), a["unk_id"],
            pre_a.ctypes.data if len(pre_a) else None, len(pre_a), suf_a.ctypes.data if len(suf_a) else None, len(suf_a),
            1 if a["lowercase"] else 0, a["max_chars"], atext, aoff.ctypes.data, len(a["added"]), C.byref(h)),
            "tsim_wordpiece_create")
        wp = cls(h, len(prefix_ids) + len(suffix_ids), tokenizer)
        wp.n_prefix, wp.n_suffix = len(prefix_ids), len(suffix_ids)     # where the special ids sit (word_spans.special_layout)
        return wp

    # ------------------------------------------------------------------------------------------------------------------
    def encode_ascii(self, docs: List[str], max_len: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """docs must all be ``str.isascii()``.  -> (ids of the handled sentences back to back, lens [n], handled [n] bool)."""
        n = len(docs)
        text = "".join(docs).encode("ascii")
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.fromiter(map(len, docs), dtype=np.int64, count=n), out=off[1:])
        cap = int(off[-1]) + n * max(self.n_special, 1)
        ids = np.empty(cap, dtype=np.int32)
        lens = np.empty(n, dtype=np.int32)
        handled = np.empty(n, dtype=np.uint8)
        _lib.check(_lib.lib().tsim_wordpiece_encode(self._h, text, off.ctypes.data, n, int(max_len), self.threads, ids.ctypes.data,
                                                   cap, lens.ctypes.data, handled.ctypes.data), "tsim_wordpiece_encode")
        return ids[:int(lens.sum(dtype=np.int64))], lens.astype(np.int64), handled.astype(bool)

    def tokenize_packed(self, docs: List[str], max_len: int, fallback) -> Tuple[np.ndarray, np.ndarray]:
        """(flat ids int32, lens int64) of ``docs`` in order.  ``fallback(list of str) -> (flat, lens)`` is the library path,
        called once with the sentences the native code does not handle (non-ASCII, added-token text)."""
        n = len(docs)
        asc = np.fromiter((s.isascii() for s in docs), dtype=bool, count=n)
        if asc.all():
            a_docs, a_idx = docs, None
        else:
            a_idx = np.flatnonzero(asc)
            a_docs = [docs[i] for i in a_idx]
        ids, lens_a, handled = self.encode_ascii(a_docs, max_len) if a_docs else (np.empty(0, np.int32), np.empty(0, np.int64),
                                                                                 np.empty(0, bool))
        if a_idx is None and handled.all():
            return ids, lens_a
        # splice: sentences of the native path and of the library path back into input order
        ok = np.zeros(n, dtype=bool)
        ok[(np.arange(n) if a_idx is None else a_idx)[handled]] = True
        rest = np.flatnonzero(~ok)
        r_flat, r_lens = fallback([docs[i] for i in rest])
        lens = np.empty(n, dtype=np.int64)
        lens[ok] = lens_a[handled]
        lens[rest] = np.asarray(r_lens, dtype=np.int64)
        cu = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(lens, out=cu[1:])
        flat = np.empty(int(cu[-1]), dtype=np.int32)

        def scatter(src, which):
            if len(which) == 0:
                return
            ln = lens[which]
            starts = np.repeat(cu[which] - (np.cumsum(ln) - ln), ln)     # destination start minus source start, per id
            flat[np.arange(int(ln.sum())) + starts] = src

        scatter(ids, np.flatnonzero(ok))
        scatter(np.asarray(r_flat, dtype=np.int32), rest)
        return flat, lens
