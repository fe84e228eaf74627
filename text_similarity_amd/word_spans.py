"""Word-to-token alignment for word-in-context embeddings (host code, no GPU).

The reference aligns a target word to WordPiece positions by tokenising the word alone and searching that id sub-list in the
sentence's ids from a running position (/root/reference/src/dataset/dataset.py:366-378 ``find_words_in_tokenized_sentence``,
:461-480 ``find_tokens_positions``, :450-458 ``build_indexes_mono``).  The functions here restate that behaviour over plain
id lists and assemble the span table ``tsim_encoder_forward_spans`` reads (include/tsim.h).  Positions count tokens of the
tokenised sentence from 0, special tokens included ([CLS] is position 0), as the reference's do.

Deviations from the reference, on purpose:

* a word that tokenises to nothing, or is not found from the running position on, yields an EMPTY span and leaves the
  running position where it was (the reference reads ``pos[1]`` before it checks ``pos`` and raises TypeError); an empty
  span pools to a zero row on the device;
* a word cut off by ``max_length`` truncation yields the positions that survive: when the whole word is not found and the
  sentence was truncated, the longest proper prefix of the word's ids that ends exactly where the sentence's content ends
  (in front of the suffix special tokens) is taken.  A sentence counts as truncated when it has ``max_length`` ids.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np


def special_layout(tokenizer) -> Tuple[int, int]:
    """(special ids in front of a single sentence, special ids behind it): (1, 1) for BERT's ``[CLS] ... [SEP]``.  Read from
    the object when it says so (``n_prefix`` / ``n_suffix``, as NativeWordPiece does), else from how it encodes a probe."""
    if hasattr(tokenizer, "n_prefix") and hasattr(tokenizer, "n_suffix"):
        return int(tokenizer.n_prefix), int(tokenizer.n_suffix)
    inner = list(tokenizer.encode("a", add_special_tokens=False))
    full = list(tokenizer.encode("a", add_special_tokens=True))
    at = find_sublist(full, inner, 0) if inner else -1
    if at < 0:
        n = len(full) - len(inner)
        return (1, n - 1) if n >= 1 else (0, 0)
    return at, len(full) - at - len(inner)


def word_ids(tokenizer, word: str) -> List[int]:
    """The ids of ``word`` tokenised alone, without special tokens (the reference's ``tokenizer.encode(w)[1:-1]``)."""
    if hasattr(tokenizer, "encode_ascii"):     # text_similarity_amd.wordpiece.NativeWordPiece
        if word.isascii():
            ids, lens, handled = tokenizer.encode_ascii([word], 1 << 20)
            if handled[0]:
                n_pre, n_suf = special_layout(tokenizer)
                return [int(t) for t in ids[n_pre:len(ids) - n_suf]]
        tokenizer = tokenizer._owner               # the library tokenizer it was built from
    return [int(t) for t in tokenizer.encode(word, add_special_tokens=False)]


def find_sublist(ids: Sequence[int], sub: Sequence[int], start: int = 0) -> int:
    """First index >= ``start`` at which ``sub`` occurs in ``ids`` as a contiguous run; -1 when it does not (or is empty)."""
    n, m = len(ids), len(sub)
    if m == 0:
        return -1
    first = sub[0]
    for i in range(max(int(start), 0), n - m + 1):
        if ids[i] == first and list(ids[i:i + m]) == list(sub):
            return i
    return -1


def align_words(sentence_ids: Sequence[int], words_ids: Sequence[Sequence[int]], n_prefix: int = 1, n_suffix: int = 1,
                truncated: bool = False) -> List[List[int]]:
    """Token positions of each word of ``words_ids`` (its ids tokenised alone) inside ``sentence_ids`` (the tokenised
    sentence, special tokens included), found in the order given: each search starts behind the previous match, so asking
    for a word twice gives its first and its second occurrence.  An absent or empty word gives ``[]``.  ``truncated``: the
    sentence was cut at max_length; a word whose tail was cut off gives the positions that are left (module docstring)."""
    ids = list(sentence_ids)
    end = len(ids) - int(n_suffix)          # one past the last content token
    current = 0
    out: List[List[int]] = []
    for w in words_ids:
        w = list(w)
        at = find_sublist(ids, w, current)
        if at >= 0:
            out.append(list(range(at, at + len(w))))
            current = at + len(w)
            continue
        span: List[int] = []
        if truncated and w:
            for keep in range(min(len(w) - 1, end - max(current, int(n_prefix))), 0, -1):   # longest surviving prefix first
                if ids[end - keep:end] == w[:keep]:
                    span = list(range(end - keep, end))
                    current = end
                    break
        out.append(span)
    return out


def spans_for_sentence(tokenizer, sentence_ids: Sequence[int], words: Sequence[str], max_length: Optional[int] = None,
                       layout: Optional[Tuple[int, int]] = None, cache: Optional[Dict[str, List[int]]] = None) -> List[List[int]]:
    """``align_words`` from strings: each word is tokenised alone (``cache``: word -> ids, shared across sentences)."""
    n_pre, n_suf = layout if layout is not None else special_layout(tokenizer)
    ids_of = []
    for w in words:
        if cache is not None and w in cache:
            ids_of.append(cache[w])
            continue
        t = word_ids(tokenizer, w)
        if cache is not None:
            cache[w] = t
        ids_of.append(t)
    return align_words(sentence_ids, ids_of, n_pre, n_suf, truncated=max_length is not None and len(sentence_ids) >= max_length)


def explicit_positions(positions) -> List[List[int]]:
    """Position lists given by the caller (``WordFeatures.indexes`` / ``tokens_indexes`` of one sentence: lists, arrays or
    tensors) as plain int lists, unchanged: no alignment, no range check (the device clamps and flags what is out of range)."""
    out = []
    for p in positions:
        if hasattr(p, "tolist"):
            p = p.tolist()
        if isinstance(p, (int, np.integer)):
            p = [p]
        out.append([int(t) for t in p])
    return out


def span_table(spans_per_sentence: Sequence[Sequence[Sequence[int]]]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """CSR span table of a batch: ``spans_per_sentence[b]`` is the list of position lists of sequence ``b``.  Returns int32
    arrays ``span_seq [S]`` (the sequence of each span), ``span_cu [S+1]`` (offsets into span_tok) and ``span_tok``
    (positions inside the sequence), spans in sentence order, then in the order given."""
    seq, lens, tok = [], [], []
    for b, spans in enumerate(spans_per_sentence):
        for sp in spans:
            seq.append(b)
            lens.append(len(sp))
            tok.extend(sp)
    span_cu = np.zeros(len(seq) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lens, dtype=np.int64), out=span_cu[1:])
    if span_cu[-1] > np.iinfo(np.int32).max:
        raise ValueError(f"{int(span_cu[-1])} span tokens do not fit the int32 span table")
    i32 = np.iinfo(np.int32)   # a position beyond int32 stays out of range (and is flagged) instead of wrapping into it
    return (np.asarray(seq, dtype=np.int32), span_cu.astype(np.int32),
            np.clip(np.asarray(tok, dtype=np.int64), i32.min, i32.max).astype(np.int32))
