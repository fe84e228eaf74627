"""Word-in-context embeddings with the reference's meaning (/root/reference/src/models/word_encoder.py):
``WordEncoderModel.encode`` (:46-50, the encoder followed by ``WordPoolingStrategy``,
/root/reference/src/modules/modules.py:68-74) and ``GWSCModel`` (:85-92, ``torch.mean(embedded_1[i][w1_c1], dim=0)`` for a
target word in two contexts), running on the native MI355X encoder: the hidden states never leave the device, one kernel
behind the last layer averages the listed token positions of every target word (``tsim_encoder_forward_spans``).

Differences from the reference, on purpose: a target word that is not found (or tokenises to nothing) gives a zero row where
``torch.mean`` of an empty selection gives NaN (and the reference's alignment raises before it gets there, see
``word_spans``); a position outside its sentence raises IndexError at the end of the call, as indexing would have.
Sense-embedding lookup (``WordSensePoolingStrategy``), training losses and merge strategies are not part of this path."""
from __future__ import annotations

import time
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .. import word_spans
from ..native_encoder import NativeEncoder
from .sentence_encoder import SentenceTransformerWrapper, _capacity_slices


class WordEncoder(SentenceTransformerWrapper):
    """A :class:`SentenceTransformerWrapper` (same constructors: ``from_preset``, ``from_pretrained``,
    ``from_sentence_transformers``; ``encode_text`` unchanged) that also embeds words in their context."""

    def encode_words(self, sentences: List[str], words: Optional[Sequence[Sequence[str]]] = None,
                     positions: Optional[Sequence[Sequence[Sequence[int]]]] = None, output_np: bool = False,
                     return_sentence_embeddings: bool = False):
        """``words[i]``: the target words of ``sentences[i]``, aligned to token positions as the reference's
        ``build_indexes_mono`` does (``word_spans.align_words``: each word is searched behind the previous one's match).
        Alternatively ``positions[i]``: one list of token positions per target word (``WordFeatures.indexes``: positions in
        the tokenised sentence, [CLS] = 0), taken as they are.
        Returns ``(embeddings [S, H] float32, span_sentence [S] int64)``: one row per target word in input order (sentence by
        sentence, words in the order given) and the sentence each row belongs to; with ``return_sentence_embeddings`` a
        third element, the mean-pooled sentence embeddings [N, H] of ``encode_text``'s default forward, from the same call.
        Sentences are batched, length-sorted and chunked exactly as in ``encode_text`` (its ``_sorted_chunks``)."""
        if (words is None) == (positions is None):
            raise ValueError("encode_words takes either words or positions")
        given = words if words is not None else positions
        n = len(sentences)
        if len(given) != n:
            raise ValueError(f"{len(given)} word lists for {n} sentences")
        enc: NativeEncoder = self.context_embedder
        dev = enc.device
        H = enc.cfg.hidden
        counts = np.fromiter((len(g) for g in given), dtype=np.int64, count=n)
        offs = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(counts, out=offs[1:])
        S = int(offs[-1])
        emb = torch.zeros((S, H), dtype=torch.float32, device=dev)
        sent = torch.empty((n, H), dtype=torch.float32, device=dev) if return_sentence_embeddings else None
        span_sentence = torch.from_numpy(np.repeat(np.arange(n, dtype=np.int64), counts)).to(dev)
        t_start, t_tok, t_align = time.perf_counter(), [0.0], 0.0
        if n:
            tok = self.params.tokenizer
            layout = word_spans.special_layout(tok) if words is not None else None
            max_length = int(self.params.sequence_max_len)
            cache = {}
            order = np.argsort([len(s) for s in sentences], kind="stable")
            with torch.no_grad():
                for lo, flat, lens in self._sorted_chunks(sentences, order, t_tok):
                    cu = np.zeros(len(lens) + 1, dtype=np.int64)
                    np.cumsum(lens, out=cu[1:])
                    flat_d = torch.from_numpy(flat).to(dev, non_blocking=True)
                    cu_d = torch.from_numpy(cu.astype(np.int32)).to(dev, non_blocking=True)
                    for s, e in _capacity_slices(enc, cu):
                        rows = order[lo + s:lo + e]            # input index of each sequence of this forward
                        t0 = time.perf_counter()
                        if words is not None:
                            spans = [word_spans.spans_for_sentence(tok, flat[cu[j]:cu[j + 1]], words[i], max_length, layout, cache)
                                     if counts[i] else [] for j, i in zip(range(s, e), rows)]
                        else:
                            spans = [word_spans.explicit_positions(positions[i]) for i in rows]
                        sseq, scu, stok = word_spans.span_table(spans)
                        t_align += time.perf_counter() - t0
                        r = enc.forward_spans(flat_d[cu[s]:cu[e]], cu_d[s:e + 1] - cu_d[s],
                                              *(torch.from_numpy(a).to(dev, non_blocking=True) for a in (sseq, scu, stok)),
                                              pooled=return_sentence_embeddings, max_len=int(lens[s:e].max()))
                        if len(sseq):
                            dest = np.concatenate([offs[i] + np.arange(counts[i]) for i in rows])
                            emb[torch.from_numpy(dest).to(dev)] = r["spans"]
                        if sent is not None:
                            sent[torch.from_numpy(rows.astype(np.int64)).to(dev)] = r["pooled"]
            enc.check()     # ids / positions / span entries out of range: indexing would have raised IndexError
        self.last_encode_stats = {"sentences": n, "spans": S, "wall_s": time.perf_counter() - t_start,
                                  "tokenizer_s": t_tok[0], "align_s": t_align}
        out = (emb, span_sentence) + ((sent,) if sent is not None else ())
        return tuple(t.cpu().numpy() for t in out) if output_np else out

    def encode_word_pairs(self, sentences_1: List[str], sentences_2: List[str], words_1: Sequence[str],
                          words_2: Sequence[str], output_np: bool = False
                          ) -> Tuple[Union[torch.Tensor, np.ndarray], Union[torch.Tensor, np.ndarray]]:
        """A WiC / GWSC batch: row i of the two [n, H] results is ``words_1[i]`` in ``sentences_1[i]`` and ``words_2[i]`` in
        ``sentences_2[i]`` (both contexts go through one ``encode_words`` call)."""
        n = len(sentences_1)
        if not (len(sentences_2) == len(words_1) == len(words_2) == n):
            raise ValueError("encode_word_pairs needs as many sentences as words on both sides")
        emb, _ = self.encode_words(list(sentences_1) + list(sentences_2), [[w] for w in list(words_1) + list(words_2)],
                                   output_np=output_np)
        return emb[:n], emb[n:]
