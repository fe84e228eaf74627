"""Embed-and-search pipelines with the reference's class names and call signatures
(/root/reference/src/pipeline/search_pipeline.py:14-93).

``SentenceMiningPipeline`` is the brute-force searcher: in the reference a Python loop over queries doing
``expand_as`` + ``F.cosine_similarity`` + ``torch.topk`` per corpus chunk (:60-89).  Here each chunk is ONE call of
the fused MFMA cosine + top-k kernel and chunks are merged on the GPU.  Shipped bugs are not reproduced
(SURVEY.md §8 A5/A6): the chunk slice (:61) takes ``corpus[i : i + chunk]``, ``topk`` runs over the corpus axis,
``__call__`` passes the stored corpus, and k is clamped by the chunk size (``reference_k_clamp=True`` restores the
reference's clamp by ``len(queries)``, :78).  Ordering within a result list is (score desc, index asc); the
reference asks for ``sorted=False`` and leaves it undefined.

``score_function`` ("cosine" | "dot") picks what ``SentenceMiningPipeline`` and ``SemanticSearchPipeline`` rank by: cosine,
or the inner product of the float32 embeddings for models trained for dot-product scoring (exact as well,
:func:`ops.dot_topk`).  The default is the model's ``similarity_fn_name`` (read from a sentence-transformers checkpoint's
config_sentence_transformers.json) when it has one, else cosine.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Union

import torch

import os

from .. import ops
from ..index import GpuFlatIndex
from ..graph_index import GpuGraphIndex
from ..ivf_index import GpuIVFIndex
from ..pq_index import GpuPQIndex
from ..ivfpq_index import GpuIVFPQIndex


SCORE_FUNCTIONS = {"cosine": "cosine", "dot": "dot", "dot_product": "dot"}


def resolve_score_function(score_function, model) -> str:
    """'cosine' | 'dot' from the pipeline argument, else the model's similarity_fn_name, else 'cosine'."""
    if score_function is None:
        score_function = getattr(model, "similarity_fn_name", None) or "cosine"
    if score_function not in SCORE_FUNCTIONS:
        raise ValueError(f"score_function={score_function!r}: one of 'cosine', 'dot'")
    return SCORE_FUNCTIONS[score_function]


def _sort_columns(cols, order):
    """Rows of equally long device columns sorted lexicographically by a chain of stable sorts: ``order`` = (column, descending)
    pairs, LEAST significant key first."""
    for k, desc in order:
        o = torch.sort(cols[k], stable=True, descending=desc)[1]
        cols = [c[o] for c in cols]
    return cols


class Pipeline:
    def __init__(self, params, model, name: Optional[str] = None):
        self.params = params
        self.model = model
        self.name = name

    def encode_corpus(self, documents: Union[List[str], torch.Tensor], convert_to_numpy: bool = False,
                      return_embeddings: bool = False):
        if isinstance(documents, list):
            return self.model.encode_text(documents, output_np=convert_to_numpy)
        return documents


class SearchPipeline(Pipeline):
    def __init__(self, *args, corpus: Optional[Union[List[str], torch.Tensor]] = None, **kwargs):
        super().__init__(*args, **kwargs)
        self.corpus = corpus

    def _index(self, corpus):
        raise NotImplementedError()

    def _search(self, queries, max_num_results: int):
        raise NotImplementedError()

    def __call__(self, queries, max_num_results):
        return self._search(queries, max_num_results)


class SentenceMiningPipeline(SearchPipeline):
    def __init__(self, corpus_chunk_size: int, *args, reference_k_clamp: bool = False, verbose: bool = False,
                 score_function: Optional[str] = None, **kwargs):
        super().__init__(*args, **kwargs)
        self.score_function = resolve_score_function(score_function, self.model)
        self.corpus_chunk_size = int(corpus_chunk_size)
        self.reference_k_clamp = reference_k_clamp
        self.verbose = verbose
        self.last_scores = None      # [Q,k] float32 of the last search (the reference only prints indices)
        self.last_indices = None

    def search_tensors(self, query_embeddings: torch.Tensor, corpus=None, max_num_results: int = 10, candidates=None):
        """Device-level search: returns (scores [Q,k] f32, indices [Q,k] i64) over the whole corpus.  Scores are the
        reference's ``F.cosine_similarity`` of the float32 embeddings (search_pipeline.py:76-77) and the order is exact for
        them: half-precision unit rows feed the MFMA kernel for candidate selection only.  With ``score_function='dot'`` the
        scores are the inner products of the float32 embeddings (each chunk scaled by its own power of two for the MFMA
        pass; results do not depend on the chunking).  1 <= max_num_results <= 1024, width <= 768.
        ``candidates`` restricts every query to its own corpus positions — re-scoring a first stage's candidates: a list of Q
        position lists, a ``[Q, m]`` tensor (-1 = padding) or ONE 1-D list shared by all queries.  Same scores, same order
        (:func:`ops.cosine_list_topk` / :func:`ops.dot_list_topk`); positions index the WHOLE corpus, so it is embedded in one
        piece and ``corpus_chunk_size`` does not apply."""
        corpus = self.corpus if corpus is None else corpus
        n = len(corpus)
        d = query_embeddings.shape[1]
        qf = query_embeddings.to(self.params.device, dtype=torch.float32).contiguous()
        k = min(max_num_results, len(query_embeddings)) if self.reference_k_clamp else max_num_results
        k = max(1, min(k, n))
        if candidates is not None:
            cf = (self.model.encode_text(corpus) if isinstance(corpus, list) else corpus).to(self.params.device, dtype=torch.float32)
            cand, lims = self._candidate_lists(candidates, qf.shape[0])
            fn = ops.dot_list_topk if self.score_function == "dot" else ops.cosine_list_topk
            return fn(qf, cf.contiguous(), cand, lims, k=k)
        qn = ops.l2norm_rows(qf)
        scores, idxs = [], []
        for start in range(0, n, self.corpus_chunk_size):
            chunk = corpus[start:start + self.corpus_chunk_size]
            if isinstance(chunk, list):
                chunk = self.model.encode_text(chunk)
            cf = chunk.to(self.params.device, dtype=torch.float32).contiguous()
            if self.score_function == "dot":
                cn, rho, scale = ops.dot_scaled_rows(cf)
                s, i = ops.dot_topk(qn, cn, d, min(k, cn.shape[0]), eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale,
                                    idx_offset=start)
            else:
                cn, rho = ops.l2norm_rows(cf, return_rho=True)     # rho: the chunk's rounding-residual maximum (guard bound)
                s, i = ops.cosine_topk(qn, cn, d, min(k, cn.shape[0]), idx_offset=start, eq_f32=qf, ec_f32=cf, rho_c=rho)
            if s.shape[1] < k:   # short last chunk: pad so lists stack
                pad = k - s.shape[1]
                s = torch.cat([s, torch.full((s.shape[0], pad), float("-inf"), device=s.device)], 1)
                i = torch.cat([i, torch.full((i.shape[0], pad), -1, dtype=torch.int64, device=i.device)], 1)
            scores.append(s)
            idxs.append(i)
        if len(scores) == 1:
            return scores[0], idxs[0]
        return ops.topk_merge(scores, idxs, k)

    def _candidate_lists(self, candidates, Q: int):
        """(cand, lims) on the device for the three forms ``search_tensors`` takes."""
        dev = self.params.device
        if isinstance(candidates, torch.Tensor):
            return candidates.to(dev), None
        if len(candidates) and not isinstance(candidates[0], (int,)) and getattr(candidates[0], "__len__", None) is not None:
            if len(candidates) != Q:
                raise ValueError(f"candidates: {len(candidates)} lists for {Q} queries")
            parts = [torch.as_tensor(c, dtype=torch.int64).reshape(-1) for c in candidates]
            lims = torch.zeros((Q + 1,), dtype=torch.int64)
            lims[1:] = torch.cumsum(torch.tensor([p.numel() for p in parts], dtype=torch.int64), 0)
            return torch.cat(parts).to(dev), lims.to(dev)
        return torch.as_tensor(candidates, dtype=torch.int64).to(dev), None

    def range_tensors(self, query_embeddings: torch.Tensor, threshold, corpus=None):
        """Device-level range search: ``(lims int64 [Q+1], scores float32 [T], indices int64 [T])`` — EVERY corpus row whose
        score (``score_function``) against a query is >= ``threshold``; the hits of query q are ``[lims[q], lims[q+1])``, ordered
        by (score desc, index asc).  Exact and complete (:func:`ops.cosine_range` / :func:`ops.dot_range`).  The corpus goes
        through in chunks of ``corpus_chunk_size``; the per-chunk results, sorted already, are merged on the device
        (:func:`ops.range_merge`).  ``threshold``: a float, or an array / tensor [Q] with one threshold per query."""
        corpus = self.corpus if corpus is None else corpus
        n = len(corpus)
        d = query_embeddings.shape[1]
        dev = self.params.device
        qf = query_embeddings.to(dev, dtype=torch.float32).contiguous()
        qn = ops.l2norm_rows(qf)
        Q = qf.shape[0]
        tau_q = ops._threshold_array("range_tensors", threshold, Q, qf.device)    # converted once, not per chunk
        if tau_q is not None:
            threshold = tau_q
        parts = []
        for start in range(0, n, self.corpus_chunk_size):
            chunk = corpus[start:start + self.corpus_chunk_size]
            if isinstance(chunk, list):
                chunk = self.model.encode_text(chunk)
            cf = chunk.to(dev, dtype=torch.float32).contiguous()
            if self.score_function == "dot":
                cn, rho, scale = ops.dot_scaled_rows(cf)
                parts.append(ops.dot_range(qn, cn, d, threshold, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale, idx_offset=start))
            else:
                cn, rho = ops.l2norm_rows(cf, return_rho=True)
                parts.append(ops.cosine_range(qn, cn, d, threshold, eq_f32=qf, ec_f32=cf, rho_c=rho, idx_offset=start))
        if len(parts) == 1:
            return parts[0]
        if not parts:
            return (torch.zeros((Q + 1,), dtype=torch.int64, device=qf.device), torch.empty((0,), dtype=torch.float32, device=qf.device),
                    torch.empty((0,), dtype=torch.int64, device=qf.device))
        out = None
        for r0 in range(0, len(parts), ops.RANGE_MERGE_MAX_LISTS - 1):      # (more chunks than one merge takes: fold them in)
            group = ([out] if out is not None else []) + parts[r0:r0 + ops.RANGE_MERGE_MAX_LISTS - 1]
            out = ops.range_merge(group, total=sum(p[1].numel() for p in group))   # (the payloads of the ops are exactly lims[-1] long)
        return out

    def mine(self, queries, threshold) -> Dict[int, list]:
        """``{query_idx: [(corpus_idx, text, score), ...]}``: every corpus entry scoring >= ``threshold`` against the query, best
        first — sentence mining with a score floor.  ``queries``: texts or embeddings; the corpus is the pipeline's.
        ``threshold``: a float, or one floor per query (array / tensor [Q])."""
        query_embeddings = self.encode_corpus(documents=queries)
        lims, scores, idx = self.range_tensors(query_embeddings, threshold)
        lims, scores, idx = lims.cpu().tolist(), scores.cpu().tolist(), idx.cpu().tolist()
        return {q: [(idx[t], self.corpus[idx[t]], scores[t]) for t in range(lims[q], lims[q + 1])]
                for q in range(len(lims) - 1)}

    def mine_pairs(self, threshold: float) -> List[tuple]:
        """The corpus against itself: every unordered pair (i < j) scoring >= ``threshold``, each once, as ``[(score, i, j)]``
        sorted by (score desc, i, j) — near-duplicate detection / paraphrase mining.  The i < j filter runs on the device on
        the CSR arrays."""
        emb = self.encode_corpus(documents=self.corpus)
        lims, scores, idx = self.range_tensors(emb, threshold)
        Q = lims.numel() - 1
        qid = torch.repeat_interleave(torch.arange(Q, device=lims.device), lims[1:] - lims[:-1])
        keep = qid < idx
        qid, idx, scores = qid[keep], idx[keep], scores[keep]
        qid, idx, scores = _sort_columns([qid, idx, scores], ((1, False), (0, False), (2, True)))
        return list(zip(scores.cpu().tolist(), qid.cpu().tolist(), idx.cpu().tolist()))

    def communities(self, threshold: float, min_community_size: int = 10) -> List[list]:
        """Community detection over the corpus ("fast clustering"; no cluster count needed): every group of at least
        ``min_community_size`` entries scoring >= ``threshold`` (``score_function``) against a centre entry, largest first, no
        entry in two groups — ``[[(corpus_idx, text, score_to_centre), ...], ...]``.  A group lists its members by (score to
        the centre desc, index asc), so the centre itself leads it (unless a larger group took it).  The definition, with its
        tie orders, is :func:`ops.community_detection`'s; the de-overlap runs on the device.  The corpus is embedded in ONE
        piece and ``corpus_chunk_size`` does not apply: every row is scored against every row."""
        emb = self.encode_corpus(documents=self.corpus)
        cf = emb.to(self.params.device, dtype=torch.float32).contiguous()
        space = "dot" if self.score_function == "dot" else "cosine"
        lims, members, _, _, info = ops.community_detection(None, cf, cf.shape[1], threshold, min_community_size, space=space,
                                                            return_info=True)
        lims, members, scores = lims.cpu().tolist(), members.cpu().tolist(), info["scores"].cpu().tolist()
        return [[(members[t], self.corpus[members[t]], scores[t]) for t in range(lims[c], lims[c + 1])]
                for c in range(len(lims) - 1)]

    def _search(self, queries, corpus=None, max_num_results: int = 10, return_embeddings: bool = False, candidates=None
                ) -> Dict[int, Union[list, torch.Tensor]]:
        query_embeddings = self.encode_corpus(documents=queries, return_embeddings=return_embeddings)
        if corpus is not None:
            self.corpus = corpus
        if candidates is None:
            scores, indices = self.search_tensors(query_embeddings, self.corpus, max_num_results)
        else:
            scores, indices = self.search_tensors(query_embeddings, self.corpus, max_num_results, candidates=candidates)
        self.last_scores, self.last_indices = scores, indices
        top_candidates = {}
        idx_host = indices.cpu()
        for query_idx in range(idx_host.shape[0]):
            actual = idx_host[query_idx]
            actual = actual[actual >= 0]
            if self.verbose:
                print(f"Top candidates indexes: {actual}")
            if return_embeddings:
                assert isinstance(self.corpus, torch.Tensor)
                top_candidates[query_idx] = self.corpus[actual.to(self.corpus.device)]
            else:
                top_candidates[query_idx] = [(int(c), self.corpus[int(c)]) for c in actual]
        return top_candidates

    def __call__(self, queries, max_num_results: int, return_embeddings: bool = False, candidates=None):
        return self._search(queries, None, max_num_results, return_embeddings, candidates)


class SemanticSearchPipeline(SearchPipeline):
    """/root/reference/src/pipeline/search_pipeline.py:96-175 with the hnswlib ANN index replaced by an exact index in
    HBM (:class:`text_similarity_amd.index.GpuFlatIndex`): same constructor (``index_path`` first), ``_index``,
    ``_search`` / ``__call__`` returning ``{query_idx: [texts best-first]}``, ``add_to_index``, ``remove_from_index``,
    ``num_indexed``.  Differences: results are exact; ``ef`` / ``ef_construction`` / ``M`` are accepted and unused (the
    reference's ``assert max_num_results < ef`` has no meaning here); ``add_to_index`` also appends the texts to
    ``self.corpus`` — the reference only grows the index, so its new ids cannot be mapped back to text.
    ``max_num_results`` up to 1024 (the reference's bound is ``ef`` = 50, search_pipeline.py:131); width <= 768.
    ``score_function='dot'`` keeps an inner-product index (``GpuFlatIndex(space='ip')``); an index file of the other space
    at ``index_path`` raises ``ValueError``.  ``index_type='ivf'`` (with ``nlist=``, ``nprobe=``) keeps a
    :class:`text_similarity_amd.ivf_index.GpuIVFIndex` instead: approximate, exact within the lists it probes.
    ``index_type='pq'`` (with ``pq_m=``) keeps a :class:`text_similarity_amd.pq_index.GpuPQIndex`, trained on the corpus embeddings
    when the index is built: ``pq_m`` bytes a row, any width up to 1024, no filters and no removal.  ``index_type='ivfpq'`` (with
    ``nlist=``, ``nprobe=``, ``pq_m=``) keeps a :class:`text_similarity_amd.ivfpq_index.GpuIVFPQIndex`, trained the same way: ``pq_m``
    bytes a row in ``nlist`` lists of which a query reads ``nprobe``; removal works, filters do not.  ``index_type='graph'`` keeps a
    :class:`text_similarity_amd.graph_index.GpuGraphIndex`, the family of the reference's hnswlib index, and for it ``ef`` /
    ``ef_construction`` / ``M`` are NOT unused: ``M`` sets the graph's degree, ``ef_construction`` the width of the kNN graph the build
    prunes and ``ef`` the beam of a search, as that class documents; removal works (tombstones), filters do not.  ``graph_entry='coarse'``
    (default ``'shared'``) starts every query from the seed rows of its ``nprobe`` nearest of ``nlist`` k-means centroids instead of
    from entry points shared by all queries — what a corpus clustered by topic needs (``nlist`` None: the index's own default,
    about sqrt(n)).  ``graph_incremental=True`` (``'graph'`` only) makes ``add_to_index`` insert the new rows into the built graph, as
hnswlib's ``add_items`` does, where the default rebuilds the graph at the next search (``GpuGraphIndex(incremental=)``; like
``ef`` it is the pipeline's word, not the file's).  ``nlist`` None means 1024 for ``'ivf'`` and ``'ivfpq'``.  ``refine='float32'`` / ``'float16'`` (``'pq'`` and
    ``'ivfpq'`` only; any other ``index_type`` raises ``ValueError``) is handed to the index, which then keeps the embeddings beside
    the codes, and every search re-scores the ``max_num_results * rescore_multiplier`` best rows of the code search exactly
    (the index's ``search(..., rescore_multiplier=)``).  The default of 4 is a stated default, not a measured optimum; it is
    unused without ``refine``.  An index file at ``index_path`` whose ``refine`` differs raises ``ValueError``."""

    def __init__(self, index_path, *args, score_function: Optional[str] = None, index_type: str = "flat",
                 nlist: Optional[int] = None, nprobe: int = 8, pq_m: int = 8, graph_entry: str = "shared",
                 graph_incremental: bool = False, refine: Optional[str] = None, rescore_multiplier: int = 4, **kwargs):
        super().__init__(*args, **kwargs)
        self.index_path = index_path
        self.score_function = resolve_score_function(score_function, self.model)
        hidden = getattr(self.params.model_parameters, "hidden_size", None) or self.model.get_sentence_embedding_dimension()
        space = "ip" if self.score_function == "dot" else "cosine"
        if graph_entry != "shared" and index_type != "graph":
            raise ValueError(f"graph_entry={graph_entry!r} needs index_type='graph'")
        if graph_incremental and index_type != "graph":
            raise ValueError(f"graph_incremental={graph_incremental!r} needs index_type='graph'")
        if refine is not None and index_type not in ("pq", "ivfpq"):
            raise ValueError(f"refine={refine!r} needs index_type='pq' or 'ivfpq', not {index_type!r}")
        self.refine, self.rescore_multiplier = refine, int(rescore_multiplier)
        graph_nlist, nlist = (0 if nlist is None else nlist), (1024 if nlist is None else nlist)
        if index_type == "flat":
            self.index = GpuFlatIndex(space=space, dim=hidden, device=self.params.device)
        elif index_type == "ivf":   # approximate: each query is scored against the nprobe of nlist lists nearest to it
            self.index = GpuIVFIndex(space=space, dim=hidden, nlist=nlist, nprobe=nprobe, device=self.params.device)
        elif index_type == "pq":    # approximate: rows are replaced by pq_m learned bytes
            self.index = GpuPQIndex(space=space, dim=hidden, M=pq_m, device=self.params.device, refine=refine)
        elif index_type == "ivfpq":   # approximate: pq_m learned bytes a row, in lists of which a query reads nprobe
            self.index = GpuIVFPQIndex(space=space, dim=hidden, nlist=nlist, nprobe=nprobe, M=pq_m, device=self.params.device,
                                       refine=refine)
        elif index_type == "graph":   # approximate: a beam search over a proximity graph; ef / ef_construction / M mean something
            self.index = GpuGraphIndex(space=space, dim=hidden, M=getattr(self.params, "M", 0),
                                       ef_construction=getattr(self.params, "ef_construction", 0), device=self.params.device,
                                       entry=graph_entry, nlist=graph_nlist, nprobe=nprobe, incremental=bool(graph_incremental))
            self.index.set_ef(getattr(self.params, "ef", 0))
        else:
            raise ValueError(f"index_type={index_type!r}: one of 'flat', 'ivf', 'pq', 'ivfpq', 'graph'")
        self.index_type = index_type
        if os.path.exists(os.path.join(self.index_path, getattr(self.index, "_FILE_NAME", "index.bin"))):
            self.index.load_index(self.index_path)
            if index_type in ("pq", "ivfpq") and self.index.refine != refine:   # (the file decides what the index holds)
                raise ValueError(f"{self.index_path} holds an index with refine={self.index.refine!r}, not {refine!r}")
            if index_type == "graph":   # (the beam is a parameter of the search, not of the file)
                self.index.set_ef(getattr(self.params, "ef", 0))
                self.index.incremental = bool(graph_incremental)
        else:
            self._index(self.corpus)

    def _index(self, corpus):
        os.makedirs(self.index_path, exist_ok=True)
        corpus_embeddings = self.encode_corpus(corpus)
        if self.index_type in ("pq", "ivfpq"):
            self.index.train(corpus_embeddings)
            self.index.add_items(corpus_embeddings, list(range(corpus_embeddings.shape[0])))
            self.index.save_index(self.index_path)
            return
        self.index.init_index(max_elements=len(corpus), ef_construction=getattr(self.params, "ef_construction", 0),
                              M=getattr(self.params, "M", 0))
        self.index.add_items(corpus_embeddings, list(range(corpus_embeddings.shape[0])))
        self.index.save_index(self.index_path)
        self.index.set_ef(getattr(self.params, "ef", 0))

    def _search(self, queries, max_num_results: int, filter=None):
        query_embeddings = self.encode_corpus(queries)
        mult = self.rescore_multiplier if self.refine is not None else None
        if self.index_type == "pq":
            if filter is not None:
                raise NotImplementedError("GpuPQIndex has no filtered search: index_type='flat' does")
            scores, labels = self.index.search(query_embeddings, max_num_results, rescore_multiplier=mult)
        elif self.index_type == "ivfpq":   # ((values, labels) as GpuPQIndex; a filter raises there)
            scores, labels = self.index.search(query_embeddings, max_num_results, filter=filter, rescore_multiplier=mult)
        elif filter is None:
            labels, scores = self.index.search(query_embeddings, max_num_results)
        else:   # (labels of this index are corpus positions; the forms GpuFlatIndex.search takes)
            labels, scores = self.index.search(query_embeddings, max_num_results, filter=filter)
        self.last_labels, self.last_scores = labels, scores
        top_results = {}
        for qidx, row in enumerate(labels.cpu().tolist()):
            top_results[qidx] = [self.corpus[i] for i in row if i >= 0]
        return top_results

    def __call__(self, queries, max_num_results: int, filter=None):
        return self._search(queries, max_num_results, filter)

    def add_to_index(self, text):
        if isinstance(text, str):
            text = [text]
        embeddings = self.encode_corpus(list(text))
        first = len(self.corpus)
        if self.index_type != "pq":   # (GpuPQIndex grows on its own)
            self.index.resize_index(self.index.get_current_count() + embeddings.shape[0])
        self.index.add_items(embeddings, list(range(first, first + embeddings.shape[0])))
        self.corpus = list(self.corpus) + list(text)

    def remove_from_index(self, ids):
        if self.index_type == "pq":
            raise NotImplementedError("GpuPQIndex has no deletion: index_type='flat' does")
        for id in ids:
            try:
                self.index.mark_deleted(id)
            except RuntimeError:
                continue      # can't find id, continue (search_pipeline.py:167-169)

    def num_indexed(self):
        """current number of indexed embeddings"""
        return self.index.num_live()


class APISearchPipeline(SemanticSearchPipeline):
    """/root/reference/src/pipeline/search_pipeline.py:178-226: the serving variant of ``SemanticSearchPipeline`` whose
    query encoder is an ``onnxruntime.InferenceSession`` over ``params.model_path``.  Here the "session" is the native
    MI355X encoder the pipeline was built with (there is no ONNX runtime on this path): same constructor
    (``params, max_n_results, *args, inference_mode=True, session_options=None``), same ``__call__`` and the same
    ``encode_corpus(documents)`` contract — a list of per-sentence embedding rows in the caller's order (the reference
    sorts by length for batching and un-sorts, :200-226; ``encode_text`` does the same on the device).  The reference's loop
    reshapes every batch to ONE row before ``session.run`` (:217-220), which only works for batches of one sentence; the
    intended per-sentence embeddings are what is returned."""

    def __init__(self, params, max_n_results: int, *args, inference_mode: bool = True, session_options=None, **kwargs):
        # the reference forwards *args to SemanticSearchPipeline(index_path, params, model): its callers pass params a second
        # time there; (index_path, model) alone is accepted as well
        args = list(args)
        if len(args) == 2 and "model" not in kwargs:
            args.insert(1, params)
        super().__init__(*args, **kwargs)
        self.params = params
        self.inference_mode = inference_mode
        self.sess_options = session_options
        self.max_n_results = max_n_results
        self.session = self.model          # what runs the encoder forward

    def __call__(self, queries, max_num_results: Optional[int] = None):
        return self._search(queries, self.max_n_results if max_num_results is None else max_num_results)

    def encode_corpus(self, documents, convert_to_numpy: bool = False, return_embeddings: bool = False):
        if not isinstance(documents, list):
            return documents
        emb = self.model.encode_text(documents, output_np=False)
        return emb
