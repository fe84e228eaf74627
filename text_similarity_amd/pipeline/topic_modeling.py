"""``TopicModelingPipeline`` (/root/reference/src/pipeline/topic_modeling.py:37-169): embed the documents, cluster the
embeddings with HDBSCAN, name every cluster by class-based TF-IDF.

The reference embeds with its encoder, reduces the embeddings with UMAP, clusters them with ``hdbscan.HDBSCAN(min_cluster_size,
metric=cluster_metric, cluster_selection_method="eom")`` and scores words with ``CountVectorizer`` and pandas.  Here the
clustering is :func:`ops.hdbscan` (the minimum spanning tree on the device, the tree stage in native host code) and c-TF-IDF is
numpy on the host.  UMAP is not a dependency and nothing stands in for it: ``reducer`` is an optional object with
``fit_transform`` (``umap.UMAP(...)`` where it is installed); without one the clustering runs on the embeddings as they are,
with ``cluster_metric`` 'euclidean' or 'cosine'.

c-TF-IDF (topic_modeling.py:106-118 with the documents of a topic joined, :79).  Tokens are the lower-cased matches of
``\\b\\w\\w+\\b`` (CountVectorizer's default pattern), minus the optional ``stop_words`` set; t[c, v] counts word v in topic c,
topic -1 (the noise) included; ``tf = t[c, v] / sum_v t[c, v]``, ``idf[v] = log(m / sum_c t[c, v])`` with m the number of
DOCUMENTS; the score is their product.  ``top_n_words`` maps every topic to its n best ``(word, score)`` pairs by (score desc,
word asc); ``topic_sizes`` is a list of ``(topic, size)`` by (size desc, topic asc).

Not built: ``reduce_n_topics`` (it does not run in the reference: it calls ``_c_tf_idf`` with arguments it does not take), the
WordNet hypernyms, translation and plotting."""
from __future__ import annotations

import re
from collections import Counter
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from .. import ops
from .search_pipeline import Pipeline

_TOKEN = re.compile(r"\b\w\w+\b")


class TopicModelingParams:
    def __init__(self, n_neighbors=15, n_components=5, reduction_metric="cosine", min_cluster_size=15, cluster_metric="euclidean",
                 min_samples=None):
        self.n_neighbors = n_neighbors
        self.n_components = n_components
        self.reduction_metric = reduction_metric
        self.min_cluster_size = min_cluster_size
        self.cluster_metric = cluster_metric
        self.min_samples = min_samples


def tokenize(doc: str, stop_words=None) -> List[str]:
    words = _TOKEN.findall(doc.lower())
    return [w for w in words if w not in stop_words] if stop_words else words


def c_tf_idf(documents: List[str], labels, stop_words=None) -> Tuple[np.ndarray, List[str], List[int]]:
    """``(scores float64 [topics, words], words, topics)``: class-based TF-IDF of the documents joined per label; words and
    topics ascending.  A topic without a token scores 0 everywhere."""
    labels = [int(t) for t in labels]
    if len(labels) != len(documents):
        raise ValueError(f"c_tf_idf: {len(documents)} documents, {len(labels)} labels")
    topics = sorted(set(labels))
    row = {t: i for i, t in enumerate(topics)}
    counts = [Counter() for _ in topics]
    for doc, t in zip(documents, labels):
        counts[row[t]].update(tokenize(doc, stop_words))
    words = sorted(set().union(*counts)) if counts else []
    col = {w: j for j, w in enumerate(words)}
    t = np.zeros((len(topics), len(words)), dtype=np.float64)
    for i, c in enumerate(counts):
        for w, n in c.items():
            t[i, col[w]] = n
    tf = t / np.maximum(t.sum(axis=1, keepdims=True), 1.0)
    idf = np.log(len(documents) / t.sum(axis=0)) if words else np.zeros((0,))
    return tf * idf[None, :], words, topics


class TopicModelingPipeline(Pipeline):
    def __init__(self, params, embedder, documents: List[str], *args, lang="eng", stop_words=None, **kwargs):
        super().__init__(params, embedder, *args, **kwargs)
        self.embedder = embedder
        self.documents = list(documents)
        self.lang = lang
        self.stop_words = set(stop_words) if stop_words else None
        self.labels_ = None

    def _cluster(self, embeddings: torch.Tensor) -> torch.Tensor:
        p = self.params
        return ops.hdbscan(embeddings, p.min_cluster_size, getattr(p, "min_samples", None), p.cluster_metric)

    def extract_top_n_words_per_topic(self, scores: np.ndarray, words: List[str], topics: List[int], n=10) -> Dict[int, list]:
        names = np.array(words)
        out = {}
        for i, t in enumerate(topics):
            order = np.lexsort((names, -scores[i]))[:n]      # (score desc, word asc)
            out[t] = [(words[j], float(scores[i, j])) for j in order]
        return out

    def extract_topic_sizes(self, labels) -> List[Tuple[int, int]]:
        return sorted(Counter(int(t) for t in labels).items(), key=lambda ts: (-ts[1], ts[0]))

    def __call__(self, max_n_words=10, embeddings=None, reducer=None):
        if embeddings is None:
            embeddings = self.embedder.encode_text(self.documents, output_np=False)
        if reducer is not None:
            embeddings = reducer.fit_transform(embeddings.detach().cpu().numpy() if isinstance(embeddings, torch.Tensor)
                                               else np.asarray(embeddings))
        if not isinstance(embeddings, torch.Tensor):
            embeddings = torch.from_numpy(np.ascontiguousarray(embeddings, dtype=np.float32))
        if embeddings.shape[0] != len(self.documents):
            raise ValueError(f"{len(self.documents)} documents, {embeddings.shape[0]} embeddings")
        if not embeddings.is_cuda:
            embeddings = embeddings.cuda()
        self.labels_ = self._cluster(embeddings.float())
        labels = self.labels_.tolist()
        scores, words, topics = c_tf_idf(self.documents, labels, self.stop_words)
        return self.extract_top_n_words_per_topic(scores, words, topics, n=max_n_words), self.extract_topic_sizes(labels)
