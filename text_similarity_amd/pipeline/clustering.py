"""``ClusteringPipeline`` (/root/reference/src/pipeline/clustering.py:8-31): k-means over corpus embeddings.

The reference delegates to ``sklearn.cluster.KMeans`` on the host, on the RAW (un-normalised) embeddings.  Here Lloyd's
iterations run on the device with the same semantics: Euclidean assignment
``argmin_j |x - c_j|^2 = argmax_j (x.c_j - |c_j|^2 / 2)`` (ties to the lower index, as sklearn's argmin), centre = mean
of its points, until the labels repeat.  The scores come from the dense cosine kernel of the search path (``tsim_cos_sim``:
``x.c = cos(x, c) |x| |c|``), the update step is a scatter-add.  Initial centres: ``init=<array>`` (what the parity
fixture uses: tests/golden/kmeans.npz pins labels / centres / inertia against sklearn with the same initial centres) or
k-means++ seeded from ``seed`` (sklearn's own k-means++ draws from its private RNG stream and cannot be reproduced).
An emptied cluster keeps its centre (sklearn relocates it to a far point; with k-means++ starts this does not occur on
the fixtures).  ``__call__`` returns ``{cluster_id: [row indices or texts]}`` (the reference builds that dict and forgets
to return it, clustering.py:20-23).

``method="community"`` clusters WITHOUT a cluster count (the reference keeps a ``method=`` argument and its topic pipeline turns
to a density method for the same reason: k is not known): community detection over the corpus' cosine scores
(:func:`ops.community_detection`) — every group of at least ``min_community_size`` rows scoring >= ``threshold`` against a
centre row, largest first, no row in two groups.  ``n_clusters`` is ignored; ``fit`` sets ``labels_`` (-1: noise, a row in no
community), ``cluster_centers_`` (the centre ROWS, not means) and ``n_iter_`` (the rounds of the de-overlap); ``inertia_`` stays
None; ``__call__`` returns the same dict without the noise.

``method="hdbscan"`` is that density method itself (:func:`ops.hdbscan`: ``hdbscan.HDBSCAN(min_cluster_size, metric=...,
cluster_selection_method="eom")``, the minimum spanning tree on the device): it needs neither a cluster count nor a threshold
and its clusters have any shape.  ``min_cluster_size``, ``min_samples`` (default: ``min_cluster_size``) and ``metric``
('euclidean' or 'cosine') are its parameters; ``fit`` sets ``labels_`` (-1: noise) and ``cluster_centers_`` (the MEAN of each
cluster's rows); ``inertia_`` stays None and ``n_iter_`` 0; ``__call__`` returns the dict without the noise."""
from __future__ import annotations

from collections import defaultdict
from typing import List, Optional, Union

import numpy as np
import torch

from .. import ops
from .search_pipeline import Pipeline


class ClusteringPipeline(Pipeline):
    def __init__(self, n_clusters, *args, method="k-means", max_iter: int = 300, seed: int = 0, init=None,
                 threshold: Optional[float] = None, min_community_size: int = 10, min_cluster_size: int = 15,
                 min_samples: Optional[int] = None, metric: str = "euclidean", **kwargs):
        super().__init__(*args, **kwargs)
        if method not in ("k-means", "community", "hdbscan"):
            raise ValueError(f"method={method!r}: 'k-means' (as in the reference), 'community' or 'hdbscan'")
        if method == "hdbscan" and metric not in ("euclidean", "cosine"):
            raise ValueError(f"metric={metric!r}: 'euclidean' or 'cosine'")
        if method == "community" and threshold is None:
            raise ValueError("method='community' needs threshold= (the score two rows of one community must reach)")
        self.method = method
        self.threshold = threshold
        self.min_community_size = int(min_community_size)
        self.min_cluster_size = int(min_cluster_size)
        self.min_samples = min_samples
        self.metric = metric
        self.n_clusters = int(n_clusters) if n_clusters is not None else 0
        self.max_iter = max_iter
        self.seed = seed
        self.init = init
        self.labels_ = None
        self.cluster_centers_ = None
        self.inertia_ = None
        self.n_iter_ = 0

    def set_n_clusters(self, n: int):
        self.n_clusters = int(n)

    @staticmethod
    def _assign(x: torch.Tensor, xn: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
        """Euclidean assignment: argmax_j (x.c_j - |c_j|^2 / 2) with x.c from the dense cosine kernel."""
        cn = c.norm(dim=1)
        cos = torch.nan_to_num(ops.cos_sim_dense(x, c), nan=0.0)     # a zero row has no direction: x.c = 0
        score = cos * xn[:, None] * cn[None, :] - 0.5 * (cn * cn)[None, :]
        return score.argmax(dim=1)                                    # first maximum = lower index, like numpy / sklearn

    def _kmeanspp(self, x: torch.Tensor, k: int) -> torch.Tensor:
        """Greedy k-means++ (the variant sklearn uses: 2 + log k candidates per step, keep the one that lowers the potential
        most) on a sample of the points; seeded."""
        import math
        g = torch.Generator(device="cpu").manual_seed(self.seed)
        n = x.shape[0]
        samp = torch.randperm(n, generator=g)[:min(n, 4096)].to(x.device)
        xs = x[samp]
        trials = 2 + int(math.log(max(k, 1)))
        centers = [xs[int(torch.randint(len(samp), (1,), generator=g))]]
        dist = (xs - centers[0]).pow(2).sum(1)
        for _ in range(1, k):
            tot = float(dist.sum())
            if tot > 0:
                cand = torch.multinomial((dist / tot).cpu(), trials, replacement=True, generator=g).to(x.device)
            else:
                cand = torch.randint(len(samp), (trials,), generator=g).to(x.device)
            dc = torch.cdist(xs[cand], xs).pow(2)                     # [trials, m]
            pot = torch.minimum(dist[None, :], dc).sum(1)
            best = int(pot.argmin())
            centers.append(xs[cand[best]])
            dist = torch.minimum(dist, dc[best])
        return torch.stack(centers)

    def fit(self, emb: torch.Tensor, init: Optional[Union[torch.Tensor, np.ndarray]] = None):
        if not emb.is_cuda:
            emb = emb.cuda()
        x = emb.float().contiguous()
        n, d = x.shape
        if self.method == "community":
            _, _, centres, labels, info = ops.community_detection(None, x, d, self.threshold, self.min_community_size,
                                                                  return_info=True)
            self.labels_ = labels
            self.cluster_centers_ = x[centres]
            self.inertia_ = None
            self.n_iter_ = info["rounds"]
            return self
        if self.method == "hdbscan":
            labels, info = ops.hdbscan(x, self.min_cluster_size, self.min_samples, self.metric, return_info=True)
            k = info["n_clusters"]
            keep = labels >= 0
            sums = torch.zeros((k, d), dtype=torch.float32, device=x.device).index_add_(0, labels[keep], x[keep])
            self.labels_ = labels
            self.cluster_centers_ = sums / torch.bincount(labels[keep], minlength=k).clamp(min=1).unsqueeze(1)
            self.inertia_ = None
            self.n_iter_ = 0
            return self
        k = min(self.n_clusters, n)
        init = self.init if init is None else init
        if init is not None:
            c = torch.as_tensor(np.asarray(init) if not isinstance(init, torch.Tensor) else init).to(x.device).float().contiguous()
            if c.shape != (k, d):
                raise ValueError(f"init must have shape ({k}, {d}), got {tuple(c.shape)}")
        else:
            c = self._kmeanspp(x, k)
        xn = x.norm(dim=1)
        labels = None
        self.n_iter_ = 0
        for it in range(self.max_iter):
            new = self._assign(x, xn, c)
            if labels is not None and torch.equal(new, labels):
                break
            labels = new
            self.n_iter_ = it + 1
            sums = torch.zeros((k, d), dtype=torch.float32, device=x.device).index_add_(0, labels, x)
            cnt = torch.bincount(labels, minlength=k).unsqueeze(1)
            c = torch.where(cnt > 0, sums / cnt.clamp(min=1), c).contiguous()      # an emptied cluster keeps its centre
        self.labels_ = labels
        self.cluster_centers_ = c
        self.inertia_ = float((x - c[labels]).pow(2).sum())
        return self

    def _cluster(self, corpus: Union[List[str], torch.Tensor, np.ndarray]):
        texts = corpus if isinstance(corpus, list) else None
        emb = self.encode_corpus(corpus) if isinstance(corpus, list) else corpus
        if isinstance(emb, np.ndarray):
            emb = torch.from_numpy(emb)
        self.fit(emb)
        results = defaultdict(list)
        for text_id, cluster_id in enumerate(self.labels_.tolist()):
            if cluster_id < 0:      # (method='community' and 'hdbscan': noise)
                continue
            results[cluster_id].append(texts[text_id] if texts is not None else text_id)
        return dict(results)

    def __call__(self, embeddings, n_clusters=None):
        if n_clusters is not None:
            self.set_n_clusters(n_clusters)
        return self._cluster(embeddings)
