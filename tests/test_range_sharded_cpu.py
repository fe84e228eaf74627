"""Two gloo ranks: the choreography of ShardedCorpusSearch.range_search — the query (and threshold) all-gather, the exchange of
the per-rank lims, the padded payload exchange and the merge — returns, on every rank, the range result of the unsharded corpus.
CPU only: numpy stand-ins take the place of the local range search and of the merge kernel (tests may do that; the product
defaults are the HIP ops)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle.search_ref import exact_cosine
from text_similarity_amd import presets
from text_similarity_amd.distributed.sharded_search import ShardedCorpusSearch, shard_bounds

D = 384


# ---------------------------------------------------------------------------------------------------------- numpy stand-ins
def _range_ref(scores, tau):
    """CSR (lims, scores, idx) of score >= float32(tau[q]) per query, ordered (score desc, index asc); tau a float or [Q]"""
    scores = np.asarray(scores, np.float32)
    tau = np.broadcast_to(np.asarray(tau, np.float32), (scores.shape[0],))
    lims, ss, ii = [0], [], []
    for s, t in zip(scores, tau):
        with np.errstate(invalid="ignore"):
            hit = np.nonzero(s >= t)[0]
        hit = hit[np.lexsort((hit, -s[hit].astype(np.float64)))]
        ss.append(s[hit])
        ii.append(hit.astype(np.int64))
        lims.append(lims[-1] + hit.size)
    return np.array(lims, np.int64), np.concatenate(ss).astype(np.float32), np.concatenate(ii).astype(np.int64)


def _oracle_local_range(q, c_unit, c_f32, d, threshold, offset):
    tau = threshold.numpy() if isinstance(threshold, torch.Tensor) else float(threshold)
    lims, s, i = _range_ref(exact_cosine(q.numpy(), c_f32.numpy()), tau)
    return torch.from_numpy(lims), torch.from_numpy(s), torch.from_numpy(i + offset)


def _oracle_range_merge(results, total):
    """per query: the lists' segments concatenated and sorted by (score desc, index asc)"""
    results = [(l.numpy(), s.numpy(), i.numpy()) for l, s, i in results]
    Q = results[0][0].size - 1
    lims, ss, ii = [0], [], []
    for q in range(Q):
        s = np.concatenate([r[1][r[0][q]:r[0][q + 1]] for r in results])
        i = np.concatenate([r[2][r[0][q]:r[0][q + 1]] for r in results])
        o = np.lexsort((i, -s.astype(np.float64)))
        ss.append(s[o])
        ii.append(i[o])
        lims.append(lims[-1] + o.size)
    assert lims[-1] == total
    return torch.from_numpy(np.array(lims, np.int64)), torch.from_numpy(np.concatenate(ss)), torch.from_numpy(np.concatenate(ii))


# ---------------------------------------------------------------------------------------------------------- data
def _data(n_total, q_total):
    corpus = presets.synthetic_embeddings(n_total, D, "rshard/c")
    queries = presets.synthetic_embeddings(q_total, D, "rshard/q")
    queries[0] = corpus[3]
    return corpus, queries


def _thresholds(mode, exact):
    """one selective float, or a per-query vector: a score of the query itself, +-inf, NaN and plain values mixed"""
    if mode == "scalar":
        return np.float32(0.08)
    Q = exact.shape[0]
    tau = np.full(Q, 0.1, np.float32)
    for qi in range(Q):
        srt = np.sort(exact[qi])[::-1]
        tau[qi] = (srt[4], np.float32(0.15), -np.inf, np.inf, np.nan, np.nextafter(srt[2], np.float32(np.inf)))[qi % 6]
    return tau


def _floor_at_zero(thr):
    """finite values and -inf raised to 0 (+inf and NaN stay): no row of negative cosine is a hit"""
    with np.errstate(invalid="ignore"):
        return np.where(thr < 0, np.float32(0.0), thr).astype(np.float32)


def _corpus_for(layout, n_total, q_total):
    corpus, queries = _data(n_total, q_total)
    lo1 = shard_bounds(n_total, 2, 1)[0]
    if layout == "rank1_empty":      # all-positive queries, all-negative rows on rank 1: every cosine there is < 0, and with
        corpus[lo1:] = -np.abs(corpus[lo1:]) - 0.05                   # thresholds >= 0 rank 1's payload is zero-length
        queries = (np.abs(queries) + 0.05).astype(np.float32)
        corpus[10:10 + q_total] = queries * 1.5                       # rank 0 holds a neighbour of every query
    else:
        corpus[n_total - 1] = corpus[3]          # a duplicate on the LAST shard: equal scores, ordered by index across ranks
    return corpus, queries


def _worker(rank, world, port, n_total, q_total, layout, mode, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        corpus, queries = _corpus_for(layout, n_total, q_total)
        thr = _thresholds(mode, exact_cosine(queries, corpus))
        thr = _floor_at_zero(thr) if layout == "rank1_empty" else thr
        lo, hi = shard_bounds(n_total, world, rank)
        qlo, qhi = shard_bounds(q_total, world, rank)
        counts = [shard_bounds(q_total, world, r)[1] - shard_bounds(q_total, world, r)[0] for r in range(world)]
        eng = ShardedCorpusSearch(torch.zeros((hi - lo, 1), dtype=torch.float16), D, lo, corpus_f32_local=torch.from_numpy(corpus[lo:hi]),
                                  local_range=_oracle_local_range, range_merge=_oracle_range_merge)
        local_thr = torch.from_numpy(thr[qlo:qhi].copy()) if mode == "vector" else float(thr)
        lims, s, i = eng.range_search(torch.from_numpy(queries[qlo:qhi]), local_thr, counts=counts)
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), lims=lims.numpy(), s=s.numpy(), i=i.numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("layout,mode,n_total,q_total", [("both", "scalar", 301, 7), ("both", "vector", 301, 7),
                                                          ("rank1_empty", "scalar", 200, 5), ("rank1_empty", "vector", 200, 6)])
def test_two_rank_range_search_equals_unsharded(tmp_path, layout, mode, n_total, q_total):
    """7 queries on 2 ranks (4 / 3: padded for the exchange, the padding dropped), shards of 151 / 150 rows; in the second
    layout rank 1's shard has no hit at all and its payload is zero-length."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    world = 2
    mp.spawn(_worker, args=(world, port, n_total, q_total, layout, mode, str(tmp_path)), nprocs=world, join=True)
    corpus, queries = _corpus_for(layout, n_total, q_total)
    exact = exact_cosine(queries, corpus)
    thr = _thresholds(mode, exact)
    thr = _floor_at_zero(thr) if layout == "rank1_empty" else thr
    ref_lims, ref_s, ref_i = _range_ref(exact, thr)
    assert ref_lims[-1] > q_total
    lo1 = shard_bounds(n_total, world, 1)[0]
    if layout == "rank1_empty":
        assert (ref_i < lo1).all()                       # every hit lives on rank 0
    else:
        seg = ref_i[ref_lims[0]:ref_lims[1]]
        assert seg[0] == 3 and seg[1] == n_total - 1     # the duplicate across ranks, by index
    for r in range(world):
        got = np.load(tmp_path / f"r{r}.npz")
        np.testing.assert_array_equal(got["lims"], ref_lims)
        np.testing.assert_array_equal(got["i"], ref_i)
        np.testing.assert_array_equal(got["s"].view(np.uint32), ref_s.view(np.uint32))


def test_range_search_argument_checks():
    eng = ShardedCorpusSearch(torch.zeros((4, 1), dtype=torch.float16), D, 0, local_range=_oracle_local_range,
                              range_merge=_oracle_range_merge)
    with pytest.raises(ValueError):                      # no float32 rows: there is no unit-rows-only range search
        eng.range_search(torch.zeros((2, D)), 0.5)
    eng = ShardedCorpusSearch(torch.zeros((4, 1), dtype=torch.float16), D, 0, corpus_f32_local=torch.ones((4, D)),
                              local_range=_oracle_local_range, range_merge=_oracle_range_merge)
    with pytest.raises(ValueError):
        eng.range_search(torch.zeros((2, D)), torch.zeros(3))
    lims, s, i = eng.range_search(torch.ones((2, D)), torch.tensor([0.5, np.inf]))      # one process: the local search itself
    assert lims.tolist() == [0, 4, 4] and i.tolist() == [0, 1, 2, 3]
