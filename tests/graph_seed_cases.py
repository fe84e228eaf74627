"""Test-local restatement of the seeded graph search (include/tsim.h tsim_graph_search_seeded), numpy only, on top of
tests/graph_cases.py and tests/list_cases.py; shared by tests/test_graph_seed_cpu.py, tests/test_graph_seed_gpu.py,
tests/test_graph_seed_index_gpu.py and tools/fuzz_graph.py.  Nothing of the search is restated here: the probes are the list
search of the query against the centroids, the entry points two table look-ups, and the search graph_search_ref, a query at a
time."""
import numpy as np

from graph_cases import ST_ROW, build_graph_ref, graph_search_ref, list_topk_ref


def probes_ref(space, q, centroids, P):
    """int64 [Q, P]: the P centroids of best score to each query, (score desc, list asc), a NaN score dropped, -1 padded."""
    centroids = np.asarray(centroids, dtype=np.float32)
    S, I, _ = list_topk_ref(space, np.asarray(q, dtype=np.float32), centroids, np.arange(centroids.shape[0]), P)
    return np.where(np.isnan(S), -1, I)      # (rank_list orders NaN behind every number, so the ids before it stand)


def entries_ref(probes, seeds, T, N):
    """(entries int64 [Q, P S], beyond bool [Q]): seeds[probes[q][p]][s] with -1 for padding at either level and for a probe
    >= T; ``beyond`` where a probe was >= T (a seed >= N stays in the entries: the search reports it).  seeds None: S = 1, T = N
    and a probe is a row."""
    probes = np.asarray(probes, dtype=np.int64)
    if seeds is None:
        seeds, T = np.arange(N, dtype=np.int64)[:, None], N
    seeds = np.asarray(seeds, dtype=np.int64)
    ok = (probes >= 0) & (probes < T)
    ent = np.where(ok[:, :, None], seeds[np.where(ok, probes, 0)], -1)
    return ent.reshape(probes.shape[0], -1), (probes >= T).any(1)


def graph_search_seeded_ref(space, q, c, graph, ef, width, max_iters, k, probes=None, centroids=None, n_probe=None, seeds=None,
                            row_ids=None, idx_offset=0):
    """(scores [Q, k], idx [Q, k], status [Q], probes [Q, P]): graph_search_ref, one query at a time, from that query's entries."""
    q = np.asarray(q, dtype=np.float32)
    N = np.asarray(c).shape[0]
    assert (probes is None) != (centroids is None)
    if probes is None:
        probes = probes_ref(space, q, centroids, n_probe)
    T = N if seeds is None else np.asarray(seeds).shape[0]
    ent, beyond = entries_ref(probes, seeds, T, N)
    S = np.empty((q.shape[0], k), dtype=np.float32)
    I = np.empty((q.shape[0], k), dtype=np.int64)
    st = np.zeros((q.shape[0],), dtype=np.int32)
    for j in range(q.shape[0]):
        S[j:j + 1], I[j:j + 1], st[j:j + 1] = graph_search_ref(space, q[j:j + 1], c, graph, ent[j], ef, width, max_iters, k,
                                                               row_ids=row_ids, idx_offset=idx_offset)
        if beyond[j]:
            st[j] |= ST_ROW
    return S, I, st, np.asarray(probes, dtype=np.int64)


# ------------------------------------------------------------------------------------------------- the island corpus
def island_corpus(seed=7, n_cent=64, per=32, d=32, Q=48, noise=0.1):
    """(rows [n_cent per, d], centres [n_cent, d], queries [Q, d]) float32: tight clusters whose exact kNN graph falls apart into
    one island a cluster — the corpus on which shared entry points find almost nothing."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((n_cent, d))
    rows = (np.repeat(cent, per, 0) + noise * rng.standard_normal((n_cent * per, d))).astype(np.float32)
    rows = rows[rng.permutation(n_cent * per)]
    qs = (cent[rng.integers(0, n_cent, Q)] + noise * rng.standard_normal((Q, d))).astype(np.float32)
    return rows, cent.astype(np.float32), qs


def seed_table_ref(space, centroids, rows, S):
    """int64 [T, S]: the S rows of best score to each centroid, rank order, -1 padded."""
    rows = np.asarray(rows, dtype=np.float32)
    return list_topk_ref(space, np.asarray(centroids, dtype=np.float32), rows, np.arange(rows.shape[0]), S)[1]


def recall(found, truth):
    """Mean fraction of each row of ``truth`` (ids >= 0) found in the same row of ``found``."""
    hit = [len(set(t[t >= 0].tolist()) & set(f.tolist())) / max(1, int((t >= 0).sum())) for f, t in zip(found, truth)]
    return float(np.mean(hit))


__all__ = ["probes_ref", "entries_ref", "graph_search_seeded_ref", "island_corpus", "seed_table_ref", "recall", "build_graph_ref"]
