"""Test-local restatement of the insertion into a built graph (include/tsim_graph_insert.h, text_similarity_amd/ops.py
graph_insert, GpuGraphIndex(incremental=True)), numpy only, shared by tests/test_graph_insert_cpu.py, the three
tests/test_graph_insert_*_gpu.py and tools/fuzz_graph.py.  Nothing that exists is restated again: the beam search is
graph_cases.graph_search_ref / graph_seed_cases.graph_search_seeded_ref, scores and the order of a list come from list_cases
(pair_scores, rank_list, list_topk_ref), the choice of the R entries of smallest (D, rank) is graph_cases.forward_lists.  New
here: the two rules as literal loops (insert_prune_loop, link_reverse_loop), their vectorised forms, the candidate merge, the
sub-batch step and the whole insertion (insert_ref).  Every GPU result is compared with these for equality."""
import numpy as np

import graph_cases as gc
import graph_seed_cases as gsc
from list_cases import list_topk_ref, pair_scores, rank_list

INSERT_ST_ROW = 1                                   # include/tsim_graph_insert.h TSIM_GRAPH_INSERT_ST_ROW
LINK_ST_CUT, LINK_ST_ROW, LINK_ST_LIMS = 1, 2, 4    # TSIM_GRAPH_LINK_ST_*
LINK_POOL = 256                                     # TSIM_GRAPH_LINK_POOL


# ------------------------------------------------------------------------------------------------- forward edges
def _neighbours(cand, graph, n, c, R):
    """N(c): the graph row of an old row, the first R candidates of a batch row."""
    return graph[c] if c < n else cand[c - n, :R]


def insert_prune_loop(cand, graph):
    """(F [B, R], D [B, K0], status [B]) by the definition, literal loops."""
    cand = np.asarray(cand, dtype=np.int64)
    graph = np.asarray(graph, dtype=np.int64)
    B, K0 = cand.shape
    n, R = graph.shape
    end = n + B
    D = np.zeros((B, K0), dtype=np.int64)
    st = np.zeros((B,), dtype=np.int32)
    for i in range(B):
        for j in range(K0):
            t = cand[i, j]
            if t >= end:
                st[i] |= INSERT_ST_ROW
            if not 0 <= t < end:
                D[i, j] = K0
                continue
            for a in range(j):
                ca = cand[i, a]
                if 0 <= ca < end and t in _neighbours(cand, graph, n, ca, R).tolist():
                    D[i, j] += 1
    return gc.forward_lists(cand, D, R), D, st


def insert_prune(cand, graph):
    """The same, a new row at a time: the K0 neighbour lists gathered once, one comparison of every list with every candidate."""
    cand = np.asarray(cand, dtype=np.int64)
    graph = np.asarray(graph, dtype=np.int64)
    B, K0 = cand.shape
    n, R = graph.shape
    end = n + B
    both = np.concatenate([graph, cand[:, :R]], axis=0)                       # row c of it is N(c)
    D = np.zeros((B, K0), dtype=np.int64)
    below = np.arange(K0)[:, None] < np.arange(K0)[None, :]                   # [a, j]: a < j
    for i in range(B):
        g = cand[i]
        ok = (g >= 0) & (g < end)
        nb = np.where(ok[:, None], both[np.where(ok, g, 0)], -1)              # [a, c]
        hit = (nb[:, None, :] == g[None, :, None]).any(2)                     # [a, j]: cand[i][j] in N(cand[i][a])
        D[i] = np.where(ok, (hit & below & ok[:, None]).sum(0), K0)
    st = np.where((cand >= end).any(1), INSERT_ST_ROW, 0).astype(np.int32)
    return gc.forward_lists(cand, D, R), D, st


# ------------------------------------------------------------------------------------------------- reverse edges
def incoming(F, n):
    """(targets [T], in_lims [T + 1], in_ids) of the forward rows F [b, R] of the new rows n .. n + b - 1: the sorted distinct rows
    some new row chose, each with its choosers in (position of the target in the chooser's row, chooser) order."""
    F = np.asarray(F, dtype=np.int64)
    b, R = F.shape
    chosen = {}
    for pos in range(R):
        for i in range(b):
            t = int(F[i, pos])
            if t >= 0:
                chosen.setdefault(t, []).append(n + i)
    targets = np.array(sorted(chosen), dtype=np.int64)
    lims = np.zeros((targets.shape[0] + 1,), dtype=np.int64)
    lims[1:] = np.cumsum([len(chosen[t]) for t in targets.tolist()])
    ids = np.array([x for t in targets.tolist() for x in chosen[t]], dtype=np.int64)
    return targets, lims, ids


def _pool(row, R, lo, hi, in_ids):
    """(kept, pool, cut) of one target's row and its incoming rows."""
    h = R // 2
    valid = [int(x) for x in row if x >= 0]
    kept, pool = valid[:h], []
    for x in valid[h:] + [int(x) for x in in_ids[lo:hi]]:
        if x >= 0 and x not in kept and x not in pool:
            pool.append(x)
    return kept, pool[:LINK_POOL], len(pool) > LINK_POOL


def _clamped(in_lims, j):
    total = max(int(in_lims[-1]), 0)
    lo, hi = int(in_lims[j]), int(in_lims[j + 1])
    lo_c = min(max(lo, 0), total)
    hi_c = min(max(hi, lo_c), total)
    return lo_c, hi_c, (lo_c, hi_c) != (lo, hi)


def link_reverse_loop(space, rows, graph, targets, in_lims, in_ids):
    """(graph' [N, R], status [T]) by the definition, a target at a time through list_topk_ref."""
    rows = np.asarray(rows, dtype=np.float32)
    G = np.array(graph, dtype=np.int64)
    N, R = G.shape
    k = R - R // 2
    st = np.zeros((len(targets),), dtype=np.int32)
    for j, t in enumerate(np.asarray(targets, dtype=np.int64).tolist()):
        if not 0 <= t < N:
            st[j] = LINK_ST_ROW
            continue
        lo, hi, moved = _clamped(in_lims, j)
        kept, pool, cut = _pool(G[t], R, lo, hi, in_ids)
        st[j] |= (LINK_ST_LIMS if moved else 0) | (LINK_ST_CUT if cut else 0)
        best = []
        if pool:
            S, I, s = list_topk_ref(space, rows[t:t + 1], rows, [pool], k, unique=False)
            st[j] |= LINK_ST_ROW if s[0] else 0
            best = [int(i) for sc, i in zip(S[0], I[0]) if i >= 0 and not np.isnan(sc)]
        out = kept + best
        G[t] = out + [-1] * (R - len(out))
    return G, st


def link_reverse(space, rows, graph, targets, in_lims, in_ids):
    """The same with ONE call of pair_scores for all targets (no target reads another's row, so the order does not matter)."""
    rows = np.asarray(rows, dtype=np.float32)
    G = np.array(graph, dtype=np.int64)
    N, R = G.shape
    k = R - R // 2
    targets = np.asarray(targets, dtype=np.int64)
    st = np.zeros((targets.shape[0],), dtype=np.int32)
    work, qi, ci = [], [], []
    for j, t in enumerate(targets.tolist()):
        if not 0 <= t < N:
            st[j] = LINK_ST_ROW
            continue
        lo, hi, moved = _clamped(in_lims, j)
        kept, pool, cut = _pool(G[t], R, lo, hi, in_ids)
        st[j] |= (LINK_ST_LIMS if moved else 0) | (LINK_ST_CUT if cut else 0)
        if any(x >= N for x in pool):
            st[j] |= LINK_ST_ROW
        pool = [x for x in pool if x < N]
        work.append((t, kept, pool, len(qi)))
        qi += [t] * len(pool)
        ci += pool
    sc = pair_scores(space, rows, rows, np.asarray(qi, dtype=np.int64), np.asarray(ci, dtype=np.int64))
    for t, kept, pool, at in work:
        s = sc[at:at + len(pool)]
        ok = ~np.isnan(s)
        _, I = rank_list(space, np.asarray(pool, dtype=np.int64)[ok], s[ok], k)
        out = kept + [int(i) for i in I if i >= 0]
        G[t] = out + [-1] * (R - len(out))
    return G, st


# ------------------------------------------------------------------------------------------------- the sub-batch step
def candidates_ref(space, rows, n, old_s, old_i, K0):
    """C [b, K0]: the first K0 of (what the beam search of the new rows over the old graph returned) + (each new row's exact best
    min(K0 + 1, b) among the new rows, itself dropped by the build's rule), by (score desc, id asc), 'l2' (dist^2 asc, id asc)."""
    rows = np.asarray(rows, dtype=np.float32)
    new = rows[n:]
    b = new.shape[0]
    kn = min(K0 + 1, b)
    S, I, _ = list_topk_ref(space, new, new, np.arange(b), kn, idx_offset=n)
    C = np.full((b, K0), -1, dtype=np.int64)
    for x in range(b):
        at = np.nonzero(I[x] == n + x)[0]
        drop = at[0] if at.size else kn - 1
        ids = np.concatenate([np.asarray(old_i[x], dtype=np.int64), np.delete(I[x], drop)])
        sc = np.concatenate([np.asarray(old_s[x], dtype=np.float32), np.delete(S[x], drop)]).astype(np.float64)
        order = np.lexsort((ids, sc if space == "l2" else -sc, ids < 0))[:K0]
        C[x, :order.shape[0]] = np.where(ids[order] >= 0, ids[order], -1)
    return C


def insert_step_ref(space, rows, graph, K0, search):
    """The graph [n + b, R] after the b new rows ``rows[n:]`` are linked into ``graph`` [n, R].  ``search(q, c, graph)`` ->
    (scores [b, K0], idx [b, K0]): the index's own search of the new rows over the graph as it stands, k = ef = K0."""
    rows = np.asarray(rows, dtype=np.float32)
    graph = np.asarray(graph, dtype=np.int64)
    n, R = graph.shape
    old_s, old_i = search(rows[n:], rows[:n], graph)
    C = candidates_ref(space, rows, n, old_s, old_i, K0)
    F, _, st = insert_prune(C, graph)
    assert not st.any()
    G = np.concatenate([graph, F], axis=0)
    targets, lims, ids = incoming(F, n)
    G, st = link_reverse(space, rows, G, targets, lims, ids)
    assert not (st & ~LINK_ST_CUT).any()
    return G


def insert_ref(space, rows, graph, new_rows, K0, R, insert_batch, width, max_iters, entries=None, seeded=None, dead=None):
    """The graph after ``new_rows`` are inserted into ``graph`` [n, R] over ``rows`` [n, d], ``insert_batch`` rows at a time, each
    sub-batch over the graph with the earlier ones linked in.  Entry mode: ``entries`` (shared), or ``seeded`` = dict(centroids,
    n_probe, seeds) — the two forms of the index's search, k = ef = K0.  ``dead`` bool [n]: tombstones route and are not returned."""
    assert (entries is None) != (seeded is None)
    rows = np.concatenate([np.asarray(rows, dtype=np.float32), np.asarray(new_rows, dtype=np.float32)], axis=0)
    G = np.asarray(graph, dtype=np.int64)
    n0 = G.shape[0]
    assert G.shape[1] == R

    def search(q, c, g):
        ids = None
        if dead is not None and np.asarray(dead).any():
            ids = np.arange(c.shape[0], dtype=np.int64)
            ids[:n0][np.asarray(dead, dtype=bool)] = -1
        if entries is not None:
            return gc.graph_search_ref(space, q, c, g, entries, K0, width, max_iters, K0, row_ids=ids)[:2]
        return gsc.graph_search_seeded_ref(space, q, c, g, K0, width, max_iters, K0, row_ids=ids, **seeded)[:2]

    for a in range(n0, rows.shape[0], insert_batch):
        b = min(insert_batch, rows.shape[0] - a)
        G = insert_step_ref(space, rows[:a + b], G, K0, search)
    return G


# ------------------------------------------------------------------------------------------------- quality, on the restatement
def manifold_rows(rng, n, d, latent=16, lift=None):
    """tools/bench_graph.py's ``manifold`` corpus: standard-normal latents through a fixed [latent, d] map, plus 0.05 noise."""
    lift = rng.standard_normal((latent, d)) if lift is None else lift
    return (rng.standard_normal((n, latent)) @ lift + 0.05 * rng.standard_normal((n, d))).astype(np.float32), lift


def knn_graph_prefiltered(space, c, K0, keep=None):
    """graph_cases.knn_graph_ref without the N^2 exact scores: float64 BLAS scores pick ``keep`` (default 2 K0 + 8) candidates a
    row, the exact search ranks those.  Safe when a row's last candidate is worse than its (K0 + 1)-th by far more than a rounding — every row left
    out is no better than that candidate up to the rounding of a float32 score — which is asserted, not assumed."""
    c = np.asarray(c, dtype=np.float32)
    N = c.shape[0]
    keep = min(N, 2 * K0 + 8 if keep is None else keep)
    x = c.astype(np.float64)
    if space == "cosine":
        x = x / np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-8)
    approx = x @ x.T
    if space == "l2":
        sq = (x * x).sum(1)
        approx = -(sq[:, None] + sq[None, :] - 2 * approx)
    part = np.argpartition(-approx, keep - 1, axis=1)[:, :keep] if keep < N else np.tile(np.arange(N), (N, 1))
    S, I, _ = list_topk_ref(space, c, c, [np.sort(r) for r in part], keep)
    if keep < N:
        gap = (S[:, keep - 1] - S[:, K0]) * (1 if space == "l2" else -1)      # float32 rounds a score by 6e-8 of it
        assert (gap > 1e-5 * np.maximum(1.0, np.abs(S[:, K0]))).all(), "the prefilter's margin is too thin for these rows"
    G0 = np.full((N, K0), -1, dtype=np.int64)
    for i in range(N):
        row = I[i, :K0 + 1]
        at = np.nonzero(row == i)[0]
        G0[i] = np.delete(row, at[0] if at.size else K0)
    return G0


def build_graph_prefiltered(space, c, K0, R):
    G0 = knn_graph_prefiltered(space, c, K0)
    return gc.merge_reverse(gc.forward_lists(G0, gc.detours(G0), R))


def zero_in_degree_share(graph, first):
    """The share of the rows ``first ..`` that no row's edge list holds."""
    graph = np.asarray(graph)
    seen = np.zeros((graph.shape[0],), dtype=bool)
    seen[graph[graph >= 0]] = True
    return float((~seen[first:]).mean())
