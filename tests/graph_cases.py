"""Test-local restatement of the graph index (include/tsim.h tsim_graph_search / tsim_graph_prune and
text_similarity_amd/graph_index.py), numpy only, shared by tests/test_graph_cpu.py, tests/test_graph_gpu.py,
tests/test_graph_index_gpu.py and tools/fuzz_graph.py.  Scores and the order of a list are NOT restated here: they come from
tests/list_cases.py (pair_scores, rank_list), so the beam ranks exactly as the list search does."""
import numpy as np

from list_cases import pair_scores, rank_list, list_topk_ref  # noqa: F401  (list_topk_ref: re-exported for the tests)

ST_ROW, ST_ITERS = 1, 2      # include/tsim.h TSIM_GRAPH_ST_ROW / TSIM_GRAPH_ST_ITERS


def table_slots(E, R, width, max_iters):
    """Slots of the visited table: the smallest power of two >= 2 (E + max_iters width R), at least 64."""
    s = 64
    while s < 2 * (E + max_iters * width * R):
        s <<= 1
    return s


def _order(space, rows, scores):
    """Positions of (rows, scores) in beam order: rank_list's key, without its padding."""
    key = scores.astype(np.float64) if space == "l2" else -scores.astype(np.float64)
    return np.lexsort((rows, key))


def graph_search_ref(space, q, c, graph, entries, ef, width, max_iters, k, row_ids=None, idx_offset=0, return_visits=False):
    """(scores [Q, k] float32, idx [Q, k] int64, status [Q] int32): the search as include/tsim.h states it.  ``visits`` (with
    return_visits): rows scored per query."""
    q = np.asarray(q, dtype=np.float32)
    c = np.asarray(c, dtype=np.float32)
    graph = np.asarray(graph, dtype=np.int64)
    entries = np.asarray(entries, dtype=np.int64).reshape(-1)
    Q, N = q.shape[0], c.shape[0]
    S = np.empty((Q, k), dtype=np.float32)
    I = np.empty((Q, k), dtype=np.int64)
    st = np.zeros((Q,), dtype=np.int32)
    visits = np.zeros((Q,), dtype=np.int64)
    for j in range(Q):
        visited, expanded = set(), set()
        beam_r = np.zeros((0,), np.int64)
        beam_s = np.zeros((0,), np.float32)

        def offer(ids):
            nonlocal beam_r, beam_s
            ids = np.asarray(ids, dtype=np.int64)
            if (ids >= N).any():
                st[j] |= ST_ROW
            new = []
            for r in ids[(ids >= 0) & (ids < N)].tolist():
                if r not in visited:
                    visited.add(r)
                    new.append(r)
            new = np.asarray(new, dtype=np.int64)
            visits[j] += new.shape[0]
            sc = pair_scores(space, q, c, np.full(new.shape, j, dtype=np.int64), new)
            ok = ~np.isnan(sc)
            rows = np.concatenate([beam_r, new[ok]])
            scores = np.concatenate([beam_s, sc[ok]])
            o = _order(space, rows, scores)[:ef]
            beam_r, beam_s = rows[o], scores[o]

        offer(entries)
        it = 0
        while True:
            parents = [r for r in beam_r.tolist() if r not in expanded][:width]
            if not parents:
                break
            if it >= max_iters:
                st[j] |= ST_ITERS
                break
            expanded.update(parents)
            offer(graph[parents].reshape(-1))
            it += 1
        live = np.ones(beam_r.shape, dtype=bool) if row_ids is None else np.asarray(row_ids)[beam_r] >= 0
        rows, scores = beam_r[live][:k], beam_s[live][:k]
        S[j], I[j] = rank_list(space, rows, scores, k)      # (already in order: rank_list pads)
        if row_ids is not None:
            I[j, :rows.shape[0]] = np.asarray(row_ids)[rows]
        else:
            I[j, :rows.shape[0]] += idx_offset
    return (S, I, st, visits) if return_visits else (S, I, st)


def reachable(graph, entries, N):
    """Rows reachable from the entry points along usable edges (host BFS), sorted."""
    graph = np.asarray(graph, dtype=np.int64)
    seen = np.zeros((N,), dtype=bool)
    front = np.unique(np.asarray(entries, dtype=np.int64))
    front = front[(front >= 0) & (front < N)]
    seen[front] = True
    while front.size:
        nxt = np.unique(graph[front].reshape(-1))
        nxt = nxt[(nxt >= 0) & (nxt < N)]
        nxt = nxt[~seen[nxt]]
        seen[nxt] = True
        front = nxt
    return np.nonzero(seen)[0]


def random_graph(rng, N, R, beyond=True, island=0):
    """graph int32 [N, R] with everything a search has to survive: a ring in column 0 (so a graph without an island is connected),
    random edges with repeats, self-loops, padding, and (``beyond``) ids >= N.  ``island``: that many rows (returned second) that no
    edge points to — unreachable unless they are entry points."""
    g = rng.integers(0, N, size=(N, R))
    g[:, 0] = (np.arange(N) + 1) % N
    if R > 1:
        g[:, 1] = np.where(rng.random(N) < 0.3, np.arange(N), g[:, 1])       # self-loops
        g[:, -1] = np.where(rng.random(N) < 0.3, g[:, 0], g[:, -1])          # a neighbour twice in one row
        g[:, 1:] = np.where(rng.random((N, R - 1)) < 0.15, -1, g[:, 1:])     # padding
        if beyond:
            g[:, 1:] = np.where(rng.random((N, R - 1)) < 0.02, N + rng.integers(0, 3), g[:, 1:])
    lost = rng.choice(N, size=min(island, max(N - 1, 0)), replace=False) if island else np.zeros((0,), np.int64)
    g[np.isin(g, lost)] = -1
    return g.astype(np.int32), lost


def random_rows(rng, N, d, dup=True):
    """float32 [N, d] standard-normal rows, a tenth of them copies of other rows (the tie rule decides between them)."""
    c = rng.standard_normal((N, d)).astype(np.float32)
    if dup and N > 1:
        n = max(1, N // 10)
        c[rng.choice(N, n, replace=False)] = c[rng.choice(N, n, replace=False)]
    return c


# ------------------------------------------------------------------------------------------------- the build
def knn_graph_ref(space, c, K0):
    """G0 [N, K0] int64: the K0 best OTHER rows of every row by the exact search (k = K0 + 1, the entry equal to the row dropped,
    or the last entry when it is absent), rank order, -1 where fewer exist."""
    c = np.asarray(c, dtype=np.float32)
    N = c.shape[0]
    _, idx, _ = list_topk_ref(space, c, c, np.arange(N), K0 + 1)
    G0 = np.full((N, K0), -1, dtype=np.int64)
    for i in range(N):
        row = idx[i]
        at = np.nonzero(row == i)[0]
        G0[i] = np.delete(row, at[0] if at.size else K0)
    return G0


def detours_loop(G0):
    """D by the definition, literal loops."""
    G0 = np.asarray(G0, dtype=np.int64)
    N, K0 = G0.shape
    D = np.zeros((N, K0), dtype=np.int64)
    for i in range(N):
        for b in range(K0):
            t = G0[i, b]
            if not 0 <= t < N:
                D[i, b] = K0
                continue
            for a in range(b):
                ga = G0[i, a]
                if 0 <= ga < N and t in G0[ga, :b].tolist():
                    D[i, b] += 1
    return D


def detours(G0):
    """D, a node at a time: the first place of G0[i][b] in each neighbour's row by one sorted lookup."""
    G0 = np.asarray(G0, dtype=np.int64)
    N, K0 = G0.shape
    D = np.zeros((N, K0), dtype=np.int64)
    B = max(N, int(G0.max(initial=0)) + 1) + 2
    ar = np.arange(K0)
    for i in range(N):
        g = G0[i]
        ok = (g >= 0) & (g < N)
        nb = np.where(ok[:, None], G0[np.where(ok, g, 0)], -1)                 # [a, c]
        keys = (nb + 1 + ar[:, None] * B).reshape(-1)                          # row a's values live in [a B, (a + 1) B)
        order = np.argsort(keys, kind="stable")
        sk = keys[order]
        want = (g[None, :] + 1 + ar[:, None] * B).reshape(-1)                  # [a, b]
        at = np.minimum(np.searchsorted(sk, want, side="left"), sk.shape[0] - 1)
        first = np.where(sk[at] == want, order[at] % K0, K0).reshape(K0, K0)   # smallest c with nb[a, c] == g[b]
        hit = (first < ar[None, :]) & (ar[:, None] < ar[None, :]) & ok[:, None] & ok[None, :]
        D[i] = np.where(ok, hit.sum(0), K0)
    return D


def forward_lists(G0, D, R):
    """F [N, R]: the R entries of G0[i] of smallest (D, rank), in that order; unusable entries (D == K0) as -1."""
    G0 = np.asarray(G0, dtype=np.int64)
    K0 = G0.shape[1]
    order = np.argsort(D, axis=1, kind="stable")[:, :R]
    F = np.take_along_axis(G0, order, 1)
    return np.where(np.take_along_axis(D, order, 1) < K0, F, -1)


def merge_reverse_loop(F):
    """The final rows, literal loops: the first R distinct ids of F[j][:R/2] ++ Rev[j][:R/2] ++ F[j][R/2:], -1 padded."""
    F = np.asarray(F, dtype=np.int64)
    N, R = F.shape
    h = R // 2
    rev = [[] for _ in range(N)]
    for pos in range(R):
        for i in range(N):
            j = F[i, pos]
            if j >= 0:
                rev[j].append(i)
    G = np.full((N, R), -1, dtype=np.int64)
    for j in range(N):
        out = []
        for x in list(F[j, :h]) + rev[j][:h] + list(F[j, h:]):
            if x >= 0 and x not in out:
                out.append(int(x))
        G[j, :min(R, len(out))] = out[:R]
    return G


def merge_reverse(F):
    """The final rows, vectorised (stable sorts), id for id what merge_reverse_loop gives."""
    F = np.asarray(F, dtype=np.int64)
    N, R = F.shape
    h = R // 2
    dst = F.T.reshape(-1)                                   # edges in (position, source) order
    src = np.tile(np.arange(N), R)
    ok = dst >= 0
    dst, src = dst[ok], src[ok]
    o = np.argsort(dst, kind="stable")
    dst, src = dst[o], src[o]
    start = np.searchsorted(dst, np.arange(N), side="left")
    rank = np.arange(dst.shape[0]) - start[dst]
    Rev = np.full((N, max(h, 1)), -1, dtype=np.int64)
    keep = rank < h
    Rev[dst[keep], rank[keep]] = src[keep]
    cat = np.concatenate([F[:, :h], Rev[:, :h], F[:, h:]], axis=1)
    L = cat.shape[1]
    o = np.argsort(cat, axis=1, kind="stable")
    sv = np.take_along_axis(cat, o, 1)
    dup_sorted = np.zeros_like(sv, dtype=bool)
    dup_sorted[:, 1:] = sv[:, 1:] == sv[:, :-1]
    dup = np.zeros_like(dup_sorted)
    np.put_along_axis(dup, o, dup_sorted, 1)
    good = (cat >= 0) & ~dup
    place = np.cumsum(good, axis=1) - 1
    G = np.full((N, R), -1, dtype=np.int64)
    rows = np.repeat(np.arange(N)[:, None], L, 1)
    sel = good & (place < R)
    G[rows[sel], place[sel]] = cat[sel]
    return G


def build_graph_ref(space, c, K0, R):
    """The index's graph [N, R] for rows ``c``: exact kNN graph, detour pruning, reverse-edge merge."""
    G0 = knn_graph_ref(space, c, K0)
    return merge_reverse(forward_lists(G0, detours(G0), R))


def degree_params(M, ef_construction):
    """(R, K0) of GpuGraphIndex for hnswlib's M and ef_construction."""
    R = min(2 * int(M), 64)
    K0 = min(2 * R, 128) if int(ef_construction) == 0 else min(max(int(ef_construction), R), 128)
    return R, K0
