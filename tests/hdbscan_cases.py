"""Test-local restatement of HDBSCAN (include/tsim.h "HDBSCAN"), shared by tests/test_hdbscan_cpu.py, tests/test_mst_prim_gpu.py,
tests/test_mst_far_rows_gpu.py, tests/test_hdbscan_gpu.py, tools/make_hdbscan_golden.py and tools/fuzz_hdbscan.py.

``mst_ref`` is the literal Prim loop of tsim_mst_prim on squared distances, d2 from list_cases.pair_scores("l2", ...) — the
float32 value the Euclidean search returns for the pair.  ``core2_ref`` is the squared core distance: the min_samples-th smallest
d2 of a row against every row, itself included.  ``tree_labels_ref`` is the literal tree stage of tsim_hdbscan_tree_labels
(cluster_selection_method="eom", allow_single_cluster=False, cluster_selection_epsilon=0).  tests/golden/hdbscan.npz pins
``tree_labels_ref(mst_ref(...))`` against scikit-learn's labels on separated blobs; elsewhere this file is the definition."""
import functools
import os

import numpy as np

from list_cases import pair_scores

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hdbscan.npz")
# (n, d, clusters, min_cluster_size, min_samples, seed) of the golden cases
GOLDEN_CASES = ((300, 16, 4, 10, 10, 11), (500, 48, 6, 15, 5, 12), (257, 33, 3, 5, 5, 13), (400, 64, 5, 8, 3, 14))


def d2_row(rows, a):
    """float32 [N]: d2(a, j) for every row j, with row a as the query"""
    n = rows.shape[0]
    return pair_scores("l2", rows, rows, np.full((n,), a, dtype=np.int64), np.arange(n, dtype=np.int64))


def core2_ref(rows, min_samples):
    """float32 [N]: the min_samples-th smallest squared distance of every row to the rows, itself included"""
    rows = np.asarray(rows, dtype=np.float32)
    if rows.shape[0] > 1000:        # (the same bits from the blocked matrix: d2 is symmetric)
        up = d2_upper(rows)
        full = np.where(np.arange(rows.shape[0])[:, None] <= np.arange(rows.shape[0])[None, :], up, up.T)
        return np.sort(full, axis=1)[:, min_samples - 1].copy()
    return np.array([np.sort(d2_row(rows, a))[min_samples - 1] for a in range(rows.shape[0])], dtype=np.float32)


def mst_ref(rows, core2=None):
    """(from int32 [N-1], to int32 [N-1], w2 float32 [N-1]): Prim from row 0 on w(a, b) = max(d2(a, b), core2[a], core2[b])."""
    rows = np.asarray(rows, dtype=np.float32)
    n = rows.shape[0]
    best = np.full((n,), np.inf, dtype=np.float32)
    frm = np.full((n,), -1, dtype=np.int32)
    free = np.ones((n,), dtype=bool)
    free[0] = False
    cur = 0
    out_f = np.empty((max(n - 1, 0),), dtype=np.int32)
    out_t = np.empty((max(n - 1, 0),), dtype=np.int32)
    out_w = np.empty((max(n - 1, 0),), dtype=np.float32)
    for t in range(n - 1):
        w = d2_row(rows, cur)
        if core2 is not None:
            w = np.where(core2[cur] > w, core2[cur], w)
            w = np.where(core2 > w, core2, w).astype(np.float32)
        upd = free & (w < best)                 # strict: the earlier endpoint keeps a tie, a NaN never updates
        best[upd] = w[upd]
        frm[upd] = cur
        key = np.where(free, best, np.float32(np.inf))
        cand = np.flatnonzero(free & (key == key.min()))     # (all +inf: the lowest free row)
        nxt = int(cand[0])
        out_f[t], out_t[t], out_w[t] = frm[nxt], nxt, best[nxt]
        free[nxt] = False
        cur = nxt
    return out_f, out_t, out_w


def d2_upper(rows, threads=8, qb=16, cb=128):
    """float32 [N, N] with d2(a, b) for b >= a - a % cb (the upper triangle and a little more; the rest is 0): the same bits as
    d2_row, made in blocks on several threads for the one test with thousands of rows (tests/test_mst_far_rows_gpu.py).  Lane l
    adds the squared differences of elements l, l + 64, ...; the xor butterfly's lane 0 is the halving tree below, because a + b
    and b + a are the same float64.  d2 is symmetric bit for bit: (a - b)^2 == (b - a)^2."""
    from concurrent.futures import ThreadPoolExecutor
    from l2_cases import _lanes
    rows = np.asarray(rows, dtype=np.float32)
    n, d = rows.shape
    lanes = np.ascontiguousarray(np.moveaxis(_lanes(rows, d), -2, 0))      # [ceil(d / 64), N, 64] float64
    out = np.zeros((n, n), dtype=np.float32)

    def work(a):
        b = min(a + qb, n)
        for c0 in range(a - a % cb, n, cb):
            c1 = min(c0 + cb, n)
            diff = lanes[0, a:b, None, :] - lanes[0, None, c0:c1, :]
            part = diff * diff
            for i in range(1, lanes.shape[0]):
                diff = lanes[i, a:b, None, :] - lanes[i, None, c0:c1, :]
                part = part + diff * diff
            h = 32
            while h >= 1:
                part = part[..., :h] + part[..., h:2 * h]
                h //= 2
            out[a:b, c0:c1] = part[..., 0]

    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, range(0, n, qb)))
    return out


def mst_ref_blocked(rows, core2=None):
    """mst_ref with d2 from d2_upper: the same loop, the same results (tests/test_hdbscan_cpu.py compares them)"""
    rows = np.asarray(rows, dtype=np.float32)
    n = rows.shape[0]
    up = d2_upper(rows)
    j = np.arange(n)
    best = np.full((n,), np.inf, dtype=np.float32)
    frm = np.full((n,), -1, dtype=np.int32)
    free = np.ones((n,), dtype=bool)
    free[0] = False
    cur = 0
    out_f, out_t = np.empty((n - 1,), dtype=np.int32), np.empty((n - 1,), dtype=np.int32)
    out_w = np.empty((n - 1,), dtype=np.float32)
    for t in range(n - 1):
        w = np.where(j < cur, up[:, cur], up[cur, :])
        if core2 is not None:
            w = np.where(core2[cur] > w, core2[cur], w)
            w = np.where(core2 > w, core2, w).astype(np.float32)
        upd = free & (w < best)
        best[upd] = w[upd]
        frm[upd] = cur
        key = np.where(free, best, np.float32(np.inf))
        nxt = int(np.flatnonzero(free & (key == key.min()))[0])
        out_f[t], out_t[t], out_w[t] = frm[nxt], nxt, best[nxt]
        free[nxt] = False
        cur = nxt
    return out_f, out_t, out_w


def w_matrix(rows, core2=None):
    """float32 [N, N]: w(a, b) with row a as the query (the diagonal is max(0, core2[a]))"""
    rows = np.asarray(rows, dtype=np.float32)
    w = np.stack([d2_row(rows, a) for a in range(rows.shape[0])])
    if core2 is not None:
        w = np.maximum(w, np.maximum(core2[:, None], core2[None, :]))
    return w


def tree_labels_ref(frm, to, w2, n, min_cluster_size):
    """(labels int32 [N], n_clusters), or None where tsim_hdbscan_tree_labels returns TSIM_EINVAL (no spanning tree)."""
    frm, to = np.asarray(frm, dtype=np.int64), np.asarray(to, dtype=np.int64)
    w2 = np.asarray(w2, dtype=np.float32)
    assert frm.shape == to.shape == w2.shape == (n - 1,) and min_cluster_size >= 2
    # 1. single linkage: edges by (w2 asc, step asc); merge k is node n + k = (component of from, component of to)
    order = np.argsort(np.where(w2 == 0, np.float32(0), w2), kind="stable")
    uf = list(range(n))
    node_of = list(range(n))
    left, right, dist, size = [], [], [], []

    def find(x):
        while uf[x] != x:
            uf[x] = uf[uf[x]]
            x = uf[x]
        return x

    def count(node):
        return 1 if node < n else size[node - n]

    for k, e in enumerate(order):
        a, b = int(frm[e]), int(to[e])
        if not (0 <= a < n and 0 <= b < n):
            return None
        ra, rb = find(a), find(b)
        if ra == rb:
            return None
        na, nb = node_of[ra], node_of[rb]
        left.append(na), right.append(nb)
        with np.errstate(invalid="ignore"):
            dist.append(float(np.sqrt(np.float64(w2[e]))))
        size.append(count(na) + count(nb))
        uf[rb] = ra
        node_of[ra] = n + k
    labels = np.full((n,), -1, dtype=np.int32)
    if n == 1:
        return labels, 0

    def bfs(top):
        out, h = [top], 0
        while h < len(out):
            if out[h] >= n:
                out += [left[out[h] - n], right[out[h] - n]]
            h += 1
        return out

    # 2. condensed tree: rows (parent cluster, child, lambda, size); clusters are numbered from n, the root first
    root = 2 * n - 2
    relabel = {root: n}
    next_label = n + 1
    ignore = set()
    cond = []
    for node in bfs(root):
        if node < n or node in ignore:
            continue
        l, r, d = left[node - n], right[node - n], dist[node - n]
        lam = 1.0 / d if d > 0.0 else np.inf
        lc, rc, me = count(l), count(r), relabel[node]
        for child, cc, other in ((l, lc, rc), (r, rc, lc)):
            if lc >= min_cluster_size and rc >= min_cluster_size:
                relabel[child] = next_label
                next_label += 1
                cond.append((me, relabel[child], lam, cc))
            elif cc < min_cluster_size:
                for s in bfs(child):
                    if s < n:
                        cond.append((me, s, lam, 1))
                    ignore.add(s)
            else:
                relabel[child] = me
        # (one child small, one large: the order of the two branches above does not matter — the large one adds no row)
    # 3. stability, float64, in row order
    C = next_label - n
    birth = np.zeros((C,), dtype=np.float64)
    stab = np.zeros((C,), dtype=np.float64)
    parent = np.full((C,), -1, dtype=np.int64)
    kids = [[] for _ in range(C)]
    for p, c, lam, _ in cond:
        if c >= n:
            birth[c - n] = lam
            parent[c - n] = p - n
            kids[p - n].append(c - n)
    birth[0] = 0.0
    with np.errstate(invalid="ignore"):
        for p, c, lam, sz in cond:
            stab[p - n] += (np.float64(lam) - birth[p - n]) * np.float64(sz)
        # 4. selection
        selected = np.ones((C,), dtype=bool)
        selected[0] = False
        for c in range(C - 1, 0, -1):
            subtree = stab[kids[c][0]] + stab[kids[c][1]] if kids[c] else np.float64(0.0)
            if subtree > stab[c]:
                selected[c] = False
                stab[c] = subtree
            else:
                todo = list(kids[c])
                while todo:
                    s = todo.pop()
                    selected[s] = False
                    todo += kids[s]
    # 5. labels
    label_of = np.full((C,), -1, dtype=np.int32)
    n_sel = 0
    for c in range(1, C):
        if selected[c]:
            label_of[c] = n_sel
            n_sel += 1
        else:
            label_of[c] = label_of[parent[c]]
    for p, c, _, _ in cond:
        if c < n:
            labels[c] = label_of[p - n]
    return labels, n_sel


def hdbscan_ref(rows, min_cluster_size, min_samples=None):
    """(labels, n_clusters, (from, to, w2), core2) of the whole restatement on float32 rows (metric="cosine": hand in the
    float32 unit rows the device made)"""
    rows = np.asarray(rows, dtype=np.float32)
    core2 = core2_ref(rows, min_cluster_size if min_samples is None else min_samples)
    edges = mst_ref(rows, core2)
    labels, n_clusters = tree_labels_ref(*edges, rows.shape[0], min_cluster_size)
    return labels, n_clusters, edges, core2


# ------------------------------------------------------------------------------------------------- cases
def blobs(n, d, clusters, seed, centre_scale=4.0):
    """Gaussian blobs: centres normal * centre_scale, one spread per blob from U(0.5, 1.5), the first tenth of the rows uniform
    noise in [-8, 8]; float32 [n, d]."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((clusters, d)) * centre_scale
    spread = rng.uniform(0.5, 1.5, size=clusters)
    which = rng.integers(0, clusters, size=n)
    x = centres[which] + spread[which, None] * rng.standard_normal((n, d))
    m = n // 10
    x[:m] = rng.uniform(-8.0, 8.0, size=(m, d))
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def golden_case(i):
    """(rows, min_cluster_size, min_samples) of golden case i, regenerated (tools/make_hdbscan_golden.py stores the same rows)"""
    n, d, clusters, mcs, ms, seed = GOLDEN_CASES[i]
    rows = blobs(n, d, clusters, seed)
    rows.setflags(write=False)
    return rows, mcs, ms


def small_cases():
    """name -> (rows, min_cluster_size, min_samples): the edges of the tree stage"""
    rng = np.random.default_rng(77)
    out = {}
    for n in (2, 3, 10):
        out[f"n{n}"] = (rng.standard_normal((n, 5)).astype(np.float32), 2, min(2, n))
    out["all_noise"] = (rng.uniform(-8, 8, size=(60, 12)).astype(np.float32), 25, 5)
    # (more than half the rows: no split has two children of that size, and the root itself is never selected)
    out["one_blob"] = (rng.standard_normal((80, 6)).astype(np.float32), 45, 5)
    out["mcs2"] = (blobs(90, 4, 3, 5), 2, 2)
    out["n_below_mcs"] = (rng.standard_normal((7, 3)).astype(np.float32), 10, 3)
    out["grid"] = (np.stack(np.meshgrid(np.arange(9), np.arange(8)), -1).reshape(-1, 2).astype(np.float32), 4, 3)
    dup = np.repeat(rng.standard_normal((6, 8)).astype(np.float32) * 3, 12, axis=0)
    out["duplicates"] = (dup[rng.permutation(dup.shape[0])], 5, 4)
    two = np.concatenate([blobs(70, 5, 2, 9), np.repeat(rng.standard_normal((1, 5)).astype(np.float32) + 9, 15, axis=0)])
    out["blobs_and_duplicates"] = (two, 6, 3)
    return out
