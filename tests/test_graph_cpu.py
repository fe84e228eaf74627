"""CPU checks of the graph index (include/tsim.h tsim_graph_search, tsim_graph_search_lds_bytes, tsim_graph_prune): the entries
validate their arguments before any launch, the LDS function is host arithmetic, and the restatement of tests/graph_cases.py
agrees with the list oracle it is built on and with its own literal-loop form."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from graph_cases import (ST_ITERS, ST_ROW, degree_params, detours, detours_loop, forward_lists, graph_search_ref, knn_graph_ref,
                         merge_reverse, merge_reverse_loop, reachable, table_slots)
from list_cases import header_define, list_topk_ref, same_bits
from text_similarity_amd import _lib

EINVAL = 1
COS, DOT, L2 = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from text_similarity_amd.build import build
        build(verbose=False)
    return _lib.lib()


def test_symbols_and_constants(lib):
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    names = {"tsim_graph_search", "tsim_graph_search_lds_bytes", "tsim_graph_prune"}
    assert all(hasattr(cdll, n) for n in names) and names <= set(_lib.DECLARED_SYMBOLS)
    assert (header_define("TSIM_GRAPH_ST_ROW"), header_define("TSIM_GRAPH_ST_ITERS")) == (_lib.GRAPH_ST_ROW, _lib.GRAPH_ST_ITERS) \
        == (ST_ROW, ST_ITERS) == (1, 2)
    assert header_define("TSIM_GRAPH_MAX_TABLE_BYTES") == _lib.GRAPH_MAX_TABLE_BYTES == 128 << 10
    assert header_define("TSIM_GRAPH_STATIC_LDS_BYTES") == _lib.GRAPH_STATIC_LDS_BYTES
    # a workgroup's LDS stays inside the 160 KiB of a CU
    assert _lib.GRAPH_STATIC_LDS_BYTES + _lib.GRAPH_MAX_TABLE_BYTES <= 160 << 10
    from text_similarity_amd import ops
    assert (header_define("TSIM_GRAPH_MAX_DEGREE"), header_define("TSIM_GRAPH_MAX_ENTRIES"), header_define("TSIM_GRAPH_MAX_WIDTH"),
            header_define("TSIM_GRAPH_MAX_EF"), header_define("TSIM_GRAPH_PRUNE_MAX_K0")) == \
        (ops.GRAPH_MAX_DEGREE, ops.GRAPH_MAX_ENTRIES, ops.GRAPH_MAX_WIDTH, ops.GRAPH_MAX_EF, ops.GRAPH_PRUNE_MAX_K0) == (64, 256, 4, 1024, 128)


def _search(lib, p, **kw):
    a = dict(space=COS, eq=p, ldq=64, Q=4, rows=p, ldr=64, N=100, d=64, graph=p, R=8, entries=p, E=4, ids=None, ef=32, width=4,
             iters=8, k=10, out_s=p, out_i=p, idx_offset=0, status=None, stream=None)
    a.update(kw)
    return lib.tsim_graph_search(a["space"], a["eq"], a["ldq"], a["Q"], a["rows"], a["ldr"], a["N"], a["d"], a["graph"], a["R"],
                                 a["entries"], a["E"], a["ids"], a["ef"], a["width"], a["iters"], a["k"], a["out_s"], a["out_i"],
                                 a["idx_offset"], a["status"], a["stream"])


def test_search_argument_validation_before_any_launch(lib):
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    for name in ("eq", "rows", "graph", "entries", "out_s", "out_i"):
        assert _search(lib, p, **{name: None}) == EINVAL, name
        assert b"null pointer" in lib.tsim_last_error()
    for R in (0, -1, 65):
        assert _search(lib, p, R=R) == EINVAL and b"degree" in lib.tsim_last_error()
    assert _search(lib, p, ef=9, k=10) == EINVAL and b"ef=9" in lib.tsim_last_error()       # ef < k
    assert _search(lib, p, ef=1025) == EINVAL and b"ef=1025" in lib.tsim_last_error()
    for w in (0, 5):
        assert _search(lib, p, width=w) == EINVAL and b"width" in lib.tsim_last_error()
    for E in (0, 257):
        assert _search(lib, p, E=E) == EINVAL and b"entry points" in lib.tsim_last_error()
    for k in (0, 1025):
        assert _search(lib, p, k=k, ef=1024) == EINVAL
    assert _search(lib, p, iters=0) == EINVAL
    for d in (0, 769):
        assert _search(lib, p, d=d, ldq=1024, ldr=1024) == EINVAL
    assert _search(lib, p, space=L2, d=768, ldq=768, ldr=768) == EINVAL and b"Euclidean" in lib.tsim_last_error()
    assert _search(lib, p, ldq=63) == EINVAL and _search(lib, p, ldr=63) == EINVAL
    assert _search(lib, p, space=3) == EINVAL and _search(lib, p, space=-1) == EINVAL
    assert _search(lib, p, Q=0) == EINVAL and _search(lib, p, N=0) == EINVAL
    assert _search(lib, p, N=(1 << 31) - 64) == EINVAL
    # a visit bound that does not fit the table in LDS: 4 + iters * 4 * 8 rows against 16 384
    fits = (16384 - 4) // 32
    assert _search(lib, p, iters=fits + 1) == EINVAL
    msg = lib.tsim_last_error()
    assert b"visit" in msg and b"max_iters" in msg and b"131072" in msg
    assert _search(lib, p, iters=1 << 30) == EINVAL and _search(lib, p, iters=(1 << 31) - 1, R=64, E=256) == EINVAL


def test_prune_argument_validation_before_any_launch(lib):
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    f = lib.tsim_graph_prune
    assert f(None, 10, 8, 4, p, None, None) == EINVAL and f(p, 10, 8, 4, None, None, None) == EINVAL
    assert b"null pointer" in lib.tsim_last_error()
    assert f(p, 0, 8, 4, p, None, None) == EINVAL
    for K0 in (0, 129):
        assert f(p, 10, K0, 1, p, None, None) == EINVAL and b"K0" in lib.tsim_last_error()
    for K0, R in ((8, 0), (8, 9), (128, 65)):
        assert f(p, 10, K0, R, p, None, None) == EINVAL and b"R=" in lib.tsim_last_error()


def test_lds_bytes_function(lib):
    f = lib.tsim_graph_search_lds_bytes
    static, cap = _lib.GRAPH_STATIC_LDS_BYTES, _lib.GRAPH_MAX_TABLE_BYTES
    for bad in ((0, 8, 4, 8), (257, 8, 4, 8), (4, 0, 4, 8), (4, 65, 4, 8), (4, 8, 0, 8), (4, 8, 5, 8), (4, 8, 4, 0), (4, 8, 4, -1)):
        assert f(*bad) == 0, bad
    Es, Rs, Ws, Is = (1, 2, 64, 256), (1, 8, 33, 64), (1, 2, 3, 4), (1, 2, 10, 63, 64, 65, 1000, 1 << 20, (1 << 31) - 1)
    val = {c: f(*c) for c in itertools.product(Es, Rs, Ws, Is)}
    for c, v in val.items():
        E, R, w, it = c
        need = 2 * (E + it * w * R)
        if need <= cap // 4:
            assert v == static + 4 * table_slots(E, R, w, it), c      # a power of two >= twice the visit bound, at least 64
            assert (v - static) // 4 >= max(need, 64) and v <= static + cap
        else:
            assert v > static + cap, c                                # refused by the call
    for axis, grid in enumerate((Es, Rs, Ws, Is)):
        for c in val:
            i = grid.index(c[axis])
            if i + 1 < len(grid):
                up = c[:axis] + (grid[i + 1],) + c[axis + 1:]
                assert val[up] >= val[c], (c, up)
    # a small search leaves room for several workgroups a CU
    assert f(64, 32, 4, 8) <= (160 << 10) // 4
    from text_similarity_amd import ops
    for E, R, w in ((1, 1, 1), (64, 64, 4), (256, 33, 3)):
        m = ops.graph_max_iters(E, R, w)
        assert f(E, R, w, m) <= static + cap < f(E, R, w, m + 1)


def test_degree_params():
    from text_similarity_amd.graph_index import degree_params as dp
    for M, efc in ((16, 0), (64, 400), (1, 0), (1, 1), (8, 20), (8, 500), (40, 0), (0, 0)):
        assert dp(M, efc) == degree_params(M if M > 0 else 16, efc)
    assert dp(64, 400) == (64, 128) and dp(16, 0) == (32, 64) and dp(8, 20) == (16, 20) and dp(8, 4) == (16, 16)


def _connected_graph(rng, N, R):
    """A ring (row r -> r + 1) plus random edges, with padding, repeats and self-loops: every row is reachable from any."""
    g = rng.integers(0, N, size=(N, R))
    g[:, 0] = (np.arange(N) + 1) % N
    if R > 2:
        g[:, 1] = np.arange(N)                    # a self-loop
        g[::3, 2] = -1                            # padding
    return g


@pytest.mark.parametrize("space", ["cosine", "dot", "l2"])
def test_restatement_is_exact_when_the_beam_holds_every_row(space):
    rng = np.random.default_rng(5)
    N, d, R, Q, k = 150, 20, 5, 3, 12
    c = rng.standard_normal((N, d)).astype(np.float32)
    c[40] = c[7]                                  # duplicate rows: the tie rule decides
    q = rng.standard_normal((Q, d)).astype(np.float32)
    q[1] = c[7]
    g = _connected_graph(rng, N, R)
    for width, entries in ((1, [3]), (4, [9, 9, -1, 100])):
        s, i, st, visits = graph_search_ref(space, q, c, g, entries, ef=N, width=width, max_iters=N, k=k, return_visits=True)
        rs, ri, _ = list_topk_ref(space, q, c, np.arange(N), k)
        assert (i == ri).all() and same_bits(s, rs) and (st == 0).all() and (visits == N).all()
    assert len(reachable(g, [3], N)) == N
    # the cap cuts the search: status, and a result that is still a subset of the exact one with its scores
    s, i, st = graph_search_ref(space, q, c, g, [3], ef=16, width=1, max_iters=2, k=k)
    assert (st == ST_ITERS).all()
    full_s, full_i, _ = list_topk_ref(space, q, c, np.arange(N), N)
    for j in range(Q):
        for t in range(k):
            if i[j, t] >= 0:
                at = np.nonzero(full_i[j] == i[j, t])[0][0]
                assert same_bits(s[j, t:t + 1], full_s[j, at:at + 1])
    # an id >= N: the status bit, never a row; tombstones are traversed and not returned; idx_offset shifts
    g2 = g.copy()
    g2[:, -1] = N + 5
    ids = np.arange(N, dtype=np.int32) * 2
    dead = ri[:, :3].reshape(-1)
    ids[dead] = -1
    s, i, st = graph_search_ref(space, q, c, g2, [3], ef=N, width=2, max_iters=N, k=k, row_ids=ids)
    assert (st == ST_ROW).all() and not np.isin(i, -1).any() and (i % 2 == 0).all() and not np.isin(i // 2, dead).any()
    s, i, st = graph_search_ref(space, q, c, g, [3], ef=N, width=2, max_iters=N, k=k, idx_offset=1000)
    assert (i == ri + 1000).all()


def test_restatement_drops_nan_scores_and_keeps_the_rows_visited():
    rng = np.random.default_rng(6)
    N, d = 30, 8
    c = rng.standard_normal((N, d)).astype(np.float32)
    c[4, 2] = np.nan
    q = rng.standard_normal((2, d)).astype(np.float32)
    q[1, 0] = np.nan
    g = _connected_graph(rng, N, 4)
    s, i, st, visits = graph_search_ref("dot", q, c, g, [0], ef=N, width=3, max_iters=N, k=N, return_visits=True)
    assert visits[0] == N and 4 not in i[0] and (i[0] >= 0).sum() == N - 1      # row 4 was expanded all the same: the ring passes it
    assert (i[1] == -1).all() and np.isneginf(s[1]).all() and st[1] == 0 and visits[1] == 1


def test_prune_and_merge_restatements_agree_with_the_literal_loops():
    rng = np.random.default_rng(8)
    for N, K0, R in ((1, 1, 1), (2, 1, 1), (2, 3, 2), (40, 8, 4), (65, 12, 5), (30, 33, 33)):
        G0 = rng.integers(-1, N + 2, size=(N, K0))         # padding, ids >= N, repeats
        D = detours(G0)
        assert (D == detours_loop(G0)).all(), (N, K0)
        F = forward_lists(G0, D, R)
        assert F.shape == (N, R) and ((F >= -1) & (F < N)).all()
        assert (merge_reverse(F) == merge_reverse_loop(F)).all(), (N, K0, R)
    # a real kNN graph: no self edge, rank order, and the detour count of the best neighbour is 0
    c = rng.standard_normal((50, 6)).astype(np.float32)
    c[9] = c[3]
    G0 = knn_graph_ref("l2", c, 10)
    assert (G0 != np.arange(50)[:, None]).all() and G0[3, 0] == 9 and G0[9, 0] == 3
    D = detours(G0)
    assert (D == detours_loop(G0)).all() and (D[:, 0] == 0).all() and (D <= np.arange(10)[None, :]).all()
    F = forward_lists(G0, D, 6)
    G = merge_reverse(F)
    assert (G == merge_reverse_loop(F)).all()
    for j in range(50):
        row = G[j][G[j] >= 0]
        assert len(set(row.tolist())) == len(row) and j not in row
