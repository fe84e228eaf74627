"""CPU checks of the insertion into a built graph (include/tsim_graph_insert.h): the two entries are exported, bound and
validate their arguments before any launch; the new header lists exactly them and each has a case in the new contract test;
the vectorised restatement of tests/graph_insert_cases.py agrees with its literal loops; and, on the restatement alone, an
inserted graph keeps the recall of the rebuilt one.

The quality test: the ``manifold`` corpus of tools/bench_graph.py (16 latent dimensions) scaled down to N = 4096, d = 32, space
'l2' (the cheapest exact score to restate), M = 8 (R = 16, K0 = 32), 16 shared entry points, width 4; the first 2048 rows built
exactly, the other 2048 inserted with insert_batch = 256; 128 fresh queries, ef = 32.  The GPU graph equals the restatement id for
id (tests/test_graph_insert_index_gpu.py), so these are the GPU's numbers too.  The bar: inserted recall@10 >= 0.8 x rebuilt
recall@10 — a substitute for the rebuild that loses more than a fifth of its recall is not one.  Measured (DESIGN.md section 7,
*Insertion*): inserted 0.9664, rebuilt 0.9836, zero-in-degree share of the inserted rows 0.0122."""
import ctypes
import os
import re

import numpy as np
import pytest

import contract_cases as cases
import graph_cases as gc
import graph_insert_cases as gic
import graph_seed_cases as gsc
from list_cases import list_topk_ref
from text_similarity_amd import _lib, ops

EINVAL = 1
COS, DOT, L2 = 0, 1, 2
HDR = os.path.join(os.path.dirname(cases.HDR), "tsim_graph_insert.h")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from text_similarity_amd.build import build
        build(verbose=False)
    return _lib.lib()


def _define(name):
    m = re.search(r"^#define\s+%s\s+(\d+)" % name, open(HDR).read(), re.M)
    assert m, f"{name} is not defined in include/tsim_graph_insert.h"
    return int(m.group(1))


def test_symbols_are_exported_bound_and_outside_the_registry(lib):
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    names = ("tsim_graph_insert_prune", "tsim_graph_link_reverse")
    assert _lib.GRAPH_INSERT_SYMBOLS == names and all(hasattr(cdll, n) for n in names)
    assert not set(names) & set(_lib.DECLARED_SYMBOLS)
    for n in names:
        fn = getattr(lib, n)
        assert fn.restype is ctypes.c_int and fn.argtypes[-1] is ctypes.c_void_p
    assert len(lib.tsim_graph_insert_prune.argtypes) == 10 and len(lib.tsim_graph_link_reverse.argtypes) == 13
    assert _define("TSIM_GRAPH_INSERT_ST_ROW") == ops.GRAPH_INSERT_ST_ROW == gic.INSERT_ST_ROW == 1
    assert (_define("TSIM_GRAPH_LINK_ST_CUT"), _define("TSIM_GRAPH_LINK_ST_ROW"), _define("TSIM_GRAPH_LINK_ST_LIMS")) == \
        (ops.GRAPH_LINK_ST_CUT, ops.GRAPH_LINK_ST_ROW, ops.GRAPH_LINK_ST_LIMS) == (gic.LINK_ST_CUT, gic.LINK_ST_ROW, gic.LINK_ST_LIMS)
    assert _define("TSIM_GRAPH_LINK_POOL") == ops.GRAPH_LINK_POOL == gic.LINK_POOL == 256


def test_the_new_header_lists_the_two_entries_and_each_has_a_contract_case(monkeypatch):
    monkeypatch.setattr(cases, "HDR", HDR)
    ws, st = cases.header_entries()
    assert ws == [] and st == ["tsim_graph_insert_prune", "tsim_graph_link_reverse"]
    import test_graph_insert_contract_gpu as contract
    named = {e for c in contract.CASES for e in c.entries}
    assert named == set(st)
    assert all(c.workspace is None and not c.host_sync for c in contract.CASES)
    monkeypatch.undo()
    assert not set(st) & set(cases.header_entries()[1]), "the entries moved into tsim.h: move their cases into the registry too"


def test_insert_prune_argument_validation_before_any_launch(lib):
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    f = lib.tsim_graph_insert_prune

    def call(cand=p, B=4, K0=8, graph=p, n=10, R=4, out=p, det=None, st=None):
        return f(cand, B, K0, graph, n, R, out, det, st, None)
    for name in ("cand", "graph", "out"):
        assert call(**{name: None}) == EINVAL and b"null pointer" in lib.tsim_last_error(), name
    for kw in (dict(B=0), dict(B=-1), dict(n=0), dict(n=-3), dict(n=(1 << 31) - 64), dict(B=1 << 31), dict(n=(1 << 31) - 70, B=6)):
        assert call(**kw) == EINVAL and b"new rows" in lib.tsim_last_error(), kw
    for K0 in (0, 129):
        assert call(K0=K0, R=1) == EINVAL and b"K0" in lib.tsim_last_error()
    for K0, R in ((8, 0), (8, 9), (128, 65)):
        assert call(K0=K0, R=R) == EINVAL and b"R=" in lib.tsim_last_error()


def test_link_reverse_argument_validation_before_any_launch(lib):
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    f = lib.tsim_graph_link_reverse

    def call(space=COS, rows=p, ld=64, N=100, d=64, graph=p, R=8, targets=p, T=4, lims=p, ids=p, st=None):
        return f(space, rows, ld, N, d, graph, R, targets, T, lims, ids, st, None)
    for name in ("rows", "graph", "targets", "lims", "ids"):
        assert call(**{name: None}) == EINVAL and b"null pointer" in lib.tsim_last_error(), name
    assert call(space=3) == EINVAL and call(space=-1) == EINVAL
    for N in (0, -1, (1 << 31) - 64):
        assert call(N=N) == EINVAL
    for T in (0, -1, 101):
        assert call(T=T) == EINVAL and b"targets" in lib.tsim_last_error()
    for R in (0, -1, 65):
        assert call(R=R) == EINVAL and b"degree" in lib.tsim_last_error()
    for d in (0, 769):
        assert call(d=d, ld=1024) == EINVAL
    assert call(space=L2, d=768, ld=768) == EINVAL and b"Euclidean" in lib.tsim_last_error()
    assert call(ld=63) == EINVAL and b"stride" in lib.tsim_last_error()


def _crafted_prune(rng, n, B, K0, R):
    graph = rng.integers(-1, n + B + 2, size=(n, R))
    cand = rng.integers(-1, n + B + 2, size=(B, K0))                       # padding, ids >= n + B, repeats, batch rows
    near = (rng.integers(0, n + B, size=(B, 1)) + rng.integers(0, 2 * K0, size=(B, K0))) % (n + B)   # local: detours exist
    cand = np.where(rng.random((B, K0)) < 0.7, near, cand)
    cand[::3, 0] = n + np.arange(B)[::3]                                   # the row itself
    return cand, graph


def test_prune_restatement_agrees_with_the_literal_loops():
    rng = np.random.default_rng(11)
    for n, B, K0, R in ((1, 1, 1, 1), (1, 5, 4, 2), (30, 7, 8, 4), (50, 20, 12, 12), (9, 33, 16, 5)):
        cand, graph = _crafted_prune(rng, n, B, K0, R)
        F, D, st = gic.insert_prune(cand, graph)
        F2, D2, st2 = gic.insert_prune_loop(cand, graph)
        assert (F == F2).all() and (D == D2).all() and (st == st2).all(), (n, B, K0, R)
        assert F.shape == (B, R) and ((F >= -1) & (F < n + B)).all() and (st == (cand >= n + B).any(1)).all()
        ok = (cand >= 0) & (cand < n + B)
        assert (D[ok] <= np.broadcast_to(np.arange(K0), cand.shape)[ok]).all() and (D[~ok] == K0).all()


def _crafted_link(rng, N, d, R, T):
    rows = rng.standard_normal((N, d)).astype(np.float32)
    rows[3] = rows[1]                                                      # equal scores, broken by id
    graph = rng.integers(-1, N, size=(N, R))
    graph[0] = -1
    graph[1, R // 2:] = -1
    targets = np.sort(rng.choice(N, size=T, replace=False))
    lens = rng.integers(0, 3 * R, size=T)
    lims = np.concatenate([[0], np.cumsum(lens)])
    ids = rng.integers(-1, N + 1, size=int(lims[-1]))                      # padding, an id >= N, repeats, ids already in the row
    return rows, graph, targets, lims, ids


@pytest.mark.parametrize("space", ["cosine", "dot", "l2"])
def test_link_restatement_agrees_with_the_literal_loops(space):
    rng = np.random.default_rng(12)
    for N, d, R, T in ((4, 3, 1, 1), (20, 5, 4, 20), (40, 9, 7, 11)):
        rows, graph, targets, lims, ids = _crafted_link(rng, N, d, R, T)
        G, st = gic.link_reverse(space, rows, graph, targets, lims, ids)
        G2, st2 = gic.link_reverse_loop(space, rows, graph, targets, lims, ids)
        assert (G == G2).all() and (st == st2).all(), (N, d, R, T)
        rest = np.setdiff1d(np.arange(N), targets)
        assert (G[rest] == graph[rest]).all()
        for t in targets:                                                  # the front half stays; behind it: distinct ids not in it
            kept = graph[t][graph[t] >= 0][:R // 2].tolist()
            back = G[t][G[t] >= 0][len(kept):].tolist()
            assert G[t][:len(kept)].tolist() == kept and len(set(back)) == len(back) and not set(back) & set(kept)
    # the cut at 256 pool entries, a NaN row, bounds that decrease
    N, R = 400, 6
    rows = rng.standard_normal((N, 4)).astype(np.float32)
    rows[12] = np.nan
    graph = np.full((N, R), -1)
    graph[0, :4] = [5, 6, 7, 8]
    ids = np.arange(10, 10 + 257)
    for n_in, cut in ((254, 0), (255, 0), (256, gic.LINK_ST_CUT)):         # + the one entry of the back half: 255, 256, 257
        G, st = gic.link_reverse(space, rows, graph, [0], [0, n_in], ids[:n_in])
        G2, st2 = gic.link_reverse_loop(space, rows, graph, [0], [0, n_in], ids[:n_in])
        assert (G == G2).all() and st[0] == st2[0] == cut and (G[0, :3] == [5, 6, 7]).all() and 12 not in G[0]
    G, st = gic.link_reverse(space, rows, graph, [0, 1], [5, 2, 257], ids)
    G2, st2 = gic.link_reverse_loop(space, rows, graph, [0, 1], [5, 2, 257], ids)
    assert (G == G2).all() and (st == st2).all() and st[0] & gic.LINK_ST_LIMS and not st[1] & gic.LINK_ST_LIMS
    assert (G[0] == graph[0]).all()                                        # (clamped to an empty list: the back half is re-ranked alone)


def test_incoming_is_the_order_of_merge_reverse():
    rng = np.random.default_rng(13)
    n, b, R = 30, 12, 6
    F = np.stack([rng.permutation(n + b)[:R] for _ in range(b)])           # distinct within a row, as forward rows are
    F[rng.random(F.shape) < 0.2] = -1
    targets, lims, ids = gic.incoming(F, n)
    assert (np.diff(targets) > 0).all() and lims[0] == 0 and lims[-1] == (F >= 0).sum() == ids.shape[0]
    for j, t in enumerate(targets):
        mine = ids[lims[j]:lims[j + 1]] - n
        pos = [int(np.nonzero(F[i] == t)[0][0]) for i in mine]
        assert all(t in F[i] for i in mine) and pos == sorted(pos)


def test_prefiltered_knn_graph_is_the_exact_one():
    rng = np.random.default_rng(14)
    c, _ = gic.manifold_rows(rng, 300, 12, latent=4)
    c[9] = c[3]
    for space in ("cosine", "dot", "l2"):
        assert (gic.knn_graph_prefiltered(space, c, 10, keep=40) == gc.knn_graph_ref(space, c, 10)).all(), space


@pytest.fixture(scope="module")
def manifold():
    rng = np.random.default_rng(2026)
    c, lift = gic.manifold_rows(rng, 4096, 32)
    q, _ = gic.manifold_rows(rng, 128, 32, lift=lift)
    return c, q


def test_an_inserted_graph_keeps_the_recall_of_the_rebuilt_one(manifold):
    space, N, m, batch, M, width, ef, k = "l2", 4096, 2048, 256, 8, 4, 32, 10
    c, q = manifold
    R, K0 = gc.degree_params(M, 0)
    entries = np.sort(np.random.default_rng(0).permutation(m)[:16])
    iters = (3 * K0 + 2 * width - 1) // (2 * width) + 8
    base = gic.build_graph_prefiltered(space, c[:m], K0, R)
    inserted = gic.insert_ref(space, c[:m], base, c[m:], K0, R, batch, width, iters, entries=entries)
    rebuilt = gic.build_graph_prefiltered(space, c, K0, R)
    assert inserted.shape == rebuilt.shape == (N, R) and (inserted[:, 0] >= 0).all()
    _, truth, _ = list_topk_ref(space, q, c, np.arange(N), k)
    s_iters = (3 * ef + 2 * width - 1) // (2 * width) + 8
    recall = {}
    for name, g in (("inserted", inserted), ("rebuilt", rebuilt)):
        _, found, _ = gc.graph_search_ref(space, q, c, g, entries, ef, width, s_iters, k)
        recall[name] = gsc.recall(found, truth)
    orphans = gic.zero_in_degree_share(inserted, m)
    print(f"recall@10 inserted {recall['inserted']:.4f} rebuilt {recall['rebuilt']:.4f} zero-in-degree share {orphans:.4f}")
    assert recall["rebuilt"] > 0.5, recall                                 # (a bar against nothing would show nothing)
    assert recall["inserted"] >= 0.8 * recall["rebuilt"], (recall, orphans)
