"""CPU checks of the seeded graph search (include/tsim.h tsim_graph_search_seeded): the entry validates its arguments before any
launch, the restatement of tests/graph_seed_cases.py reduces to graph_search_ref where it must, and — on the restatement — per-query
entry points from a coarse quantiser find the neighbours that shared entry points miss on a corpus of islands."""
import ctypes
import os

import numpy as np
import pytest

from graph_cases import ST_ROW, graph_search_ref, random_graph, random_rows, reachable
from graph_seed_cases import (build_graph_ref, entries_ref, graph_search_seeded_ref, island_corpus, probes_ref, recall,
                              seed_table_ref)
from list_cases import SPACES, header_define, list_topk_ref, same_bits
from text_similarity_amd import _lib

EINVAL = 1
COS, DOT, L2 = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from text_similarity_amd.build import build
        build(verbose=False)
    return _lib.lib()


def test_symbol_and_constant(lib):
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(cdll, "tsim_graph_search_seeded") and "tsim_graph_search_seeded" in set(_lib.DECLARED_SYMBOLS)
    from text_similarity_amd import ops
    assert header_define("TSIM_GRAPH_MAX_COARSE_LISTS") == _lib.GRAPH_MAX_COARSE_LISTS == ops.GRAPH_MAX_COARSE_LISTS == 4096
    assert callable(ops.graph_search_seeded)


def _seeded(lib, p, **kw):
    a = dict(space=COS, eq=p, ldq=64, Q=4, rows=p, ldr=64, N=100, d=64, graph=p, R=8, seeds=p, T=10, S=2, probes=p, ldp=4, P=4,
             cent=None, ldc=0, ids=None, ef=32, width=4, iters=8, k=10, out_s=p, out_i=p, idx_offset=0, status=None, out_p=None,
             stream=None)
    a.update(kw)
    return lib.tsim_graph_search_seeded(a["space"], a["eq"], a["ldq"], a["Q"], a["rows"], a["ldr"], a["N"], a["d"], a["graph"], a["R"],
                                        a["seeds"], a["T"], a["S"], a["probes"], a["ldp"], a["P"], a["cent"], a["ldc"], a["ids"],
                                        a["ef"], a["width"], a["iters"], a["k"], a["out_s"], a["out_i"], a["idx_offset"], a["status"],
                                        a["out_p"], a["stream"])


def test_argument_validation_before_any_launch(lib):
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    for name in ("eq", "rows", "graph", "out_s", "out_i"):
        assert _seeded(lib, p, **{name: None}) == EINVAL, name
        assert b"null pointer" in lib.tsim_last_error()
    # both, or neither, of probes and centroids
    assert _seeded(lib, p, cent=p, ldc=64) == EINVAL and b"exactly one of probes and centroids" in lib.tsim_last_error()
    assert _seeded(lib, p, probes=None) == EINVAL and b"exactly one of probes and centroids" in lib.tsim_last_error()
    # S * P outside 1..256
    for S, P in ((0, 4), (2, 0), (-1, 4), (2, -3), (2, 129), (257, 1), (16, 17), (1 << 16, 1 << 16)):
        assert _seeded(lib, p, S=S, P=P, ldp=1 << 20) == EINVAL and b"entry points" in lib.tsim_last_error(), (S, P)
    assert _seeded(lib, p, seeds=None, P=257, ldp=257) == EINVAL and b"entry points" in lib.tsim_last_error()     # (S = 1)
    # T: at least one list; at most 4096 centroids for the kernel's own coarse phase (given probes: no such cap)
    assert _seeded(lib, p, T=0) == EINVAL and b"lists" in lib.tsim_last_error()
    assert _seeded(lib, p, probes=None, cent=p, ldc=64, T=4097) == EINVAL and b"4096" in lib.tsim_last_error()
    assert _seeded(lib, p, probes=None, cent=p, ldc=64, seeds=None, N=4097) == EINVAL and b"4096" in lib.tsim_last_error()   # T = N
    assert _seeded(lib, p, probes=None, cent=p, ldc=63) == EINVAL and b"strides" in lib.tsim_last_error()
    assert _seeded(lib, p, ldp=3) == EINVAL and b"probes row stride" in lib.tsim_last_error()
    # what tsim_graph_search refuses
    for R in (0, 65):
        assert _seeded(lib, p, R=R) == EINVAL and b"degree" in lib.tsim_last_error()
    assert _seeded(lib, p, ef=9, k=10) == EINVAL and _seeded(lib, p, ef=1025) == EINVAL
    for w in (0, 5):
        assert _seeded(lib, p, width=w) == EINVAL and b"width" in lib.tsim_last_error()
    assert _seeded(lib, p, iters=0) == EINVAL and _seeded(lib, p, k=0) == EINVAL
    assert _seeded(lib, p, space=L2, d=768, ldq=768, ldr=768) == EINVAL and b"Euclidean" in lib.tsim_last_error()
    assert _seeded(lib, p, space=3) == EINVAL and _seeded(lib, p, Q=0) == EINVAL and _seeded(lib, p, N=0) == EINVAL
    # the visited table is sized by E = P S: 8 + iters * 4 * 8 rows against 16 384
    fits = (16384 - 8) // 32
    assert _seeded(lib, p, iters=fits + 1) == EINVAL
    msg = lib.tsim_last_error()
    assert b"visit" in msg and b"max_iters" in msg and b" 8 + " in msg


def test_entries_ref():
    seeds = np.array([[0, 1], [2, -1], [9, 3]])
    ent, beyond = entries_ref(np.array([[1, 1], [2, 0], [-1, 3], [5, 0]]), seeds, 3, 4)
    assert ent.tolist() == [[2, -1, 2, -1], [9, 3, 0, 1], [-1, -1, -1, -1], [-1, -1, 0, 1]] and beyond.tolist() == [False, False, True, True]
    ent, beyond = entries_ref(np.array([[3, -1, 4], [0, 0, 2]]), None, None, 4)      # a probe is a row
    assert ent.tolist() == [[3, -1, -1], [0, 0, 2]] and beyond.tolist() == [True, False]


@pytest.mark.parametrize("space", SPACES)
def test_restatement_reduces_to_shared_entries(space):
    """P = 1 and one seed row repeated for every list: every query starts from the same rows, whatever its probe."""
    rng = np.random.default_rng(3)
    N, R, d, Q, T, k = 300, 6, 12, 5, 7, 8
    c, q = random_rows(rng, N, d), random_rows(rng, Q, d, dup=False)
    g, _ = random_graph(rng, N, R)
    row = np.array([5, 17, -1, 250, N + 1, 17])
    seeds = np.tile(row, (T, 1))
    want = graph_search_ref(space, q, c, g, row, 24, 2, 6, k, idx_offset=3)
    S, I, st, _ = graph_search_seeded_ref(space, q, c, g, 24, 2, 6, k, probes=rng.integers(0, T, (Q, 1)), seeds=seeds, idx_offset=3)
    assert same_bits(S, want[0]) and (I == want[1]).all() and (st == want[2]).all() and (st & ST_ROW).all()
    # ... and with centroids: whichever centroid wins, the seeds are the same
    S, I, st, pr = graph_search_seeded_ref(space, q, c, g, 24, 2, 6, k, centroids=random_rows(rng, T, d), n_probe=1, seeds=seeds,
                                           idx_offset=3)
    assert same_bits(S, want[0]) and (I == want[1]).all() and (st == want[2]).all() and ((pr >= 0) & (pr < T)).all()


def test_probes_ref_drops_nan_and_pads():
    rng = np.random.default_rng(4)
    cent = rng.standard_normal((5, 8)).astype(np.float32)
    cent[1] = cent[3]                # a tie: the lower list first
    cent[2, 5] = np.nan              # no score in any space
    q = rng.standard_normal((3, 8)).astype(np.float32)
    for space in SPACES:
        pr = probes_ref(space, q, cent, 5)
        assert (pr[:, 4] == -1).all() and (np.sort(pr[:, :4], 1) == [0, 1, 3, 4]).all(), space
        assert all(list(r).index(1) + 1 == list(r).index(3) for r in pr), space
    # a zero centroid HAS a cosine here, 0 (x.y / (max(|x|, eps) max(|y|, eps)), as in every search of this project): it ranks
    cent[2] = 0
    pr = probes_ref("cosine", q, cent, 5)
    assert (np.sort(pr, 1) == np.arange(5)).all()
    q[1] = np.nan                    # a query without scores has no probes
    assert (probes_ref("cosine", q, cent, 5)[1] == -1).all() and (probes_ref("l2", q, cent, 2)[1] == -1).all()


def test_island_corpus_recall_on_the_restatement():
    """The effect the seeded search exists for, l2, numpy only: 64 tight clusters, a graph of islands.  Eight shared entry points
    reach a tenth of the rows; two seeds of each of the two nearest centres reach the query's own island."""
    rows, cent, qs = island_corpus()
    N, k, ef, width, iters = rows.shape[0], 5, 16, 2, 32
    g = build_graph_ref("l2", rows, 16, 8)
    truth = list_topk_ref("l2", qs, rows, np.arange(N), k)[1]
    shared = np.sort(np.random.default_rng(0).permutation(N)[:8])
    assert reachable(g, shared, N).shape[0] < N // 4
    r_shared = recall(graph_search_ref("l2", qs, rows, g, shared, ef, width, iters, k)[1], truth)
    seeds = seed_table_ref("l2", cent, rows, 2)
    r_coarse = recall(graph_search_seeded_ref("l2", qs, rows, g, ef, width, iters, k, centroids=cent, n_probe=2, seeds=seeds)[1], truth)
    print(f"recall@5: shared {r_shared:.3f}, coarse {r_coarse:.3f}")
    assert r_shared <= 0.25
    assert r_coarse >= 0.9
