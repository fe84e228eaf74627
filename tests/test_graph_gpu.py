"""The graph search and the pruning kernel on the GPU (ops.graph_search, ops.graph_prune, ops.graph_merge_reverse): scores, ids
and status are compared bit for bit with the numpy restatement of tests/graph_cases.py.  No tolerance anywhere.  The graphs are
crafted (graph_cases.random_graph): a ring, repeated neighbours, self-loops, padding, ids >= N, unreachable rows; the corpus
holds duplicate rows, so equal scores are ordered by the tie rule.

Shapes.  The value sets of the search are covered a few at a time, not as a product: every width of a row (d), every N, R, E,
ef, width and Q appears in at least one case, the large ones (Q = 257, ef = 1 024, R = 64) each in a case that keeps the others
small, so that a case takes well under a second of GPU time and a few seconds of the restatement."""
import numpy as np
import pytest
import torch

from graph_cases import (ST_ITERS, ST_ROW, detours, forward_lists, graph_search_ref, merge_reverse, random_graph, random_rows,
                         reachable)
from list_cases import list_topk_ref, same_bits
from text_similarity_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPACES = ("cosine", "dot", "l2")


def _dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(DEV)


def _search(space, q, c, g, entries, k, ef, width, max_iters, row_ids=None, idx_offset=0):
    out = ops.graph_search(space, _dev(q), _dev(c), _dev(g, np.int32), _dev(entries, np.int32), k, ef, width=width, max_iters=max_iters,
                           row_ids=None if row_ids is None else _dev(row_ids, np.int32), idx_offset=idx_offset, return_status=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _assert_same(got, ref, what):
    assert (got[1] == ref[1]).all(), (what, np.argwhere(got[1] != ref[1])[:5])
    assert same_bits(got[0], ref[0]), (what, np.argwhere(got[0].view(np.int32) != ref[0].view(np.int32))[:5])
    assert (got[2] == ref[2]).all(), (what, got[2][:8], ref[2][:8])
    pad = ref[1] < 0
    assert np.isinf(got[0][pad]).all() and (got[1][pad] == -1).all()


def _entries(rng, N, E, lost=()):
    """E entry points with repeats, padding and an id >= N among them (when E allows), none on the island."""
    ok = np.setdiff1d(np.arange(N), lost)
    e = rng.choice(ok, size=E, replace=True)
    if E >= 4:
        e[1], e[2] = -1, N + 1
    return e


@pytest.mark.parametrize("d", [1, 63, 64, 65, 384, 768])
@pytest.mark.parametrize("space", SPACES)
def test_row_widths(space, d):
    d = 767 if space == "l2" and d == 768 else d
    rng = np.random.default_rng(100 + d)
    N, R, E, Q, k = 200, 8, 4, 3, 10
    c = random_rows(rng, N, d)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    q[0] = c[5]
    g, lost = random_graph(rng, N, R, island=5)
    e = _entries(rng, N, E, lost)
    for ef, width in ((32, 2), (10, 4)):
        ref = graph_search_ref(space, q, c, g, e, ef, width, 40, k)
        _assert_same(_search(space, q, c, g, e, k, ef, width, 40), ref, (space, d, ef, width))
        assert not np.isin(ref[1], lost).any() and (ref[2] & ST_ROW).all()


# (N, R, E, ef, width, Q, k, d, max_iters): every value of the issue's sets, the large ones one at a time
SHAPES = [
    (1, 1, 1, 1, 1, 1, 1, 7, 3),
    (2, 8, 64, 63, 2, 3, 10, 33, 5),
    (65, 33, 256, 64, 3, 3, 64, 40, 30),
    (65, 8, 1, 65, 4, 3, 65, 40, 100),
    (2000, 8, 1, 10, 1, 257, 10, 16, 12),
    (2000, 64, 64, 65, 4, 3, 10, 24, 20),
    (2000, 8, 64, 1024, 4, 3, 1024, 24, 300),
    (2000, 33, 256, 64, 2, 3, 5, 24, 25),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-R%d-E%d-ef%d-w%d-Q%d-k%d" % s[:7])
@pytest.mark.parametrize("space", SPACES)
def test_shapes(space, shape):
    N, R, E, ef, width, Q, k, d, iters = shape
    rng = np.random.default_rng(N * 7 + R)
    c = random_rows(rng, N, d)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    g, lost = random_graph(rng, N, R, island=3 if N > 10 else 0)
    e = _entries(rng, N, E, lost)
    ref = graph_search_ref(space, q, c, g, e, ef, width, iters, k, return_visits=True)
    _assert_same(_search(space, q, c, g, e, k, ef, width, iters), ref[:3], (space, shape))
    if N == 2000:
        assert ref[3].max() > E + 2 * width * R    # more rows than the entry points and two full expansions: several iterations ran
        assert not np.isin(ref[1], lost).any()     # unreachable rows stay out


@pytest.mark.parametrize("space", SPACES)
def test_exact_when_the_beam_holds_every_row(space):
    """A connected graph, ef >= N and no effective cap: every row is visited, and the result is the exact search's."""
    rng = np.random.default_rng(31)
    N, d, R, Q, k = 300, 48, 6, 3, 20
    c = random_rows(rng, N, d)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    g, _ = random_graph(rng, N, R, beyond=False)
    assert len(reachable(g, [17], N)) == N
    for width in (1, 2, 3, 4):
        got = _search(space, q, c, g, [17], k, 512, width, 400)
        rs, ri, _ = list_topk_ref(space, q, c, np.arange(N), k)
        assert (got[1] == ri).all() and same_bits(got[0], rs) and (got[2] == 0).all(), (space, width)
        _assert_same(got, graph_search_ref(space, q, c, g, [17], 512, width, 400, k), (space, width))


@pytest.mark.parametrize("space", SPACES)
def test_nan_tombstones_cap_and_offset(space):
    rng = np.random.default_rng(77)
    N, d, R, Q, k = 400, 20, 8, 4, 12
    c = random_rows(rng, N, d)
    c[11, 3] = np.nan                             # a NaN row: scored, dropped, stays visited
    q = rng.standard_normal((Q, d)).astype(np.float32)
    q[2, 0] = np.nan                              # a NaN query: every score is dropped, the result is padding
    g, lost = random_graph(rng, N, R, island=4)
    g[10, 2] = 11                                 # (the NaN row is somebody's neighbour)
    e = _entries(rng, N, 8, lost)
    e[0] = 11
    full = graph_search_ref(space, q, c, g, e, 64, 3, 200, k)
    got = _search(space, q, c, g, e, k, 64, 3, 200)
    _assert_same(got, full, (space, "nan"))
    assert (got[1][2] == -1).all() and 11 not in got[1] and not (got[2] & ST_ITERS).any()
    # tombstones among the best rows of each query: traversed, not returned; labels come from row_ids
    ids = (np.arange(N) * 3 + 1).astype(np.int32)
    ids[np.unique(full[1][:, :5][full[1][:, :5] >= 0])] = -1
    ref = graph_search_ref(space, q, c, g, e, 64, 3, 200, k, row_ids=ids)
    got = _search(space, q, c, g, e, k, 64, 3, 200, row_ids=ids)
    _assert_same(got, ref, (space, "tombstones"))
    assert (got[1][got[1] >= 0] % 3 == 1).all()
    # ... so many of them that fewer than k rows are left: the tail is padding
    few = np.full((N,), -1, dtype=np.int32)
    few[full[1][0, :3]] = 7
    ref = graph_search_ref(space, q, c, g, e, 64, 3, 200, k, row_ids=few)
    got = _search(space, q, c, g, e, k, 64, 3, 200, row_ids=few)
    _assert_same(got, ref, (space, "few"))
    assert (got[1][0, :3] == 7).all() and (got[1][0, 3:] == -1).all()
    # the cap cuts the search: the status bit, and still the restatement's rows
    for iters in (1, 2, 5):
        ref = graph_search_ref(space, q, c, g, e, 64, 3, iters, k)
        got = _search(space, q, c, g, e, k, 64, 3, iters)
        _assert_same(got, ref, (space, "cap", iters))
        assert (got[2][[0, 1, 3]] & ST_ITERS).all() and not got[2][2] & ST_ITERS
    # idx_offset; and status is written, not accumulated (a clean graph after a dirty one)
    ref = graph_search_ref(space, q, c, g, e, 64, 3, 200, k, idx_offset=1 << 33)
    _assert_same(_search(space, q, c, g, e, k, 64, 3, 200, idx_offset=1 << 33), ref, (space, "offset"))
    g2, _ = random_graph(rng, N, R, beyond=False)
    got = _search(space, q, c, g2, [0], k, 64, 3, 200)
    _assert_same(got, graph_search_ref(space, q, c, g2, [0], 64, 3, 200, k), (space, "clean"))
    assert (got[2] == 0).all()


def test_refusals():
    q, c = torch.zeros((2, 8), device=DEV), torch.zeros((10, 8), device=DEV)
    g = torch.zeros((10, 4), dtype=torch.int32, device=DEV)
    e = torch.zeros((2,), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="visit"):
        ops.graph_search("cosine", q, c, g, e, 1, 8, width=4, max_iters=ops.graph_max_iters(2, 4, 4) + 1)
    with pytest.raises(ValueError, match="ef="):
        ops.graph_search("cosine", q, c, g, e, 9, 8)
    with pytest.raises(ValueError, match="int32"):
        ops.graph_search("cosine", q, c, g.long(), e, 1, 8)
    s, i = ops.graph_search("cosine", q, c, g, e, 1, 8)          # the default cap is the largest that fits
    assert s.shape == (2, 1) and i.shape == (2, 1)


@pytest.mark.parametrize("N,K0,R", [(1, 1, 1), (2, 8, 8), (2, 1, 1), (65, 8, 3), (65, 33, 33), (65, 128, 64), (1000, 33, 16),
                                     (1000, 128, 64), (1000, 8, 8)])
def test_prune_kernel(N, K0, R):
    """Detour counts and forward lists against the restatement, on rows with repeats, padding and ids >= N; then the reverse
    merge (torch stable sorts on the device) against its restatement."""
    rng = np.random.default_rng(N + K0)
    G0 = rng.integers(-1, N + 2, size=(N, K0)).astype(np.int32)
    if N >= 65:                                    # mostly local neighbours, so that detours exist
        near = (np.arange(N)[:, None] + rng.integers(1, 2 * K0 + 2, size=(N, K0))) % N
        G0 = np.where(rng.random((N, K0)) < 0.9, near, G0).astype(np.int32)
    fwd, det = ops.graph_prune(_dev(G0), R, return_detours=True)
    D = detours(G0)
    assert (det.cpu().numpy() == D).all()
    F = forward_lists(G0, D, R)
    assert (fwd.cpu().numpy() == F).all()
    assert (ops.graph_prune(_dev(G0), R).cpu().numpy() == F).all()
    if N >= 65:
        assert (D[D < K0] > 0).mean() > 0.2
    assert (ops.graph_merge_reverse(fwd).cpu().numpy() == merge_reverse(F)).all()
