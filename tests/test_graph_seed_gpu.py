"""The seeded graph search on the GPU (ops.graph_search_seeded): scores, ids, status and probes are compared bit for bit with the
numpy restatement of tests/graph_seed_cases.py, in the three spaces.  No tolerance anywhere.  Graphs and rows are those of
tests/test_graph_gpu.py (graph_cases.random_graph / random_rows); probes and seeds carry repeats, padding and ids past their
tables.  The large values (Q = 257, E = 256, S = 256, T = 4 096, d = 768) come one at a time, so a case takes well under a second
of GPU time."""
import numpy as np
import pytest
import torch

from graph_cases import ST_ROW, random_graph, random_rows
from graph_seed_cases import graph_search_seeded_ref, probes_ref
from list_cases import same_bits
from text_similarity_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPACES = ("cosine", "dot", "l2")


def _dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(DEV)


def _search(space, q, c, g, k, ef, width, iters, probes=None, centroids=None, n_probe=None, seeds=None, row_ids=None, idx_offset=0,
            ld_probes=None):
    pr = None
    if probes is not None:
        pr = _dev(probes, np.int32)
        if ld_probes is not None:      # rows of a wider table
            wide = torch.full((pr.shape[0], ld_probes), 7, dtype=torch.int32, device=DEV)
            wide[:, :pr.shape[1]] = pr
            pr = wide[:, :pr.shape[1]]
            assert pr.stride(0) == ld_probes
    out = ops.graph_search_seeded(space, _dev(q), _dev(c), _dev(g, np.int32), k, ef, probes=pr,
                                  centroids=None if centroids is None else _dev(centroids, np.float32), n_probe=n_probe,
                                  seeds=None if seeds is None else _dev(seeds, np.int32), width=width, max_iters=iters,
                                  row_ids=None if row_ids is None else _dev(row_ids, np.int32), idx_offset=idx_offset,
                                  return_status=True, return_probes=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _assert_same(got, ref, what):
    assert (got[3] == ref[3]).all(), (what, "probes", np.argwhere(got[3] != ref[3])[:5])
    assert (got[1] == ref[1]).all(), (what, np.argwhere(got[1] != ref[1])[:5])
    assert same_bits(got[0], ref[0]), (what, np.argwhere(got[0].view(np.int32) != ref[0].view(np.int32))[:5])
    assert (got[2] == ref[2]).all(), (what, got[2][:8], ref[2][:8])
    pad = ref[1] < 0
    assert np.isinf(got[0][pad]).all() and (got[1][pad] == -1).all()


def _tables(rng, N, T, S, P, Q, lost=()):
    """(probes [Q, P], seeds [T, S]) with repeats, -1 and ids past the table at both levels (where the sizes allow), no seed on
    the island."""
    ok = np.setdiff1d(np.arange(N), lost)
    seeds = rng.choice(ok, size=(T, S), replace=True)
    probes = rng.integers(0, T, size=(Q, P))
    if S >= 3:
        seeds[:, 1] = np.where(rng.random(T) < 0.3, -1, seeds[:, 1])
        seeds[0, 2] = N + 2
    if P >= 2 and Q >= 3:
        probes[0, 0] = 0                    # meets the seed >= N (S >= 3)
        probes[1, 1] = probes[1, 0]         # a repeat
        probes[2, 0] = -1
        probes[2, 1] = T + 1                # never dereferenced: ST_ROW
    return probes, seeds


# (N, R, T, S, P, ef, width, Q, k, d)
SHAPES = [
    (1, 1, 1, 1, 1, 1, 1, 1, 1, 7),
    (65, 8, 5, 3, 2, 16, 2, 3, 10, 40),
    (2000, 8, 64, 4, 64, 64, 4, 3, 10, 24),      # E = 256
    (2000, 33, 300, 1, 256, 64, 3, 257, 5, 16),
    (2000, 64, 40, 256, 1, 65, 4, 3, 10, 24),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "N%d-R%d-T%d-S%d-P%d-ef%d-w%d-Q%d-k%d" % s[:9])
@pytest.mark.parametrize("space", SPACES)
def test_given_probes(space, shape):
    N, R, T, S, P, ef, width, Q, k, d = shape
    rng = np.random.default_rng(N * 11 + T)
    c = random_rows(rng, N, d)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    g, lost = random_graph(rng, N, R, island=3 if N > 10 else 0)
    probes, seeds = _tables(rng, N, T, S, P, Q, lost)
    iters = 12
    ref = graph_search_seeded_ref(space, q, c, g, ef, width, iters, k, probes=probes, seeds=seeds)
    _assert_same(_search(space, q, c, g, k, ef, width, iters, probes=probes, seeds=seeds), ref, (space, shape))
    if P >= 2 and Q >= 3:
        assert ref[2][2] & ST_ROW and (S < 3 or ref[2][0] & ST_ROW)
    assert not np.isin(ref[1], lost).any()


@pytest.mark.parametrize("space", SPACES)
def test_island_through_one_query_strided_probes_tombstones_and_offset(space):
    N, R, T, S, P, ef, width, Q, k, d = 400, 8, 9, 3, 2, 32, 2, 4, 12, 20
    rng = np.random.default_rng(5)
    c = random_rows(rng, N, d)
    g, lost = random_graph(rng, N, R, island=4)
    g[lost] = np.concatenate([lost[1:], lost[:1]])[:, None]      # the island's rows point at one another only ...
    c[lost] = c[lost[:1]] + 0.01 * rng.standard_normal((4, d)).astype(np.float32)      # ... and lie together, where the queries are
    q = c[lost[:1]].repeat(Q, 0) + 0.01 * rng.standard_normal((Q, d)).astype(np.float32)
    probes, seeds = _tables(rng, N, T - 1, S, P, Q, lost)
    seeds = np.concatenate([seeds, [[lost[0], -1, lost[0]]]])     # list T - 1 opens the island ...
    probes[1, 0] = T - 1                                          # ... to query 1 alone
    ref = graph_search_seeded_ref(space, q, c, g, ef, width, 30, k, probes=probes, seeds=seeds)
    got = _search(space, q, c, g, k, ef, width, 30, probes=probes, seeds=seeds, ld_probes=P + 3)
    _assert_same(got, ref, space)
    on = np.isin(got[1], lost).any(1)
    assert on.tolist() == [False, True, False, False] and np.isin(lost, got[1][1]).all()
    # tombstones route and are not returned; row_ids name the rows
    row_ids = np.arange(N, dtype=np.int32) + 1000
    row_ids[lost[0]] = -1
    row_ids[rng.choice(np.setdiff1d(np.arange(N), lost), 40, replace=False)] = -1
    ref = graph_search_seeded_ref(space, q, c, g, ef, width, 30, k, probes=probes, seeds=seeds, row_ids=row_ids)
    got = _search(space, q, c, g, k, ef, width, 30, probes=probes, seeds=seeds, row_ids=row_ids)
    _assert_same(got, ref, space)
    assert np.isin(lost[1:] + 1000, got[1][1]).all() and lost[0] + 1000 not in got[1]
    ref = graph_search_seeded_ref(space, q, c, g, ef, width, 30, k, probes=probes, seeds=seeds, idx_offset=1 << 33)
    _assert_same(_search(space, q, c, g, k, ef, width, 30, probes=probes, seeds=seeds, idx_offset=1 << 33), ref, space)


@pytest.mark.parametrize("space", SPACES)
def test_probes_as_rows(space):
    """seeds=None: the plain entries [Q, E] form, other rows for every query."""
    N, R, E, ef, width, Q, k, d = 500, 8, 6, 24, 3, 5, 8, 33
    rng = np.random.default_rng(6)
    c = random_rows(rng, N, d)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    g, lost = random_graph(rng, N, R, island=3)
    entries = rng.choice(np.setdiff1d(np.arange(N), lost), size=(Q, E))
    entries[0, 1], entries[1, 2], entries[2, 0], entries[3, 3] = -1, N, N + 5, entries[3, 0]
    entries[4, :] = lost[0]
    q[4] = c[lost[0]]      # (so that the island's row, which query 4 alone enters through, is among its best)
    ref = graph_search_seeded_ref(space, q, c, g, ef, width, 20, k, probes=entries)
    got = _search(space, q, c, g, k, ef, width, 20, probes=entries)
    _assert_same(got, ref, space)
    assert (got[2][1:3] & ST_ROW).all() and lost[0] in got[1][4] and not np.isin(got[1][:4], lost).any()


def _coarse_case(space, T, P, d, rng, N=300, Q=3):
    c = random_rows(rng, N, d)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    g, _ = random_graph(rng, N, 8)
    cent = rng.standard_normal((T, d)).astype(np.float32)
    seeds = rng.integers(-1, N + 1, size=(T, 2))
    return q, c, g, cent, seeds


# T: one centroid, a partial block, the 256 of one block of the running list exactly, one past it, and the cap (16 blocks)
@pytest.mark.parametrize("P", [1, 8, 64])
@pytest.mark.parametrize("T", [1, 7, 256, 257, 4096])
@pytest.mark.parametrize("space", SPACES)
def test_kernel_coarse_phase_lists(space, T, P):
    rng = np.random.default_rng(T * 3 + P)
    q, c, g, cent, seeds = _coarse_case(space, T, P, 24, rng)
    if T >= 7:
        cent[T - 1] = cent[0]          # duplicates across the first and the last block: the tie goes to the lower list
        cent[T // 2] = cent[1]
        q[0] = cent[0] if space != "dot" else q[0]
    ref = graph_search_seeded_ref(space, q, c, g, 16, 2, 10, 5, centroids=cent, n_probe=P, seeds=seeds)
    got = _search(space, q, c, g, 5, 16, 2, 10, centroids=cent, n_probe=P, seeds=seeds)
    _assert_same(got, ref, (space, T, P))
    assert ((got[3] >= 0).sum(1) == min(P, T)).all() and (got[3][:, min(P, T):] == -1).all()
    if T >= 7 and space != "dot" and P >= 2:
        assert got[3][0, :2].tolist() == [0, T - 1]
    # the other route: the same probes handed in give the same search
    again = _search(space, q, c, g, 5, 16, 2, 10, probes=got[3], seeds=seeds)
    for a, b in zip(got, again):
        assert (a.view(np.int32) == b.view(np.int32)).all() if a.dtype == np.float32 else (a == b).all()


@pytest.mark.parametrize("d", [1, 65, 384, 768])
@pytest.mark.parametrize("space", SPACES)
def test_kernel_coarse_phase_widths(space, d):
    d = 767 if space == "l2" and d == 768 else d
    rng = np.random.default_rng(d)
    q, c, g, cent, seeds = _coarse_case(space, 40, 8, d, rng, N=120)
    ref = graph_search_seeded_ref(space, q, c, g, 16, 2, 10, 5, centroids=cent, n_probe=8, seeds=seeds)
    _assert_same(_search(space, q, c, g, 5, 16, 2, 10, centroids=cent, n_probe=8, seeds=seeds), ref, (space, d))


@pytest.mark.parametrize("space", SPACES)
def test_kernel_coarse_phase_unusable_scores(space):
    """Centroids without a score (NaN) are dropped and leave -1 padding; a zero centroid has the cosine 0 — the project's
    x.y / (max(|x|, eps) max(|y|, eps)) — and ranks with it; a NaN query has no probes, no entry points and an empty result."""
    rng = np.random.default_rng(9)
    T, P = 12, 10
    q, c, g, cent, seeds = _coarse_case(space, T, P, 16, rng)
    cent[[2, 5, 11], 3] = np.nan
    cent[4] = 0
    q[1, 0] = np.nan
    ref = graph_search_seeded_ref(space, q, c, g, 16, 2, 10, 5, centroids=cent, n_probe=P, seeds=seeds)
    got = _search(space, q, c, g, 5, 16, 2, 10, centroids=cent, n_probe=P, seeds=seeds)
    _assert_same(got, ref, space)
    assert (got[3][0] >= 0).sum() == 9 and got[3][0, 9] == -1 and not np.isin(got[3], [2, 5, 11]).any() and 4 in got[3][0]
    assert (got[3][1] == -1).all() and (got[1][1] == -1).all() and np.isinf(got[0][1]).all() and got[2][1] == 0


def test_refusals():
    rng = np.random.default_rng(1)
    q, c, g, cent, seeds = _coarse_case("dot", 4097, 1, 8, rng)
    with pytest.raises(ValueError, match="4096"):
        _search("dot", q, c, g, 5, 16, 2, 10, centroids=cent, n_probe=1, seeds=seeds)
    # given probes know no such cap
    probes = probes_ref("dot", q, cent, 2)
    ref = graph_search_seeded_ref("dot", q, c, g, 16, 2, 10, 5, probes=probes, seeds=seeds)
    _assert_same(_search("dot", q, c, g, 5, 16, 2, 10, probes=probes, seeds=seeds), ref, "T = 4097")
    with pytest.raises(ValueError, match="exactly one"):
        ops.graph_search_seeded("dot", _dev(q), _dev(c), _dev(g, np.int32), 5, 16)
    with pytest.raises(ValueError, match="exactly one"):
        ops.graph_search_seeded("dot", _dev(q), _dev(c), _dev(g, np.int32), 5, 16, probes=_dev(probes, np.int32),
                                centroids=_dev(cent), n_probe=2)
    with pytest.raises(ValueError, match="int32"):
        ops.graph_search_seeded("dot", _dev(q), _dev(c), _dev(g, np.int32), 5, 16, probes=_dev(probes, np.int64))
    with pytest.raises(ValueError, match="entry points"):
        ops.graph_search_seeded("dot", _dev(q), _dev(c), _dev(g, np.int32), 5, 16, probes=_dev(np.zeros((3, 129)), np.int32),
                                seeds=_dev(seeds, np.int32))
