"""The two insertion kernels (include/tsim_graph_insert.h) on crafted inputs against the restatement of
tests/graph_insert_cases.py, for equality: ids, detour counts and status words.

Prune: (K0, R) with K0 in {8, 64, 128} and R in {4, 32, 64}, B in {1, 7, 300} new rows (more rows than one wave of workgroups
needs; the grid strides past 16 384 only far above what a test may cost), candidate rows with padding in the middle and at the end,
repeated ids, batch rows — the row itself among them — and ids >= n + B; and n = 1.
Link: d in {8, 384, 768} (767 for 'l2': the two widths of the exact kernel's row loader and its last element), all three spaces, one
crafted graph of 300 rows — rows with fewer than R/2, exactly R/2 and no valid entries, incoming rows already in the front and in
the back half, pools of 255, 256 and 257 entries (the cut and its status bit), duplicate rows (equal scores, broken by id), a NaN
row and an id >= N in a pool — linked with T = every row, and T = 1.  Rows beyond 2^31 bytes are not needed here:
tests/test_far_rows_gpu.py pins the shared loaders."""
import functools

import numpy as np
import pytest
import torch

import graph_insert_cases as gic
from text_similarity_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


# ------------------------------------------------------------------------------------------------- forward edges
@functools.lru_cache(maxsize=None)
def _prune_case(n, B, K0, R):
    rng = np.random.default_rng(1000 * K0 + 10 * R + B + n)
    end = n + B
    graph = rng.integers(-1, end + 2, size=(n, R))                         # (an id >= n + B inside a list matches nothing usable)
    near = (rng.integers(0, end, size=(B, 1)) + rng.integers(0, 2 * K0, size=(B, K0))) % end        # local: detours exist
    cand = np.where(rng.random((B, K0)) < 0.8, near, rng.integers(0, end, size=(B, K0)))
    cand[rng.random((B, K0)) < 0.1] = -1                                   # padding in the middle
    cand[::2, K0 - max(1, K0 // 8):] = -1                                  # ... and at the end
    cand[rng.random((B, K0)) < 0.03] = end + rng.integers(0, 3)            # ids >= n + B
    cand[::3, 0] = n + np.arange(B)[::3]                                   # the row itself
    if K0 > 2:
        cand[1::3, 2] = cand[1::3, 1]                                      # a repeated id
    if B > 5:
        cand[5] = -1                                                       # a row of padding alone
    ref = gic.insert_prune(cand, graph)
    return cand, graph, ref


@pytest.mark.parametrize("B", [1, 7, 300])
@pytest.mark.parametrize("K0,R", [(8, 4), (64, 4), (64, 32), (128, 32), (128, 64), (64, 64)])
def test_prune_is_the_restatement(K0, R, B):
    n = 50
    cand, graph, (F, D, st) = _prune_case(n, B, K0, R)
    fwd, det, status = ops.graph_insert_prune(_dev(cand, np.int32), _dev(graph, np.int32), return_detours=True)
    assert fwd.dtype == det.dtype == status.dtype == torch.int32 and fwd.shape == (B, R)
    assert (det.cpu().numpy() == D).all() and (fwd.cpu().numpy() == F).all() and (status.cpu().numpy() == st).all()
    if B == 300:
        assert st.any() and not st.all() and ((D > 0) & (D < K0)).any() and (F[5] == -1).all()     # the cases above are all in
    fwd2, status2 = ops.graph_insert_prune(_dev(cand, np.int32), _dev(graph, np.int32))      # without the counts
    assert torch.equal(fwd2, fwd) and torch.equal(status2, status)


def test_prune_over_a_graph_of_one_row_and_bad_arguments():
    for B, K0, R in ((1, 1, 1), (9, 8, 4)):
        cand, graph, (F, D, st) = _prune_case(1, B, K0, R)
        fwd, det, status = ops.graph_insert_prune(_dev(cand, np.int32), _dev(graph, np.int32), return_detours=True)
        assert (det.cpu().numpy() == D).all() and (fwd.cpu().numpy() == F).all() and (status.cpu().numpy() == st).all()
    g = torch.zeros((4, 8), dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.graph_insert_prune(torch.zeros((3, 4), dtype=torch.int32, device=DEV), g)                  # K0 < R
    with pytest.raises(ValueError):
        ops.graph_insert_prune(torch.zeros((3, 8), dtype=torch.int64, device=DEV), g)
    with pytest.raises(ValueError):
        ops.graph_insert_prune(torch.zeros((3, 8), dtype=torch.int32, device=DEV), g[:0])
    empty = ops.graph_insert_prune(torch.zeros((0, 8), dtype=torch.int32, device=DEV), g)
    assert empty[0].shape == (0, 8) and empty[1].shape == (0,)


# ------------------------------------------------------------------------------------------------- reverse edges
LINK_N = 300


@functools.lru_cache(maxsize=None)
def _link_inputs(d, R):
    """One graph with every crafted row, and incoming lists for every row of it."""
    rng = np.random.default_rng(100 * d + R)
    N, h = LINK_N, R // 2
    rows = rng.standard_normal((N, d)).astype(np.float32)
    rows[40:50] = rows[30:40]                                              # equal scores, broken by id
    rows[7] = np.nan                                                       # a NaN row
    graph = rng.integers(0, N, size=(N, R))
    graph[rng.random((N, R)) < 0.1] = -1                                   # padding anywhere
    graph[0] = -1                                                          # no valid entry
    graph[1, h:] = -1
    graph[1, :h] = np.arange(100, 100 + h)                                 # exactly R/2 valid entries
    graph[2] = -1
    graph[2, :max(h - 1, 0)] = np.arange(100, 100 + max(h - 1, 0))         # fewer than R/2
    graph[10:13] = -1                                                      # the rows whose pools are 255, 256 and 257 entries long
    lists = []
    for t in range(N):
        ids = np.concatenate([rng.integers(0, N, size=rng.integers(0, 12)), rng.integers(30, 50, size=4),
                              graph[t, :1], graph[t, -1:], [7] if t % 5 == 0 else [], [N + 1] if t % 50 == 3 else []])
        lists.append(rng.permutation(ids.astype(np.int64)))               # (ids of the front half, of the back half, -1: all in)
    for t, size in ((10, 255), (11, 256), (12, 257)):
        perm = rng.permutation(N)                                          # size distinct ids, five of them twice
        lists[t] = np.concatenate([perm[~np.isin(perm, np.arange(30, 50))][:size - 20], np.arange(30, 50), np.arange(30, 35)])
    return rows, graph, lists


def _csr(lists, targets):
    lims = np.concatenate([[0], np.cumsum([len(lists[t]) for t in targets])]).astype(np.int64)
    ids = np.concatenate([lists[t] for t in targets] + [np.zeros((0,), np.int64)])
    return lims, ids


@pytest.mark.parametrize("space", ["cosine", "dot", "l2"])
@pytest.mark.parametrize("d,R", [(8, 8), (384, 5), (768, 64)])
def test_link_is_the_restatement(space, d, R):
    d = min(d, 767) if space == "l2" else d
    rows, graph, lists = _link_inputs(d, R)
    N = LINK_N
    for targets in (np.arange(N), np.array([11]), np.array([2])):
        lims, ids = _csr(lists, targets)
        G, st = gic.link_reverse(space, rows, graph, targets, lims, ids)
        g = _dev(graph, np.int32)
        status = ops.graph_link_reverse(space, _dev(rows, np.float32), g, _dev(targets, np.int32), _dev(lims, np.int64),
                                        _dev(ids, np.int32))
        assert (g.cpu().numpy() == G).all(), (space, d, R, len(targets))
        assert (status.cpu().numpy() == st).all(), (space, d, R, len(targets))
    lims, ids = _csr(lists, np.arange(N))
    G, st = gic.link_reverse(space, rows, graph, np.arange(N), lims, ids)
    assert (st[10:13] == [0, 0, gic.LINK_ST_CUT]).all() and (st[3] & gic.LINK_ST_ROW) and not (st & gic.LINK_ST_LIMS).any()
    assert 7 not in G[0] and (G[0] >= 0).sum() == min(R - R // 2, len(set(lists[0][lists[0] >= 0].tolist()) - {7, N + 1}))
    assert (G[1, :R // 2] == graph[1, :R // 2]).all()
    pairs = [(t, a) for t in range(N) for a in range(30, 40) if {a, a + 10} <= set(G[t, R // 2:].tolist())]
    assert pairs, "no row ranks two duplicate rows: the tie rule is not exercised"
    for t, a in pairs:                                                     # equal scores: side by side, the lower id first
        back = G[t, R // 2:].tolist()
        assert back.index(a) + 1 == back.index(a + 10), (t, a)


def test_link_literal_loops_once_and_clamped_bounds():
    """The vectorised restatement the cases above compare with is the literal loops' on this graph, and bounds that decrease or
    leave the list are clamped with their status bit."""
    rows, graph, lists = _link_inputs(8, 8)
    targets = np.arange(0, LINK_N, 7)
    lims, ids = _csr(lists, targets)
    G, st = gic.link_reverse("dot", rows, graph, targets, lims, ids)
    G2, st2 = gic.link_reverse_loop("dot", rows, graph, targets, lims, ids)
    assert (G == G2).all() and (st == st2).all()
    bad = lims.copy()
    bad[1], bad[3] = -5, bad[-1] + 9                                       # below 0; past the end (and so above its successor)
    G, st = gic.link_reverse("dot", rows, graph, targets, bad, ids)
    g = _dev(graph, np.int32)
    status = ops.graph_link_reverse("dot", _dev(rows, np.float32), g, _dev(targets, np.int32), _dev(bad, np.int64), _dev(ids, np.int32))
    assert (g.cpu().numpy() == G).all() and (status.cpu().numpy() == st).all() and (st & gic.LINK_ST_LIMS).sum() >= 3
    # a target outside the rows is skipped with its bit; the others are linked
    t2 = targets.copy()
    t2[0], t2[1] = -1, LINK_N
    G, st = gic.link_reverse("dot", rows, graph, t2, lims, ids)
    g = _dev(graph, np.int32)
    status = ops.graph_link_reverse("dot", _dev(rows, np.float32), g, _dev(t2, np.int32), _dev(lims, np.int64), _dev(ids, np.int32))
    assert (g.cpu().numpy() == G).all() and (status.cpu().numpy() == st).all() and (st[:2] == gic.LINK_ST_ROW).all()
