"""Operands that cannot be strided — the half rows of the MFMA pass and the graph adjacency — at sizes where their own offsets
cross 2^32 bytes, with the exact answer still derivable on the CPU.

A flat corpus of 2 900 000 x 768: the half rows are 4.45 GB and cross 2^32 bytes (2^31 elements) inside row 2 796 202, the
float32 rows are 8.9 GB and cross 2^32 bytes inside row 1 398 101 and 2^33 bytes further on.  It is a seeded 4 096-row block
tiled on the device, with 128 planted rows written over it (tests/far_cases.py large_inputs: the first rows, the rows around both
boundaries, the last two rows, the rest spread out).  tests/test_far_cases_cpu.py asserts that every planted row beats every
block row for every query by a margin, in every space; so the first 128 places of every query are exactly the planted rows,
whatever the 700 copies of each block row do among themselves, and the oracle needs the planted rows only.
The Euclidean entries take rows of 767 elements at most, so they run on the first 767 columns: the float32 operand is then a
view with ld = 768 of the same 8.9 GB, and l2_rows' half rows are 768 wide like the others.
"every status exact" is read as: every status is one the library defines for an exact answer (top-k 0, 1 or 2; range 1 or 2);
they are printed.

A graph adjacency of [2^24 + 4096, 64] int32, 4.29 GB: every row from 2^24 on lies beyond 2^32 bytes.  It is the ring lattice
i +- 1 .. 32 (mod N); the rows are float32 [N, 8].  Entry points sit on both sides of row 2^24 and near the last row.  A search of
max_iters iterations cannot leave the windows of 32 (max_iters + 2) rows around its entry points (a lattice step moves 32 rows at
most), so tests/graph_cases.py graph_search_ref runs on those windows alone, renumbered in ascending order (which keeps the
(score, row) order) and numbered back.

Needs 24 GB of free device memory (the float32 rows, the contiguous copy ops.l2_rows makes of the 767-column view, one set of
half rows), the graph 6 GB."""
import gc

import numpy as np
import pytest
import torch

import far_cases as fc
from graph_cases import graph_search_ref
from l2_cases import aug_corpus
from oracle.search_ref import flush_safe_err, rho_rows, unit_rows
from text_similarity_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, D = fc.LARGE_N, fc.LARGE_D
GRAPH_N, GRAPH_R, GRAPH_D = (1 << 24) + 4096, 64, 8


class _Big:
    """the flat corpus or the graph, one at a time"""

    def __init__(self):
        self.kind, self.data = None, None

    def _switch(self, kind, need):
        self.release()
        free = torch.cuda.mem_get_info()[0]
        if free < need:
            pytest.skip(f"the {kind} needs {need / 1e9:.0f} GB of device memory, {free / 1e9:.1f} GB are free")
        self.kind = kind

    def flat(self):
        """float32 [N, 768] on the device"""
        if self.kind != "flat":
            self._switch("flat corpus", 24 << 30)
            q, block, pos, planted = fc.large_inputs()
            cf = _dev(block).repeat(-(-N // fc.LARGE_BLOCK), 1)[:N]     # pure data movement
            cf[_dev(pos)] = _dev(planted)
            assert cf.is_contiguous() and cf.shape == (N, D) and cf.numel() * 4 > 1 << 33
            self.data = cf
        return self.data

    def graph(self):
        """(adjacency int32 [GRAPH_N, 64], rows float32 [GRAPH_N, 8]) on the device"""
        if self.kind != "graph":
            self._switch("graph", 10 << 30)
            off = torch.cat([torch.arange(1, 33), -torch.arange(1, 33)]).to(device=DEV, dtype=torch.int32)
            g = torch.arange(GRAPH_N, dtype=torch.int32, device=DEV)[:, None] + off[None, :]
            g.remainder_(GRAPH_N)
            assert g.dtype == torch.int32 and g.is_contiguous() and (1 << 24) * GRAPH_R * 4 == 1 << 32
            gen = torch.Generator(device=DEV).manual_seed(24)
            rows = torch.randn((GRAPH_N, GRAPH_D), generator=gen, dtype=torch.float32, device=DEV)
            self.data = (g, rows)
        return self.data

    def release(self):
        self.kind, self.data = None, None
        gc.collect()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def big():
    torch.cuda.reset_peak_memory_stats()
    holder = _Big()
    yield holder
    holder.release()
    print(f"\ntests/test_large_corpus_gpu.py: peak device memory allocated {torch.cuda.max_memory_allocated() / 1e9:.2f} GB")


def _dev(x, dtype=None):
    return torch.from_numpy(np.array(x, dtype=dtype, order="C")).to(DEV)


def _check_rows():
    """the boundary rows of both operands, the first and last rows, every planted row and 1 000 seeded rows"""
    rng = np.random.default_rng(11)
    near = [b + o for b in (fc.LARGE_HALF_ROW, fc.LARGE_F32_ROW, 2 * fc.LARGE_F32_ROW) for o in range(-3, 4)]
    return np.unique(np.concatenate([[0, 1, N - 2, N - 1], near, fc.large_inputs()[2], rng.integers(0, N, 1000)]))


def _whole_corpus_rows():
    """every DISTINCT row of the corpus: the block and the planted rows (a maximum over the corpus is a maximum over these)"""
    _, block, _, planted = fc.large_inputs()
    return np.concatenate([block, planted])


def _halves(t, idx):
    torch.cuda.synchronize()
    return t[torch.from_numpy(idx).to(DEV)].float().cpu().numpy()


def test_l2norm_rows_whole_corpus(big):
    cf = big.flat()
    cu, rho = ops.l2norm_rows(cf, return_rho=True)
    assert cu.shape == (N, D) and cu.numel() * 2 > 1 << 32
    idx = _check_rows()
    np.testing.assert_array_equal(_halves(cu, idx), unit_rows(fc.large_row(idx)))
    want = rho_rows(_whole_corpus_rows()).max()
    assert want <= float(rho.item()) <= want * (1 + 3e-6)        # (the bar of tests/test_search_f32_gpu.py)


def test_dot_scaled_rows_whole_corpus(big):
    cf = big.flat()
    cn, rho, scale = ops.dot_scaled_rows(cf)
    assert cn.shape == (N, D)
    every = _whole_corpus_rows()
    norm = float(np.sqrt((every.astype(np.float64) ** 2).sum(1)).max())
    S = ops.dot_scale(scale)
    assert S == 2.0 ** np.ceil(np.log2(norm)) and norm <= float(scale.item()) <= S
    idx = _check_rows()
    np.testing.assert_array_equal(_halves(cn, idx), (fc.large_row(idx).astype(np.float64) / S).astype(np.float16).astype(np.float32))
    v = every.astype(np.float64) / S
    want = float(np.sqrt((flush_safe_err(v.astype(np.float16).astype(np.float64), v) ** 2).sum(1)).max())
    assert want <= float(rho.item()) <= want * (1 + 1e-5)


def test_l2_rows_whole_corpus(big):
    cf = big.flat()
    cn, rho, scale = ops.l2_rows(cf[:, :D - 1])
    assert cn.shape == (N, D)
    A = ops.dot_scale(scale)
    idx = _check_rows()
    np.testing.assert_array_equal(_halves(cn, idx), aug_corpus(fc.large_row(idx)[:, :D - 1], A)[0].astype(np.float32))
    want = aug_corpus(_whole_corpus_rows()[:, :D - 1], A)[1]
    assert want <= float(rho.item()) <= want * (1 + 1e-5)        # (the bar of tests/test_l2_search_gpu.py)


def _planted_lists(space, k):
    """the oracle's first k places of every query: the planted rows by (score desc, row asc) — l2: (distance asc, row asc)"""
    q, _, pos, planted = fc.large_inputs()
    w = D - 1 if space == "l2" else D
    sp = fc.scores(space, q[:, :w], planted[:, :w])
    S = np.empty((fc.Q, k), np.float32)
    I = np.empty((fc.Q, k), np.int64)
    for j in range(fc.Q):
        key = sp[j].astype(np.float64)
        o = np.lexsort((pos, key if space == "l2" else -key))[:k]
        S[j], I[j] = sp[j][o], pos[o]
    return S, I


def _operands(space, cf):
    q = fc.large_inputs()[0]
    if space == "l2":
        qf, cv = _dev(q[:, :D - 1]), cf[:, :D - 1]
        cn, rho, scale = ops.l2_rows(cv)
        return ops.l2_query_rows(qf, scale), cn, D - 1, dict(eq_f32=qf, ec_f32=cv, rho_c=rho, scale_c=scale)
    qf = _dev(q)
    if space == "dot":
        cn, rho, scale = ops.dot_scaled_rows(cf)
        return ops.l2norm_rows(qf), cn, D, dict(eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale)
    cn, rho = ops.l2norm_rows(cf, return_rho=True)
    return ops.l2norm_rows(qf), cn, D, dict(eq_f32=qf, ec_f32=cf, rho_c=rho)


@pytest.mark.parametrize("space", ["cosine", "dot", "l2"])
def test_topk_is_exactly_the_planted_rows(big, space):
    """cosine_topk / dot_topk / l2_topk at k = 10 (the list kernels) and k = 100 (the large entry) over half rows that cross 2^32
    bytes: planted rows sit in the last tile below the boundary, in the row that straddles it, above it and in the last rows"""
    cf = big.flat()
    qu, cn, d, kw = _operands(space, cf)
    fn = {"cosine": ops.cosine_topk, "dot": ops.dot_topk, "l2": ops.l2_topk}[space]
    for k in (10, 100):
        s, i, st = fn(qu, cn, d, k, return_status=True, **kw)
        torch.cuda.synchronize()
        s, i, st = s.cpu().numpy(), i.cpu().numpy(), st.cpu().numpy()
        print(f"{space} k={k}: status {st.tolist()}")
        rs, ri = _planted_lists(space, k)
        np.testing.assert_array_equal(i, ri)
        np.testing.assert_array_equal(s.view(np.uint32), rs.view(np.uint32))
        assert np.isin(st, (0, 1, 2)).all(), st
    beyond = fc.large_inputs()[2] >= fc.LARGE_HALF_ROW
    assert beyond.sum() >= 5 and np.isin(fc.large_inputs()[2][beyond], ri).all()      # rows beyond 2^32 bytes are in the lists


def test_cosine_range_is_exactly_the_planted_rows(big):
    """cosine_range with the threshold in the middle of the margin: all 128 planted rows for every query, nothing else"""
    cf = big.flat()
    q, block, pos, planted = fc.large_inputs()
    tau = 0.5 * (float(fc.scores("cosine", q, block).max()) + float(fc.scores("cosine", q, planted).min()))
    qu, cn, d, kw = _operands("cosine", cf)
    lims, s, i, st = ops.cosine_range(qu, cn, d, tau, return_status=True, **kw)
    torch.cuda.synchronize()
    lims, s, i, st = lims.cpu().numpy(), s.cpu().numpy(), i.cpu().numpy(), st.cpu().numpy()
    print(f"cosine_range tau={tau:.4f}: hits {np.diff(lims).tolist()} status {st.tolist()}")
    rs, ri = _planted_lists("cosine", fc.LARGE_PLANTS)
    np.testing.assert_array_equal(lims, np.arange(fc.Q + 1) * fc.LARGE_PLANTS)
    np.testing.assert_array_equal(i.reshape(fc.Q, -1), ri)
    np.testing.assert_array_equal(s.reshape(fc.Q, -1).view(np.uint32), rs.view(np.uint32))
    assert np.isin(st, (1, 2)).all(), st


# ------------------------------------------------------------------------------------------------- the graph adjacency
GRAPH_ITERS, GRAPH_WIDTH, GRAPH_EF, GRAPH_K = 20, 4, 64, 10
GRAPH_ENTRIES = np.array([(1 << 24) + o for o in (-520, -300, -33, -1, 0, 1, 31, 290, 610)] + [GRAPH_N - 1500, GRAPH_N - 1200, -1],
                         dtype=np.int64)


@pytest.mark.parametrize("space", ["cosine", "dot", "l2"])
def test_graph_search_adjacency_beyond_4gib(big, space):
    g, rows = big.graph()
    W = 32 * (GRAPH_ITERS + 2)
    ent = GRAPH_ENTRIES[GRAPH_ENTRIES >= 0]
    U = np.unique(np.concatenate([np.arange(e - W, e + W + 1) for e in ent]))
    assert U[0] >= 32 and U[-1] < GRAPH_N - 32 and U.size < 8000             # the windows stay clear of the ring's seam
    assert (U < 1 << 24).sum() > 500 and (U >= 1 << 24).sum() > 500
    Ud = torch.from_numpy(U).to(DEV)
    c_loc = rows[Ud].cpu().numpy()
    g_glob = g[Ud].cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(g_glob[:, :32], U[:, None] + np.arange(1, 33)[None, :])      # the lattice, as written
    np.testing.assert_array_equal(g_glob[:, 32:], U[:, None] - np.arange(1, 33)[None, :])
    at = np.searchsorted(U, g_glob)
    inside = (at < U.size) & (U[np.minimum(at, U.size - 1)] == g_glob)
    g_loc = np.where(inside, at, -1)                                         # (edges out of the windows: never reached, see above)
    # the queries: rows around the boundary, so that the beams stay there; one near the end of the adjacency
    qrows = np.array([(1 << 24) + o for o in (-400, -40, -2, 0, 3, 45, 500)] + [GRAPH_N - 1300])
    q = (rows[torch.from_numpy(qrows).to(DEV)].cpu().numpy() + np.float32(0.05)).astype(np.float32)
    e_loc = np.where(GRAPH_ENTRIES >= 0, np.searchsorted(U, np.maximum(GRAPH_ENTRIES, 0)), -1)
    rs, ri, rst, visits = graph_search_ref(space, q, c_loc, g_loc, e_loc, GRAPH_EF, GRAPH_WIDTH, GRAPH_ITERS, GRAPH_K, return_visits=True)
    ri = np.where(ri >= 0, U[np.maximum(ri, 0)], -1)
    assert visits.min() > 4 * GRAPH_R and (ri >= 1 << 24).any() and (ri < 1 << 24).any()
    s, i, st = ops.graph_search(space, _dev(q), rows, g, _dev(GRAPH_ENTRIES, np.int32), GRAPH_K, GRAPH_EF, width=GRAPH_WIDTH,
                                max_iters=GRAPH_ITERS, return_status=True)
    torch.cuda.synchronize()
    print(f"graph {space}: visits {visits.tolist()} status {st.tolist()}")
    np.testing.assert_array_equal(i.cpu().numpy(), ri)
    np.testing.assert_array_equal(s.cpu().numpy().view(np.uint32), rs.view(np.uint32))
    np.testing.assert_array_equal(st.cpu().numpy(), rst)
