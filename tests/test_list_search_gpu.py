"""Exact top-k within candidate lists on the GPU (ops.cosine_list_topk / dot_list_topk / l2_list_topk): every result — scores
and indices — is compared bit for bit with the numpy oracle of tests/list_cases.py.  No tolerance anywhere.

Shapes.  N = 5 000 rows.  The width test scores, once per (space, d), query j against the first 2 S + 1 rows of its own fixed
permutation of the corpus (S = TSIM_LIST_SLICE read from the header): a list of length L of query j is the first L entries of
that permutation, so every list of every (Q, k) case of the test is a prefix of what was scored once."""
import functools

import numpy as np
import pytest
import torch

from list_cases import ST_LIMS, ST_ROW, csr, header_define, list_topk_ref, pair_scores, rank_list, same_bits
from text_similarity_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 5000
S = header_define("TSIM_LIST_SLICE")
SL_NB = 1024
QS = (1, 5, 70)
KS = (1, 10, 64, 65, 1024)
WIDTHS = (1, 63, 64, 65, 300, 384, 385, 768)
FN = {"cosine": ops.cosine_list_topk, "dot": ops.dot_list_topk, "l2": ops.l2_list_topk}
PAD = 37


def _lengths(k):
    return [0, 1, k - 1, k, k + 1, 63, 64, 65, SL_NB - 1, SL_NB, SL_NB + 1, S - 1, S, S + 1, 2 * S + 1]


def _n_rows():
    return N if 2 * S + 1 <= N else 2 * S + 2


@functools.lru_cache(maxsize=None)
def _rows(d, n=N, nq=max(QS)):
    rng = np.random.default_rng(100 + d)
    c = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    return q, c


@functools.lru_cache(maxsize=None)
def _prefix_scores(space, d):
    """(perm [Qmax, M], scores [Qmax, M]): query j against the first M = 2 S + 1 rows of its own permutation."""
    n = _n_rows() if S > N else N
    q, c = _rows(d, n)
    M = 2 * S + 1
    rng = np.random.default_rng(7)
    perm = np.stack([rng.permutation(n)[:M] for _ in range(q.shape[0])])
    sc = np.empty(perm.shape, dtype=np.float32)
    for j in range(q.shape[0]):
        sc[j] = pair_scores(space, q, c, np.full((M,), j), perm[j])
    return perm, sc


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _run(space, qf, cf, cand, lims=None, **kw):
    out = FN[space](qf, cf, cand, lims, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _assert_same(got_s, got_i, ref_s, ref_i, what):
    assert (got_i == ref_i).all(), (what, np.argwhere(got_i != ref_i)[:5])
    assert same_bits(got_s, ref_s), (what, np.argwhere(got_s.view(np.int32) != ref_s.view(np.int32))[:5])


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("space", ["cosine", "dot", "l2"])
def test_widths_lengths_and_k(space, d):
    """The lane tail and both NI paths (d), one to many queries, every k regime of the LDS list (64 = one bitonic block, 65 the
    next power of two, 1 024 the cap), and list lengths around k, a wave, a block of the list and one, two and three slices."""
    if space == "l2" and d == 768:
        d = 767      # the Euclidean limit (tsim_l2_topk_ex)
    if S > N and d != 64:
        pytest.skip("TSIM_LIST_SLICE > 5 000: the slice boundaries are covered at d = 64 alone")
    perm, sc = _prefix_scores(space, d)
    q, c = _rows(d, _n_rows() if S > N else N)
    qf, cf = _dev(q), _dev(c)
    for k in KS:
        lens = _lengths(k)
        for Q in QS:
            ncalls = -(-len(lens) // Q)
            for call in range(ncalls):
                ls = [lens[(call * Q + j) % len(lens)] for j in range(Q)]
                lists = [perm[j, :ls[j]] for j in range(Q)]
                cand, lims = csr(lists)
                s, i, st = _run(space, qf[:Q], cf, _dev(cand), _dev(lims), k=k, return_status=True, assume_unique=True)
                for j in range(Q):
                    rs, ri = rank_list(space, lists[j], sc[j, :ls[j]], k)
                    _assert_same(s[j], i[j], rs, ri, (space, d, k, Q, call, j, ls[j]))
                assert not st.any()


@functools.lru_cache(maxsize=None)
def _tied_rows(d=65):
    rng = np.random.default_rng(5)
    c = rng.standard_normal((N, d)).astype(np.float32)
    c[17] = 0.0                      # a zero row: cosine 0 by the eps rule
    c[[40, 999, 1024, 3000, 4999]] = c[39]       # five copies of one row
    q = rng.standard_normal((6, d)).astype(np.float32)
    q[2] = c[39]
    q[3] = 0.0
    return q, c


def _full_search(space, qf, cf, k):
    d = qf.shape[1]
    if space == "cosine":
        cn, rho = ops.l2norm_rows(cf, return_rho=True)
        return ops.cosine_topk(ops.l2norm_rows(qf), cn, d, k, eq_f32=qf, ec_f32=cf, rho_c=rho)
    if space == "dot":
        cn, rho, scale = ops.dot_scaled_rows(cf)
        return ops.dot_topk(ops.l2norm_rows(qf), cn, d, k, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale)
    cn, rho, scale = ops.l2_rows(cf)
    return ops.l2_topk(ops.l2_query_rows(qf, scale), cn, d, k, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale)


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("space", ["cosine", "dot", "l2"])
def test_full_list_equals_the_full_search(space, k):
    q, c = _tied_rows()
    qf, cf = _dev(q), _dev(c)
    fs, fi = _full_search(space, qf, cf, k)
    torch.cuda.synchronize()
    fs, fi = fs.cpu().numpy(), fi.cpu().numpy()
    rs, ri, _ = list_topk_ref(space, q, c, np.arange(N), k)
    _assert_same(fs, fi, rs, ri, "full search vs oracle")
    full = torch.arange(N, device=DEV)
    s, i = _run(space, qf, cf, full, k=k)
    _assert_same(s, i, fs, fi, "shared arange")
    cand, lims = csr([np.arange(N)] * q.shape[0])
    s, i = _run(space, qf, cf, _dev(cand), _dev(lims), k=k)
    _assert_same(s, i, fs, fi, "CSR arange")
    s, i = _run(space, qf, cf, _dev(cand), _dev(lims), k=k, assume_unique=True)
    _assert_same(s, i, fs, fi, "CSR arange, untouched")


@pytest.mark.parametrize("space", ["cosine", "dot", "l2"])
def test_forms_dtypes_offset_and_views(space):
    d, Q, k, m = 300, 5, 10, 1500
    q, c = _rows(d)
    q = q[:Q]
    rng = np.random.default_rng(11)
    shared = rng.permutation(N)[:m]
    rs, ri, _ = list_topk_ref(space, q, c, shared, k)
    qf, cf = _dev(q), _dev(c)
    for uniq in (False, True):
        kw = dict(k=k, assume_unique=uniq)
        s, i = _run(space, qf, cf, _dev(shared), **kw)
        _assert_same(s, i, rs, ri, ("shared", uniq))
        cand, lims = csr([shared] * Q)
        s, i = _run(space, qf, cf, _dev(cand), _dev(lims), **kw)
        _assert_same(s, i, rs, ri, ("replicated CSR", uniq))
        s, i = _run(space, qf, cf, _dev(np.tile(shared, (Q, 1))), **kw)
        _assert_same(s, i, rs, ri, ("2-D", uniq))
        s, i = _run(space, qf, cf, _dev(shared.astype(np.int32)), **kw)
        _assert_same(s, i, rs, ri, ("shared int32", uniq))
        s, i = _run(space, qf, cf, _dev(cand.astype(np.int32)), _dev(lims), **kw)
        _assert_same(s, i, rs, ri, ("CSR int32", uniq))
        s, i = _run(space, qf, cf, _dev(np.tile(shared, (Q, 1)).astype(np.int32)), **kw)
        _assert_same(s, i, rs, ri, ("2-D int32", uniq))
        s, i = _run(space, qf, cf, _dev(shared), idx_offset=10 ** 10, **kw)
        _assert_same(s, i, rs, ri + 10 ** 10, ("idx_offset", uniq))
    # different lists per query, in the 2-D form padded with -1
    lists = [rng.permutation(N)[:n] for n in (m, 3, 0, 700, 64)]
    rs, ri, _ = list_topk_ref(space, q, c, lists, k)
    two_d = np.full((Q, m), -1, dtype=np.int64)
    for j, l in enumerate(lists):
        two_d[j, :len(l)] = l
    for uniq in (False, True):
        s, i = _run(space, qf, cf, _dev(two_d), k=k, assume_unique=uniq)
        _assert_same(s, i, rs, ri, ("2-D padded", uniq))
    # strided views of wider buffers whose other columns hold NaN and 1e30 (tests/test_search_strided_gpu.py)
    def view(x, off):
        buf = np.empty((x.shape[0], d + PAD), dtype=np.float32)
        buf[:, 0::2] = np.nan
        buf[:, 1::2] = 1e30
        buf[:, off:off + d] = x
        v = _dev(buf)[:, off:off + d]
        assert v.stride() == (d + PAD, 1) and not v.is_contiguous()
        return v
    cand, lims = csr(lists)
    for qv, cv in ((view(q, 1), view(c, 1)), (view(q, 0), cf), (qf, view(c, 1))):
        s, i = _run(space, qv, cv, _dev(cand), _dev(lims), k=k)
        _assert_same(s, i, rs, ri, "views")
    with pytest.raises(_lib.TsimError):
        FN[space](torch.from_numpy(q), torch.from_numpy(c), torch.from_numpy(shared), k=k)


@pytest.mark.parametrize("space", ["cosine", "dot", "l2"])
def test_ties_go_to_the_lowest_rows(space):
    """200 copies of one row and 50 others, k = 100: the copies score exactly alike by construction (the same bits in, the
    same arithmetic), so the answer is the 100 lowest row numbers among them — checked on the CPU first."""
    d, k = 70, 100
    rng = np.random.default_rng(23)
    c = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((2, d)).astype(np.float32)
    copies = np.sort(rng.permutation(N)[:200])
    c[copies] = q[0] * np.float32(2.0)                     # query 0's own direction: ahead of every other row in all three spaces
    others = np.setdiff1d(rng.permutation(N)[:400], copies)[:50]
    q[1] = q[0]
    lst = rng.permutation(np.concatenate([copies, others]))
    c[others] = -c[others] if space != "l2" else c[others] + np.float32(50.0)
    rs, ri, _ = list_topk_ref(space, q, c, [lst, lst[::-1].copy()], k)
    assert np.isin(ri, copies).all() and (ri == np.sort(copies)[:k]).all()        # the oracle's top 100 are all copies
    assert (rs == rs[0, 0]).all()
    cand, lims = csr([lst, lst[::-1]])
    for uniq in (False, True):
        s, i = _run(space, _dev(q), _dev(c), _dev(cand), _dev(lims), k=k, assume_unique=uniq)
        _assert_same(s, i, rs, ri, ("ties", uniq))
        assert (i == np.sort(copies)[:k]).all()


@pytest.mark.parametrize("space", ["cosine", "dot", "l2"])
def test_entries_padding_out_of_range_bad_lims_and_repeats(space):
    d, k = 65, 10
    q, c = _rows(d)
    q = q[:6]
    qf, cf = _dev(q), _dev(c)
    rng = np.random.default_rng(31)
    good = rng.permutation(N)[:40]
    lists = [np.concatenate([[-1, -1], good[:20], [-1], good[20:], [-7]]),       # 0: padding in between
             np.full((33,), -1),                                                # 1: all padding
             np.concatenate([good, [N, N + 10 ** 9, 2 ** 31 - 1]]),              # 2: rows beyond the corpus
             np.array([5, 9, 5, 11, 9, 5]),                                     # 3: repeats
             good[:3],                                                          # 4: fewer than k
             np.zeros((0,), np.int64)]                                          # 5: empty
    cand, lims = csr(lists)
    for uniq in (False, True):
        rs, ri, rst = list_topk_ref(space, q, c, lists, k, unique=not uniq)
        s, i, st = _run(space, qf, cf, _dev(cand), _dev(lims), k=k, return_status=True, assume_unique=uniq)
        _assert_same(s, i, rs, ri, ("entries", uniq))
        assert (st == rst).all() and st.tolist() == [0, 0, ST_ROW, 0, 0, 0], st
        assert (i[1] == -1).all() and (np.isposinf(s[1]) if space == "l2" else np.isneginf(s[1])).all()
        n3 = (i[3] >= 0).sum()
        assert n3 == (6 if uniq else 3)
        if uniq:      # a row listed twice comes out twice, adjacent
            assert sorted(i[3, :6].tolist()) == [5, 5, 5, 9, 9, 11]
            for r in (5, 9):
                at = np.nonzero(i[3] == r)[0]
                assert (np.diff(at) == 1).all() and len(set(s[3, at].view(np.int32).tolist())) == 1
    # int32 candidates: INT32_MAX is the largest entry there is
    c32 = np.concatenate([good, [N, 2 ** 31 - 1]]).astype(np.int32)
    rs, ri, _ = list_topk_ref(space, q, c, good, k)
    for uniq in (False, True):
        s, i, st = _run(space, qf, cf, _dev(c32), k=k, return_status=True, assume_unique=uniq)
        _assert_same(s, i, rs, ri, ("int32 beyond", uniq))
        assert (st == ST_ROW).all()
    # lims: a decreasing pair is an empty list (bit 2), pairs outside [0, T] are clamped
    cand = rng.permutation(N)[:100]
    lims = np.array([0, 30, 20, 60, 60, 500, 500], dtype=np.int64)          # query 1: [30, 20) decreasing
    want = [cand[0:30], cand[0:0], cand[30:60], cand[60:60], cand[60:100], cand[0:0]]
    want_st = [0, ST_LIMS, ST_LIMS, 0, ST_LIMS, ST_LIMS]
    rs, ri, _ = list_topk_ref(space, q, c, want, k)
    for uniq in (False, True):
        s, i, st = _run(space, qf, cf, _dev(cand), _dev(lims), k=k, return_status=True, assume_unique=uniq)
        _assert_same(s, i, rs, ri, ("bad lims", uniq))
        assert st.tolist() == want_st, st
    lims = np.array([-5, 10, 10, 10, 10, 10, 10], dtype=np.int64)
    rs, ri, _ = list_topk_ref(space, q, c, [cand[:10]] + [cand[:0]] * 5, k)
    s, i, st = _run(space, qf, cf, _dev(cand), _dev(lims), k=k, return_status=True, assume_unique=True)
    _assert_same(s, i, rs, ri, "negative lims")
    assert st.tolist() == [ST_LIMS, 0, 0, 0, 0, 0]


def test_round_trip_of_a_search_result():
    """idx of cosine_topk(k = 50) fed back as a 2-D cand with k = 10 reproduces the first 10 columns."""
    q, c = _tied_rows()
    qf, cf = _dev(q), _dev(c)
    fs, fi = _full_search("cosine", qf, cf, 50)
    for uniq in (False, True):
        s, i = ops.cosine_list_topk(qf, cf, fi, k=10, assume_unique=uniq)
        assert torch.equal(i, fi[:, :10]) and torch.equal(s.view(torch.int32), fs[:, :10].contiguous().view(torch.int32))
    short, si = _full_search("cosine", qf, cf[:30], 50)      # -1 padded beyond 30 rows
    assert (si[:, 30:] == -1).all()
    s, i = ops.cosine_list_topk(qf, cf, si, k=40, assume_unique=True)
    assert torch.equal(i, si[:, :40]) and torch.equal(s.view(torch.int32), short[:, :40].contiguous().view(torch.int32))
