"""Float32 rows that are VIEWS of wider buffers.  Every exact re-score kernel takes the row strides ldq / ldc of the float32
matrices, and ops passes stride(0) through (only stride(1) == 1 is required) — a Matryoshka-style truncated view emb[:, :256]
of wider rows is a legal input — but every other test passes ld == d.  Here the embeddings are buf[:, off:off + d] of a
[rows, d + 37] buffer (off = 1: the base is only 4-byte aligned) whose unused columns hold NaN and 1e30, so a kernel that used
d where it should use ld, or read past a row's d elements, cannot return the right bits.

The corpora are those of tests/test_search_boundary_gpu.py (same recipe and seed, at d = 256 and 300), so the first pass, the
widening pass and brute force all run: Gaussian rows; 1 500 near-ties of query 0 (brute force); a 900-row shard (brute force
for k > 28).  Bars: scores and indices array_equal to the run on .contiguous() copies AND to the oracle; the statuses are the
ones that file asserts."""
import functools

import numpy as np
import pytest
import torch

from oracle.search_ref import _lane_sum, cosine_topk_f32, exact_cosine, topk_rows
from text_similarity_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q, PAD = 8, 37
KS = (10, 29, 100)
CORPORA = ("gauss", "near_ties", "small")
VIEWS = ((256, 0), (256, 1), (300, 0), (300, 1))


@functools.lru_cache(maxsize=None)
def _rows(corpus, d):
    rng = np.random.default_rng(1729)
    c = rng.standard_normal((6000, d)).astype(np.float32)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    if corpus == "near_ties":
        base = rng.standard_normal(d).astype(np.float32)
        c[500:2000] = base + 1e-6 * rng.standard_normal((1500, d)).astype(np.float32)
        q[0] = base
    elif corpus == "small":
        c = c[:900].copy()
    return q, c


def _view(x, off):
    """x [rows, d] as a device view buf[:, off:off + d] of a [rows, d + PAD] buffer filled with NaN and 1e30 elsewhere."""
    rows, d = x.shape
    buf = np.empty((rows, d + PAD), dtype=np.float32)
    buf[:, 0::2] = np.nan
    buf[:, 1::2] = 1e30
    buf[:, off:off + d] = x
    v = torch.from_numpy(buf).to(DEV)[:, off:off + d]
    assert v.stride() == (d + PAD, 1) and not v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16
    return v


def _dot_scores(q, c):
    return np.concatenate([_lane_sum(q[a:a + 2, None, :], c[None, :, :]).astype(np.float32) for a in range(0, q.shape[0], 2)])


@functools.lru_cache(maxsize=None)
def _exact(corpus, d, space):
    q, c = _rows(corpus, d)
    return exact_cosine(q, c) if space == "cosine" else _dot_scores(q, c)


@functools.lru_cache(maxsize=None)
def _oracle(corpus, d, space):
    """The oracle's k = 100 lists, sorted by (score desc, index asc): its k lists are their first k columns."""
    if space == "cosine":
        return cosine_topk_f32(*_rows(corpus, d), max(KS))
    return topk_rows(_exact(corpus, d, space), max(KS))


def _operands(space, qf, cf):
    """Unit / scaled half rows made FROM the views (the row kernels copy); the views themselves are the float32 operands."""
    if space == "dot":
        cn, rho, scale = ops.dot_scaled_rows(cf)
        return ops.l2norm_rows(qf), cn, dict(rho_c=rho, scale_c=scale)
    cn, rho = ops.l2norm_rows(cf, return_rho=True)
    return ops.l2norm_rows(qf), cn, dict(rho_c=rho)


def _topk(space, qf, cf, k):
    d = qf.shape[1]
    qu, cn, kw = _operands(space, qf, cf)
    fn = ops.dot_topk if space == "dot" else ops.cosine_topk
    s, i, st = fn(qu, cn, d, k, eq_f32=qf, ec_f32=cf, return_status=True, **kw)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy(), st.cpu().numpy()


def _range(space, qf, cf, tau):
    d = qf.shape[1]
    qu, cn, kw = _operands(space, qf, cf)
    fn = ops.dot_range if space == "dot" else ops.cosine_range
    r = fn(qu, cn, d, tau, eq_f32=qf, ec_f32=cf, return_status=True, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in r)


def _check_status(corpus, k, st):
    """tests/test_search_boundary_gpu.py: which pass served the queries"""
    if corpus == "gauss":
        assert (st == 1).all() if k > 28 else (st <= 1).all(), st
    if corpus == "near_ties":
        assert st[0] == 2, st
    if corpus == "small" and k > 28:
        assert (st == 2).all(), st


@pytest.mark.parametrize("d,off", VIEWS)
@pytest.mark.parametrize("space", ["cosine", "dot"])
@pytest.mark.parametrize("corpus", CORPORA)
def test_topk_on_views_matches_contiguous_and_oracle(corpus, space, d, off):
    q, c = _rows(corpus, d)
    qv, cv = _view(q, off), _view(c, off)
    qc, cc = qv.contiguous(), cv.contiguous()
    rs, ri = _oracle(corpus, d, space)
    for k in KS:
        s, i, st = _topk(space, qv, cv, k)
        cs, ci, cst = _topk(space, qc, cc, k)
        print(f"{corpus} {space} d={d} off={off} k={k}: status {st.tolist()} (contiguous {cst.tolist()})")
        np.testing.assert_array_equal(i, ci)
        np.testing.assert_array_equal(s, cs)
        np.testing.assert_array_equal(i, ri[:, :k])
        np.testing.assert_array_equal(s, rs[:, :k])
        np.testing.assert_array_equal(st, cst)
        _check_status(corpus, k, st)


@pytest.mark.parametrize("which", ["queries", "corpus"])
@pytest.mark.parametrize("space", ["cosine", "dot"])
def test_topk_with_one_side_strided(space, which):
    """ldq != ldc: only the queries, or only the corpus, are views (d = 300, off = 1; near-ties: every pass runs)."""
    d, corpus = 300, "near_ties"
    q, c = _rows(corpus, d)
    qf = _view(q, 1) if which == "queries" else torch.from_numpy(q).to(DEV)
    cf = _view(c, 1) if which == "corpus" else torch.from_numpy(c).to(DEV)
    assert qf.stride(0) != cf.stride(0)
    rs, ri = _oracle(corpus, d, space)
    for k in KS:
        s, i, st = _topk(space, qf, cf, k)
        print(f"{which} strided, {space} k={k}: status {st.tolist()}")
        np.testing.assert_array_equal(i, ri[:, :k])
        np.testing.assert_array_equal(s, rs[:, :k])
        _check_status(corpus, k, st)


@pytest.mark.parametrize("space", ["cosine", "dot"])
def test_one_row_with_a_meaningless_row_stride(space):
    """A [1, d] tensor may carry any stride(0): numpy's x[None] has 0 and contiguous() keeps it.  ops must hand the kernels
    a valid ld (found by tests/test_search_subnormal_gpu.py: l2norm_rows refused 'ld_in=0')."""
    d = 300
    q, c = _rows("gauss", d)
    one = torch.as_strided(torch.from_numpy(q[3].copy()).to(DEV), (1, d), (0, 1))
    assert one.stride(0) == 0 and one.is_contiguous()
    cf = torch.from_numpy(c).to(DEV)
    rs, ri = _oracle("gauss", d, space)
    for k in KS:
        s, i, st = _topk(space, one, cf, k)
        np.testing.assert_array_equal(i, ri[3:4, :k])
        np.testing.assert_array_equal(s, rs[3:4, :k])
    exact = _exact("gauss", d, space)[3:4]
    tau = float(np.sort(exact[0])[::-1][5])
    lims, s, i, st = _range(space, one, cf, tau)
    ref = _range_ref(exact, tau)[0]
    assert lims.tolist() == [0, 6]
    np.testing.assert_array_equal(i, ref)
    np.testing.assert_array_equal(s.view(np.uint32), exact[0, ref].view(np.uint32))
    # the row kernels on their own: the same bits as for the row inside its matrix
    want = _operands(space, torch.from_numpy(q).to(DEV), cf[:64])[0][3:4]
    assert torch.equal(ops.l2norm_rows(one), want)
    if space == "dot":
        crow = torch.as_strided(cf[17].clone(), (1, d), (0, 1))
        rows, rho, scale = ops.dot_scaled_rows(crow)
        wrows, wrho, wscale = ops.dot_scaled_rows(cf[17:18].clone())
        assert torch.equal(rows, wrows) and torch.equal(rho, wrho) and torch.equal(scale, wscale)


def _range_ref(exact, tau):
    """tests/test_range_search_gpu.py range_ref: per query the rows with score >= float32(tau), (score desc, index asc)."""
    out = []
    for s in exact:
        hit = np.nonzero(s >= np.float32(tau))[0]
        out.append(hit[np.lexsort((hit, -s[hit].astype(np.float64)))])
    return out


@pytest.mark.parametrize("d,off", VIEWS)
@pytest.mark.parametrize("space", ["cosine", "dot"])
@pytest.mark.parametrize("corpus", CORPORA)
def test_range_on_views_matches_contiguous_and_oracle(corpus, space, d, off):
    """A selective tau (query 1's exact score at rank 5: six hits there, '>=' meets a tie on tau; the near-ties give query 0
    1 500 hits) through the collect path, and on the small shard tau = -inf as well: every row, the exact pass (status 2)."""
    q, c = _rows(corpus, d)
    exact = _exact(corpus, d, space)
    qv, cv = _view(q, off), _view(c, off)
    qc, cc = qv.contiguous(), cv.contiguous()
    taus = [float(np.sort(exact[1])[::-1][5])] + ([float("-inf")] if corpus == "small" else [])
    for tau in taus:
        lims, s, i, st = _range(space, qv, cv, tau)
        clims, cs, ci, cst = _range(space, qc, cc, tau)
        print(f"{corpus} {space} d={d} off={off} tau={tau:.6g}: hits {np.diff(lims).tolist()} status {st.tolist()}")
        np.testing.assert_array_equal(lims, clims)
        np.testing.assert_array_equal(i, ci)
        np.testing.assert_array_equal(s.view(np.uint32), cs.view(np.uint32))
        np.testing.assert_array_equal(st, cst)
        ref = _range_ref(exact, tau)
        np.testing.assert_array_equal(np.diff(lims), [r.size for r in ref])
        for qi, r in enumerate(ref):
            a, b = int(lims[qi]), int(lims[qi + 1])
            np.testing.assert_array_equal(i[a:b], r)
            np.testing.assert_array_equal(s[a:b].view(np.uint32), exact[qi, r].view(np.uint32))
        assert lims[2] - lims[1] == (6 if tau > float("-inf") else c.shape[0])
        assert (st == 2).all() if tau == float("-inf") else np.isin(st, (1, 2)).all(), st
