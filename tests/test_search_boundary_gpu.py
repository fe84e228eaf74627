"""One widening and brute-force path serves every k: results on both sides of the k = 28 / 29 (list kernels) and k = 64 / 65
(_ex / _large entries) boundaries agree with the oracle bit for bit and with each other.  Corpora: Gaussian rows (widening
resolves), 1 500 near-ties of query 0 (more than the 1 024 entries a slot collects: brute force, status 2), and a shard too
small for the block-maxima bound (every query brute force for k > 28).  Spaces: cosine and dot on the float32 rows, unit rows
alone, squared Euclidean distance.  Then the edges of the tail itself: a slot filled exactly, k = 1, a NaN corpus row."""
import functools

import numpy as np
import pytest
import torch

from l2_cases import l2_topk_ref
from oracle.search_ref import _lane_sum, cosine_topk, cosine_topk_f32, topk_rows, unit_rows
from text_similarity_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, Q, KMAX = 256, 8, 128
KS = (10, 28, 29, 64, 65, 128)
CORPORA = ("gauss", "near_ties", "small")


@functools.lru_cache(maxsize=None)
def _rows(corpus, ndup=1500):
    rng = np.random.default_rng(1729)
    c = rng.standard_normal((6000, D)).astype(np.float32)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    if corpus == "near_ties":
        base = rng.standard_normal(D).astype(np.float32)
        c[500:500 + ndup] = base + 1e-6 * rng.standard_normal((ndup, D)).astype(np.float32)
        q[0] = base
    elif corpus == "small":
        c = c[:900].copy()
    return q, c


def _search(corpus, space, k, rows=None):
    q, c = rows if rows is not None else _rows(corpus)
    qf, cf = torch.from_numpy(q).to(DEV), torch.from_numpy(c).to(DEV)
    if space == "dot":
        cn, rho, scale = ops.dot_scaled_rows(cf)
        s, i, st = ops.dot_topk(ops.l2norm_rows(qf), cn, D, k, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale, return_status=True)
    elif space == "l2":
        cn, rho, scale = ops.l2_rows(cf)
        s, i, st = ops.l2_topk(ops.l2_query_rows(qf, scale), cn, D, k, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale, return_status=True)
    elif space == "unit":   # no float32 matrices: the scores of the unit rows as stored
        cu, rho = ops.l2norm_rows(cf, return_rho=True)
        s, i, st = ops.cosine_topk(ops.l2norm_rows(qf), cu, D, k, rho_c=rho, return_status=True)
    else:
        cu, rho = ops.l2norm_rows(cf, return_rho=True)
        s, i, st = ops.cosine_topk(ops.l2norm_rows(qf), cu, D, k, eq_f32=qf, ec_f32=cf, rho_c=rho, return_status=True)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy(), st.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _widest(corpus, space):
    return _search(corpus, space, KMAX)


@functools.lru_cache(maxsize=None)
def _oracle_widest(corpus, space):
    """The oracle's k = 128 lists; it sorts by (score desc, index asc), so its k lists are their first k columns."""
    q, c = _rows(corpus)
    if space == "cosine":
        return cosine_topk_f32(q, c, KMAX)
    if space == "unit":
        return cosine_topk(unit_rows(q), unit_rows(c), KMAX)
    if space == "l2":   # distances ascending, ties to the lower index
        return l2_topk_ref(q, c, KMAX)
    # float32(q.c) summed in float64 in the canonical lane order (tests/test_topk_large_gpu.py dot_topk_ref)
    return topk_rows(_lane_sum(q[:, None, :], c[None, :, :]).astype(np.float32), KMAX)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("space", ["cosine", "dot", "unit", "l2"])
@pytest.mark.parametrize("corpus", CORPORA)
def test_every_k_matches_oracle_and_k128_prefix(corpus, space, k):
    s, i, st = _search(corpus, space, k)
    rs, ri = _oracle_widest(corpus, space)
    print(f"{corpus} {space} k={k}: status {st.tolist()}")
    np.testing.assert_array_equal(i, ri[:, :k])
    np.testing.assert_array_equal(s, rs[:, :k])
    ws, wi, _ = _widest(corpus, space)
    np.testing.assert_array_equal(i, wi[:, :k])
    np.testing.assert_array_equal(s, ws[:, :k])
    # which pass served the queries: the list kernels or the widening pass on Gaussian rows (never brute force; k > 28 has
    # no list kernel), brute force for the near-ties and, for k > 28, for every query of the small shard
    if corpus == "gauss":
        assert (st == 1).all() if k > 28 else (st <= 1).all(), st
    if corpus == "near_ties":
        assert st[0] == 2, st
    if corpus == "small" and k > 28:
        assert (st == 2).all(), st


@pytest.mark.parametrize("ndup", [1023, 1024, 1025])
def test_slot_filled_exactly(ndup):
    """Query 0 has ndup near-ties around the 1 024 entries a slot collects: one below, exactly, one above (cosine, k = 40)."""
    q, c = _rows("near_ties", ndup)
    s, i, st = _search("near_ties", "cosine", 40, rows=(q, c))
    print(f"ndup={ndup}: status {st.tolist()}")   # query 0: how many other rows fall into the band depends on the data
    rs, ri = cosine_topk_f32(q, c, 40)
    np.testing.assert_array_equal(i, ri)
    np.testing.assert_array_equal(s, rs)


def test_k1_small_shard():
    """k = 1: the k-th entry of every list is its first."""
    s, i, st = _search("small", "dot", 1)
    rs, ri = _oracle_widest("small", "dot")
    print(f"small dot k=1: status {st.tolist()}")
    np.testing.assert_array_equal(i, ri[:, :1])
    np.testing.assert_array_equal(s, rs[:, :1])


@pytest.mark.parametrize("k", [10, 40])
def test_nan_corpus_row_is_never_returned(k):
    """A NaN in one corpus row sends every query to brute force, which returns the lists over the other 5 999 rows."""
    q, c = _rows("gauss")
    c = c.copy()
    c[17, 3] = np.nan
    s, i, st = _search("gauss", "dot", k, rows=(q, c))
    print(f"nan row k={k}: status {st.tolist()}")
    ref = _lane_sum(q[:, None, :], c[None, :, :]).astype(np.float32)
    assert np.isnan(ref[:, 17]).all() and not np.isnan(np.delete(ref, 17, axis=1)).any()
    ref[:, 17] = -np.inf   # the other rows keep their row numbers
    rs, ri = topk_rows(ref, k)
    np.testing.assert_array_equal(i, ri)
    np.testing.assert_array_equal(s, rs)
    assert (st == 2).all(), st
