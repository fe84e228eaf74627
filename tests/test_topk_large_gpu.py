"""GPU parity of top-k for 64 < k <= 1024 (include/tsim.h tsim_cosine_topk_large / tsim_dot_topk_large, tsim_topk_merge_strided
with k_out > 64) and of the layers built on them.  Bar: indices identical and float32 scores bit-identical to the oracle
(oracle/search_ref: cosine_topk_f32 for float32 rows, cosine_topk for unit rows, a test-local dot oracle), ordered by
(score desc, index asc), (-inf, -1) padding when the shard has fewer than k rows."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle.search_ref import _lane_sum, cosine_topk, cosine_topk_f32, topk_rows
from text_similarity_amd import _lib, ops, presets
from text_similarity_amd.index import GpuFlatIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------------- oracles
def dot_topk_ref(q, c, k, idx_offset=0, qblock=8, nblock=4096):
    """float32(q.c) summed in float64 in the canonical lane order, top-k by (score desc, index asc)."""
    q = np.asarray(q, dtype=np.float32)
    c = np.asarray(c, dtype=np.float32)
    sc = np.empty((q.shape[0], c.shape[0]), dtype=np.float32)
    for a in range(0, q.shape[0], qblock):
        for b in range(0, c.shape[0], nblock):
            sc[a:a + qblock, b:b + nblock] = _lane_sum(q[a:a + qblock, None, :], c[None, b:b + nblock, :]).astype(np.float32)
    s, i = topk_rows(sc, k)
    return s, i + idx_offset


def merge_ref(s, i, k_out):
    """topk_merge restated: entries with index < 0 skipped, (score desc, index asc), an entry equal in (score, index) to the
    one before it emitted once, (-inf, -1) padding."""
    nl, Q, _ = s.shape
    out_s = np.full((Q, k_out), -np.inf, dtype=np.float32)
    out_i = np.full((Q, k_out), -1, dtype=np.int64)
    for q in range(Q):
        ss, ii = s[:, q, :].ravel(), i[:, q, :].ravel()
        keep = ii >= 0
        ss, ii = ss[keep], ii[keep]
        order = np.lexsort((ii, -ss.astype(np.float64)))
        got = []
        for o in order:
            e = (ss[o], ii[o])
            if got and got[-1] == e:
                continue
            got.append(e)
            if len(got) == k_out:
                break
        for t, (a, b) in enumerate(got):
            out_s[q, t], out_i[q, t] = a, b
    return out_s, out_i


# ---------------------------------------------------------------------------------------------------------- helpers
def _gauss(rng, n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


def _cos(q, c, k, idx_offset=0):
    qf = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(DEV)
    cf = torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).to(DEV)
    cu, rho = ops.l2norm_rows(cf, return_rho=True)
    s, i, st = ops.cosine_topk(ops.l2norm_rows(qf), cu, q.shape[1], k, eq_f32=qf, ec_f32=cf, rho_c=rho, idx_offset=idx_offset,
                               return_status=True)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy(), st.cpu().numpy()


def _dot(q, c, k, idx_offset=0):
    qf = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(DEV)
    cf = torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).to(DEV)
    cn, rho, scale = ops.dot_scaled_rows(cf)
    s, i, st = ops.dot_topk(ops.l2norm_rows(qf), cn, q.shape[1], k, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale,
                            idx_offset=idx_offset, return_status=True)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy(), st.cpu().numpy()


def _check(got_s, got_i, ref_s, ref_i, k):
    kk = ref_i.shape[1]
    np.testing.assert_array_equal(got_i[:, :kk], ref_i)
    np.testing.assert_array_equal(got_s[:, :kk], ref_s)
    if kk < k:
        assert (got_i[:, kk:] == -1).all() and np.isneginf(got_s[:, kk:]).all()


# ---------------------------------------------------------------------------------------------------------- 1. random rows
@pytest.mark.parametrize("n,k,d", [(3000, 65, 384), (3000, 65, 768), (20000, 100, 384), (20000, 1024, 384), (20000, 300, 128)])
def test_random_rows_cos(n, k, d):
    rng = np.random.default_rng(n + k + d)
    c = _gauss(rng, n, d) * rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    q = _gauss(rng, 12, d)
    s, i, st = _cos(q, c, k, idx_offset=5)
    rs, ri = cosine_topk_f32(q, c, k, idx_offset=5)
    _check(s, i, rs, ri, k)
    print(f"N={n} k={k} d={d}: status counts {np.bincount(st, minlength=3).tolist()}")


def test_large_shard_k256_sampled_queries():
    rng = np.random.default_rng(11)
    n, d, k = 300_000, 384, 256
    c = _gauss(rng, n, d)
    q = _gauss(rng, 64, d)
    s, i, st = _cos(q, c, k)
    assert (st == 1).all(), np.bincount(st, minlength=3)
    sel = [0, 37, 63]
    rs, ri = cosine_topk_f32(q[sel], c, k)
    _check(s[sel], i[sel], rs, ri, k)


def test_unit_rows_mode():
    rng = np.random.default_rng(12)
    n, d, k = 20000, 384, 200
    cu = ops.l2norm_rows(torch.from_numpy(_gauss(rng, n, d)).to(DEV))
    qu = ops.l2norm_rows(torch.from_numpy(_gauss(rng, 16, d)).to(DEV))
    s, i, st = ops.cosine_topk(qu, cu, d, k, return_status=True)
    rs, ri = cosine_topk(qu.float().cpu().numpy(), cu.float().cpu().numpy(), k)
    _check(s.cpu().numpy(), i.cpu().numpy(), rs, ri, k)


@pytest.mark.parametrize("k", [100, 1000])
def test_dot_random_rows(k):
    rng = np.random.default_rng(k)
    n, d = 20000, 384
    c = _gauss(rng, n, d) * rng.uniform(0.2, 3.0, (n, 1)).astype(np.float32)
    q = _gauss(rng, 10, d)
    s, i, st = _dot(q, c, k, idx_offset=3)
    rs, ri = dot_topk_ref(q, c, k, idx_offset=3)
    _check(s, i, rs, ri, k)


# ---------------------------------------------------------------------------------------------------------- 2. small shards
@pytest.mark.parametrize("n,k", [(70, 100), (50, 1024), (1000, 1024), (900, 65)])
def test_small_shards_brute_force(n, k):
    rng = np.random.default_rng(n * 7 + k)
    d = 256
    c = _gauss(rng, n, d)
    q = _gauss(rng, 5, d)
    s, i, st = _cos(q, c, k, idx_offset=11)
    rs, ri = cosine_topk_f32(q, c, k, idx_offset=11)
    _check(s, i, rs, ri, k)
    if n < k:
        assert (st == 2).all()
    s, i, st = _dot(q, c, k)
    rs, ri = dot_topk_ref(q, c, k)
    _check(s, i, rs, ri, k)


# ---------------------------------------------------------------------------------------------------------- 3. ties
def test_identical_rows_straddling_rank_k():
    """1 500 identical rows take ranks 1 .. 1 500: k = 1 000 cuts through them, resolved in index order."""
    rng = np.random.default_rng(21)
    n, d, k = 20000, 384, 1000
    c = _gauss(rng, n, d)
    c[5000:6500] = c[123]
    q = np.concatenate([c[123][None] * 0.5, _gauss(rng, 3, d)]).astype(np.float32)
    s, i, st = _cos(q, c, k)
    rs, ri = cosine_topk_f32(q, c, k)
    _check(s, i, rs, ri, k)
    assert i[0, 0] == 123 and (i[0, 1:k] == np.arange(5000, 5000 + k - 1)).all()
    s, i, st = _dot(q, c, k)
    rs, ri = dot_topk_ref(q, c, k)
    _check(s, i, rs, ri, k)


def test_near_ties_overflow_collection_zero_rows_zero_query():
    rng = np.random.default_rng(22)
    n, d, k = 6000, 256, 100
    base = _gauss(rng, 1, d)[0]
    c = _gauss(rng, n, d)
    c[500:2000] = base + 1e-6 * _gauss(rng, 1500, d)       # 1 500 near-ties: more than the 1 024 a slot collects at k = 100
    c[2100:2110] = c[7]                                     # exact duplicates
    c[2200:2300] = 0.0                                      # zero rows
    q = np.concatenate([base[None], base[None] * 3.0, c[7][None], np.zeros((1, d)), _gauss(rng, 4, d)]).astype(np.float32)
    s, i, st = _cos(q, c, k)
    rs, ri = cosine_topk_f32(q, c, k)
    _check(s, i, rs, ri, k)
    assert st[0] == 2 and st[1] == 2
    s, i, st = _dot(q, c, k)
    rs, ri = dot_topk_ref(q, c, k)
    _check(s, i, rs, ri, k)
    assert st[0] == 2


# ---------------------------------------------------------------------------------------------------------- 4. status
def test_gaussian_k1000_resolved_by_widening():
    rng = np.random.default_rng(31)
    n, d, k = 200_000, 384, 1000
    c = _gauss(rng, n, d)
    q = _gauss(rng, 48, d)
    s, i, st = _cos(q, c, k)
    assert (st == 1).all(), np.bincount(st, minlength=3)
    rs, ri = cosine_topk_f32(q[:2], c, k)
    _check(s[:2], i[:2], rs, ri, k)
    s, i, st = _dot(q, c, k)
    assert (st == 1).all(), np.bincount(st, minlength=3)


# ---------------------------------------------------------------------------------------------------------- 5. workspace
def test_exact_workspace_size_at_full_shape():
    """tsim_topk_large_workspace_bytes is the exact size: canary bytes behind it survive, one byte less is refused."""
    N, d, Q, k = 1_000_000, 384, 300, 1024
    g = torch.Generator(device=DEV).manual_seed(3)
    cu = ops.l2norm_rows(torch.randn((N, d), generator=g, device=DEV))
    qu = ops.l2norm_rows(torch.randn((Q, d), generator=g, device=DEV))
    L = _lib.lib()
    need = L.tsim_topk_large_workspace_bytes(Q, N, k)
    buf = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
    s = torch.empty((Q, k), dtype=torch.float32, device=DEV)
    i = torch.empty((Q, k), dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    args = (qu.data_ptr(), None, 0, Q, cu.data_ptr(), None, 0, None, N, d, 384, k, s.data_ptr(), i.data_ptr(), None, 0,
            buf.data_ptr())
    rc = L.tsim_cosine_topk_large(*args, need, st)
    torch.cuda.synchronize()
    assert rc == 0 and bool((buf[need:] == 0x5A).all())
    s2, i2 = ops.cosine_topk(qu, cu, d, k)
    assert torch.equal(s, s2) and torch.equal(i, i2)
    assert L.tsim_cosine_topk_large(*args, need - 1, st) == 3      # TSIM_ENOMEM


# ---------------------------------------------------------------------------------------------------------- 6. paths agree
@pytest.mark.parametrize("k", [10, 29, 64])
def test_small_k_through_large_entry_is_ex(k):
    rng = np.random.default_rng(41 + k)
    n, d, Q = 30000, 384, 40
    qf = torch.from_numpy(_gauss(rng, Q, d)).to(DEV)
    cf = torch.from_numpy(_gauss(rng, n, d)).to(DEV)
    cu, rho = ops.l2norm_rows(cf, return_rho=True)
    cn, drho, scale = ops.dot_scaled_rows(cf)
    qu = ops.l2norm_rows(qf)
    L = _lib.lib()
    assert L.tsim_topk_large_workspace_bytes(Q, n, k) == L.tsim_cosine_topk_workspace_bytes(Q, n, k)
    ws = torch.empty((L.tsim_topk_large_workspace_bytes(Q, n, k),), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    outs = []
    for fn in (L.tsim_cosine_topk_ex, L.tsim_cosine_topk_large, L.tsim_dot_topk_ex, L.tsim_dot_topk_large):
        s = torch.empty((Q, k), dtype=torch.float32, device=DEV)
        i = torch.empty((Q, k), dtype=torch.int64, device=DEV)
        status = torch.empty((Q,), dtype=torch.int32, device=DEV)
        dot = fn in (L.tsim_dot_topk_ex, L.tsim_dot_topk_large)
        head = (qu.data_ptr(), qf.data_ptr(), d, Q, (cn if dot else cu).data_ptr(), cf.data_ptr(), d)
        words = (scale.data_ptr(), drho.data_ptr()) if dot else (rho.data_ptr(),)
        rc = fn(*head, *words, n, d, 384, k, s.data_ptr(), i.data_ptr(), status.data_ptr(), 0, ws.data_ptr(), ws.numel(), st)
        assert rc == 0
        torch.cuda.synchronize()
        outs.append((s.cpu(), i.cpu(), status.cpu()))
    for a, b in ((0, 1), (2, 3)):
        for x, y in zip(outs[a], outs[b]):
            assert torch.equal(x, y)


def test_independent_of_query_slicing_and_idx_offset(monkeypatch):
    rng = np.random.default_rng(51)
    n, d, k = 20000, 384, 500
    q = _gauss(rng, 40, d)
    c = _gauss(rng, n, d)
    s0, i0, st0 = _cos(q, c, k)
    s1, i1, st1 = _cos(q, c, k, idx_offset=1_000_000)
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(i1, i0 + 1_000_000)
    one = ops._lib.lib().tsim_topk_large_workspace_bytes(1, n, k)
    monkeypatch.setattr(ops, "MAX_LARGE_WORKSPACE", 7 * one)      # slices of a few queries
    s2, i2, st2 = _cos(q, c, k)
    np.testing.assert_array_equal(s2, s0)
    np.testing.assert_array_equal(i2, i0)
    np.testing.assert_array_equal(st2, st0)


# ---------------------------------------------------------------------------------------------------------- 7. merge
@pytest.mark.parametrize("nlists,k_in,k_out", [(1, 300, 100), (2, 100, 150), (7, 64, 200), (40, 50, 1024), (7, 200, 65)])
def test_topk_merge_large(nlists, k_in, k_out):
    rng = np.random.default_rng(nlists * 1000 + k_in + k_out)
    Q = 9
    s = np.round(rng.standard_normal((nlists, Q, k_in)) * 4.0).astype(np.float32) / 4   # coarse: many equal scores
    i = rng.integers(0, 3 * k_in, (nlists, Q, k_in)).astype(np.int64)
    i[rng.random(i.shape) < 0.1] = -1                     # skipped entries
    if nlists > 1:                                        # exact (score, index) duplicates across lists
        s[1, :, :10], i[1, :, :10] = s[0, :, :10], np.abs(i[0, :, :10])
    s[:, 0, :] = -np.inf                                  # a query with -inf scores on real indices
    i[:, 1, :] = -1                                       # a query with nothing at all
    for l in range(nlists):                               # each list sorted by (score desc, index asc)
        for qq in range(Q):
            o = np.lexsort((i[l, qq], -s[l, qq].astype(np.float64)))
            s[l, qq], i[l, qq] = s[l, qq][o], i[l, qq][o]
    rs, ri = merge_ref(s, i, k_out)
    gs, gi = ops.topk_merge(torch.from_numpy(s).to(DEV), torch.from_numpy(i).to(DEV), k_out)
    np.testing.assert_array_equal(gi.cpu().numpy(), ri)
    np.testing.assert_array_equal(gs.cpu().numpy(), rs)


# ---------------------------------------------------------------------------------------------------------- 8. surfaces
def test_flat_index_knn_query_k100_both_spaces():
    rng = np.random.default_rng(61)
    d, n = 384, 3000
    x = _gauss(rng, n, d) * rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    q = _gauss(rng, 10, d)
    labels = np.arange(n, dtype=np.int64) + 7000
    for space in ("cosine", "ip"):
        idx = GpuFlatIndex(space=space, dim=d, device=DEV)
        idx.init_index(max_elements=n)
        idx.add_items(x, labels)
        lab, dist = idx.knn_query(q, k=100)
        rs, ri = cosine_topk_f32(q, x, 100) if space == "cosine" else dot_topk_ref(q, x, 100)
        np.testing.assert_array_equal(lab, labels[ri])
        np.testing.assert_array_equal(dist, (1.0 - torch.from_numpy(rs)).numpy())


def test_chunked_mining_k200_equals_unchunked():
    from text_similarity_amd.pipeline.search_pipeline import SentenceMiningPipeline
    rng = np.random.default_rng(62)
    d = 384
    c = _gauss(rng, 5000, d)
    c[4321] = c[17]
    q = np.concatenate([c[17][None], _gauss(rng, 15, d)]).astype(np.float32)
    params = SimpleNamespace(device=torch.device(DEV))
    ct, qt = torch.from_numpy(c).to(DEV), torch.from_numpy(q).to(DEV)
    one = SentenceMiningPipeline(len(c), params, None, corpus=ct)
    s1, i1 = one.search_tensors(qt, ct, 200)
    rs, ri = cosine_topk_f32(q, c, 200)
    np.testing.assert_array_equal(i1.cpu().numpy(), ri)
    np.testing.assert_array_equal(s1.cpu().numpy(), rs)
    for chunk in (1000, 777, 150):                       # 150: chunks shorter than k are padded before the merge
        pipe = SentenceMiningPipeline(chunk, params, None, corpus=ct)
        s2, i2 = pipe.search_tensors(qt, ct, 200)
        assert torch.equal(i2, i1) and torch.equal(s2, s1), chunk
    dot1 = SentenceMiningPipeline(len(c), params, None, corpus=ct, score_function="dot").search_tensors(qt, ct, 200)
    dot2 = SentenceMiningPipeline(777, params, None, corpus=ct, score_function="dot").search_tensors(qt, ct, 200)
    assert torch.equal(dot1[0], dot2[0]) and torch.equal(dot1[1], dot2[1])


class _FakeModel:
    """Stands in for the sentence encoder: text 'w<i>' -> row i of a fixed embedding table."""

    def __init__(self, table):
        self.table = torch.from_numpy(table).to(DEV)

    def encode_text(self, documents, output_np=False):
        return self.table[[int(t[1:]) for t in documents]]


class _FakeCross:
    def predict(self, pairs):
        return [float(int(t[1:]) % 7) for _, t in pairs]


def test_ranking_pipeline_top_k_100():
    from text_similarity_amd.pipeline.ranking_pipeline import RankingPipeline
    n, d, k = 1500, 384, 100
    table = presets.normal("topk_large/rank", n * d).reshape(n, d)
    corpus = [f"w{i}" for i in range(100, 1400)]
    queries = ["w3", "w250", "w77"]
    pipe = RankingPipeline(_FakeCross(), 512, SimpleNamespace(device=DEV), _FakeModel(table))
    out = pipe(queries, corpus, top_k=k)
    sc, ix = cosine_topk_f32(table[[3, 250, 77]], table[100:1400], k)
    for qi, res in enumerate(out):
        assert len(res["results"]) == k
        assert sorted(r["corpus_id"] for r in res["results"]) == sorted(ix[qi].tolist())
        cs = [r["cross-score"] for r in res["results"]]
        assert cs == sorted(cs, reverse=True) and res["avg_score"] == pytest.approx(sum(cs) / k)
        by_id = {r["corpus_id"]: r["score"] for r in res["results"]}
        for r, i in enumerate(ix[qi]):
            assert by_id[int(i)] == sc[qi][r]
