"""GPU parity of the exact Euclidean search (ops.l2_topk, include/tsim.h tsim_l2_topk_ex / tsim_l2_topk_large) and of
GpuFlatIndex(space='euclidean').  Bar: indices identical and float32 squared distances bit-equal to the test-local oracle
(tests/l2_cases.py: the canonical float64 evaluation restated in numpy, top-k by (distance asc, index asc))."""
import numpy as np
import pytest
import torch

from l2_cases import aug_corpus, aug_queries, l2_topk_ref
from oracle.search_ref import cosine_topk_f32, _lane_sum, topk_rows
from text_similarity_amd import ops
from text_similarity_amd.index import GpuFlatIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def _search_t(qf, cf, k, idx_offset=0):
    d = qf.shape[1]
    cn, rho, scale = ops.l2_rows(cf)
    s, i, st = ops.l2_topk(ops.l2_query_rows(qf, scale), cn, d, k, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale,
                           idx_offset=idx_offset, return_status=True)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy(), st.cpu().numpy()


def _check_exact(q, c, k, idx_offset=0):
    s, i, st = _search_t(_dev(q), _dev(c), k, idx_offset)
    kk = min(k, c.shape[0])
    rs, ri = l2_topk_ref(q, c, k, idx_offset)
    np.testing.assert_array_equal(i[:, :kk], ri)
    np.testing.assert_array_equal(s[:, :kk], rs)
    if kk < k:
        assert (i[:, kk:] == -1).all() and np.isposinf(s[:, kk:]).all()
    return s, i, st


def _gauss(rng, n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


def _spread(rng, n, d, lo=-3.0, hi=3.0):
    """rows with random directions and norms spread log-uniformly over 10^lo .. 10^hi"""
    x = rng.standard_normal((n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return (x * 10.0 ** rng.uniform(lo, hi, (n, 1))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- 0. operands
def test_operand_rows_bit_equal():
    """tsim_l2_rows / tsim_l2_query_rows against their numpy restatement: every half, the zero padding, the residual word."""
    rng = np.random.default_rng(90)
    d = 300
    c = _gauss(rng, 257, d) * rng.uniform(0.5, 2.0, (257, 1)).astype(np.float32)
    c[3] = 0.0
    q = np.concatenate([_gauss(rng, 5, d), np.zeros((1, d), np.float32)])
    cn, rho, scale = ops.l2_rows(_dev(c))
    A = ops.dot_scale(scale)
    hc, rho_c = aug_corpus(c, A)
    assert cn.shape == (257, 384)
    np.testing.assert_array_equal(cn[:, :d + 1].float().cpu().numpy(), hc.astype(np.float32))
    assert not cn[:, d + 1:].any()
    assert rho_c <= float(rho.item()) <= rho_c * (1 + 1e-5)
    hq, _, _, _ = aug_queries(q, A)
    qn = ops.l2_query_rows(_dev(q), scale)
    np.testing.assert_array_equal(qn[:, :d + 1].float().cpu().numpy(), hq.astype(np.float32))
    assert not qn[:, d + 1:].any()
    assert float(qn[5, d]) == 1.0                                   # the zero query: (0, .., 0, A) / A
    with pytest.raises(ValueError):
        ops.l2_rows(_dev(_gauss(rng, 4, 768)))
    wide = _dev(_gauss(rng, 4, 768))
    half = torch.zeros((4, 768), dtype=ops.UNIT_DTYPE, device=DEV)
    with pytest.raises(ValueError):                                 # d > 767 is refused by the search itself too
        ops.l2_topk(half, half, 768, 2, eq_f32=wide, ec_f32=wide, rho_c=rho, scale_c=scale)


# ---------------------------------------------------------------------------------------------------------- 1. random rows
@pytest.mark.parametrize("d", [127, 128, 300, 384, 767])     # half widths 128 / 256 / 384 / 512 / 768
@pytest.mark.parametrize("k", [1, 10, 28, 29, 64, 65, 100])
def test_random_rows_exact(d, k):
    rng = np.random.default_rng(1000 * d + k)
    c = _gauss(rng, 3000, d) * rng.uniform(0.5, 2.0, (3000, 1)).astype(np.float32)
    q = _gauss(rng, 24, d)
    _check_exact(q, c, k, idx_offset=7)


# ---------------------------------------------------------------------------------------------------------- 2. spread norms
def _dot_topk_idx(q, c, k):
    out = np.empty((q.shape[0], c.shape[0]), dtype=np.float32)
    for a in range(0, q.shape[0], 4):
        out[a:a + 4] = _lane_sum(q[a:a + 4, None, :], c[None, :, :]).astype(np.float32)
    return topk_rows(out, k)[1]


def test_spread_norms_exact_and_neither_cosine_nor_dot():
    rng = np.random.default_rng(2)
    d = 384
    c = _spread(rng, 3000, d)
    q = _spread(rng, 24, d, -1.0, 1.0)
    s, i, st = _check_exact(q, c, 10)
    _, ci = cosine_topk_f32(q, c, 10)
    di = _dot_topk_idx(q, c, 10)
    assert (ci != i).any(axis=1).mean() > 0.5, "on this corpus the Euclidean ranking must differ from cosine's"
    assert (di != i).any(axis=1).mean() > 0.5, "on this corpus the Euclidean ranking must differ from the inner product's"
    print(f"spread norms: status counts {np.bincount(st, minlength=3).tolist()}")


# ---------------------------------------------------------------------------------------------------------- 3. subnormal halves
@pytest.mark.parametrize("n", [900, 3000])
def test_huge_row_subnormal_halves_and_near_ties(n):
    """One row of norm 1e6 sets A = 2^20: the other rows (norm ~1) become half subnormals — of both kinds: large enough to be kept
    as subnormals and so small that they round to zero — and a cluster of 40 rows 1e-7 apart sits around rank k.  Whatever pass
    answers, every list is exact."""
    rng = np.random.default_rng(3 + n)
    d = 384
    c = _gauss(rng, n, d) / np.sqrt(d)
    c[0] *= 1e6 / np.linalg.norm(c[0])
    base = _gauss(rng, 1, d)[0] / np.sqrt(d)
    c[100:140] = base + 1e-7 * _gauss(rng, 40, d)
    q = np.concatenate([base[None] + 1e-3 * _gauss(rng, 12, d), _gauss(rng, 12, d)]).astype(np.float32)
    cn, rho, scale = ops.l2_rows(_dev(c))
    assert ops.dot_scale(scale) == 2.0 ** 20
    halves = cn[1:, :d].float().abs()
    assert bool((halves < 2.0 ** -14).all()) and bool((halves > 0).any()) and bool((halves == 0).any())
    _, _, st = _check_exact(q, c, 10)
    print(f"huge row, N = {n}: status counts {np.bincount(st, minlength=3).tolist()}")


# ---------------------------------------------------------------------------------------------------------- 4. ties and zeros
@pytest.mark.parametrize("k", [10, 40, 100])
def test_duplicates_equal_distances_zero_rows_zero_query(k):
    rng = np.random.default_rng(4)
    d = 256
    c = _gauss(rng, 3000, d)
    c[2100:2110] = c[7]                                       # exact duplicates: ties, lower index first
    c[2200:2300] = 0.0                                        # zero rows: all at distance |q|^2
    q = np.concatenate([c[7][None], np.zeros((1, d)), c[2250][None], _gauss(rng, 9, d)]).astype(np.float32)
    s, i, st = _check_exact(q, c, k)
    assert s[0, 0] == 0.0 and not np.signbit(s[0, 0])         # a query equal to a row: distance exactly +0.0 first
    np.testing.assert_array_equal(i[0, :min(k, 11)], ([7] + list(range(2100, 2110)))[:k])
    assert (s[0, :min(k, 11)] == 0.0).all()
    np.testing.assert_array_equal(i[1, :min(k, 100)], np.arange(2200, 2300)[:k])   # zero query: the zero rows, by index
    assert (s[1, :min(k, 100)] == 0.0).all()


def test_far_query_whose_distances_tie_in_float32():
    """|q| = 1e4 A: one float32 ulp of a distance is far above the guard's 2^-22 (in MFMA units); many rows round to the same
    distance and the lower index must win every such tie."""
    rng = np.random.default_rng(41)
    d = 128
    c = _gauss(rng, 3000, d) * rng.uniform(0.5, 2.0, (3000, 1)).astype(np.float32)
    u = rng.standard_normal((3, d))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    q = np.concatenate([u * 32.0 * np.array([[1e4], [1e3], [1e-4]]), _gauss(rng, 5, d)]).astype(np.float32)
    for k in (10, 40):
        s, i, st = _check_exact(q, c, k)
        print(f"far query, k = {k}: status {st.tolist()}")
    assert np.unique(s[0]).size < s[0].size                   # ties inside the returned list


def test_square_and_sum_are_rounded_separately():
    """A directed pair at d = 65, where lane 0 holds two terms (elements 0 and 64) and every other difference is zero: the
    canonical sum round(round(d0^2) + round(d1^2)) and a fused chain fma(d1, d1, d0^2) are neighbouring float64 values on either
    side of a float32 rounding boundary, so a kernel that lets the compiler fuse the multiply into the add returns another
    float32 distance (2.7964418 instead of 2.7964416) and fails here.  Every pass is covered: the list kernel's finalize (k = 10),
    the k <= 64 widening (k = 40), the sorted-list widening (k = 100), and brute force (a corpus of near-ties)."""
    from fractions import Fraction
    d = 65
    q0, q1, c1 = (float.fromhex(h) for h in ("0x1.a763c4p+0", "0x1.fa8492p-3", "-0x1.f8326ap-28"))
    assert all(float(np.float32(v)) == v for v in (q0, q1, c1))
    d0, d1 = q0 - 0.0, q1 - c1
    unfused = np.float32(d0 * d0 + d1 * d1)                  # (d0^2 is exact; Python rounds the product and the sum separately)
    fused = np.float32(float(Fraction(d1) * Fraction(d1) + Fraction(d0 * d0)))
    assert unfused != fused and unfused == np.float32(2.7964415550231934)
    rng = np.random.default_rng(8)
    qrow = _gauss(rng, 1, d)[0]
    crow = qrow.copy()
    qrow[0], qrow[64] = q0, q1
    crow[0], crow[64] = 0.0, c1
    c = _gauss(rng, 3000, d)
    c[5] = crow
    q = np.concatenate([qrow[None], _gauss(rng, 3, d)])
    for k in (10, 40, 100):
        s, i, st = _check_exact(q, c, k)
        assert i[0, 0] == 5 and s[0, 0] == unfused, (k, s[0, 0], fused)
    step = np.zeros(d, np.float32)
    step[1] = 0.05                                            # (along an element where the pair does not differ: 0.0025 farther)
    c[1000:2600] = crow + step + 1e-6 * _gauss(rng, 1600, d)  # 1 600 rows inside the guard's window: the collection overflows
    s, i, st = _check_exact(q, c, 10)
    assert st[0] == 2 and s[0, 0] == unfused and i[0, 0] == 5


# ---------------------------------------------------------------------------------------------------------- 5. small corpus
def test_fewer_rows_than_k_pads():
    rng = np.random.default_rng(5)
    s, i, _ = _check_exact(_gauss(rng, 6, 300), _gauss(rng, 5, 300), 10)
    assert (i[:, 5:] == -1).all() and np.isposinf(s[:, 5:]).all() and np.isfinite(s[:, :5]).all()


# ---------------------------------------------------------------------------------------------------------- 6. strided views
@pytest.mark.parametrize("k", [10, 40])
def test_strided_float32_views_give_the_same_bits(k):
    rng = np.random.default_rng(6)
    d = 300
    c, q = _gauss(rng, 3000, d), _gauss(rng, 24, d)
    s0, i0, _ = _search_t(_dev(q), _dev(c), k)
    cbuf = torch.full((3000, d + 9), 7.0, device=DEV)
    qbuf = torch.full((24, d + 5), -3.0, device=DEV)
    cbuf[:, 1:1 + d] = _dev(c)
    qbuf[:, 1:1 + d] = _dev(q)
    cv, qv = cbuf[:, 1:1 + d], qbuf[:, 1:1 + d]
    assert not cv.is_contiguous()
    cn, rho, scale = ops.l2_rows(cv)
    s1, i1 = ops.l2_topk(ops.l2_query_rows(qv, scale), cn, d, k, eq_f32=qv, ec_f32=cv, rho_c=rho, scale_c=scale)
    np.testing.assert_array_equal(i1.cpu().numpy(), i0)
    np.testing.assert_array_equal(s1.cpu().numpy(), s0)
    rs, ri = l2_topk_ref(q, c, k)
    np.testing.assert_array_equal(i0, ri)
    np.testing.assert_array_equal(s0, rs)


# ---------------------------------------------------------------------------------------------------------- 7. index
def test_flat_index_euclidean(tmp_path):
    rng = np.random.default_rng(7)
    d = 384
    a = _gauss(rng, 500, d)
    b = _gauss(rng, 300, d) * 50.0                            # a larger norm: A grows, the stored rows are re-derived
    q = _gauss(rng, 16, d)
    idx = GpuFlatIndex(space="euclidean", dim=d, device=DEV)
    idx.init_index(max_elements=100)
    lab, dist = idx.search(q, 3)                              # empty index: -1 / +inf
    assert bool((lab == -1).all()) and bool(torch.isposinf(dist).all())
    idx.add_items(a, np.arange(500) + 10_000)
    a0 = ops.dot_scale(idx._maxnorm)
    lab, dist = idx.knn_query(q, k=10)
    rs, ri = l2_topk_ref(q, a, 10)
    np.testing.assert_array_equal(lab, ri + 10_000)
    np.testing.assert_array_equal(dist, rs)                   # squared distances, ascending
    idx.add_items(b, np.arange(300) + 20_000)
    assert ops.dot_scale(idx._maxnorm) > a0
    rows, labels = np.concatenate([a, b]), np.concatenate([np.arange(500) + 10_000, np.arange(300) + 20_000])
    lab, dist = idx.knn_query(q, k=12)
    rs, ri = l2_topk_ref(q, rows, 12)
    np.testing.assert_array_equal(lab, labels[ri])
    np.testing.assert_array_equal(dist, rs)
    # delete the best hit of every query
    for lb in set(lab[:, 0].tolist()):
        idx.mark_deleted(int(lb))
    live = ~np.isin(labels, lab[:, 0])
    lab2, _ = idx.knn_query(q, k=12)
    rs2, ri2 = l2_topk_ref(q, rows[live], 12)
    np.testing.assert_array_equal(lab2, labels[live][ri2])
    # fewer live rows than k: -1 / +inf
    labp, distp = idx.search(q[:2], 1000)
    nlive = int(live.sum())
    assert bool((labp[:, nlive:] == -1).all()) and bool(torch.isposinf(distp[:, nlive:]).all())
    # save / load
    path = str(tmp_path / "l2.bin")
    idx.save_index(path)
    idx2 = GpuFlatIndex(space="euclidean", device=DEV)
    idx2.load_index(path)
    lab3, dist3 = idx2.knn_query(q, k=12)
    np.testing.assert_array_equal(lab3, lab2)
    np.testing.assert_array_equal(dist3, rs2)
    for other in ("cosine", "ip"):
        with pytest.raises(ValueError):
            GpuFlatIndex(space=other, device=DEV).load_index(path)
    cpath = str(tmp_path / "cos.bin")
    cidx = GpuFlatIndex(space="cosine", dim=d, device=DEV)
    cidx.add_items(a)
    cidx.save_index(cpath)
    with pytest.raises(ValueError):
        GpuFlatIndex(space="euclidean", device=DEV).load_index(cpath)
    bad = a[:4].copy()
    bad[2, 5] = np.nan
    with pytest.raises(ValueError):
        idx2.add_items(bad)
    with pytest.raises(NotImplementedError):
        idx2.range_search(q, 1.0)
    with pytest.raises(ValueError):
        GpuFlatIndex(space="euclidean", dim=768, device=DEV)
    with pytest.raises(ValueError):
        GpuFlatIndex(space="euclidean", device=DEV).add_items(_gauss(rng, 4, 768))
    with pytest.raises(ValueError):
        GpuFlatIndex(space="l2", dim=d, device=DEV)               # the name stays refused
