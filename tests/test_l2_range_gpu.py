"""GPU parity of the exact Euclidean range search (ops.l2_range, include/tsim.h tsim_l2_range_scan + tsim_range_fill with
TSIM_SPACE_L2, ops.range_merge(ascending=True)) and of GpuFlatIndex.radius_search / radius_query.
Bar: lims, indices and float32 squared-distance bits identical to the numpy oracle — tests/l2_cases.l2_dists gives the mask
dist <= r, a stable sort by (distance, index) the order.  No tolerance anywhere."""
import numpy as np
import pytest
import torch

from l2_cases import l2_dists
from l2_range_cases import (GAUSS_DIMS, fused_pair, gauss_case, mirror, must_be_collected, range_ref, selective_radii,
                            unit_norm_rows)
from text_similarity_amd import ops
from text_similarity_amd.index import GpuFlatIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF, NAN = float("inf"), float("nan")


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(DEV)


def _operands(qf, cf, c_operand=None):
    cn, rho, scale = ops.l2_rows(cf if c_operand is None else c_operand)
    return ops.l2_query_rows(qf, scale), cn, rho, scale


def _run(q, c, radius, idx_offset=0):
    """(lims, dist2, idx, status) as numpy; q, c numpy or device tensors"""
    qf = q if isinstance(q, torch.Tensor) else _dev(q)
    cf = c if isinstance(c, torch.Tensor) else _dev(c)
    qn, cn, rho, scale = _operands(qf, cf)
    r = ops.l2_range(qn, cn, qf.shape[1], radius, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale, idx_offset=idx_offset,
                     return_status=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in r)


def _radius_of(radius, qi):
    return radius[qi] if isinstance(radius, (np.ndarray, list, tuple)) else radius


def _compare(res, dist, radius, idx_offset=0):
    """bit equality with the oracle for every query; returns the hits per query"""
    lims, s, i = res[:3]
    assert lims[0] == 0 and lims.shape == (dist.shape[0] + 1,)
    assert s.shape == (lims[-1],) and i.shape == (lims[-1],) and s.dtype == np.float32 and i.dtype == np.int64
    sizes = []
    for qi in range(dist.shape[0]):
        ref = range_ref(dist[qi], _radius_of(radius, qi))
        a, b = int(lims[qi]), int(lims[qi + 1])
        np.testing.assert_array_equal(i[a:b], ref + idx_offset, err_msg=f"query {qi}: indices")
        np.testing.assert_array_equal(s[a:b].view(np.uint32), dist[qi, ref].view(np.uint32), err_msg=f"query {qi}: distance bits")
        sizes.append(ref.size)
    return sizes


def _must_be_collected(q, c, radii, queries):
    """The derived status-1 condition (l2_range_cases.must_be_collected) for the given queries, from the oracle alone."""
    D = l2_dists(q, c, dtype=np.float64)
    _, eps, nqs, _ = mirror(q, c, ops.pad_dim(q.shape[1] + 1))
    return all(must_be_collected(D[qi], radii[qi], eps[qi], nqs[qi]) for qi in queries)


def _check(q, c, radius, idx_offset=0, dist=None):
    dist = l2_dists(q, c) if dist is None else dist
    res = _run(q, c, radius, idx_offset)
    _compare(res, dist, radius.tolist() if isinstance(radius, torch.Tensor) else radius, idx_offset)
    assert np.isin(res[3], (1, 2)).all()
    return res


# ---------------------------------------------------------------------------------------------------------- 1. random rows
@pytest.mark.parametrize("d", GAUSS_DIMS)     # half widths 128 / 256 / 384 / 512 / 768
def test_gaussian_rows_exact(d):
    q, c = gauss_case(d)
    D = l2_dists(q, c, dtype=np.float64)
    dist = D.astype(np.float32)
    ld = ops.pad_dim(d + 1)
    _, eps, nqs, _ = mirror(q, c, ld)
    r, r_below = selective_radii(dist[0])
    for radius, n0 in ((r, 10), (r_below, 9)):             # the radius ON a row's distance: '<=' meets a real tie
        # derived, not guessed: every row the collect pass can gather fits the slot (checked for this seed without a GPU in
        # tests/test_l2_range_cpu.py), so the query is answered from the collected rows
        assert all(must_be_collected(D[qi], radius, eps[qi], nqs[qi]) for qi in range(q.shape[0]))
        lims, s, i, st = _check(q, c, float(radius), idx_offset=7, dist=dist)
        assert lims[1] - lims[0] == n0
        assert (st == 1).all(), st
    assert s[lims[1] - 1].view(np.uint32) == np.sort(dist[0])[8].view(np.uint32)
    lims, s, i, st = _check(q, c, INF, dist=dist)          # every row
    assert lims[-1] == q.shape[0] * c.shape[0] and (st == 2).all()
    lims, s, i, st = _check(q, c, -1.0, dist=dist)         # none
    assert lims[-1] == 0 and (st == 1).all()


# ---------------------------------------------------------------------------------------------------------- 2. per-query radii
def test_per_query_radius_tensor_and_the_edge_radii():
    rng = np.random.default_rng(22)
    d = 300
    c = unit_norm_rows(rng, 3000, d)
    q = unit_norm_rows(rng, 6, d)
    c[[40, 1700, 2999]] = q[1]                              # exact duplicates of query 1; query 2 has none
    dist = l2_dists(q, c)
    sel = np.sort(dist[3])[9]
    radii = np.array([-1.0, 0.0, 0.0, sel, INF, NAN], dtype=np.float32)
    assert _must_be_collected(q, c, radii, range(4))        # (+inf and NaN have no finite collect threshold: status 2)
    lims, s, i, st = _check(q, c, torch.from_numpy(radii), idx_offset=5, dist=dist)
    np.testing.assert_array_equal(np.diff(lims), [0, 3, 0, 10, 3000, 0])
    np.testing.assert_array_equal(i[lims[1]:lims[2]], np.array([40, 1700, 2999]) + 5)
    assert (s[lims[1]:lims[2]] == 0).all() and not np.signbit(s[lims[1]:lims[2]]).any()
    assert st.tolist() == [1, 1, 1, 1, 2, 2], st
    seg = s[lims[4]:lims[5]]
    assert (np.diff(seg) >= 0).all()                        # all N rows, distance ascending
    # the same through a numpy array, and each query equal to the scalar call with its own radius
    res_np = _run(q, c, radii, idx_offset=5)
    for a, b in zip(res_np, (lims, s, i, st)):
        np.testing.assert_array_equal(a, b)
    for qi in range(5):                                     # (the scalar call refuses NaN)
        l1, s1, i1, st1 = _run(q[qi:qi + 1], c, float(radii[qi]), idx_offset=5)
        np.testing.assert_array_equal(i1, i[lims[qi]:lims[qi + 1]])
        np.testing.assert_array_equal(s1.view(np.uint32), s[lims[qi]:lims[qi + 1]].view(np.uint32))
        assert st1[0] == st[qi]
    qf, cf = _dev(q), _dev(c)
    qn, cn, rho, scale = _operands(qf, cf)
    with pytest.raises(ValueError):
        ops.l2_range(qn, cn, d, torch.zeros(5), eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale)
    with pytest.raises(ValueError):
        ops.l2_range(qn, cn, d, NAN, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale)
    with pytest.raises(ValueError):
        ops.l2_range(qn, cn, d, 1.0, eq_f32=qf, ec_f32=cf, rho_c=None, scale_c=scale)


# ---------------------------------------------------------------------------------------------------------- 3. overflow
def test_overflowing_cluster_takes_the_exact_pass():
    """5 000 rows in a tight cluster inside the radius of query 0: more than the 2 048-entry slot and more than range_bf_sort's
    4 096-entry LDS block, so the segment is sorted through the global-stride merge; query 1 is far from it."""
    rng = np.random.default_rng(33)
    d, ncl = 128, 5000
    c = unit_norm_rows(rng, 9000, d)
    centre = unit_norm_rows(rng, 1, d, 1.0, 1.0)[0]
    where = np.sort(rng.choice(9000, ncl, replace=False))
    c[where] = centre + (1e-3 * rng.standard_normal((ncl, d))).astype(np.float32)
    q = np.concatenate([centre[None], -centre[None]]).astype(np.float32)
    dist = l2_dists(q, c)
    r0 = float(dist[0, where].max())
    radii = np.array([r0, np.sort(dist[1])[4]], dtype=np.float32)
    assert _must_be_collected(q, c, radii, [1])
    lims, s, i, st = _check(q, c, radii, dist=dist)
    assert st.tolist() == [2, 1], st
    assert lims[1] - lims[0] >= ncl and lims[2] - lims[1] == 5
    assert set(where.tolist()) <= set(i[:lims[1]].tolist())


# ---------------------------------------------------------------------------------------------------------- 4. float32 ties
def test_far_query_whose_distances_tie_in_float32():
    """|q| = 1e4 A (tests/test_l2_search_gpu.py): many rows round to the same float32 distance; inside a tie the order is index
    ascending, with the offset added."""
    rng = np.random.default_rng(41)
    d = 128
    c = rng.standard_normal((3000, d)).astype(np.float32) * rng.uniform(0.5, 2.0, (3000, 1)).astype(np.float32)
    u = rng.standard_normal((3, d))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    q = np.concatenate([u * 32.0 * np.array([[1e4], [1e3], [1e-4]]), rng.standard_normal((5, d))]).astype(np.float32)
    dist = l2_dists(q, c)
    radii = np.array([np.sort(dist[qi])[39] for qi in range(q.shape[0])], dtype=np.float32)
    lims, s, i, st = _check(q, c, radii, idx_offset=12_345, dist=dist)
    seg_s, seg_i = s[:lims[1]], i[:lims[1]]
    assert np.unique(seg_s).size < seg_s.size               # ties inside the returned list ...
    tie = np.diff(seg_s) == 0
    assert tie.any() and (np.diff(seg_i)[tie] > 0).all()    # ... ordered by index
    assert seg_i.min() >= 12_345
    print(f"far query: hits {np.diff(lims).tolist()} status {st.tolist()}")


# ---------------------------------------------------------------------------------------------------------- 5. unfused arithmetic
def test_square_and_sum_are_rounded_separately_in_every_pass():
    """A pair at d = 65 whose fused and unfused float64 sums round to different float32 distances.  With the radius equal to
    the smaller of the two values the row's membership is decided by the arithmetic; the collect path (status 1) and the exact
    pass (a second call in which near-copies of the row overflow the slot and a neighbouring query has r = +inf) must both give the
    oracle's answer."""
    d = 65
    q0, q1, c1, unfused, fused = fused_pair(d)
    rng = np.random.default_rng(8)
    qrow = rng.standard_normal(d).astype(np.float32)
    crow = qrow.copy()
    qrow[0], qrow[64] = q0, q1
    crow[0], crow[64] = 0.0, c1
    c = rng.standard_normal((3000, d)).astype(np.float32)
    c[5] = crow
    q = np.concatenate([qrow[None], rng.standard_normal((3, d)).astype(np.float32)])
    dist = l2_dists(q, c)
    assert dist[0, 5] == unfused
    r = min(unfused, fused)
    member = bool(dist[0, 5] <= r)                           # whichever way it falls, the oracle decides
    assert _must_be_collected(q, c, [max(unfused, fused)] * 4, [0])
    lims, s, i, st = _check(q, c, float(r), dist=dist)
    assert st[0] == 1 and ((lims[1] - lims[0] >= 1 and i[0] == 5) == member)
    lims, s, i, st = _check(q, c, float(max(unfused, fused)), dist=dist)
    assert st[0] == 1 and i[0] == 5 and s[0] == unfused
    # the exact pass: 2 100 near-copies of the row just OUTSIDE the radius overflow query 0's slot; the neighbouring query is the
    # same row with r = +inf, so the exact pass also returns the pair's distance itself
    step = np.zeros(d, np.float32)
    step[1] = 0.05                                           # (along an element where the pair does not differ: 0.0025 farther)
    c2 = c.copy()
    c2[600:2700] = crow + step + (1e-6 * rng.standard_normal((2100, d))).astype(np.float32)
    q2 = np.concatenate([qrow[None], qrow[None], q[2:]])
    dist2 = l2_dists(q2, c2)
    for rr in (r, max(unfused, fused)):
        radii = np.array([rr, INF, -1.0, -1.0], dtype=np.float32)
        lims, s, i, st = _check(q2, c2, radii, dist=dist2)
        assert st[0] == 2 and st[1] == 2, st
        assert ((lims[1] - lims[0] >= 1 and i[0] == 5) == bool(dist2[0, 5] <= rr))
        assert lims[2] - lims[1] == 3000 and i[lims[1]] == 5 and s[lims[1]] == unfused


# ---------------------------------------------------------------------------------------------------------- 6. corrupted operand
def test_corrupted_operand_is_detected_and_answered_exactly():
    """A far row's half operand is overwritten with that of query 0's nearest row: it is collected with a high MFMA score, its
    exact distance contradicts the score beyond eps, and the exact pass answers query 0 — with the oracle's result."""
    rng = np.random.default_rng(66)
    d = 384
    c = unit_norm_rows(rng, 3000, d)
    q = unit_norm_rows(rng, 4, d)
    dist = l2_dists(q, c)
    near, far = int(np.argmin(dist[0])), int(np.argmax(dist[0]))
    r = float(np.sort(dist[0])[9])
    qf, cf = _dev(q), _dev(c)
    qn, cn, rho, scale = _operands(qf, cf)
    cn[far] = cn[near]
    res = ops.l2_range(qn, cn, d, r, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale, return_status=True)
    torch.cuda.synchronize()
    res = tuple(t.cpu().numpy() for t in res)
    _compare(res, dist, r)
    assert res[3][0] == 2, res[3]
    assert far not in res[2][:res[0][1]].tolist() and near in res[2][:res[0][1]].tolist()


# ---------------------------------------------------------------------------------------------------------- 7. strided views
def test_strided_float32_views_give_the_same_bits():
    rng = np.random.default_rng(77)
    d = 300
    c, q = unit_norm_rows(rng, 3000, d), unit_norm_rows(rng, 8, d)
    dist = l2_dists(q, c)
    radii = np.array([np.sort(dist[qi])[19] for qi in range(8)], dtype=np.float32)
    radii[7] = INF                                           # one query through the exact pass
    base = _check(q, c, radii, dist=dist)
    cbuf = torch.full((3000, d + 37), NAN, device=DEV)
    qbuf = torch.full((8, d + 37), NAN, device=DEV)
    cbuf[:, 1:1 + d] = _dev(c)
    qbuf[:, 1:1 + d] = _dev(q)
    cv, qv = cbuf[:, 1:1 + d], qbuf[:, 1:1 + d]
    assert not cv.is_contiguous() and not qv.is_contiguous()
    view = _run(qv, cv, radii)
    for a, b in zip(view, base):
        np.testing.assert_array_equal(a.view(np.uint32) if a.dtype == np.float32 else a,
                                      b.view(np.uint32) if b.dtype == np.float32 else b)


# ---------------------------------------------------------------------------------------------------------- 8. merge
def test_chunks_merged_ascending_equal_the_single_call():
    rng = np.random.default_rng(88)
    d = 128
    c, q = unit_norm_rows(rng, 3000, d), unit_norm_rows(rng, 8, d)
    cuts = [0, 700, 1900, 3000]
    c[700:1900] = unit_norm_rows(rng, 1200, d, 5.0, 6.0)     # the middle chunk: dist^2 >= 9, no hit for any query (and another A)
    dist = l2_dists(q, c)
    radii = np.array([np.sort(dist[qi])[29] for qi in range(8)], dtype=np.float32)
    radii[3] = np.sort(dist[3])[299]                         # a long segment too
    radii[6] = -1.0                                          # no hit anywhere
    assert float(radii.max()) < float(dist[:, 700:1900].min())
    single = _check(q, c, radii, dist=dist)
    qf, cf = _dev(q), _dev(c)
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        qn, cn, rho, scale = _operands(qf, cf[a:b])
        parts.append(ops.l2_range(qn, cn, d, torch.from_numpy(radii), eq_f32=qf, ec_f32=cf[a:b], rho_c=rho, scale_c=scale,
                                  idx_offset=a))
    assert int(parts[1][0][-1]) == 0 and int(parts[0][0][-1]) > 0 and int(parts[2][0][-1]) > 0
    lims, s, i = (t.cpu().numpy() for t in ops.range_merge(parts, ascending=True))
    np.testing.assert_array_equal(lims, single[0])
    np.testing.assert_array_equal(i, single[2])
    np.testing.assert_array_equal(s.view(np.uint32), single[1].view(np.uint32))


# ---------------------------------------------------------------------------------------------------------- 9. index
def test_flat_index_radius_search():
    rng = np.random.default_rng(99)
    d = 200
    rows = unit_norm_rows(rng, 1200, d)
    q = unit_norm_rows(rng, 6, d)
    labels = np.arange(1200, dtype=np.int64) * 3 + 50_000
    idx = GpuFlatIndex(space="euclidean", dim=d, device=DEV)
    lims, s, lab = idx.radius_search(q, 1.0)                  # empty index
    assert lims.tolist() == [0] * 7 and s.numel() == 0 and lab.numel() == 0 and lab.dtype == torch.int64
    with pytest.raises(ValueError):
        idx.radius_search(q, np.zeros(5, np.float32))         # the length check comes first
    idx.add_items(rows[:800], labels[:800])
    idx.add_items(rows[800:], labels[800:])
    dead = [3, 411, 799, 800, 1199]
    for r_ in dead:
        idx.mark_deleted(int(labels[r_]))
    live = np.setdiff1d(np.arange(1200), dead)
    dist = l2_dists(q, rows[live])
    scalar = float(np.sort(dist[0])[14])
    per_q = np.array([np.sort(dist[qi])[5 + 3 * qi] for qi in range(6)], dtype=np.float32)
    per_q[4] = INF
    for radius in (scalar, per_q):
        lims, s, lab = (t.cpu().numpy() for t in idx.radius_search(q, radius))
        nl, nlab, ndist = idx.radius_query(q, radius)
        np.testing.assert_array_equal(nl, lims)
        np.testing.assert_array_equal(nlab, lab)
        np.testing.assert_array_equal(ndist.view(np.uint32), s.view(np.uint32))   # the squared distances themselves
        for qi in range(6):
            ref = range_ref(dist[qi], _radius_of(radius, qi))
            a, b = int(lims[qi]), int(lims[qi + 1])
            np.testing.assert_array_equal(lab[a:b], labels[live][ref])
            np.testing.assert_array_equal(s[a:b].view(np.uint32), dist[qi, ref].view(np.uint32))
    with pytest.raises(NotImplementedError, match="radius_search"):
        idx.range_search(q, 1.0)
    for other in ("cosine", "ip"):
        oidx = GpuFlatIndex(space=other, dim=d, device=DEV)
        oidx.add_items(rows[:10])
        with pytest.raises(ValueError):
            oidx.radius_search(q, 1.0)


# ---------------------------------------------------------------------------------------------------------- 10. empty shapes
def test_empty_shapes_return_empty_results():
    rng = np.random.default_rng(10)
    d = 127
    c, q = unit_norm_rows(rng, 7, d), unit_norm_rows(rng, 6, d)
    _check(q, c, INF, idx_offset=3)                           # a corpus smaller than one tile
    _check(q, c, float(np.median(l2_dists(q, c))), idx_offset=3)
    qf, cf = _dev(q), _dev(c)
    qn, cn, rho, scale = _operands(qf, cf)
    kw = dict(rho_c=rho, scale_c=scale)
    lims, s, i = ops.l2_range(qn[:0], cn, d, 0.5, eq_f32=qf[:0], ec_f32=cf, **kw)
    assert lims.tolist() == [0] and s.numel() == 0 and i.numel() == 0
    lims, s, i, st = ops.l2_range(qn, cn[:0], d, 0.5, eq_f32=qf, ec_f32=cf[:0], return_status=True, **kw)
    assert lims.tolist() == [0] * 7 and s.numel() == 0 and i.numel() == 0 and i.dtype == torch.int64 and s.dtype == torch.float32
    wide = torch.zeros((4, 768), device=DEV)
    half = torch.zeros((4, 768), dtype=ops.UNIT_DTYPE, device=DEV)
    with pytest.raises(ValueError):                           # d > 767
        ops.l2_range(half, half, 768, 1.0, eq_f32=wide, ec_f32=wide, **kw)
