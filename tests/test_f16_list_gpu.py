"""Exact top-k within candidate lists over FLOAT16 rows on the GPU (ops.f16_list_topk).  Every result — scores, indices and
status — is compared bit for bit with (a) the float32 op of the same space on ``ec_f16.float()`` and, on finite data, (b) the
numpy oracle of tests/list_cases.py on the widened rows.  No tolerance anywhere: widening a half is exact."""
import functools
import gc

import numpy as np
import pytest
import torch

import far_cases as fc
from list_cases import ST_LIMS, ST_ROW, csr, list_topk_ref, pair_scores, rank_list, same_bits
from refine_cases import to_f16
from text_similarity_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 2100
SPACES = ("cosine", "dot", "l2")
WIDTHS = (1, 2, 63, 64, 65, 384, 385, 767, 768)
KS = (1, 10, 64, 65, 1024)
F32 = {"cosine": ops.cosine_list_topk, "dot": ops.dot_list_topk, "l2": ops.l2_list_topk}
CSR_LENGTHS = (1, 0, 1024, 0, 0, 1025, 2049, 10)        # per query; empty lists between others


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _np(out):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _view(x, ld, off=0, fill=np.nan):
    """x [n, d] on the device as a view with row stride ld of a buffer whose other elements hold ``fill``"""
    n, d = x.shape
    buf = np.full((n, ld), fill, dtype=x.dtype)
    buf[:, off:off + d] = x
    v = _dev(buf)[:, off:off + d]
    assert v.stride() == (ld, 1)
    return v


def _assert_same(got, want, what):
    assert (got[1] == want[1]).all(), (what, np.argwhere(got[1] != want[1])[:5])
    a, b = np.ascontiguousarray(got[0]).view(np.int32), np.ascontiguousarray(want[0]).view(np.int32)
    assert (a == b).all(), (what, np.argwhere(a != b)[:5])
    if len(got) > 2 and len(want) > 2:
        assert (got[2] == want[2]).all(), (what, got[2], want[2])


def _both(space, qv, cv16, cand, lims=None, **kw):
    """(f16 result, the float32 op on the widened rows): the same lists, the same arguments"""
    got = _np(ops.f16_list_topk(space, qv, cv16, cand, lims, **kw))
    want = _np(F32[space](qv, cv16.float(), cand, lims, **kw))
    return got, want


@functools.lru_cache(maxsize=None)
def _rows(d, nq=8):
    rng = np.random.default_rng(300 + d)
    return rng.standard_normal((nq, d)).astype(np.float32), to_f16(rng.standard_normal((N, d)))


@pytest.mark.parametrize("space,d", [(s, d) for s in SPACES for d in WIDTHS if not (s == "l2" and d == 768)])
def test_widths_strides_lengths_and_k(space, d):
    """The lane tail and both NI paths (d), row strides d, d + 1 (odd: rows only 2-byte aligned) and d + 7 at an odd offset, the
    query stride above d, CSR lists of length 0, 1, 1 024, 1 025 and 2 049 with empty ones between, every k regime, k above a
    list's length."""
    q, c16 = _rows(d)
    rng = np.random.default_rng(d)
    lists = [rng.permutation(N)[:n] for n in CSR_LENGTHS]
    sc = [pair_scores(space, q, c16.astype(np.float32), np.full((len(l),), j), l) for j, l in enumerate(lists)]
    cand, lims = (_dev(x) for x in csr(lists))
    qv = _view(q, d + 3, 1)
    for cv in (_dev(c16), _view(c16, d + 1), _view(c16, d + 7, 3)):
        for k in KS:
            got, want = _both(space, qv, cv, cand, lims, k=k, return_status=True, assume_unique=True)
            _assert_same(got, want, (space, d, cv.stride(0), k, "vs float32 op"))
            for j, l in enumerate(lists):
                rs, ri = rank_list(space, l, sc[j], k)
                _assert_same((got[0][j], got[1][j]), (rs, ri), (space, d, cv.stride(0), k, j, "vs oracle"))
            assert not got[2].any()


def test_width_768_is_refused_under_l2():
    q, c16 = _rows(768)
    with pytest.raises(ValueError):
        ops.f16_list_topk("l2", _dev(q), _dev(c16), torch.arange(10, device=DEV), k=3)


@pytest.mark.parametrize("space", SPACES)
def test_forms_dtypes_offset_and_query_counts(space):
    d, k = 65, 10
    rng = np.random.default_rng(41)
    c16 = to_f16(rng.standard_normal((N, d)))
    q = rng.standard_normal((300, d)).astype(np.float32)
    cv = _view(c16, d + 1)
    cf = c16.astype(np.float32)
    for Q in (1, 5, 300):
        qv = _view(q[:Q], d + 5, 2)
        for m in (1, 10, 1023, 1024, 1025):                                      # fixed-width lists, -1 padded tails
            two_d = np.stack([rng.permutation(N)[:m] for _ in range(Q)])
            two_d[::2, m // 2:] = -1
            for dt in (np.int64, np.int32):
                got, want = _both(space, qv, cv, _dev(two_d.astype(dt)), k=k, assume_unique=True, return_status=True)
                _assert_same(got, want, (space, Q, m, dt, "2-D"))
            if Q == 5:
                rs, ri, rst = list_topk_ref(space, q[:Q], cf, list(two_d), k)
                _assert_same(got, (rs, ri, rst), (space, m, "2-D vs oracle"))
        shared = rng.permutation(N)[:1500]
        for dt in (np.int64, np.int32):
            for uniq in (False, True):
                got, want = _both(space, qv, cv, _dev(shared.astype(dt)), k=k, assume_unique=uniq, idx_offset=(1 << 32) + 7)
                _assert_same(got, want, (space, Q, dt, uniq, "shared"))
        if Q == 5:
            rs, ri, _ = list_topk_ref(space, q[:Q], cf, shared, k, idx_offset=(1 << 32) + 7)
            _assert_same(got, (rs, ri), (space, "shared vs oracle"))
            assert got[1].min() > 1 << 32
    with pytest.raises(_lib.TsimError):                                          # CPU tensors
        ops.f16_list_topk(space, torch.from_numpy(q[:2]), torch.from_numpy(c16), torch.arange(5), k=3)
    with pytest.raises(ValueError):                                              # float32 rows are the other ops' business
        ops.f16_list_topk(space, _dev(q[:2]), _dev(cf), torch.arange(5, device=DEV), k=3)
    with pytest.raises(ValueError):                                              # ... and half rows are not theirs
        F32[space](_dev(q[:2]), _dev(c16), torch.arange(5, device=DEV), k=3)
    with pytest.raises(ValueError):
        ops.f16_list_topk("hamming", _dev(q[:2]), _dev(c16), torch.arange(5, device=DEV), k=3)
    with pytest.raises(ValueError):
        ops.f16_list_topk(space, _dev(q[:2]), _dev(c16)[:, ::2], torch.arange(5, device=DEV), k=3)   # inner stride 2


@pytest.mark.parametrize("space", SPACES)
def test_entries_out_of_range_bad_lims_and_repeats(space):
    d, k = 63, 10
    q, c16 = _rows(d)
    q = q[:6]
    cf = c16.astype(np.float32)
    qv, cv = _dev(q), _view(c16, d + 1)
    rng = np.random.default_rng(31)
    good = rng.permutation(N)[:40]
    lists = [np.concatenate([[-1, -1], good[:20], [-1], good[20:], [-7]]), np.full((33,), -1),
             np.concatenate([good, [N, N + 10 ** 9, 2 ** 31 - 1]]), np.array([5, 9, 5, 11, 9, 5]), good[:3], np.zeros((0,), np.int64)]
    cand, lims = csr(lists)
    for uniq in (False, True):
        got, want = _both(space, qv, cv, _dev(cand), _dev(lims), k=k, return_status=True, assume_unique=uniq)
        _assert_same(got, want, ("entries", uniq))
        _assert_same(got, list_topk_ref(space, q, cf, lists, k, unique=not uniq), ("entries vs oracle", uniq))
        assert got[2].tolist() == [0, 0, ST_ROW, 0, 0, 0]
        assert (got[1][3] >= 0).sum() == (6 if uniq else 3)                      # a row listed twice comes out twice
    # entries >= N are never read: the corpus ends at the end of an allocation filled with NaN behind a short view
    c32 = np.concatenate([good, [N, 2 ** 31 - 1]]).astype(np.int32)
    got, want = _both(space, qv, cv, _dev(c32), k=k, return_status=True, assume_unique=True)
    _assert_same(got, want, "int32 beyond")
    assert (got[2] == ST_ROW).all()
    cand = rng.permutation(N)[:100]
    lims = np.array([0, 30, 20, 60, 60, 500, 500], dtype=np.int64)              # query 1: [30, 20) decreasing
    lists = [cand[0:30], cand[0:0], cand[30:60], cand[60:60], cand[60:100], cand[0:0]]
    for uniq in (False, True):
        got, want = _both(space, qv, cv, _dev(cand), _dev(lims), k=k, return_status=True, assume_unique=uniq)
        _assert_same(got, want, ("bad lims", uniq))
        _assert_same(got[:2], list_topk_ref(space, q, cf, lists, k)[:2], ("bad lims vs oracle", uniq))
        assert got[2].tolist() == [0, ST_LIMS, ST_LIMS, 0, ST_LIMS, ST_LIMS]


def _subnormal_case():
    """64 rows made only of subnormal halves (multiples of 2^-24) and queries of that size: a conversion that flushes them
    reads 64 zero rows, which tie, and the answer becomes the lowest row numbers"""
    d = 70
    rng = np.random.default_rng(77)
    c16 = to_f16(rng.standard_normal((N, d)))
    sub = np.arange(100, 164)
    c16[sub] = (rng.integers(-1023, 1024, size=(64, d)).astype(np.float64) * 2.0 ** -24).astype(np.float16)
    assert (np.abs(c16[sub].astype(np.float64)) < 2.0 ** -14).all() and (c16[sub] != 0).any(1).all()
    q = (rng.standard_normal((4, d)) * 2.0 ** -14).astype(np.float32)
    return q, c16, sub


@pytest.mark.parametrize("space", SPACES)
def test_subnormal_halves_are_widened_not_flushed(space):
    q, c16, sub = _subnormal_case()
    cf = c16.astype(np.float32)
    rs, ri, _ = list_topk_ref(space, q, cf, sub, 10)
    flushed = cf.copy()
    flushed[sub] = 0.0
    fs, fi, _ = list_topk_ref(space, q, flushed, sub, 10)
    assert (fi != ri).any() and (fi == sub[:10]).all()                           # the test has teeth, shown on the CPU
    got, want = _both(space, _dev(q), _view(c16, c16.shape[1] + 1), _dev(sub), k=10)
    _assert_same(got, want, "subnormal vs float32 op")
    _assert_same(got, (rs, ri), "subnormal vs oracle")


@pytest.mark.parametrize("space", SPACES)
def test_special_values(space):
    d, k = 65, 12
    rng = np.random.default_rng(5)
    c = rng.standard_normal((N, d)).astype(np.float32)
    c[17] = 0.0                                                                  # a zero row: cosine 0 by the eps rule
    c[18] = -0.0
    c[[40, 999, 1024, 2000, 2099]] = c[39]                                       # copies: the tie goes to the lower row
    c[50, ::2], c[50, 1::2] = 65504.0, -65504.0
    c[51] = 65504.0
    c[52, 3] = -65504.0
    c16 = to_f16(c)
    q = rng.standard_normal((6, d)).astype(np.float32)
    q[2] = c16[39].astype(np.float32)
    q[3] = 0.0
    q[4, ::2] *= -0.0
    lst = np.concatenate([np.arange(60), [999, 1024, 2000, 2099], rng.permutation(N)[:300]])
    cv, qv = _view(c16, d + 1), _dev(q)
    got, want = _both(space, qv, cv, _dev(lst), k=k)
    _assert_same(got, want, "finite specials vs float32 op")
    rs, ri, _ = list_topk_ref(space, q, c16.astype(np.float32), lst, k)
    _assert_same(got, (rs, ri), "finite specials vs oracle")
    first = [39, 40, 999, 1024, 2000, 2099]
    assert got[1][2, :6].tolist() == first or space == "dot"                     # (dot: a longer row may score higher)
    # rows holding inf or NaN halves: compared with the float32 op only
    c16[60, 5] = np.inf
    c16[61, 0] = -np.inf
    c16[62, 64] = np.nan
    c16[63] = np.nan
    got, want = _both(space, qv, _view(c16, d + 1), _dev(lst), k=k, return_status=True)
    _assert_same(got, want, "inf and NaN rows vs float32 op")


def test_f16_rows():
    from refine_cases import F16_TABLE
    vals = np.array([v for v, _ in F16_TABLE if abs(v) < 65520], dtype=np.float32).reshape(1, -1)
    want = np.array([b for v, b in F16_TABLE if abs(v) < 65520], dtype=np.uint16)
    got = ops.f16_rows(_dev(vals))
    assert got.dtype == torch.float16 and (got.cpu().numpy().view(np.uint16).reshape(-1) == want).all()
    x = np.random.default_rng(3).standard_normal((500, 33)).astype(np.float32) * np.float32(2.0 ** -12)    # subnormals among them
    assert (ops.f16_rows(_dev(x)).cpu().numpy().view(np.uint16) == to_f16(x).view(np.uint16)).all()
    for bad in (65520.0, -1e5, np.inf, np.nan):
        y = x.copy()
        y[7, 2] = bad
        with pytest.raises(ValueError, match="row 7"):
            ops.f16_rows(_dev(y))
    with pytest.raises(_lib.TsimError):
        ops.f16_rows(torch.from_numpy(x))


# ------------------------------------------------------------------------------------------------- rows far apart
# tests/far_cases.py's Layout F with 2-byte elements: 6 000 rows 719 184 halves apart, 8.63 GB, filled with 0xFF (NaN halves)
# first.  Rows 1 493, 2 986 and 5 972 start 112, 224 and 448 elements below 2^30, 2^31 and 2^32 elements: at 512 halves they
# straddle 2^31, 2^32 and 2^33 bytes.
LAYOUT_H = fc.Layout("H", 2, fc.LAYOUT_F.stride, 1493, (1 << 31, 1 << 32, 1 << 33))
FAR_D = 512


def _far_rows():
    """far_cases.rows' recipe on this layout's sentinels: Gaussian rows; sentinel t is query 1 + t % 7 plus noise"""
    rng = np.random.default_rng(1729)
    c = rng.standard_normal((fc.N, FAR_D)).astype(np.float32)
    q = rng.standard_normal((fc.Q, FAR_D)).astype(np.float32)
    prng = np.random.default_rng(4242)
    for t, r in enumerate(LAYOUT_H.sentinels()):
        c[r] = q[1 + t % (fc.Q - 1)] + np.float32(0.25) * prng.standard_normal(FAR_D).astype(np.float32)
    return q, to_f16(c)


def test_far_layout_arithmetic():
    assert [LAYOUT_H.start(r) + 2 * FAR_D - b for r, b in ((1493, 1 << 31), (2986, 1 << 32), (5972, 1 << 33))] == [800, 576, 128]
    assert [b - LAYOUT_H.start(r) for r, b in ((1493, 1 << 31), (2986, 1 << 32), (5972, 1 << 33))] == [224, 448, 896]
    assert LAYOUT_H.sentinels() == [0, 1492, 1493, 1494, 2985, 2986, 2987, 5971, 5972, 5973, 5999]
    assert LAYOUT_H.nbytes == 8_630_208_000


@pytest.mark.parametrize("space", SPACES)
def test_far_rows(space):
    need = LAYOUT_H.nbytes + fc.LAYOUT_F.nbytes + (5 << 28)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"the far buffers need {need / 1e9:.1f} GB of device memory, {free / 1e9:.1f} GB are free")
    q, c16 = _far_rows()
    try:
        cbuf, qbuf = fc.FarBuffer(LAYOUT_H, DEV), fc.FarBuffer(fc.LAYOUT_F, DEV)
        cv = cbuf.place(c16)
        qv = qbuf.place(q, fc.QUERY_STRIDE_F)
        assert cv.stride(0) == LAYOUT_H.stride and qv.stride(0) == fc.QUERY_STRIDE_F and cv.dtype == torch.float16
        rng = np.random.default_rng(9)
        lists = [np.unique(np.concatenate([rng.choice(fc.N, 700, replace=False), LAYOUT_H.sentinels()])) for _ in range(fc.Q)]
        cand, lims = (_dev(x) for x in csr(lists))
        cc = cv.contiguous()
        for k in (10, 100):
            got = _np(ops.f16_list_topk(space, qv, cv, cand, lims, k, return_status=True))
            want = list_topk_ref(space, q, c16.astype(np.float32), lists, k)
            _assert_same(got, want, (space, k, "far vs oracle"))
            _assert_same(got, _np(ops.f16_list_topk(space, _dev(q), cc, cand, lims, k, return_status=True)), (space, k, "far vs compact"))
            assert set(LAYOUT_H.sentinels()) <= set(got[1][:, :10].ravel().tolist())      # every sentinel sits in a top-10
    finally:
        cbuf = qbuf = cv = qv = None
        gc.collect()
        torch.cuda.empty_cache()
