"""Product quantisation on the GPU (ops.pq_encode_rows / pq_tables / pq_adc_topk_tables / pq_adc_topk): every result is compared
for equality with the numpy restatement of tests/pq_cases.py.  No tolerance anywhere.

Shapes are the smallest at which each kernel can go wrong: (d, M) with one sub-space, an odd M, M over two and three 16-byte words
and the largest (dsub 8, 4, 2, 8, 16); row counts around a step of 256 rows and one block of the running list (1 024), more than
one chunk (5 000) and a wrapped encoder grid (70 000 > 256 x 256); k around the list lengths (64, 128, 1 024); a few queries
(1, 5, 17) and hundreds (256, 257): a workgroup serves one query and one chunk of rows."""
import functools

import numpy as np
import pytest
import torch

import pq_cases as pc
from text_similarity_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _eq(t, a):
    return np.array_equal(t.cpu().numpy(), a)


@functools.lru_cache(maxsize=None)
def _encoder_case(d, M):
    rng = np.random.default_rng(100 * d + M)
    cb = pc.tied_codebooks(rng, d, M)
    x = pc.encoder_rows(rng, 300, cb)
    return cb, x, pc.encode_ref(x, cb), pc.encode_ref(pc.bf16_round(x), cb)


# ------------------------------------------------------------------------------------------------- the encoder
@pytest.mark.parametrize("d,M", pc.SHAPES)
def test_encode_rows(d, M):
    cb, x, want, want_bf16 = _encoder_case(d, M)
    w = pc.code_bytes(M)
    got = ops.pq_encode_rows(_dev(x), _dev(cb))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (300, w)
    g = got.cpu().numpy()
    bad = np.argwhere(g != want)
    assert bad.size == 0, (bad[:5], [(g[r, c], want[r, c]) for r, c in bad[:5]])
    assert not g[:, M:].any()
    wide = np.full((300, d + 5), np.float32(7.0))                                          # ld_in = d + 5
    wide[:, :d] = x
    assert _eq(ops.pq_encode_rows(_dev(wide)[:, :d], _dev(cb)), want)
    xb = _dev(wide).to(torch.bfloat16)[:, :d]                                              # bf16 rows, ld_in = d + 5
    assert np.array_equal(xb.float().cpu().numpy(), pc.bf16_round(x), equal_nan=True)
    assert _eq(ops.pq_encode_rows(xb, _dev(cb)), want_bf16)
    out = torch.full((300, w + 16), 0xA5, dtype=torch.uint8, device=DEV)                   # ld_code = stride + 16
    ops.pq_encode_rows(_dev(x), _dev(cb), out=out[:, :w])
    o = out.cpu().numpy()
    assert np.array_equal(o[:, :w], want) and (o[:, w:] == 0xA5).all()
    assert _eq(ops.pq_codes_from_numpy(want[:, :M], M, device=DEV), want)
    assert np.array_equal(ops.pq_decode_rows(got, _dev(cb)).cpu().numpy().view(np.uint32), pc.decode_ref(want, cb).view(np.uint32))


def test_encode_rows_grid_wraps():
    rng = np.random.default_rng(7)
    cb = pc.tied_codebooks(rng, 12, 3)
    x = pc.encoder_rows(rng, 70_000, cb)
    want = np.concatenate([pc.encode_ref(x[i:i + 10_000], cb) for i in range(0, 70_000, 10_000)])
    assert _eq(ops.pq_encode_rows(_dev(x), _dev(cb)), want)


def test_lossless_rows_decode_to_themselves():
    rng = np.random.default_rng(8)
    cb = pc.random_codebooks(rng, 66, 33)
    x, codes = pc.lossless(rng, 300, cb)
    got = ops.pq_encode_rows(_dev(x), _dev(cb))
    assert _eq(got[:, :33], codes)
    assert np.array_equal(ops.pq_decode_rows(got, _dev(cb)).cpu().numpy().view(np.uint32), x.view(np.uint32))


def test_widest_sub_vector():
    """dsub = 64: the encoder's codebook fills 64 KiB of LDS and a lane holds 64 elements"""
    rng = np.random.default_rng(9)
    d, M = 1024, 16
    cb = pc.tied_codebooks(rng, d, M)
    x = pc.encoder_rows(rng, 70, cb)
    assert _eq(ops.pq_encode_rows(_dev(x), _dev(cb)), pc.encode_ref(x, cb))
    q = _queries(rng, 5, d)
    for space in ("ip", "l2"):
        want_t, want_e = pc.tables_ref(q, cb, space)
        t, e = ops.pq_tables(_dev(q), _dev(cb), space)
        assert _eq(t, want_t) and _eq(e, want_e)


def test_codebooks_must_be_finite_and_match():
    cb = np.zeros((3, 256, 4), np.float32)
    cb[1, 5, 2] = np.inf
    x = torch.zeros((2, 12), device=DEV)
    for call in (lambda: ops.pq_encode_rows(x, _dev(cb)), lambda: ops.pq_tables(x, _dev(cb), "ip")):
        with pytest.raises(ValueError, match="finite"):
            call()
    with pytest.raises(ValueError):
        ops.pq_encode_rows(torch.zeros((2, 16), device=DEV), _dev(np.zeros((3, 256, 4), np.float32)))      # width mismatch
    with pytest.raises(ValueError):
        ops.pq_tables(x, _dev(np.zeros((3, 255, 4), np.float32)), "ip")


# ------------------------------------------------------------------------------------------------- the tables
def _queries(rng, Q, d):
    q = rng.standard_normal((Q, d)).astype(np.float32)
    if Q >= 5:
        q[1] *= np.float32(1e-20)
        q[2] *= np.float32(1e20)
        q[3] = 0
        q[4, d // 2] = np.nan
    return q


@pytest.mark.parametrize("space", ("ip", "l2"))
@pytest.mark.parametrize("d,M", pc.SHAPES)
def test_tables(d, M, space):
    rng = np.random.default_rng(1000 * d + M)
    cb = pc.random_codebooks(rng, d, M)
    for Q in (1, 5):
        q = _queries(rng, Q, d)
        want_t, want_e = pc.tables_ref(q, cb, space)
        t, e = ops.pq_tables(_dev(q), _dev(cb), space)
        assert t.dtype == torch.int32 and tuple(t.shape) == (Q, M, 256) and e.dtype == torch.int32
        assert _eq(e, want_e), (e.cpu().numpy(), want_e)
        bad = np.argwhere(t.cpu().numpy() != want_t)
        assert bad.size == 0, bad[:5]
        if Q == 5:
            assert not want_t[4].any() and want_e[4] == 0 and len(set(want_e.tolist())) >= 3
            wide = np.full((Q, d + 3), np.float32(2.0))                                    # ldq = d + 3
            wide[:, :d] = q
            t2, e2 = ops.pq_tables(_dev(wide)[:, :d], _dev(cb), space)
            assert _eq(t2, want_t) and _eq(e2, want_e)
    for scale in (1e-20, 1e20):                                                             # scaled codebooks as well
        cbs = (cb * np.float32(scale)).astype(np.float32)
        q = (rng.standard_normal((1, d)) * scale).astype(np.float32)
        want_t, want_e = pc.tables_ref(q, cbs, space)
        t, e = ops.pq_tables(_dev(q), _dev(cbs), space)
        assert _eq(t, want_t) and _eq(e, want_e) and want_t.any()


# ------------------------------------------------------------------------------------------------- ADC top-k
# (N, Q, k, M, space, tables, codes, wide stride with junk, idx_offset)
ADC_CASES = [
    (0, 1, 10, 3, "ip", "random", "uniform", False, 0),            # an empty corpus: padding only
    (1, 5, 10, 16, "l2", "random", "uniform", False, 5),           # k > N
    (255, 17, 64, 17, "ip", "small", "binary", True, 0),           # a short last step; M one byte into a second word; ties
    (257, 5, 100, 48, "l2", "small", "binary", True, 11),          # just over a step; ties under l2
    (1025, 17, 1024, 64, "ip", "random", "uniform", True, 0),      # just over a list block; the longest list; one query a group
    (1025, 1, 1, 64, "l2", "random", "uniform", False, 0),
    (5000, 5, 10, 48, "ip", "small", "binary", False, 1 << 40),    # several chunks; ties across chunks
    (5000, 17, 100, 3, "l2", "random", "uniform", True, 3),        # seventeen groups by several chunks; the smallest odd M
    (5000, 17, 64, 17, "ip", "one_hot", "uniform", True, 0),       # byte m meets table m
    (257, 5, 257, 33, "l2", "one_hot", "uniform", False, 0),
    (5000, 5, 1, 16, "ip", "random", "binary", False, 0),
    (1025, 257, 10, 17, "ip", "random", "uniform", True, 0),       # many queries by two chunks: a grid of 257 x 2 workgroups
    (600, 256, 100, 48, "l2", "small", "binary", False, 9),        # the same under l2 with ties
    (300, 256, 1024, 64, "ip", "random", "uniform", False, 0),     # M = 64 with the longest list: the largest LDS image, 80 KiB
]


@functools.lru_cache(maxsize=None)
def _adc_case(i):
    N, Q, k, M, space, tk, ck, wide, off = ADC_CASES[i]
    rng = np.random.default_rng(50 + i)
    tables = {"random": pc.random_tables, "small": pc.small_tables}[tk](rng, Q, M, space) if tk != "one_hot" else \
        pc.one_hot_tables(Q, M, space)
    codes = (pc.uniform_codes if ck == "uniform" else pc.binary_codes)(rng, N, M)
    w = pc.code_bytes(M)
    padded = pc.pad_codes(codes, 2 * w, junk_rng=rng) if wide else pc.pad_codes(codes)
    assert (pc.table_bound(tables) <= 2 ** 24).all()
    return tables, padded, pc.adc_topk_ref(tables, padded, k, space, off)


@pytest.mark.parametrize("i", range(len(ADC_CASES)))
def test_adc_topk(i):
    N, Q, k, M, space, tk, ck, wide, off = ADC_CASES[i]
    tables, codes, (want_v, want_i) = _adc_case(i)
    if tk == "one_hot" and space == "ip":
        assert (want_v[:, 0] >= 1000).all() and (want_v[:, -1] == 0).all()                 # both kinds of row are ranked
    if tk == "small":
        assert min(len(set(r.tolist())) for r in want_v) < want_v.shape[1] or k == 1      # ties decide places
    c = _dev(codes) if N else torch.zeros((0, pc.code_bytes(M)), dtype=torch.uint8, device=DEV)
    if wide:
        c = c[:, :pc.code_bytes(M)]                                                        # row views: stride 2 x code_bytes(M)
    v, ix = ops.pq_adc_topk_tables(_dev(tables), c, k, space, idx_offset=off)
    assert v.dtype == torch.int32 and ix.dtype == torch.int64 and tuple(v.shape) == (Q, k)
    gv, gi = v.cpu().numpy(), ix.cpu().numpy()
    bad = np.argwhere((gv != want_v) | (gi != want_i))
    assert bad.size == 0, (bad[:5], [(gv[q, t], want_v[q, t], gi[q, t], want_i[q, t]) for q, t in bad[:5]])


@pytest.mark.parametrize("space", ("ip", "l2"))
def test_adc_topk_from_float_queries(space, monkeypatch):
    rng = np.random.default_rng(77)
    d, M, N, Q, k = 66, 33, 300, 5, 10
    cb = pc.random_codebooks(rng, d, M)
    x = rng.standard_normal((N, d)).astype(np.float32)
    q = _queries(rng, Q, d)
    codes = pc.encode_ref(x, cb)
    tables, exps = pc.tables_ref(q, cb, space)
    want_v, want_i = pc.adc_topk_ref(tables, codes, k, space)
    v, ix, e = ops.pq_adc_topk(_dev(q), _dev(cb), _dev(codes), k, space, raw=True)
    assert _eq(v, want_v) and _eq(ix, want_i) and _eq(e, exps)
    s, ix2 = ops.pq_adc_topk(_dev(q), _dev(cb), _dev(codes), k, space)
    want_f = pc.values_to_float(want_v, exps, space)
    assert s.dtype == torch.float32 and _eq(ix2, want_i)
    assert np.array_equal(s.cpu().numpy().view(np.uint32), want_f.view(np.uint32))
    assert np.isinf(want_f[2]).all() or np.abs(want_f[2]).max() > 1e18                     # the 1e20 query: 2^-e is large
    # the scores ARE the reconstruction's: each of the M entries is within half a unit of 2^-e, then one float32 rounding
    rec = pc.decode_ref(codes, cb).astype(np.float64)
    exact = rec @ q[0].astype(np.float64) if space == "ip" else ((rec - q[0].astype(np.float64)) ** 2).sum(1)
    atol = M / 2 * 2.0 ** -float(exps[0]) + np.abs(exact).max() * 2.0 ** -23
    assert np.allclose(want_f[0], exact[want_i[0]], rtol=0, atol=atol)
    # fewer rows than k: padding becomes -inf / +inf; slices of the query set give the same answer
    monkeypatch.setattr(ops, "PQ_TABLE_BUDGET", 2 * M * 1024)
    s3, ix3 = ops.pq_adc_topk(_dev(q), _dev(cb), _dev(codes[:4]), k, space)
    wv, wi = pc.adc_topk_ref(tables, codes[:4], k, space)
    assert _eq(ix3, wi) and (wi[:, 4:] == -1).all()
    assert np.array_equal(s3.cpu().numpy().view(np.uint32), pc.values_to_float(wv, exps, space).view(np.uint32))
    assert (s3[:, 4:].cpu().numpy() == (-np.inf if space == "ip" else np.inf)).all()
