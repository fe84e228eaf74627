"""IVF-PQ on the host: the C ABI (symbols, TSIM_IVFPQ_SEG, the workspace functions, argument checks before any launch) and the
properties of the numpy restatement in tests/ivfpq_cases.py that the GPU tests compare with."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ivfpq_cases as ic
import pq_cases as pc
from text_similarity_amd import _lib, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tsim_ivfpq_tables_workspace_bytes", "tsim_ivfpq_tables", "tsim_ivfpq_scan_workspace_bytes", "tsim_ivfpq_scan_topk")
IP, L2 = _lib.SPACE_DOT, _lib.SPACE_L2


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        from text_similarity_amd.build import build
        build(verbose=False)
    return _lib.lib()


# ------------------------------------------------------------------------------------------------- the C ABI, no launch
def test_header_symbols_exported_and_bound(L):
    hdr = open(os.path.join(REPO, "include", "tsim.h")).read()
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert f"{name}(" in hdr, name
        assert name in _lib.DECLARED_SYMBOLS, name
        assert hasattr(cdll, name), name
        assert getattr(L, name).argtypes is not None, name
    seg = int(re.search(r"#define TSIM_IVFPQ_SEG (\d+)", hdr).group(1))
    assert seg == _lib.IVFPQ_SEG == ops.IVFPQ_SEG and seg % 256 == 0 and seg > 0


def test_workspace_bytes(L):
    ws = L.tsim_ivfpq_scan_workspace_bytes                       # (Q, nprobe, max_list_len, k)
    base = (4, 8, 10_000, 10)
    assert ws(*base) > 0
    for arg, values in enumerate(((1, 2, 16, 256, 4096, 65536), (1, 2, 8, 64, 1024), (0, 1, 4095, 4096, 4097, 10 ** 5, 10 ** 7, 10 ** 9),
                                  (1, 2, 10, 100, 1023, 1024))):
        sizes = [ws(*(base[:arg] + (v,) + base[arg + 1:])) for v in values]
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (arg, sizes)
    for bad in ((0, 8, 100, 10), (4, 0, 100, 10), (4, 8, -1, 10), (4, 8, 100, 0), (4, 8, 100, 1025)):
        assert ws(*bad) == 0, bad
    wt = L.tsim_ivfpq_tables_workspace_bytes                     # (Q, nprobe)
    assert [wt(Q, 8) for Q in (1, 2, 100, 10 ** 6)] == sorted(wt(Q, 8) for Q in (1, 2, 100, 10 ** 6)) and wt(1, 8) > 0
    assert [wt(16, p) for p in (1, 2, 64, 1024)] == sorted(wt(16, p) for p in (1, 2, 64, 1024)) and wt(16, 1) > 0
    assert wt(0, 8) == 0 and wt(16, 0) == 0 and wt(-1, 8) == 0 and wt(1 << 30, 1 << 10) == 0


def test_argument_validation_returns_error_codes(L):
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15
    big = 1 << 30

    def tab(space=IP, q=p, ldq=8, Q=1, cent=p, ldc=8, nlist=3, probes=p, nprobe=2, cb=p, d=8, M=2, tables=p, bias=p, exps=p, ws=p,
            nbytes=big):
        return L.tsim_ivfpq_tables(space, q, ldq, Q, cent, ldc, nlist, probes, nprobe, cb, d, M, tables, bias, exps, ws, nbytes, None)

    assert tab(space=_lib.SPACE_COSINE) == 1 and tab(space=7) == 1
    assert b"space" in L.tsim_last_error()
    for name in ("q", "cent", "probes", "cb", "tables", "exps"):
        assert tab(**{name: None}) == 1, name
    assert tab(bias=None) == 1 and tab(space=L2, bias=None, Q=0) == 0        # (l2 takes no bias)
    assert tab(M=3) == 1                                             # d % M != 0
    assert b"d % M" in L.tsim_last_error()
    assert tab(M=0) == 1 and tab(d=65, ldq=65, ldc=65, M=65) == 1 and tab(d=130, ldq=130, ldc=130, M=2) == 1
    assert tab(d=1040, ldq=1040, ldc=1040, M=52) == 1
    assert tab(nprobe=0) == 1
    assert b"nprobe" in L.tsim_last_error()
    assert tab(ldq=7) == 1 and tab(ldc=7) == 1 and tab(nlist=0) == 1 and tab(Q=-1) == 1
    assert tab(tables=p + 4) == 1
    assert b"16-byte" in L.tsim_last_error()
    assert tab(Q=0) == 0                                             # no queries: nothing to launch
    need = L.tsim_ivfpq_tables_workspace_bytes(1, 2)
    assert tab(space=L2, nbytes=need - 1) == 3 and tab(space=L2, ws=None) == 3

    def scan(space=IP, tables=p, per_pair=0, bias=p, Q=1, codes=p, ldc=16, N=10, M=2, off=p, nlist=3, ids=p, probes=p, nprobe=2,
             hint=10, k=5, ov=p, oi=p, status=p, ws=p, nbytes=big):
        return L.tsim_ivfpq_scan_topk(space, tables, per_pair, bias, Q, codes, ldc, N, M, off, nlist, ids, probes, nprobe, hint, k, ov, oi, 0,
                                      status, ws, nbytes, None)

    assert scan(space=_lib.SPACE_COSINE) == 1 and scan(space=3) == 1
    for name in ("tables", "codes", "off", "ids", "probes", "ov", "oi"):
        assert scan(**{name: None}) == 1, name
    assert scan(M=0) == 1 and scan(M=65, ldc=80) == 1
    assert b"M=" in L.tsim_last_error()
    assert scan(k=0) == 1 and scan(k=1025) == 1
    assert b"k=" in L.tsim_last_error()
    assert scan(nprobe=0) == 1
    assert b"nprobe" in L.tsim_last_error()
    assert scan(Q=0) == 1 and scan(N=0) == 1 and scan(nlist=0) == 1 and scan(hint=-1) == 1
    assert scan(ldc=24) == 1                                         # stride not a multiple of 16
    assert b"multiple of 16" in L.tsim_last_error()
    assert scan(M=17, ldc=16) == 1                                   # stride below tsim_pq_code_bytes(17) = 32
    assert scan(codes=p + 8) == 1                                    # rows not on a 16-byte boundary
    assert scan(tables=p + 4) == 1                                   # tables not on a 16-byte boundary
    assert b"tables" in L.tsim_last_error()
    need = L.tsim_ivfpq_scan_workspace_bytes(1, 2, 10, 5)
    assert scan(nbytes=need - 1) == 3 and scan(ws=None) == 3


def test_ops_refuse_without_a_gpu():
    cb, x, cent = torch.zeros(2, 256, 4), torch.zeros(3, 8), torch.zeros(4, 8)
    codes = torch.zeros(5, 16, dtype=torch.uint8)
    tables = torch.zeros(3, 2, 256, dtype=torch.int32)
    off, ids, probes = torch.zeros(5, dtype=torch.int64), torch.zeros(5, dtype=torch.int32), torch.zeros(3, 2, dtype=torch.int64)
    for call in (lambda: ops.ivfpq_tables(x, cent, probes, cb, "ip"), lambda: ops.ivfpq_scan_topk("ip", tables, None, codes, off, ids, probes, 2),
                 lambda: ops.ivfpq_search(x, cent, cb, codes, off, ids, probes, 2)):
        with pytest.raises(_lib.TsimError):
            call()
    with pytest.raises(ValueError):
        ops.ivfpq_tables(x, cent, probes, cb, "cosine")


# ------------------------------------------------------------------------------------------------- the restatement
def _case(rng, d, M, Q=3, nlist=5, nprobe=3, cscale=3.0, scale=1.0):
    cb = pc.random_codebooks(rng, d, M, scale)
    cent = (rng.standard_normal((nlist, d)) * cscale * scale).astype(np.float32)
    q = (rng.standard_normal((Q, d)) * scale).astype(np.float32)
    probes = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(Q)]).astype(np.int64)
    return cb, cent, q, probes


@pytest.mark.parametrize("d,M", pc.SHAPES)
def test_score_bound(d, M):
    """max |bias| + sum_m max_j |T| < 2^24: every score is an exact int32 and an exact float32 in any order of additions"""
    rng = np.random.default_rng(d)
    for scale in (1e-18, 1.0, 1e15):
        for cscale in (1e-3, 1.0, 3.0, 100.0):
            cb, cent, q, probes = _case(rng, d, M, cscale=cscale, scale=scale)
            t, b, e = ic.tables_ip_ref(q, cent, probes, cb)
            assert (ic.score_bound(t, b) < 2 ** 24).all(), (scale, cscale)
            assert (ic.score_bound(t, b) >= 2 ** 22 // (2 * (M + 1))).all()    # and the scale is used: 2^clog < 2 (M + 1)
            t, e = ic.tables_l2_ref(q, cent, probes, cb)
            assert (ic.score_bound(t) < 2 ** 24).all() and (t <= 0).all()
            assert (ic.score_bound(t) >= 2 ** 22 // (2 * M)).all()


def test_bias_sets_the_exponent_and_padding_probes_are_skipped():
    rng = np.random.default_rng(1)
    cb, cent, q, probes = _case(rng, 12, 3, Q=4, nlist=7, nprobe=4, cscale=30.0)
    t0, e0 = pc.tables_ref(q, cb, "ip")
    t, b, e = ic.tables_ip_ref(q, cent, probes, cb)
    assert (e < e0).all() and (np.abs(b).max(axis=1) > np.abs(t).max(axis=(1, 2))).all()
    pad = probes.copy()
    pad[:, 1], pad[:, 3] = -1, 7 + 3
    t, b, e = ic.tables_ip_ref(q, cent, pad, cb)
    assert not b[:, 1].any() and not b[:, 3].any() and b[:, 0].all()
    t2, b2, e2 = ic.tables_ip_ref(q, cent, pad[:, [0, 2]], cb)                  # the padding changes nothing else
    assert np.array_equal(t, t2) and np.array_equal(b[:, [0, 2]], b2) and np.array_equal(e, e2)
    tl, el = ic.tables_l2_ref(q, cent, pad, cb)
    tl2, el2 = ic.tables_l2_ref(q, cent, pad[:, [0, 2]], cb)
    assert np.array_equal(tl[:, [0, 2]], tl2) and np.array_equal(el, el2) and not tl[:, [1, 3]].any()


def test_l2_exponent_is_common_to_a_querys_pairs():
    rng = np.random.default_rng(2)
    cb, cent, q, probes = _case(rng, 12, 3, Q=3, nlist=6, nprobe=3)
    cent[probes[0, 1]] *= 64                                          # one far centroid: its pair alone would take a smaller e
    t, e = ic.tables_l2_ref(q, cent, probes, cb)
    alone = [ic.tables_l2_ref(q, cent, probes[:, j:j + 1], cb) for j in range(3)]
    assert e[0] == min(a[1][0] for a in alone) == alone[1][1][0] and alone[0][1][0] > e[0]
    for j in range(3):                                               # a pair's table is its own float64 table on the query's exponent
        rq = ic.residuals(q[0:1], cent, probes[0, j:j + 1])
        Lm = -pc.sqdist(rq[:, :4], cb[0])
        assert np.array_equal(t[0, j, 0], np.rint(np.ldexp(Lm[0], int(e[0]))).astype(np.int32))


def test_non_finite_and_zero_queries_give_zero_tables():
    rng = np.random.default_rng(3)
    cb, cent, q, probes = _case(rng, 12, 3, Q=5, nlist=6, nprobe=3)
    q[1] = 0
    q[2, 5] = np.nan
    q[3, 0] = np.inf
    q[4, 7], cent[probes[4, 2], 7] = 3e38, -3e38                      # finite, but ONE pair's residual overflows to +inf
    t, b, e = ic.tables_ip_ref(q, cent, probes, cb)
    assert t[0].any() and b[0].any() and e[0] != 0
    assert not t[1:4].any() and not b[1:4].any() and (e[1:4] == 0).all()
    assert b[4].any() and e[4] != 0                                  # (no float32 subtraction in the inner product)
    t, e = ic.tables_l2_ref(q, cent, probes, cb)
    assert t[0].any() and t[1].any() and e[1] != 0                   # a zero query is not at distance zero
    assert not t[2:].any() and (e[2:] == 0).all()
    t, e = ic.tables_l2_ref(q[4:], cent, probes[4:, :2], cb)          # without that pair the query is usable
    assert t.any() and e[0] != 0
    zero = np.zeros((1, 12), np.float32)
    t, b, e = ic.tables_ip_ref(q[:1], np.zeros_like(cent), probes[:1], np.zeros_like(cb))
    assert not t.any() and not b.any() and e[0] == 0
    t, e = ic.tables_l2_ref(zero, np.zeros_like(cent), probes[:1], np.zeros_like(cb))
    assert not t.any() and e[0] == 0


def test_tables_against_a_literal_loop():
    rng = np.random.default_rng(4)
    cb, cent, q, probes = _case(rng, 4, 2, Q=3, nlist=4, nprobe=3)
    probes[0, 1], probes[1, 0] = -1, 9
    q[2, 1] = np.nan
    t, b, e = ic.tables_ip_ref(q, cent, probes, cb)
    lt, lb, le = ic.tables_loop(q, cent, probes, cb, "ip")
    assert np.array_equal(t, lt) and np.array_equal(b, lb) and np.array_equal(e, le) and e[0] != 0
    t, e = ic.tables_l2_ref(q, cent, probes, cb)
    lt, _, le = ic.tables_loop(q, cent, probes, cb, "l2")
    assert np.array_equal(t, lt) and np.array_equal(e, le) and e[0] != 0


@pytest.mark.parametrize("space", ("ip", "l2"))
def test_without_residuals_and_all_lists_it_is_the_flat_adc(space):
    rng = np.random.default_rng(5)
    M, N, Q, nlist = 3, 400, 4, 6
    codes = pc.pad_codes(pc.binary_codes(rng, N, M), junk_rng=rng)               # arrival order
    lists = rng.integers(0, nlist, size=N)
    order, list_off, row_ids = ic.pack(lists, nlist)
    probes = np.stack([rng.permutation(nlist) for _ in range(Q)]).astype(np.int64)
    t = pc.small_tables(rng, Q, M, space)
    for k in (1, 10, 500):
        v, i, st = ic.scan_ref(t, None, codes[order], list_off, row_ids, probes, k, space, idx_offset=7)
        wv, wi = pc.adc_topk_ref(t, codes, k, space, idx_offset=7)
        assert np.array_equal(v, wv) and np.array_equal(i, wi) and not st.any()


def test_scan_restatement_details():
    rng = np.random.default_rng(6)
    M, Q = 2, 2
    list_off = np.array([0, 3, 3, 8], np.int64)
    codes = pc.pad_codes(pc.uniform_codes(rng, 8, M))
    ids = np.array([5, -1, 2, 7, 0, -3, 1, 4], np.int32)
    t = pc.random_tables(rng, Q, M, "ip") // 2
    bias = np.array([[100, -7, 9], [0, 0, 5]], np.int32)
    probes = np.array([[2, 5, 0], [1, -1, 2]], np.int64)
    v, i, st = ic.scan_ref(t, bias, codes, list_off, ids, probes, 10, "ip")
    assert st.tolist() == [ic.ST_LIST, 0]
    s = pc.scores_ref(t, codes)
    want0 = sorted([(-(int(s[0, r]) + (100 if r >= 3 else 9)), int(ids[r])) for r in range(8) if ids[r] >= 0])
    assert i[0].tolist() == [w[1] for w in want0] + [-1] * 4 and v[0].tolist() == [-w[0] for w in want0] + [pc.INT32_MIN] * 4
    assert set(i[1][:4].tolist()) == {7, 0, 1, 4} and (i[1][4:] == -1).all()
    bad = np.array([0, 6, 2, 9], np.int64)                           # decreasing, and beyond N = 8
    assert ic.clean_offsets(bad, 8).tolist() == [0, 6, 6, 8]
    v, i, st = ic.scan_ref(t, bias, codes, bad, ids, np.array([[0, -1, -1], [1, 2, -1]], np.int64), 10, "ip")
    assert st.tolist() == [0, ic.ST_OFF] and (i[1] >= 0).sum() == 2
