"""Product quantisation on the host: the C ABI (symbols, tsim_pq_code_bytes, the workspace function, argument checks before any
launch), the ops' refusals, and the properties of the numpy restatement in tests/pq_cases.py that the GPU tests compare with."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pq_cases as pc
from text_similarity_amd import _lib, ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tsim_pq_code_bytes", "tsim_pq_encode_rows", "tsim_pq_tables", "tsim_pq_adc_topk_workspace_bytes", "tsim_pq_adc_topk")
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
    assert L.tsim_version() == 104


def test_code_bytes(L):
    assert [L.tsim_pq_code_bytes(M) for M in (1, 15, 16, 17, 48, 64)] == [16, 16, 16, 32, 48, 64]
    assert [L.tsim_pq_code_bytes(M) for M in (0, 65, -1)] == [0, 0, 0]
    assert [pc.code_bytes(M) for M in (0, 1, 15, 16, 17, 48, 64, 65)] == [0, 16, 16, 16, 32, 48, 64, 0]
    assert ops.pq_code_bytes(33) == 48
    for M in (0, 65):
        with pytest.raises(ValueError):
            ops.pq_code_bytes(M)


def test_workspace_bytes(L):
    ws = L.tsim_pq_adc_topk_workspace_bytes
    sizes = [ws(Q, 100_000, 48, 10) for Q in (1, 2, 16, 256, 4096, 16384)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert ws(16, 100_000, 48, 1024) >= ws(16, 100_000, 48, 1023) > 0
    assert ws(16, 0, 48, 10) > 0
    assert ws(16, 1000, 48, 1025) == 0 and ws(16, 1000, 48, 0) == 0
    assert ws(0, 1000, 48, 10) == 0 and ws(16, -1, 48, 10) == 0
    assert ws(16, 1000, 0, 10) == 0 and ws(16, 1000, 65, 10) == 0


def test_argument_validation_returns_error_codes(L):
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15
    enc, tab, adc = L.tsim_pq_encode_rows, L.tsim_pq_tables, L.tsim_pq_adc_topk
    # encode: x, x_dtype, rows, d, ld_in, codebooks, M, codes, ld_code, stream
    assert enc(None, 0, 4, 8, 8, p, 2, p, 16, None) == 1
    assert enc(p, 0, 4, 8, 8, None, 2, p, 16, None) == 1
    assert enc(p, 0, 4, 8, 8, p, 2, None, 16, None) == 1
    assert enc(p, 0, 4, 8, 8, p, 3, p, 16, None) == 1            # d % M != 0
    assert b"d % M" in L.tsim_last_error()
    assert enc(p, 0, 4, 130, 130, p, 2, p, 16, None) == 1        # dsub = 65 > 64
    assert enc(p, 0, 4, 1040, 1040, p, 52, p, 64, None) == 1     # d > 1024
    assert enc(p, 0, 4, 65, 65, p, 65, p, 80, None) == 1         # M > 64
    assert enc(p, 0, 4, 8, 8, p, 0, p, 16, None) == 1
    assert enc(p, 0, 4, 8, 7, p, 2, p, 16, None) == 1            # ld_in < d
    assert enc(p, 7, 4, 8, 8, p, 2, p, 16, None) == 1            # unknown dtype
    assert enc(p, 0, 4, 8, 8, p, 2, p, 24, None) == 1            # stride not a multiple of 16
    assert b"multiple of 16" in L.tsim_last_error()
    assert enc(p, 0, 4, 34, 34, p, 17, p, 16, None) == 1         # stride below tsim_pq_code_bytes(17) = 32
    assert enc(p, 0, 4, 8, 8, p, 2, p + 4, 16, None) == 1        # rows not on a 16-byte boundary
    assert enc(p, 0, -1, 8, 8, p, 2, p, 16, None) == 1
    assert enc(p, 0, 0, 8, 8, p, 2, p, 16, None) == 0            # no rows: nothing to launch
    # tables: space, eq_f32, ldq, Q, codebooks, d, M, tables, exps, stream
    assert tab(IP, None, 8, 1, p, 8, 2, p, p, None) == 1
    assert tab(IP, p, 8, 1, None, 8, 2, p, p, None) == 1
    assert tab(IP, p, 8, 1, p, 8, 2, None, p, None) == 1
    assert tab(IP, p, 8, 1, p, 8, 2, p, None, None) == 1
    assert tab(_lib.SPACE_COSINE, p, 8, 1, p, 8, 2, p, p, None) == 1
    assert tab(IP, p, 8, 1, p, 8, 3, p, p, None) == 1
    assert tab(L2, p, 130, 1, p, 130, 2, p, p, None) == 1
    assert tab(L2, p, 7, 1, p, 8, 2, p, p, None) == 1
    assert tab(L2, p, 8, 1, p, 8, 2, p + 4, p, None) == 1        # tables not 16-byte aligned
    assert tab(L2, p, 8, 0, p, 8, 2, p, p, None) == 0
    # adc: space, tables, Q, codes, ldc, N, M, k, out_val, out_idx, idx_offset, workspace, bytes, stream
    big = 1 << 30
    assert adc(IP, None, 1, p, 16, 10, 2, 5, p, p, 0, p, big, None) == 1
    assert adc(IP, p, 1, None, 16, 10, 2, 5, p, p, 0, p, big, None) == 1
    assert adc(IP, p, 1, p, 16, 10, 2, 5, None, p, 0, p, big, None) == 1
    assert adc(IP, p, 1, p, 16, 10, 2, 5, p, None, 0, p, big, None) == 1
    assert adc(3, p, 1, p, 16, 10, 2, 5, p, p, 0, p, big, None) == 1
    assert adc(IP, p, 1, p, 16, 10, 0, 5, p, p, 0, p, big, None) == 1
    assert adc(IP, p, 1, p, 16, 10, 65, 5, p, p, 0, p, big, None) == 1
    assert adc(IP, p, 1, p, 16, 10, 2, 0, p, p, 0, p, big, None) == 1
    assert adc(IP, p, 1, p, 16, 10, 2, 1025, p, p, 0, p, big, None) == 1
    assert adc(IP, p, 0, p, 16, 10, 2, 5, p, p, 0, p, big, None) == 1
    assert adc(IP, p, 1, p, 24, 10, 2, 5, p, p, 0, p, big, None) == 1          # stride not a multiple of 16
    assert adc(IP, p, 1, p, 16, 10, 17, 5, p, p, 0, p, big, None) == 1         # stride below tsim_pq_code_bytes(17)
    assert adc(L2, p, 1, p + 8, 16, 10, 2, 5, p, p, 0, p, big, None) == 1      # rows not on a 16-byte boundary
    need = L.tsim_pq_adc_topk_workspace_bytes(1, 10, 2, 5)
    assert adc(IP, p, 1, p, 16, 10, 2, 5, p, p, 0, p, need - 1, None) == 3     # short workspace
    assert adc(IP, p, 1, p, 16, 10, 2, 5, p, p, 0, None, big, None) == 3


def test_ops_refuse_without_a_gpu():
    cb = torch.zeros(2, 256, 4)
    x = torch.zeros(3, 8)
    codes = torch.zeros(3, 16, dtype=torch.uint8)
    tables = torch.zeros(1, 2, 256, dtype=torch.int32)
    for call in (lambda: ops.pq_encode_rows(x, cb), lambda: ops.pq_tables(x, cb, "ip"), lambda: ops.pq_adc_topk(x, cb, codes, 2),
                 lambda: ops.pq_adc_topk_tables(tables, codes, 2), lambda: ops.pq_decode_rows(codes, cb),
                 lambda: ops.pq_codes_from_numpy(codes, 16)):
        with pytest.raises(_lib.TsimError):
            call()
    with pytest.raises(ValueError):
        ops.pq_tables(x, cb, "cosine")


# ------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("M,d", [(1, 8), (3, 12), (33, 66), (48, 384), (64, 1024)])
def test_table_bound(M, d):
    rng = np.random.default_rng(M)
    for scale in (1e-20, 1.0, 1e20):
        cb = pc.random_codebooks(rng, d, M, scale)
        q = (rng.standard_normal((3, d)) * scale).astype(np.float32)
        for space in ("ip", "l2"):
            t, e = pc.tables_ref(q, cb, space)
            assert (pc.table_bound(t) <= 2 ** 24).all(), (space, scale)
            assert (pc.table_bound(t) >= 2 ** 22 // (2 * M)).all()       # and the scale is used: the largest entry has ~23 - log2 M bits
            assert np.abs(t).max() <= 2 ** 23
            if space == "l2":
                assert (t <= 0).all()
            # the integer table is the float64 one to within half a unit
            m, dsub = 0, d // M
            Lm = pc.dot(q[:, :dsub], cb[m]) if space == "ip" else -pc.sqdist(q[:, :dsub], cb[m])
            assert (np.abs(np.ldexp(Lm, e[:, None].astype(np.int64)) - t[:, m]) <= 0.5).all()


def test_zero_and_nan_queries_give_zero_tables():
    rng = np.random.default_rng(2)
    cb = pc.random_codebooks(rng, 12, 3)
    q = rng.standard_normal((4, 12)).astype(np.float32)
    q[1] = 0
    q[2, 5] = np.nan
    q[3, 0] = np.inf
    t, e = pc.tables_ref(q, cb, "ip")
    assert t[0].any() and e[0] != 0
    assert not t[1:].any() and (e[1:] == 0).all()
    t, e = pc.tables_ref(q, cb, "l2")
    assert t[0].any() and t[1].any()                  # a zero query is not at distance zero from the centroids
    assert not t[2:].any() and (e[2:] == 0).all()
    t, e = pc.tables_ref(np.zeros((1, 12), np.float32), np.zeros_like(cb), "l2")
    assert not t.any() and e[0] == 0


def test_encoding_ties_and_non_finite():
    rng = np.random.default_rng(3)
    cb = pc.tied_codebooks(rng, 12, 3)
    on3 = pc.decode_ref(np.full((1, 3), 200, np.uint8), cb)         # sits on centroids 3 = 7 = 200: the lowest wins
    on0 = pc.decode_ref(np.full((1, 3), 255, np.uint8), cb)
    assert pc.encode_ref(on3, cb)[0, :3].tolist() == [3, 3, 3]
    assert pc.encode_ref(on0, cb)[0, :3].tolist() == [0, 0, 0]
    x = rng.standard_normal((3, 12)).astype(np.float32)
    x[0, 5], x[1, 9], x[2, 0] = np.nan, np.inf, -np.inf
    codes = pc.encode_ref(x, cb)
    assert codes.shape == (3, 16) and not codes[:, 3:].any()
    assert codes[0, 1] == 0 and codes[1, 2] == 0 and codes[2, 0] == 0
    rows = pc.encoder_rows(rng, 40, cb)
    assert np.isnan(rows).any() and np.isinf(rows).any()
    assert np.array_equal(pc.encode_ref(rows, cb)[:, :3], pc.encode_loop(rows, cb))


def test_lossless_round_trip():
    rng = np.random.default_rng(4)
    for d, M in ((8, 1), (12, 3), (66, 33)):
        cb = pc.random_codebooks(rng, d, M)
        x, codes = pc.lossless(rng, 300, cb)
        got = pc.encode_ref(x, cb)
        assert np.array_equal(got[:, :M], codes)
        assert np.array_equal(pc.decode_ref(got, cb).view(np.uint32), x.view(np.uint32))


def test_adc_restatement_against_a_loop():
    rng = np.random.default_rng(5)
    M, N, Q = 3, 23, 4
    codes = pc.pad_codes(pc.binary_codes(rng, N, M), junk_rng=rng)
    for space in ("ip", "l2"):
        t = pc.small_tables(rng, Q, M, space)
        loop = [[sum(int(t[q, m, codes[r, m]]) for m in range(M)) for r in range(N)] for q in range(Q)]
        assert pc.scores_ref(t, codes).tolist() == loop
        for k in (1, 5, 30):
            v, i = pc.adc_topk_ref(t, codes, k, space, idx_offset=7)
            for q in range(Q):
                ranked = sorted(range(N), key=lambda r: (-loop[q][r], r))[:k]
                pad = k - len(ranked)
                sign, padv = (1, pc.INT32_MIN) if space == "ip" else (-1, pc.INT32_MAX)
                assert v[q].tolist() == [sign * loop[q][r] for r in ranked] + [padv] * pad
                assert i[q].tolist() == [r + 7 for r in ranked] + [-1] * pad
    f = pc.values_to_float(np.array([[3, pc.INT32_MIN]], np.int32), np.array([400], np.int32), "ip")
    assert f[0, 0] == 0 and f[0, 1] == -np.inf                       # 3 x 2^-400 is no float32; 2^-400 need not be one
    f = pc.values_to_float(np.array([[3, pc.INT32_MAX]], np.int32), np.array([-2], np.int32), "l2")
    assert f[0].tolist() == [12.0, np.inf]
