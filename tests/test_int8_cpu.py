"""int8 embeddings on the host: the numpy restatement of tests/int8_cases.py against sentence-transformers' literal expression and
a plain Python loop, the C ABI (symbols, tsim_int8_bytes, the workspace function, argument checks before any launch), the ops'
refusals, and the index file format."""
import os

import numpy as np
import pytest

import int8_cases as ic
from text_similarity_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tsim_int8_bytes", "tsim_quantize_int8_rows", "tsim_int8_ip_topk_workspace_bytes", "tsim_int8_ip_topk", "tsim_int8_rescore_topk")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        from text_similarity_amd.build import build
        build(verbose=False)
    return _lib.lib()


# ------------------------------------------------------------------------------------------------- the restatement
def test_quantize_ref_is_the_sentence_transformers_expression_in_range():
    rng = np.random.default_rng(5)
    for d in (1, 17, 384):
        x = ic.random_rows(rng, 300, d)
        ranges = ic.ranges_of(x)                       # calibrated on x itself: every value lies in its column's range
        assert (ranges[1] > ranges[0]).all()
        with np.errstate(invalid="ignore"):
            want = ic.st_quantize(x, ranges)
        got = ic.quantize_ref(x, ranges)
        assert got.dtype == np.int8 and got.shape == (300, ic.int8_bytes(d))
        t = ic.quantize_t(x, ranges)
        ok = (t > -129) & (t < 128)                    # where numpy's cast is defined (the column maximum gives t = 127 or so)
        assert ok.mean() > 0.99
        assert np.array_equal(got[:, :d][ok], want[ok])
        assert (got[:, d:] == 0).all()
        assert got[:, :d].min() == -128 and got[:, :d].max() >= 126


def test_quantize_ref_saturation_nan_and_constant_column():
    ranges = np.array([[0.0, -255.0, 2.0, 0.0], [255.0, 255.0, 2.0, 255.0]], np.float32)      # steps 1, 2, 0, 1: all exact
    x = np.array([[-1000.0, -255.0, 2.0, 127.5],      # far below; at the start; ON the constant: 0 / 0 = NaN -> 0; t = -0.5 -> 0
                  [1000.0, 255.0, 2.5, 128.5],        # far above; at the maximum; above the constant: +inf -> 127; t = 0.5 -> 0
                  [np.inf, -np.inf, 1.5, 129.0],      # +-inf saturate; below the constant: -inf -> -128; t = 1 -> 1
                  [np.nan, np.nan, np.nan, 126.0],    # NaN -> 0; t = -2 -> -2
                  [0.0, 0.0, np.inf, 255.0],          # the start: -128; the middle: t = -0.5 -> 0; +inf: 127; the maximum: 127
                  [-0.5, 1000.0, -np.inf, 256.0]], np.float32)   # t = -128.5 -> -128; t = 499.5 -> 127; -128; t = 128 -> 127
    got = ic.quantize_ref(x, ranges)[:, :4]
    want = np.array([[-128, -128, 0, 0], [127, 127, 127, 0], [127, -128, -128, 1], [0, 0, 0, -2], [-128, 0, 127, 127],
                     [-128, 127, -128, 127]], np.int8)
    assert got.tolist() == want.tolist()
    # trunc is towards zero on both sides of zero
    r = np.array([[0.0], [255.0]], np.float32)
    xs = np.array([[128.0 - 1.75], [128.0 - 0.25], [128.0 + 0.25], [128.0 + 1.75]], np.float32)
    assert ic.quantize_ref(xs, r)[:, 0].tolist() == [-1, 0, 0, 1]


def test_quantiser_rows_hold_every_kind():
    x, ranges = ic.quantiser_rows(257, 65, seed=1)
    t = ic.quantize_t(x, ranges)
    assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
    assert (x < ranges[0]).any() and (x > ranges[1]).any() and (x == ranges[0]).any() and (x == ranges[1]).any()
    assert ranges[0, 2] == ranges[1, 2] and np.isnan(t[:, 2]).any() and np.isinf(t[:, 2]).any()
    fin = t[np.isfinite(t)]
    assert (fin == np.round(fin)).sum() > 100          # t exactly on integers
    c = ic.quantize_ref(x, ranges)
    assert c[:, :65].min() == -128 and c[:, :65].max() == 127 and (c[:, 65:] == 0).all()


def test_ip_and_rescore_restatement_against_a_loop():
    rng = np.random.default_rng(13)
    d, Q, N = 13, 7, 23
    qc, cc = ic.uniform_codes(rng, Q, d), ic.ternary_codes(rng, N, d)
    cc[3], cc[17] = cc[5], cc[5]                                  # ties
    assert qc.shape == (Q, 16) and cc.shape == (N, 16)
    loop = [[sum(int(qc[i, j]) * int(cc[r, j]) for j in range(d)) for r in range(N)] for i in range(Q)]
    assert ic.ip_ref(qc, cc, d).tolist() == loop
    junk = cc.copy()
    junk[:, d:] = 0x5A
    assert (ic.ip_ref(qc, junk, d) == ic.ip_ref(qc, cc, d)).all()
    for k in (1, 5, 23, 30):
        os_, oi = ic.ip_topk_ref(qc, cc, d, k, idx_offset=100)
        for i in range(Q):
            ranked = sorted(range(N), key=lambda r: (-loop[i][r], r))[:k]
            pad = k - len(ranked)
            assert os_[i].tolist() == [loop[i][r] for r in ranked] + [ic.INT32_MIN] * pad
            assert oi[i].tolist() == [r + 100 for r in ranked] + [-1] * pad
    q = ic.random_rows(rng, Q, d)
    cand = np.stack([rng.permutation(N)[:9] for _ in range(Q)]).astype(np.int64)
    cand[:, 2] = -1
    cand[1, 4] = N
    cand[2, 5] = cand[2, 0]                                       # a row listed twice
    cand[3, :2] = (17, 3)                                         # two equal code rows: the lower row first
    s, ix, st = ic.rescore_ref(q, cc, d, cand, 4)
    assert st.tolist() == [0, 1, 0, 0, 0, 0, 0]
    for i in range(Q):
        ent = []
        for r in cand[i]:
            if 0 <= r < N:
                v = [float(q[i, j]) * float(cc[r, j]) for j in range(d)] + [0.0] * (64 - d)    # d < 64: one element a lane
                for o in (32, 16, 8, 4, 2, 1):
                    v = [v[l] + v[l ^ o] for l in range(64)]
                ent.append((-float(np.float32(v[0])), int(r)))
        ent.sort()
        assert ix[i].tolist() == [r for _, r in ent[:4]] + [-1] * max(0, 4 - len(ent))
        assert s[i, :min(4, len(ent))].tolist() == [-x for x, _ in ent[:4]]
    _, ix9, _ = ic.rescore_ref(q, cc, d, cand, 9)
    assert ix9[2].tolist().count(int(cand[2, 0])) == 2 and ix9[2, 8] == -1


# ------------------------------------------------------------------------------------------------- the C ABI, no launch
def test_header_symbols_exported_and_bound(L):
    hdr = open(os.path.join(REPO, "include", "tsim.h")).read()
    for name in NEW:
        assert f"{name}(" in hdr, name
        assert name in _lib.DECLARED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name


def test_int8_bytes(L):
    ds = (0, 1, 16, 17, 1024, 1025)
    want = [0, 16, 16, 32, 1024, 0]
    assert [L.tsim_int8_bytes(d) for d in ds] == want
    assert [ic.int8_bytes(d) for d in ds] == want
    assert L.tsim_int8_bytes(-5) == 0


def test_workspace_function(L):
    ws = L.tsim_int8_ip_topk_workspace_bytes
    for Q, N, k in ((4, 100, 0), (4, 100, 1025), (0, 100, 10), (-1, 100, 10), (4, -1, 10), (4, 100, -2)):
        assert ws(Q, N, k) == 0, (Q, N, k)
    Qs = (1, 2, 15, 16, 17, 64, 100, 256, 4096, 16384)
    Ns = (0, 1, 1023, 1024, 1025, 5000, 70_000, 1_000_000, 16_000_000, 2_000_000_000)
    ks = (1, 10, 64, 65, 100, 1024)
    grid = np.array([[[ws(Q, N, k) for k in ks] for N in Ns] for Q in Qs], dtype=np.int64)
    assert (grid > 0).all()
    assert (np.diff(grid, axis=0) >= 0).all() and (np.diff(grid, axis=1) >= 0).all() and (np.diff(grid, axis=2) >= 0).all()
    for qi, Q in enumerate(Qs):
        for ki, k in enumerate(ks):
            assert grid[qi, :, ki].max() <= max(64 << 20, Q * k * 8) + 512, (Q, k)


def _einval(L, rc, *words):
    assert rc == 1, rc
    msg = L.tsim_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)


def test_quantize_argument_errors(L):
    p = 1 << 20    # a fake, never dereferenced, 16-byte aligned device pointer
    call = L.tsim_quantize_int8_rows
    for args in ((None, 4, 384, 384, p, p, 384, None), (p, 4, 384, 384, None, p, 384, None), (p, 4, 384, 384, p, None, 384, None)):
        _einval(L, call(*args), "quantize_int8_rows", "null pointer")
    _einval(L, call(p, 4, 1025, 1025, p, p, 1040, None), "quantize_int8_rows", "d=1025")
    _einval(L, call(p, 4, 0, 8, p, p, 16, None), "quantize_int8_rows", "d=0")
    _einval(L, call(p, 4, 384, 383, p, p, 384, None), "quantize_int8_rows", "ld_in")
    _einval(L, call(p, 4, 384, 384, p, p, 392, None), "quantize_int8_rows", "ld_code", "multiple of 16")
    _einval(L, call(p, 4, 385, 385, p, p, 384, None), "quantize_int8_rows", "ld_code", "tsim_int8_bytes")
    _einval(L, call(p, 4, 384, 384, p, p + 8, 384, None), "quantize_int8_rows", "16-byte boundary")


def test_int8_ip_topk_argument_errors(L):
    p = 1 << 20
    ws = L.tsim_int8_ip_topk_workspace_bytes(4, 1000, 10)
    base = dict(q=p, ldq=384, Q=4, c=p, ldc=384, N=1000, d=384, k=10, os=p, oi=p, ws=p, wsb=ws)

    def call(**kw):
        a = {**base, **kw}
        return L.tsim_int8_ip_topk(a["q"], a["ldq"], a["Q"], a["c"], a["ldc"], a["N"], a["d"], a["k"], a["os"], a["oi"], 0, a["ws"],
                                   a["wsb"], None)

    for kw in ({"q": None}, {"c": None}, {"os": None}, {"oi": None}):
        _einval(L, call(**kw), "int8_ip_topk", "null pointer")
    _einval(L, call(ldq=392), "int8_ip_topk", "ldq", "multiple of 16")
    _einval(L, call(ldc=392), "int8_ip_topk", "ldc", "multiple of 16")
    _einval(L, call(ldq=368), "int8_ip_topk", "ldq", "tsim_int8_bytes")
    _einval(L, call(ldc=368), "int8_ip_topk", "ldc", "tsim_int8_bytes")
    _einval(L, call(q=p + 4), "int8_ip_topk", "ldq", "16-byte boundary")
    _einval(L, call(c=p + 8), "int8_ip_topk", "ldc", "16-byte boundary")
    _einval(L, call(d=1025, ldq=1040, ldc=1040), "int8_ip_topk", "d=1025")
    _einval(L, call(d=0), "int8_ip_topk", "d=0")
    _einval(L, call(k=0), "int8_ip_topk", "k=0")
    _einval(L, call(k=1025), "int8_ip_topk", "k=1025")
    _einval(L, call(Q=0), "int8_ip_topk", "Q=0")
    _einval(L, call(N=(1 << 31) - 64), "int8_ip_topk", "32-bit")
    assert call(wsb=ws - 1) == 3 and call(ws=None) == 3      # TSIM_ENOMEM: the workspace


def test_int8_rescore_argument_errors(L):
    p = 1 << 20
    base = dict(q=p, ldq=384, Q=4, c=p, ldc=384, N=1000, d=384, cand=p, m=100, k=10, os=p, oi=p)

    def call(**kw):
        a = {**base, **kw}
        return L.tsim_int8_rescore_topk(a["q"], a["ldq"], a["Q"], a["c"], a["ldc"], a["N"], a["d"], a["cand"], a["m"], a["k"], a["os"],
                                        a["oi"], 0, None, None)

    for kw in ({"q": None}, {"c": None}, {"cand": None}, {"os": None}, {"oi": None}):
        _einval(L, call(**kw), "int8_rescore_topk", "null pointer")
    _einval(L, call(ldc=392), "int8_rescore_topk", "ldc", "multiple of 16")
    _einval(L, call(ldc=368), "int8_rescore_topk", "ldc", "tsim_int8_bytes")
    _einval(L, call(c=p + 8), "int8_rescore_topk", "16-byte boundary")
    _einval(L, call(ldq=383), "int8_rescore_topk", "ldq_f32")
    _einval(L, call(d=1025, ldq=1025, ldc=1040), "int8_rescore_topk", "d=1025")
    _einval(L, call(k=0), "int8_rescore_topk", "k=0")
    _einval(L, call(k=1025), "int8_rescore_topk", "k=1025")
    _einval(L, call(m=-1), "int8_rescore_topk", "m=-1")


# ------------------------------------------------------------------------------------------------- Python surface, no device
def test_ops_refuse_cpu_tensors_and_bad_widths(L):
    import torch
    from text_similarity_amd import ops
    assert ops.int8_bytes(384) == 384 and ops.int8_bytes(385) == 400
    for d in (0, 1025):
        with pytest.raises(ValueError):
            ops.int8_bytes(d)
    c4, c9 = torch.zeros(4, 384, dtype=torch.int8), torch.zeros(9, 384, dtype=torch.int8)
    with pytest.raises(_lib.TsimError):
        ops.int8_ranges(torch.zeros(4, 384))
    with pytest.raises(_lib.TsimError):
        ops.quantize_int8_rows(torch.zeros(4, 384), torch.zeros(2, 384))
    with pytest.raises(_lib.TsimError):
        ops.int8_ip_topk(c4, c9, 384, 2)
    with pytest.raises(_lib.TsimError):
        ops.int8_rescore_topk(torch.zeros(4, 384), c9, 384, torch.zeros(4, 3, dtype=torch.int64), 2)
    with pytest.raises(_lib.TsimError):
        ops.int8_codes_from_numpy(c4, 384)                                   # a CPU tensor (numpy arrays are moved, tensors not)
    with pytest.raises(ValueError):
        ops.int8_codes_from_numpy(np.zeros((4, 384), np.uint8), 384)         # wrong dtype
    with pytest.raises(ValueError):
        ops.int8_codes_from_numpy(np.zeros((4, 384), np.int8), 1025)         # wrong width


def test_index_file_round_trip(tmp_path):
    from text_similarity_amd import int8_index
    rng = np.random.default_rng(2)
    d = 37
    codes = rng.integers(-128, 128, size=(50, d)).astype(np.int8)
    labels = rng.permutation(1000)[:50].astype(np.int64)
    ranges = ic.ranges_of(ic.random_rows(rng, 20, d))
    path = str(tmp_path / "i8.npz")
    int8_index.pack_index_file(path, codes, labels, d, ranges)
    z = np.load(path, allow_pickle=False)                                     # plain arrays: loads without pickling
    assert sorted(z.files) == ["dim", "int8_codes", "labels", "ranges"] and int(z["dim"]) == d
    assert z["int8_codes"].dtype == np.int8 and z["int8_codes"].shape == (50, d)
    c2, l2, r2 = int8_index.unpack_index_file(path, d)
    assert np.array_equal(c2, codes) and np.array_equal(l2, labels) and np.array_equal(r2, ranges) and r2.dtype == np.float32
    int8_index.pack_index_file(path, codes[:0], labels[:0], d, None)          # empty and uncalibrated
    c2, l2, r2 = int8_index.unpack_index_file(path, d)
    assert c2.shape == (0, d) and l2.shape == (0,) and r2 is None
    with pytest.raises(ValueError):
        int8_index.unpack_index_file(path, d + 1)
    with pytest.raises(ValueError):
        int8_index.pack_index_file(path, codes, labels[:3], d, ranges)
    np.savez(open(path, "wb"), codes=np.zeros((1, 5), np.uint8), labels=np.zeros(1, np.int64), dim=np.int64(d))
    with pytest.raises(ValueError):
        int8_index.unpack_index_file(path, d)                                  # a binary index's file
