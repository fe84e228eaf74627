"""Binary embeddings on the host: the C ABI (symbols, tsim_code_bytes, the workspace function, argument checks before any launch)
and the numpy restatement of tests/hamming_cases.py against a plain Python double loop."""
import os

import numpy as np
import pytest

import hamming_cases as hc
from text_similarity_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tsim_code_bytes", "tsim_pack_sign_rows", "tsim_hamming_topk_workspace_bytes", "tsim_hamming_topk", "tsim_sign_rescore_topk")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        from text_similarity_amd.build import build
        build(verbose=False)
    return _lib.lib()


def test_header_symbols_exported_and_bound(L):
    hdr = open(os.path.join(REPO, "include", "tsim.h")).read()
    for name in NEW:
        assert f"{name}(" in hdr, name
        assert name in _lib.DECLARED_SYMBOLS, name
        assert getattr(L, name).argtypes is not None, name
    assert L.tsim_version() == 104


def test_code_bytes(L):
    ds = (0, 1, 8, 121, 128, 129, 384, 1024, 1025)
    want = [0, 16, 16, 16, 16, 32, 48, 128, 0]
    assert [L.tsim_code_bytes(d) for d in ds] == want
    assert [hc.code_bytes(d) for d in ds] == want
    assert L.tsim_code_bytes(-5) == 0


def test_workspace_function(L):
    ws = L.tsim_hamming_topk_workspace_bytes
    for Q, N, k in ((0, 100, 10), (-1, 100, 10), (4, -1, 10), (4, 100, 0), (4, 100, 1025), (4, 100, -2)):
        assert ws(Q, N, k) == 0, (Q, N, k)
    Qs = (1, 2, 7, 8, 9, 16, 100, 256, 1000, 4096, 16384)
    Ns = (0, 1, 1023, 1024, 1025, 5000, 70_000, 1_000_000, 16_000_000, 2_000_000_000)
    ks = (1, 10, 64, 65, 100, 1024)
    grid = np.array([[[ws(Q, N, k) for k in ks] for N in Ns] for Q in Qs], dtype=np.int64)
    assert (grid > 0).all()
    assert (np.diff(grid, axis=0) >= 0).all() and (np.diff(grid, axis=1) >= 0).all() and (np.diff(grid, axis=2) >= 0).all()
    # the chunk lists stay within a fixed budget unless one list per query already exceeds it
    for qi, Q in enumerate(Qs):
        for ki, k in enumerate(ks):
            assert grid[qi, :, ki].max() <= max(64 << 20, Q * k * 8) + 512, (Q, k)


def _einval(L, rc, *words):
    assert rc == 1, rc
    msg = L.tsim_last_error().decode()
    for w in words:
        assert w in msg, (w, msg)


def test_pack_argument_errors(L):
    p = 1 << 20    # a fake, never dereferenced, 16-byte aligned device pointer
    call = L.tsim_pack_sign_rows
    _einval(L, call(None, 0, 4, 384, 384, p, 48, None), "pack_sign_rows", "null pointer")
    _einval(L, call(p, 0, 4, 384, 384, None, 48, None), "pack_sign_rows", "null pointer")
    _einval(L, call(p, 0, 4, 384, 384, p, 56, None), "pack_sign_rows", "ld_code", "multiple of 16")
    _einval(L, call(p, 0, 4, 384, 384, p, 32, None), "pack_sign_rows", "ld_code", "tsim_code_bytes")
    _einval(L, call(p, 0, 4, 1025, 1025, p, 144, None), "pack_sign_rows", "d=1025")
    _einval(L, call(p, 0, 4, 0, 8, p, 16, None), "pack_sign_rows", "d=0")
    _einval(L, call(p, 0, 4, 384, 383, p, 48, None), "pack_sign_rows", "ld_in")
    _einval(L, call(p, 7, 4, 384, 384, p, 48, None), "pack_sign_rows", "x_dtype")


def test_hamming_topk_argument_errors(L):
    p = 1 << 20
    ws = L.tsim_hamming_topk_workspace_bytes(4, 1000, 10)
    base = dict(q=p, ldq=48, Q=4, c=p, ldc=48, N=1000, d=384, k=10, od=p, oi=p, ws=p, wsb=ws)

    def call(**kw):
        a = {**base, **kw}
        return L.tsim_hamming_topk(a["q"], a["ldq"], a["Q"], a["c"], a["ldc"], a["N"], a["d"], a["k"], a["od"], a["oi"], 0, a["ws"],
                                   a["wsb"], None)

    for kw in ({"q": None}, {"c": None}, {"od": None}, {"oi": None}):
        _einval(L, call(**kw), "hamming_topk", "null pointer")
    _einval(L, call(ldq=56), "hamming_topk", "ldq", "multiple of 16")
    _einval(L, call(ldc=40), "hamming_topk", "ldc", "multiple of 16")
    _einval(L, call(ldq=32), "hamming_topk", "ldq", "tsim_code_bytes")
    _einval(L, call(ldc=32), "hamming_topk", "ldc", "tsim_code_bytes")
    _einval(L, call(d=1025, ldq=144, ldc=144), "hamming_topk", "d=1025")
    _einval(L, call(k=0), "hamming_topk", "k=0")
    _einval(L, call(k=1025), "hamming_topk", "k=1025")
    _einval(L, call(Q=0), "hamming_topk", "Q=0")
    _einval(L, call(N=(1 << 31) - 64), "hamming_topk", "32-bit")
    assert call(wsb=ws - 1) == 3 and call(ws=None) == 3      # TSIM_ENOMEM: the workspace


def test_sign_rescore_argument_errors(L):
    p = 1 << 20
    base = dict(q=p, ldq=384, Q=4, c=p, ldc=48, N=1000, d=384, cand=p, m=100, k=10, os=p, oi=p)

    def call(**kw):
        a = {**base, **kw}
        return L.tsim_sign_rescore_topk(a["q"], a["ldq"], a["Q"], a["c"], a["ldc"], a["N"], a["d"], a["cand"], a["m"], a["k"], a["os"],
                                        a["oi"], 0, None, None)

    for kw in ({"q": None}, {"c": None}, {"cand": None}, {"os": None}, {"oi": None}):
        _einval(L, call(**kw), "sign_rescore_topk", "null pointer")
    _einval(L, call(ldc=56), "sign_rescore_topk", "ldc", "multiple of 16")
    _einval(L, call(ldc=32), "sign_rescore_topk", "ldc", "tsim_code_bytes")
    _einval(L, call(ldq=383), "sign_rescore_topk", "ldq_f32")
    _einval(L, call(d=1025, ldq=1025, ldc=144), "sign_rescore_topk", "d=1025")
    _einval(L, call(k=0), "sign_rescore_topk", "k=0")
    _einval(L, call(k=1025), "sign_rescore_topk", "k=1025")
    _einval(L, call(m=-1), "sign_rescore_topk", "m=-1")


def test_ops_refuse_cpu_tensors_and_bad_widths(L):
    import torch
    from text_similarity_amd import ops
    assert ops.code_bytes(384) == 48
    for d in (0, 1025):
        with pytest.raises(ValueError):
            ops.code_bytes(d)
    with pytest.raises(_lib.TsimError):
        ops.pack_sign_rows(torch.zeros(4, 384))
    with pytest.raises(_lib.TsimError):
        ops.hamming_topk(torch.zeros(4, 48, dtype=torch.uint8), torch.zeros(9, 48, dtype=torch.uint8), 384, 2)


def test_restatement_against_a_double_loop():
    """7 queries x 23 rows at d = 13: packing, distances, the (dist, row) top-k with padding, and the re-score."""
    rng = np.random.default_rng(13)
    d, Q, N = 13, 7, 23
    q, c = hc.random_rows(rng, Q, d), hc.random_rows(rng, N, d)
    c[3], c[17] = c[5], c[5]                                     # ties
    c[0, :4] = (0.0, -0.0, np.nan, -np.inf)
    qc, cc = hc.pack_ref(q), hc.pack_ref(c)
    assert qc.shape == (Q, 16) and cc.shape == (N, 16)
    for codes, x in ((qc, q), (cc, c)):
        for r in range(x.shape[0]):
            want = [0] * 16
            for j in range(d):
                if x[r, j] > 0:
                    want[j // 8] |= 0x80 >> (j % 8)
            assert codes[r].tolist() == want
    dist = hc.hamming_ref(qc, cc, d)
    loop = [[sum((float(q[i, j]) > 0) != (float(c[r, j]) > 0) for j in range(d)) for r in range(N)] for i in range(Q)]
    assert dist.tolist() == loop
    junk = cc.copy()
    junk[:, 1] |= 0x07                                           # bits 13..15: beyond d
    junk[:, 2:] = 0xA5
    assert (hc.hamming_ref(qc, junk, d) == dist).all()
    for k in (1, 5, 23, 30):
        od, oi = hc.hamming_topk_ref(qc, cc, d, k, idx_offset=100)
        for i in range(Q):
            ranked = sorted(range(N), key=lambda r: (loop[i][r], r))[:k]
            pad = k - len(ranked)
            assert od[i].tolist() == [loop[i][r] for r in ranked] + [hc.INT32_MAX] * pad
            assert oi[i].tolist() == [r + 100 for r in ranked] + [-1] * pad
    cand = np.stack([rng.permutation(N)[:9] for _ in range(Q)]).astype(np.int64)
    cand[:, 2] = -1
    cand[1, 4] = N
    cand[2, 5] = cand[2, 0]                                      # a row listed twice
    cand[3, :2] = (3, 17)                                        # two equal code rows
    s, ix, st = hc.rescore_ref(q, cc, d, cand, 4)
    assert st.tolist() == [0, 1, 0, 0, 0, 0, 0]
    for i in range(Q):
        ent = []
        for r in cand[i]:
            if 0 <= r < N:
                # d < 64: one element a lane, the butterfly adds 13 values and zeros — any float64 order of +-q_j that follows
                # the butterfly's tree; here the tree of 16 lanes is restated directly
                v = [float(q[i, j]) if c[r, j] > 0 else -float(q[i, j]) for j in range(d)] + [0.0] * (64 - d)
                for o in (32, 16, 8, 4, 2, 1):
                    v = [v[l] + v[l ^ o] for l in range(64)]
                ent.append((-float(np.float32(v[0])), int(r)))
        ent.sort()
        assert ix[i].tolist() == [r for _, r in ent[:4]] + [-1] * max(0, 4 - len(ent))
        assert s[i, :min(4, len(ent))].tolist() == [-x for x, _ in ent[:4]]
    _, ix9, _ = hc.rescore_ref(q, cc, d, cand, 9)
    assert ix9[2].tolist().count(int(cand[2, 0])) == 2 and ix9[2, 8] == -1           # listed twice: returned twice; 8 usable entries
