"""The refine stage on the host: the C ABI of tsim_list_topk_f16 (symbol, argument checks before any launch), the float16
rounding table, and the theorems that tie the two-stage restatement (tests/refine_cases.py) to the one-stage ones — they hold
for any data, because both stages rank by a total order, and the GPU tests check the indexes against the same restatement."""
import os

import numpy as np
import pytest

import ivfpq_cases as ic
import pq_cases as pc
import refine_cases as rc
from list_cases import HDR, header_define, list_topk_ref, same_bits
from text_similarity_amd import _lib

SPACE_ID = {"cosine": 0, "dot": 1, "l2": 2}
MULTS = (1, 2, 4, 8, 16, 32, 64, 128)
EINVAL, ENOMEM = header_define("TSIM_EINVAL"), header_define("TSIM_ENOMEM")


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtsim.so is not built")
    return _lib.lib()


def test_symbol_in_header_exported_and_bound():
    assert "tsim_list_topk_f16(" in open(HDR).read()
    assert "tsim_list_topk_f16" in _lib.DECLARED_SYMBOLS
    L = _lib_or_skip()
    assert len(L.tsim_list_topk_f16.argtypes) == 21
    assert (_lib.SPACE_COSINE, _lib.SPACE_DOT, _lib.SPACE_L2) == (0, 1, 2)


@pytest.mark.parametrize("space", ("cosine", "dot", "l2"))
def test_argument_errors_before_any_launch(space):
    """Fake (never dereferenced) device pointers: every refusal comes back before a launch, with the entry's name."""
    L = _lib_or_skip()
    p = 1 << 20
    ws = L.tsim_list_topk_workspace_bytes(4, 100, 10)
    base = dict(space=SPACE_ID[space], eq=p, ldq=384, Q=4, ec=p, ldc=384, N=1000, d=384, cand=p, dt=_lib.TSIM_I64, T=100, lims=p,
                shared=0, k=10, out_s=p, out_i=p, ws=p, wsb=ws)

    def call(**kw):
        a = {**base, **kw}
        return L.tsim_list_topk_f16(a["space"], a["eq"], a["ldq"], a["Q"], a["ec"], a["ldc"], a["N"], a["d"], a["cand"], a["dt"], a["T"],
                                    a["lims"], a["shared"], a["k"], a["out_s"], a["out_i"], 0, None, a["ws"], a["wsb"], None)

    bad = [{"eq": None}, {"ec": None}, {"cand": None}, {"out_s": None}, {"out_i": None},      # null pointers
           {"Q": 0}, {"Q": -1}, {"Q": 1 << 31}, {"N": 0}, {"N": 1 << 31}, {"T": -1}, {"T": 1 << 40},   # shapes out of range
           {"k": 0}, {"k": 1025},                                                             # k outside 1..1024
           {"d": 0}, {"d": 769, "ldq": 769, "ldc": 769},                                      # d outside 1..768
           {"ldq": 383}, {"ldc": 383},                                                        # strides below d
           {"lims": None, "shared": 0}, {"lims": p, "shared": 1},                             # neither, both
           {"dt": 0}, {"dt": 7},                                                              # unknown index dtype
           {"space": 3}, {"space": -1}]                                                       # unknown space
    if space == "l2":
        bad.append({"d": 768, "ldq": 768, "ldc": 768})
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert b"list_topk_f16" in L.tsim_last_error(), (kw, L.tsim_last_error())
    for kw in ({"wsb": ws - 1}, {"ws": None}, {"wsb": 0}):                                    # a short workspace
        assert call(**kw) == ENOMEM, kw
    if space != "l2":                                                                         # 768 is legal there: only the
        assert call(d=768, ldq=768, ldc=768, ws=None) == ENOMEM                     # workspace is refused


def test_to_f16_at_the_rounding_boundaries():
    vals = np.array([v for v, _ in rc.F16_TABLE], dtype=np.float32)
    assert (vals.astype(np.float64) == np.array([v for v, _ in rc.F16_TABLE])).all()          # the table's values ARE float32
    want = np.array([b for _, b in rc.F16_TABLE], dtype=np.uint16)
    got = rc.to_f16(vals).view(np.uint16)
    assert (got == want).all(), [(hex(a), hex(b)) for a, b in zip(got, want) if a != b]
    assert np.isinf(rc.to_f16(np.float32(65520.0))) and np.isfinite(rc.to_f16(np.float32(65504.0)))
    sub = rc.to_f16(np.float32(2.0 ** -24))
    assert sub.astype(np.float32) == np.float32(2.0 ** -24)                                   # widening is exact


def _two_stage(kind, space, refine):
    """(search(mult) -> (scores, rows, cand), exact top-k ids, full (scores, rows) over every row)"""
    cent, cb, x, q = rc.small_data()
    xs, qs = (rc.normalise_np(x), rc.normalise_np(q)) if space == "cosine" else (x, q)
    store = rc.store_rows(x, refine)
    if kind == "pq":
        codes = pc.encode_ref(xs, cb)
        run = lambda mult: rc.pq_refined_ref(space, q, qs, cb, codes, store, rc.K, mult)
    else:
        lists = rc.nearest_lists_np(space, xs, cent, 1)[:, 0]
        probes = rc.nearest_lists_np(space, qs, cent, rc.NLIST)
        codes = ic.encode_ref(xs, cent, lists, cb)
        run = lambda mult: rc.ivfpq_refined_ref(space, q, qs, cent, cb, codes, lists, probes, store, rc.K, mult)
    fs, fi, _ = list_topk_ref(rc.LIST_SPACE[space], q, store.astype(np.float32), np.arange(rc.N_ROWS), rc.K)
    return run, fs, fi, (xs, qs, cb, codes)


@pytest.mark.parametrize("refine", ("float32", "float16"))
@pytest.mark.parametrize("space", ("ip", "l2", "cosine"))
@pytest.mark.parametrize("kind", ("pq", "ivfpq"))
def test_restatement_theorems(kind, space, refine):
    run, fs, fi, (xs, qs, cb, codes) = _two_stage(kind, space, refine)
    out = {m: run(m) for m in MULTS}
    Q = fi.shape[0]
    # 1. the candidate sets are nested (a first stage of width m' >= m begins with the one of width m)
    for a, b in zip(MULTS, MULTS[1:]):
        ca, cb_ = out[a][2], out[b][2]
        assert (cb_[:, :ca.shape[1]] == ca).all(), (a, b)
    # 2. at multiplier 1 the refined ids are the ADC ids as a set
    for j in range(Q):
        assert sorted(out[1][1][j].tolist()) == sorted(out[1][2][j].tolist())
    if kind == "pq":
        _, adc_i = rc.pq_adc_ref(space, qs, cb, codes, rc.K)
        assert (adc_i == out[1][2]).all()
    # 3. the refined top-k keeps exactly the exact top-k rows that were candidates; their number never falls
    hits = []
    for m in MULTS:
        s, i, cand = out[m]
        per_q = [len(set(i[j].tolist()) & set(fi[j].tolist())) for j in range(Q)]
        assert per_q == [len(set(cand[j][cand[j] >= 0].tolist()) & set(fi[j].tolist())) for j in range(Q)], m
        hits.append(per_q)
    assert all((np.array(a) <= np.array(b)).all() for a, b in zip(hits, hits[1:]))
    # ... strictly somewhere on this seed: below 1 at multiplier 1, 1 at the largest (else the GPU twin shows nothing)
    assert rc.recall(out[1][1], fi) < 1.0 and rc.recall(out[MULTS[-1]][1], fi) == 1.0, (rc.recall(out[1][1], fi),)
    # 4. once every row is a candidate the refined result is the exact search, bit for bit
    assert rc.first_stage_width(rc.K, 128, rc.N_ROWS) == rc.N_ROWS
    s, i, cand = out[128]
    assert (np.sort(cand, axis=1) == np.arange(rc.N_ROWS)).all()
    assert same_bits(s, fs) and (i == fi).all()


def test_refine_ref_drops_padding_and_keeps_the_order():
    cent, cb, x, q = rc.small_data()
    cand = np.array([[5, -1, 7, 9, -1]] * q.shape[0])
    s, i = rc.refine_ref("l2", q, x, cand, 4)
    assert (np.sort(i[:, :3], axis=1) == [5, 7, 9]).all() and (i[:, 3] == -1).all() and np.isposinf(s[:, 3]).all()
    assert (np.diff(s[:, :3], axis=1) >= 0).all()
    s16, i16 = rc.refine_ref("l2", q, rc.to_f16(x), cand, 4)
    w, wi, _ = list_topk_ref("l2", q, rc.to_f16(x).astype(np.float32), [[5, 7, 9]] * q.shape[0], 4)
    assert same_bits(s16, w) and (i16 == wi).all()
