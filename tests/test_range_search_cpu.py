"""Host side of the exact range search (include/tsim.h tsim_cosine_range_scan / tsim_dot_range_scan / tsim_range_fill): symbols,
workspace sizes, the argument checks that run before any launch, and a CPU replay of the guard: on adversarial data every hit
of the oracle has a model MFMA score strictly above the collect threshold that ops.range_collect_threshold (the host mirror of
the set-up kernel) computes — the executable statement of the proof in the header."""
import os
import re

import numpy as np
import pytest

from oracle.search_ref import _lane_sum, exact_cosine, mfma_model_scores, rho_rows, unit_rows
from text_similarity_amd import _lib, ops

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tsim.h")
NEW = ("tsim_range_workspace_bytes", "tsim_cosine_range_scan", "tsim_dot_range_scan", "tsim_range_fill")


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtsim.so is not built")
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------- test-local oracle
def range_ref(scores_f32, tau):
    """per query the indices with score >= float32(tau), ordered (score desc, index asc)"""
    tau = np.float32(tau)
    out = []
    for s in np.asarray(scores_f32, dtype=np.float32):
        hit = np.nonzero(s >= tau)[0]
        out.append(hit[np.lexsort((hit, -s[hit].astype(np.float64)))])
    return out


def dot_scores(q, c):
    return _lane_sum(np.asarray(q, np.float32)[:, None, :], np.asarray(c, np.float32)[None, :, :]).astype(np.float32)


def _gauss(rng, n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


def _rho_up(r):
    """csrc/common.h rho_round_up"""
    return np.minimum(np.float32(np.asarray(r, np.float64) * (1.0 + 1e-6)), np.float32(2.0))


# ---------------------------------------------------------------------------------------------------------- symbols, sizes
def test_symbols_declared_bound_and_exported():
    hdr = open(HDR).read()
    m = re.search(r"#define TSIM_RANGE_SLOT_CAP (\d+)", hdr)
    assert m, "TSIM_RANGE_SLOT_CAP is not defined"
    cap = int(m.group(1))
    assert cap >= 1024 and cap & (cap - 1) == 0
    assert ops.RANGE_SLOT_CAP == cap
    for name in NEW:
        assert f"{name}(" in hdr, name
        assert name in _lib.DECLARED_SYMBOLS, name
    L = _lib_or_skip()
    assert L.tsim_version() == 104
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name
    assert callable(ops.cosine_range) and callable(ops.dot_range)


def test_workspace_bytes():
    L = _lib_or_skip()
    N = 1_000_000
    assert L.tsim_range_workspace_bytes(0, N) == 0
    assert L.tsim_range_workspace_bytes(-1, N) == 0
    assert L.tsim_range_workspace_bytes(256, 0) == 0
    w1, w256, w4096 = (L.tsim_range_workspace_bytes(q, N) for q in (1, 256, 4096))
    assert 0 < w1 < w256 < w4096
    assert w256 >= 256 * ops.RANGE_SLOT_CAP * 8
    # at most linear in Q (per-array 256-byte alignment aside)
    assert w4096 <= 16 * w256 + 16 * 4096
    assert w4096 < (1 << 28)
    assert L.tsim_range_workspace_bytes(256, 7) <= w256


def _scan_args(p, tau, ws, dot, f32=True, words=True):
    f = p if f32 else None
    head = (p, f, 384, 4, p, f, 384)
    tail = (100, 384, 384, tau, p, None, p, ws, None)
    if dot:
        return head + ((p, p) if words else (None, None)) + tail
    return head + (p,) + tail


@pytest.mark.parametrize("dot", [False, True])
def test_argument_checks_before_any_launch(dot):
    """Fake (never dereferenced) 16-byte aligned device pointers: every refusal happens on the host."""
    L = _lib_or_skip()
    fn = L.tsim_dot_range_scan if dot else L.tsim_cosine_range_scan
    p = 1 << 20
    big = 1 << 40
    need = L.tsim_range_workspace_bytes(4, 100)
    assert need > 0
    assert fn(*_scan_args(p, float("nan"), big, dot)) == 1            # TSIM_EINVAL: NaN threshold
    assert b"NaN" in L.tsim_last_error()
    assert fn(*_scan_args(p, 0.5, big, dot, f32=False)) == 1          # the float32 matrices are required
    assert b"float32" in L.tsim_last_error()
    if dot:
        assert fn(*_scan_args(p, 0.5, big, dot, words=False)) == 1    # ec_maxnorm / ec_rho_max are required
        assert b"max-norm" in L.tsim_last_error()
    assert fn(*_scan_args(p, 0.5, need - 1, dot)) == 3                # TSIM_ENOMEM: short workspace
    # the fill: NaN, unknown space, missing matrices, short workspace
    fill = L.tsim_range_fill
    ok = (p, 384, 4, p, 384, 100, 384)
    assert fill(0, *ok, float("nan"), p, p, p, 0, p, big, None) == 1
    assert fill(7, *ok, 0.5, p, p, p, 0, p, big, None) == 1
    assert fill(0, None, 384, 4, None, 384, 100, 384, 0.5, p, p, p, 0, p, big, None) == 1
    assert fill(1, *ok, 0.5, p, p, p, 0, p, need - 1, None) == 3


def test_collect_threshold_mirror_basics():
    thr, eps = ops.range_collect_threshold(0.8, 2e-4, 2.5e-4, 384)
    assert 4e-4 < eps < 6e-4
    assert thr is not None and float(thr) + float(eps) < 0.8 and 0.8 - float(eps) - float(thr) < 3e-7
    assert ops.range_collect_threshold(float("-inf"), 2e-4, 2.5e-4, 384)[0] is None
    assert ops.range_collect_threshold(0.5, 2e-4, 2.0, 384)[0] is not None          # rho 2 (a NaN row): a low, finite threshold
    assert ops.range_collect_threshold(0.0, 2e-4, 2.5e-4, 384, nqs=float("inf"))[0] is None
    # a zero query (nq = 1e-8) in the dot domain: tau > 0 puts the threshold far above every score, tau < 0 below the float range
    assert float(ops.range_collect_threshold(0.5, 0.0, 2.5e-4, 384, nqs=1e-8 * 4.0)[0]) > 1e6
    assert ops.range_collect_threshold(-1e31, 0.0, 2.5e-4, 384, nqs=1e-8)[0] is None


# ---------------------------------------------------------------------------------------------------------- guard replay
def _assert_hits_above(model, exact, taus_per_query, thr_of):
    """every hit of range_ref has a model score strictly above the query's collect threshold; returns (hits, extras)"""
    nhit = nextra = 0
    for qi in range(exact.shape[0]):
        for tau in taus_per_query(qi):
            thr = thr_of(qi, tau)
            hits = range_ref(exact[qi:qi + 1], tau)[0]
            if thr is None:      # no finite threshold: the kernel sends the query to the exact pass
                continue
            for m in model:
                assert (m[qi, hits] > thr).all(), (qi, float(tau), float(thr), float(m[qi, hits].min()))
                nextra += int((m[qi] > thr).sum()) - hits.size
            nhit += hits.size
    return nhit, nextra


def test_guard_replay_cosine_gaussian_and_cluster():
    rng = np.random.default_rng(11)
    d, n = 384, 3000
    c = _gauss(rng, n, d)
    base = _gauss(rng, 1, d)[0]
    c[100:140] = base + 1e-7 * _gauss(rng, 40, d)            # (b) a cluster 1e-7 apart
    c[200:260] = c[7]                                         # bit-equal duplicates
    q = np.concatenate([base[None] + 1e-3 * _gauss(rng, 4, d), c[7][None], c[120][None], _gauss(rng, 7, d)]).astype(np.float32)
    exact = exact_cosine(q, c)
    assert len(set(exact[4, 200:260].view(np.uint32).tolist())) == 1      # bit-equal rows get bit-equal exact scores
    model = [mfma_model_scores(q, c, order) for order in ("f64", "f32seq")]
    rq = _rho_up(rho_rows(q))
    rc = _rho_up(rho_rows(c).max())

    def taus(qi):
        srt = np.sort(exact[qi])[::-1]
        return [srt[5], np.float32(np.median(exact[qi, 100:140])), exact[qi, 7], np.float32(0.05)]   # on a row's score: >= has a tie

    def thr_of(qi, tau):
        thr, eps = ops.range_collect_threshold(tau, rq[qi], rc, d)
        assert 4.5e-4 < eps < 5.5e-4
        for m in model:
            assert np.abs(m[qi].astype(np.float64) - exact[qi]).max() <= eps       # the bound itself
        return thr

    nhit, nextra = _assert_hits_above(model, exact, taus, thr_of)
    assert nhit > 1000
    print(f"cosine replay: {nhit} hits above their thresholds, {nextra} non-hits collected with them (two accumulation orders)")


def _dot_operands(q, c):
    """S, half(c / S) as float64, flush-safe residuals (csrc/common.h flush_safe_err) and nq S per query"""
    nc = np.sqrt(_lane_sum(c, c)).max() * (1.0 + 1e-12)
    word = np.float32(nc)
    if float(word) < nc:
        word = np.nextafter(word, np.float32(np.inf))
    fr, e = np.frexp(float(word))
    S = 2.0 ** (e - 1 if fr == 0.5 else e)
    v = c.astype(np.float64) / S
    h = v.astype(np.float16).astype(np.float64)

    def flush_safe(hh, vv):
        e_ = hh - vv
        return np.where(np.abs(hh) < 2.0 ** -14, np.maximum(np.abs(e_), np.abs(vv)), e_)

    rc = _rho_up(np.sqrt((flush_safe(h, v) ** 2).sum(-1)).max())
    nq = np.maximum(np.sqrt(_lane_sum(q, q)), np.float64(np.float32(1e-8)))
    uq = q.astype(np.float64) / nq[:, None]
    hq = uq.astype(np.float16).astype(np.float64)
    rq = _rho_up(np.sqrt((flush_safe(hq, uq) ** 2).sum(-1)))
    return S, h, hq, rq, rc, nq * S


def _model_dot(hq, h, order, flush):
    if flush:
        hq = np.where(np.abs(hq) < 2.0 ** -14, 0.0, hq)
        h = np.where(np.abs(h) < 2.0 ** -14, 0.0, h)
    if order == "f64":
        return (hq @ h.T).astype(np.float32)
    acc = np.zeros((hq.shape[0], h.shape[0]), dtype=np.float32)
    for j in range(hq.shape[1]):
        acc = (acc + (hq[:, j:j + 1] * h[None, :, j]).astype(np.float32)).astype(np.float32)
    return acc


def test_guard_replay_dot_huge_row_subnormal_halves():
    """(c) the corpus of tests/test_dot_search_gpu.py case 3: one row of norm 1e6 makes S = 2^20 and every other stored half
    subnormal; the MFMA may keep or flush them, and the threshold must hold either way."""
    rng = np.random.default_rng(3)
    d, n = 384, 3000
    c = _gauss(rng, n, d) / np.sqrt(d)
    c[0] = _gauss(rng, 1, d)[0] / np.sqrt(d) * 1e6
    base = _gauss(rng, 1, d)[0] / np.sqrt(d)
    c[100:140] = base + 1e-7 * _gauss(rng, 40, d)
    q = np.concatenate([base[None] + 1e-3 * _gauss(rng, 6, d), _gauss(rng, 6, d), np.zeros((1, d))]).astype(np.float32)
    S, h, hq, rq, rc, nqs = _dot_operands(q, c)
    assert S == 2.0 ** 20
    assert (np.abs(h[1:]) < 2.0 ** -14).all() and (h[1:] != 0).any()
    exact = dot_scores(q, c)
    model = [_model_dot(hq, h, order, flush) for order in ("f64", "f32seq") for flush in (False, True)]

    def taus(qi):
        srt = np.sort(exact[qi])[::-1]
        return [srt[5], np.float32(np.median(exact[qi, 100:140])), srt[100], np.float32(1e30)]

    def thr_of(qi, tau):
        return ops.range_collect_threshold(tau, rq[qi], rc, d, nqs=nqs[qi])[0]

    nhit, nextra = _assert_hits_above(model, exact, taus, thr_of)
    assert nhit > 500
    print(f"dot replay (S = 2^20): {nhit} hits above their thresholds, {nextra} non-hits collected (2 orders x kept / flushed)")
