"""Exact Euclidean range search on the host (include/tsim.h tsim_l2_range_scan / tsim_l2_range_scan_tau / tsim_range_fill with
TSIM_SPACE_L2 / tsim_range_merge_asc): symbols, the argument checks that run before any launch, and a CPU replay of the guard on
adversarial data — every row whose float32 squared distance is <= the radius has a model MFMA score strictly above the collect
threshold the library computes (tsim_l2_guard_host), and no row farther than the band the guard's inequality allows is above it."""
import ctypes
import os

import numpy as np
import pytest

from l2_cases import aug_corpus, aug_queries, corpus_scale, l2_dists
from l2_range_cases import (GAUSS_DIMS, SLOT_CAP, band, dist_up, gauss_case, mirror, must_be_collected, range_ref,
                            selective_radii)
from oracle import search_ref
from text_similarity_amd import _lib, ops

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tsim.h")
NEW = ("tsim_l2_range_scan", "tsim_l2_range_scan_tau", "tsim_range_merge_asc")
EINVAL, ENOMEM = 1, 3


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtsim.so is not built")
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------- C ABI
def test_symbols_declared_bound_and_exported():
    hdr = open(HDR).read()
    assert "#define TSIM_SPACE_L2 2" in hdr and _lib.SPACE_L2 == 2
    for name in NEW:
        assert f"{name}(" in hdr, name
        assert name in _lib.DECLARED_SYMBOLS, name
    assert ops.RANGE_SLOT_CAP == SLOT_CAP
    assert callable(ops.l2_range)
    L = _lib_or_skip()
    assert L.tsim_version() == 104
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name


def test_l2_range_entries_refuse_bad_arguments_before_any_launch():
    """Fake (never dereferenced) 16-byte aligned device pointers: every refusal happens on the host."""
    L = _lib_or_skip()
    p, big = 1 << 20, 1 << 40
    need = L.tsim_range_workspace_bytes(4, 100)
    assert need > 0
    base = dict(eq=p, eq_f32=p, ec=p, ec_f32=p, maxnorm=p, rho=p, d=383, ld=384, ws=big)

    def call(fn, radius, **kw):
        a = {**base, **kw}
        return fn(a["eq"], a["eq_f32"], a["d"], 4, a["ec"], a["ec_f32"], a["d"], a["maxnorm"], a["rho"], 100, a["d"], a["ld"],
                  radius, p, None, p, a["ws"], None)

    for fn, r in ((L.tsim_l2_range_scan, 1.5), (L.tsim_l2_range_scan_tau, p)):
        for kw in ({"eq_f32": None}, {"ec_f32": None}, {"maxnorm": None}, {"rho": None},
                   {"d": 384, "ld": 384},                          # ld != pad_dim(d + 1) = 512
                   {"d": 127, "ld": 256}, {"d": 128, "ld": 128},   # the width boundary: pad_dim(128) = 128, pad_dim(129) = 256
                   {"d": 768, "ld": 768}):                         # d + 1 > 768
            assert call(fn, r, **kw) == EINVAL, kw
            assert b"l2_range_scan" in L.tsim_last_error()
        assert call(fn, r, ws=need - 1) == ENOMEM
    assert call(L.tsim_l2_range_scan, float("nan")) == EINVAL
    assert b"NaN" in L.tsim_last_error()
    assert call(L.tsim_l2_range_scan_tau, None) == EINVAL        # a null radius array


def test_fill_accepts_the_l2_space_and_checks_it():
    L = _lib_or_skip()
    p, big = 1 << 20, 1 << 40
    need = L.tsim_range_workspace_bytes(4, 100)
    ok = (p, 383, 4, p, 383, 100, 383)
    assert L.tsim_range_fill(2, *ok, 0.5, p, p, p, 0, p, need - 1, None) == ENOMEM     # the space is known: its workspace is checked
    assert L.tsim_range_fill_tau(2, *ok, p, p, p, p, 0, p, need - 1, None) == ENOMEM
    assert L.tsim_range_fill(7, *ok, 0.5, p, p, p, 0, p, need - 1, None) == EINVAL
    assert L.tsim_range_fill(2, *ok, float("nan"), p, p, p, 0, p, big, None) == EINVAL
    assert L.tsim_range_fill(2, p, 768, 4, p, 768, 100, 768, 0.5, p, p, p, 0, p, big, None) == EINVAL   # d = 768


def test_merge_asc_refuses_bad_list_counts():
    L = _lib_or_skip()
    p = 1 << 20
    for nlists in (0, 65):
        assert L.tsim_range_merge_asc(p, p, p, nlists, 4, p, 10, p, p, None) == EINVAL
        assert b"range_merge_asc" in L.tsim_last_error()
    assert L.tsim_range_merge_asc(p, p, p, 3, 4, p, 0, p, p, None) == 0      # nothing to merge: no launch
    assert L.tsim_range_merge_asc(None, p, p, 3, 4, p, 10, p, p, None) == EINVAL


# ---------------------------------------------------------------------------------------------------------- guard replay
def _collect_threshold(eps, nqs, qq, r):
    """guard_tau_l2(r, eps, nqs, qq): the library's l2_tau_lo (tsim_l2_guard_host, out[2]) stepped one float32 down
    (csrc/search.hip float_below, restated by ops._f32_below).  None: no finite threshold (the query goes to the exact pass)."""
    out = (ctypes.c_double * 3)()
    assert _lib_or_skip().tsim_l2_guard_host(0.0, float(eps), float(nqs), float(qq), float(r), out) == 0
    if not out[2] > -3.0e38:
        return None
    return ops._f32_below(np.float32(out[2]))


def _flush(h):
    return np.where(np.abs(h) < 2.0 ** -14, 0.0, h)


def _model_scores(hq, hc):
    """Model MFMA scores of the augmented half rows as tests/test_l2_search_cpu.py builds them: float32 accumulation element by
    element and float64 accumulation rounded once, subnormal halves kept and flushed on either operand."""
    out = []
    for hh in (hc, _flush(hc)):
        for uu in (hq, _flush(hq)):
            m = np.zeros((hq.shape[0], hc.shape[0]), dtype=np.float32)
            for j in range(hq.shape[1]):
                m = (m + (uu[:, j:j + 1] * hh[None, :, j]).astype(np.float32)).astype(np.float32)
            out.append(m)
            out.append((uu @ hh.T).astype(np.float32))
    return out


def _replay_data():
    """The shapes of tests/test_l2_search_cpu.py _replay_data at d = 97: rows over six decades of norm, a huge row that sets A, a
    cluster whose distances to query 0 step by about one float32 ulp, exact duplicates of query 1, a far and a near query."""
    rng = np.random.default_rng(61)
    d = 97
    c = rng.standard_normal((400, d)).astype(np.float32) / np.sqrt(d)
    c *= (10.0 ** rng.uniform(-3, 3, (400, 1))).astype(np.float32)   # norms over six decades: most rows subnormal halves
    c[5] *= 1e4 / np.linalg.norm(c[5])                              # one huge row: A = 2^14
    q0 = (rng.standard_normal(d) * 40.0).astype(np.float32)
    off = rng.standard_normal(d) * 3.0
    for k in range(60):                                              # dist^2 ~ |off|^2 (1 + k 2^-23): one-ulp steps
        c[100 + k] = (q0.astype(np.float64) + off * (1.0 + k * 2.0 ** -24)).astype(np.float32)
    q1 = (rng.standard_normal(d) * 7.0).astype(np.float32)
    c[200:206] = q1                                                  # exact duplicates of query 1
    c[206] = q1 + np.float32(1e-3)                                   # and a near miss
    A = corpus_scale(c)
    u = rng.standard_normal((2, d))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    q = np.concatenate([q0[None], q1[None], (u[0] * 1e4 * A)[None], (u[1] * 1e-4 * A)[None],
                        rng.standard_normal((2, d))]).astype(np.float32)
    return q, c, A, d


def test_guard_replay_every_hit_is_above_the_collect_threshold():
    L = _lib_or_skip()
    q, c, A, d = _replay_data()
    assert A == 2.0 ** 14
    ld = L.tsim_pad_dim(d + 1)
    S = 2.0 * A
    hc, rho_c = aug_corpus(c, A)
    hq, rho_q, qq, nq = aug_queries(q, A)
    D = l2_dists(q, c, dtype=np.float64)
    d32 = D.astype(np.float32)
    models = _model_scores(hq, hc)
    cl = d32[0, 100:160]
    assert np.unique(cl).size >= 20 and float(cl.max() - cl.min()) <= 256 * float(np.spacing(cl.min()))   # ulp-scale steps
    assert (d32[1, 200:206] == 0).all() and d32[1, 206] > 0
    below = lambda r: np.nextafter(np.float32(r), np.float32(-np.inf))
    radii = {qi: list(selective_radii(d32[qi])) for qi in range(q.shape[0])}
    radii[0] += [cl[30], below(cl[30]), np.sort(cl)[0], below(np.sort(cl)[0]), np.sort(cl)[-1]]   # r EQUAL to a row's distance
    radii[1] += [np.float32(0.0), np.float32(-1.0), d32[1, 206], below(d32[1, 206])]
    nhit = nband = nfinite = 0
    for qi in range(q.shape[0]):
        eps = float(np.float32(search_ref.guard_eps(rho_q[qi], rho_c, ld)))
        nqs = float(nq[qi]) * S
        conv = (float(qq[qi]) - D[qi]) / (2.0 * nqs)
        for m in models:
            assert np.abs(m[qi].astype(np.float64) - conv).max() <= eps, qi          # the bound itself
        for r in radii[qi]:
            thr = _collect_threshold(eps, nqs, qq[qi], r)
            assert thr is not None, (qi, float(r))
            nfinite += 1
            hits = d32[qi] <= np.float32(r)
            far = D[qi] >= dist_up(r) + band(eps, nqs)
            for m in models:
                assert (m[qi][hits] > thr).all(), (qi, float(r), float(thr))         # every hit is collected
                assert not (m[qi][far] > thr).any(), (qi, float(r), float(thr))      # and nothing beyond the band
                nband += int((m[qi] > thr).sum()) - int(hits.sum())
            nhit += int(hits.sum())
    assert int((d32[1] <= 0).sum()) == 6                                             # r = 0: exactly the duplicates
    assert nhit >= 6 * 19 + 60          # 10 + 9 hits of every query's selective radii, the whole cluster at its largest distance
    # no finite threshold: +inf and NaN radii, a non-finite nqs
    assert _collect_threshold(1e-3, 10.0, 1.0, np.inf) is None
    assert _collect_threshold(1e-3, 10.0, 1.0, np.nan) is None
    assert _collect_threshold(1e-3, np.inf, 1.0, 1.0) is None
    print(f"l2 range replay: {nhit} hits above {nfinite} thresholds, {nband} band rows collected with them (8 models)")


@pytest.mark.parametrize("d", GAUSS_DIMS)
def test_gaussian_case_of_the_gpu_test_must_be_answered_from_the_collected_rows(d):
    """The seed of tests/test_l2_range_gpu.py's Gaussian case, checked with the oracle alone: at the selective radius every one
    of the 8 queries gathers at most TSIM_RANGE_SLOT_CAP rows, so the GPU test may demand status 1 of all of them."""
    ld = _lib_or_skip().tsim_pad_dim(d + 1)
    q, c = gauss_case(d)
    D = l2_dists(q, c, dtype=np.float64)
    r, r_below = selective_radii(D[0].astype(np.float32))
    assert range_ref(D[0].astype(np.float32), r).size == 10 and range_ref(D[0].astype(np.float32), r_below).size == 9
    _, eps, nqs, _ = mirror(q, c, ld)
    for qi in range(q.shape[0]):
        assert must_be_collected(D[qi], r, eps[qi], nqs[qi]), qi
