"""Exact Euclidean search on the host: the C ABI of the L2 path (symbols, argument checks before any launch) and a CPU replay of
its guard on adversarial data — the bound |m - (|q|^2 - dist^2) / (2 nqs)| <= eps on model MFMA scores of the augmented half
rows, and the two decisions the kernels take from it, INCLUDING the float32 ulp of the k-th distance (include/tsim.h)."""
import os

import numpy as np
import pytest

from l2_cases import aug_corpus, aug_queries, corpus_scale, l2_dists
from oracle import search_ref
from text_similarity_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tsim.h")
NEW = ("tsim_l2_rows", "tsim_l2_query_rows", "tsim_l2_topk_ex", "tsim_l2_topk_large", "tsim_l2_guard_host")


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtsim.so is not built")
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------- C ABI
def test_header_symbols_exported_and_bound():
    hdr = open(HDR).read()
    for name in NEW:
        assert f"{name}(" in hdr, name
        assert name in _lib.DECLARED_SYMBOLS, name
    L = _lib_or_skip()
    assert L.tsim_version() == 104
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name


def test_l2_entries_refuse_bad_arguments_before_any_launch():
    """Fake (never dereferenced) 16-byte aligned device pointers are enough: every case returns TSIM_EINVAL from the checks."""
    L = _lib_or_skip()
    p = 1 << 20
    base = dict(eq=p, eq_f32=p, ec=p, ec_f32=p, maxnorm=p, rho=p, d=383, ld=384, k=10)

    def call(fn, **kw):
        a = {**base, **kw}
        ws = L.tsim_topk_large_workspace_bytes(4, 100, a["k"])
        return fn(a["eq"], a["eq_f32"], a["d"], 4, a["ec"], a["ec_f32"], a["d"], a["maxnorm"], a["rho"], 100, a["d"], a["ld"],
                  a["k"], p, p, None, 0, p, ws, None)

    for fn in (L.tsim_l2_topk_ex, L.tsim_l2_topk_large):
        for kw in ({"eq_f32": None}, {"ec_f32": None}, {"eq_f32": None, "ec_f32": None}, {"rho": None}, {"maxnorm": None},
                   {"d": 384, "ld": 384},          # ld != pad_dim(d + 1) = 512
                   {"d": 127, "ld": 256}, {"d": 128, "ld": 128},   # the width boundary: pad_dim(128) = 128, pad_dim(129) = 256
                   {"d": 768, "ld": 768}):         # d + 1 > 768
            assert call(fn, **kw) == 1, kw                       # TSIM_EINVAL
            assert b"l2_topk" in L.tsim_last_error()
    assert call(L.tsim_l2_topk_ex, k=65) == 1
    assert L.tsim_l2_rows(p, 0, 4, 384, 384, None, p, 512, None, None) == 1      # NULL word
    assert L.tsim_l2_rows(p, 0, 4, 384, 384, p, p, 384, None, None) == 1         # ld_out < d + 1
    assert L.tsim_l2_rows(p, 0, 4, 384, 384, p, None, 512, None, None) == 1
    assert L.tsim_l2_query_rows(p, 0, 4, 384, 384, None, p, 512, None) == 1
    assert L.tsim_l2_query_rows(p, 0, 4, 384, 384, p, p, 384, None) == 1
    assert L.tsim_l2_rows(p, 7, 4, 384, 384, p, p, 512, None, None) == 1         # unknown dtype


# ---------------------------------------------------------------------------------------------------------- guard replay
# The replay takes the guard's conversions from the LIBRARY (tsim_l2_guard_host: csrc/search.hip l2_dist_up / l2_bound_low /
# l2_tau_lo compiled for the host, the functions the kernels call), so a wrong constant or sign there fails these tests; the
# float64 restatements below are checked against it.
def _guard(m, eps, nqs, qq, dk):
    """(up(dk), lower bound of dist^2 for MFMA scores <= m, collection threshold tau) as the library evaluates them."""
    import ctypes
    out = (ctypes.c_double * 3)()
    assert _lib_or_skip().tsim_l2_guard_host(float(m), float(eps), float(nqs), float(qq), float(dk), out) == 0
    tau = np.nextafter(np.float32(out[2]), np.float32(-np.inf)) if np.isfinite(out[2]) else np.float32(-3.4028234e38)
    return out[0], out[1], tau


def test_guard_conversions_of_the_library_match_their_restatement():
    rng = np.random.default_rng(31)
    for _ in range(200):
        m, eps = rng.uniform(-1, 1), 10.0 ** rng.uniform(-4, -2)
        qq, A = 10.0 ** rng.uniform(-6, 10), 2.0 ** rng.integers(-3, 15)
        nqs = np.sqrt(qq + A * A) * 2 * A
        dk = np.float32(qq * rng.uniform(0.5, 1.5))
        up, low, tau = _guard(m, eps, nqs, qq, dk)
        m, eps = float(np.float32(m)), float(np.float32(eps))
        assert abs(up - _dist_up(dk)) <= 1e-13 * up
        assert abs(low - _bound_low(m, eps, nqs, qq)) <= 1e-13 * (qq + 2 * nqs)
        assert abs(float(tau) - float(_tau(dk, eps, nqs, qq))) <= 2.5e-7 * max(abs(float(tau)), 1e-30)
        assert low < qq - (m + eps) * 2 * nqs and up > float(dk) * (1 + 2.0 ** -23)      # slack on the safe side
    assert _guard(0.0, np.inf, 1.0, 1.0, 1.0)[2] == np.float32(-3.4028234e38)              # no finite threshold: collect all
    assert _guard(0.0, 1e-3, np.inf, 1.0, 1.0)[2] == np.float32(-3.4028234e38)
    assert not (_guard(0.0, np.inf, 1.0, 1.0, 1.0)[1] > 0)                                 # and never "safe"


def _dist_up(dk):
    return float(dk) * (1.0 + 1.1921e-7) + 1e-44


def _bound_low(m, eps, nqs, qq):
    b = (float(m) + float(eps) + 1e-13) * 2.0 * nqs
    return qq - b - (qq + abs(b)) * 1e-14


def _tau(dk, eps, nqs, qq):
    up = _dist_up(dk)
    t = (qq - up - (qq + up) * 1e-14) / (2.0 * nqs)
    lo = t - float(eps) - 1e-13 - (abs(t) + float(eps)) * 1e-15
    return np.nextafter(np.float32(lo), np.float32(-np.inf))


def _flush(h):
    return np.where(np.abs(h) < 2.0 ** -14, 0.0, h)


def _replay_data():
    rng = np.random.default_rng(23)
    d = 128
    c = rng.standard_normal((600, d)).astype(np.float32) / np.sqrt(d)
    c *= (10.0 ** rng.uniform(-3, 3, (600, 1))).astype(np.float32)   # norms over six decades: most rows subnormal halves
    c[5] *= 1e4 / np.linalg.norm(c[5])                              # one huge row: A = 2^14
    base = rng.standard_normal(d).astype(np.float32)
    c[200:260] = base + 1e-6 * rng.standard_normal((60, d)).astype(np.float32)   # near-ties
    c[300:310] = 0.0
    far = (rng.standard_normal(d) / np.sqrt(d) * 3000.0).astype(np.float32)      # a cluster far from the origin, radius << |c|
    c[400:440] = far + 1e-2 * rng.standard_normal((40, d)).astype(np.float32)
    A = corpus_scale(c)
    u = rng.standard_normal((2, d))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    q = np.concatenate([(u[0] * 1e4 * A)[None], (u[1] * 1e-4 * A)[None], np.zeros((1, d)), c[17][None], c[210][None],
                        base[None], far[None], rng.standard_normal((4, d))]).astype(np.float32)
    return q, c, A, d


def _replay(q, c, A, d, ld, k=10, KL=16):
    """The three assertions of the replay on one data set; returns how many first passes the guard lets stand."""
    S = 2.0 * A
    hc, rho_c = aug_corpus(c, A)
    hq, rho_q, qq, nq = aug_queries(q, A)
    assert np.abs(hc).max() <= 1.0 and rho_c > 0
    D = l2_dists(q, c, dtype=np.float64)                             # canonical float64 distances
    d32 = D.astype(np.float32)
    rows = np.arange(c.shape[0])
    nsafe = 0
    for hh in (hc, _flush(hc)):
        for uu in (hq, _flush(hq)):
            m = np.zeros((q.shape[0], c.shape[0]), dtype=np.float32)
            for j in range(d + 1):        # float32 accumulation element by element (mfma_model_scores 'f32seq')
                m = (m + (uu[:, j:j + 1] * hh[None, :, j]).astype(np.float32)).astype(np.float32)
            for qi in range(q.shape[0]):
                eps = float(np.float32(search_ref.guard_eps(rho_q[qi], rho_c, ld)))
                nqs = float(nq[qi]) * S
                conv = (float(qq[qi]) - D[qi]) / (2.0 * nqs)
                assert np.abs(m[qi].astype(np.float64) - conv).max() <= eps, qi
                order = np.lexsort((rows, -m[qi].astype(np.float64)))
                cand, outside = order[:KL], order[KL:]
                cut = float(m[qi][cand[-1]])
                dk = np.sort(d32[qi][cand])[k - 1]                   # the k-th distance of the first pass's list
                up, low, _ = _guard(cut, eps, nqs, float(qq[qi]), dk)
                assert (D[qi][outside] >= low).all(), qi             # l2_bound_low holds for every row outside
                if low > up:                                         # the guard lets the list stand:
                    nsafe += 1
                    assert (d32[qi][outside] > dk).all(), qi         # nothing outside rounds to a distance <= the k-th
                for target in (dk, np.sort(d32[qi])[k - 1]):
                    tau = _guard(cut, eps, nqs, float(qq[qi]), target)[2]
                    assert (m[qi][d32[qi] <= target] > tau).all(), qi   # guard_tau_l2 collects every row that can tie or beat it
    return nsafe, d32


def test_guard_covers_every_distance_and_its_float32_ulp():
    """Model MFMA scores of the augmented rows ('f32seq' accumulation, kept and flushed subnormals, both operands).  For every
    (query, row): |m - (|q|^2 - dist^2) / (2 nqs)| <= eps.  For every query, with the first pass's 16 candidates: every row
    outside them has dist^2 >= l2_bound_low(cut), and when the guard calls the list safe no such row ROUNDS to a float32 distance
    <= the k-th; every row whose float32 distance is <= the k-th has m > guard_tau_l2 — with the TRUE k-th distance too."""
    q, c, A, d = _replay_data()
    assert A == 2.0 ** 14
    nsafe, d32 = _replay(q, c, A, d, 256)                            # ld = tsim_pad_dim(d + 1)
    assert d32[3, 17] == 0.0 and d32[4, 210] == 0.0                  # a query equal to a corpus row
    print(f"guard replay, adversarial rows: {nsafe} of {4 * q.shape[0]} first passes stand")


def test_guard_lets_first_passes_stand_on_plain_rows():
    """The same replay on Gaussian rows with norms in 0.5 .. 2 (no huge row: A = 32), where the 'safe' branch is taken — among
    the queries one 1e4 A long, whose distances tie in float32, and one equal to a corpus row."""
    rng = np.random.default_rng(29)
    d = 128
    c = rng.standard_normal((600, d)).astype(np.float32) * rng.uniform(0.5, 2.0, (600, 1)).astype(np.float32)
    A = corpus_scale(c)
    u = rng.standard_normal(d)
    q = np.concatenate([rng.standard_normal((10, d)), (u / np.linalg.norm(u) * 1e4 * A)[None], c[33][None]]).astype(np.float32)
    nsafe, _ = _replay(q, c, A, d, 256)
    print(f"guard replay, plain rows: {nsafe} of {4 * q.shape[0]} first passes stand")
    assert nsafe >= 4


def test_float32_ulp_of_a_far_querys_distance_exceeds_the_rounding_term_of_guard_eps():
    """|q| = 1e4 A: one float32 ulp of a distance (~|q|^2 2^-23) is (|q| / A) 2^-24 ~ 6e-4 in MFMA units — far above the 2^-22 of
    guard_eps, which therefore cannot stand in for it — and many rows round to the SAME float32 distance."""
    q, c, A, d = _replay_data()
    _, _, qq, nq = aug_queries(q[:1], A)
    d32 = l2_dists(q[:1], c)[0]
    ulp_mfma = float(np.spacing(d32.max())) / (2.0 * float(nq[0]) * 2.0 * A)
    assert ulp_mfma > 100 * 2.0 ** -22
    assert np.unique(d32).size < d32.size
