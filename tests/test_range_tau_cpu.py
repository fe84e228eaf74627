"""Host side of the per-query thresholds and of the merge (include/tsim.h tsim_cosine_range_scan_tau / tsim_dot_range_scan_tau /
tsim_range_fill_tau / tsim_range_merge): the argument checks that run before any launch, and a CPU replay of the set-up with a
threshold VECTOR — ops.range_collect_threshold mirrors the set-up kernel, which reads tau_q[q]: on model MFMA scores no hit of
any query lies at or below that query's own collect threshold."""
import os

import numpy as np
import pytest

from oracle.search_ref import exact_cosine, mfma_model_scores, rho_rows
from text_similarity_amd import _lib, ops


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtsim.so is not built")
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------- argument checks
@pytest.mark.parametrize("dot", [False, True])
def test_tau_entries_check_arguments_before_any_launch(dot):
    """Fake (never dereferenced) 16-byte aligned device pointers: every refusal happens on the host."""
    L = _lib_or_skip()
    fn = L.tsim_dot_range_scan_tau if dot else L.tsim_cosine_range_scan_tau
    p, big = 1 << 20, 1 << 40
    need = L.tsim_range_workspace_bytes(4, 100)

    def scan(tau_q, ws, f32=p):
        head = (p, f32, 384, 4, p, f32, 384) + ((p, p) if dot else (p,))
        return fn(*head, 100, 384, 384, tau_q, p, None, p, ws, None)

    assert scan(None, big) == 1 and b"threshold" in L.tsim_last_error()      # TSIM_EINVAL: no array
    assert scan(p, big, f32=None) == 1 and b"float32" in L.tsim_last_error()
    assert scan(p, need - 1) == 3                                            # TSIM_ENOMEM: short workspace
    fill = L.tsim_range_fill_tau
    ok = (p, 384, 4, p, 384, 100, 384)
    assert fill(0, *ok, None, p, p, p, 0, p, big, None) == 1
    assert fill(7, *ok, p, p, p, p, 0, p, big, None) == 1
    assert fill(1, *ok, p, p, p, p, 0, p, need - 1, None) == 3
    assert L.tsim_version() == 104


def test_range_merge_checks_arguments_before_any_launch():
    L = _lib_or_skip()
    p = 1 << 20
    merge = L.tsim_range_merge
    assert _lib.RANGE_MERGE_MAX_LISTS == ops.RANGE_MERGE_MAX_LISTS == 64
    assert merge(p, p, p, 0, 4, p, 10, p, p, None) == 1 and b"lists" in L.tsim_last_error()
    assert merge(p, p, p, 65, 4, p, 10, p, p, None) == 1
    assert merge(p, p, p, 2, -1, p, 10, p, p, None) == 1
    assert merge(p, p, p, 2, 4, p, -1, p, p, None) == 1
    assert merge(None, p, p, 2, 4, p, 10, p, p, None) == 1
    assert merge(p, p, p, 2, 4, p, 10, None, p, None) == 1
    # Q = 0 or a total of 0: TSIM_OK without a launch (nothing is dereferenced, the outputs may be null)
    assert merge(p, p, p, 2, 0, p, 0, None, None, None) == 0
    assert merge(p, None, None, 64, 4, p, 0, None, None, None) == 0


# ---------------------------------------------------------------------------------------------------------- guard replay
def _rho_up(r):
    """csrc/common.h rho_round_up"""
    return np.minimum(np.float32(np.asarray(r, np.float64) * (1.0 + 1e-6)), np.float32(2.0))


def test_guard_replay_with_a_threshold_vector():
    """ops.range_collect_threshold is the host mirror of the set-up kernel, which now reads tau_q[q]: replayed on model MFMA
    scores (two accumulation orders) with one threshold per query, every hit of a query has a model score strictly above that
    query's OWN collect threshold — also where the neighbouring query's threshold is far higher or lower."""
    rng = np.random.default_rng(12)
    d, n, Q = 384, 3000, 24
    c = rng.standard_normal((n, d)).astype(np.float32)
    base = rng.standard_normal(d).astype(np.float32)
    c[100:140] = base + 1e-7 * rng.standard_normal((40, d)).astype(np.float32)     # a cluster 1e-7 apart
    c[200:260] = c[7]                                                               # bit-equal duplicates
    q = rng.standard_normal((Q, d)).astype(np.float32)
    q[:6] = base + 1e-3 * rng.standard_normal((6, d)).astype(np.float32)
    q[6] = c[7]
    exact = exact_cosine(q, c)
    model = [mfma_model_scores(q, c, order) for order in ("f64", "f32seq")]
    rq = _rho_up(rho_rows(q))
    rc = _rho_up(rho_rows(c).max())
    tau = np.empty(Q, np.float32)
    for qi in range(Q):
        srt = np.sort(exact[qi])[::-1]
        tau[qi] = (srt[5], np.float32(np.median(exact[qi, 100:140])), exact[qi, 7], np.float32(0.05), -np.inf, np.inf, np.nan,
                   np.nextafter(srt[9], np.float32(np.inf)))[qi % 8]
    nhit = nfinite = 0
    for qi in range(Q):
        thr, eps = ops.range_collect_threshold(tau[qi], rq[qi], rc, d)
        with np.errstate(invalid="ignore"):
            hits = np.nonzero(exact[qi] >= tau[qi])[0]
        if tau[qi] != tau[qi] or tau[qi] == -np.inf:
            assert thr is None                       # no finite threshold: the exact pass answers (NaN: with no hit)
            assert tau[qi] == -np.inf or hits.size == 0
            continue
        assert thr is not None
        nfinite += 1
        for m in model:
            assert np.abs(m[qi].astype(np.float64) - exact[qi]).max() <= eps
            assert (m[qi, hits] > thr).all(), (qi, float(tau[qi]), float(thr))
        assert float(thr) + float(eps) < float(tau[qi]) or tau[qi] == np.inf
        nhit += hits.size
    assert nhit > 300 and nfinite == Q - 2 * (Q // 8)
