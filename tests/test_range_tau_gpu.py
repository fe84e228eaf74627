"""Per-query thresholds of the exact range search (include/tsim.h tsim_cosine_range_scan_tau / tsim_dot_range_scan_tau /
tsim_range_fill_tau; ops.cosine_range / ops.dot_range with a threshold tensor [Q]) and of the layers above them
(GpuFlatIndex.range_search, SentenceMiningPipeline.mine).
Bar: per query the rows whose exact score (oracle/search_ref.exact_cosine, or float32 of the lane-ordered float64 inner product)
is >= float32(tau[q]), ordered by (score desc, index asc): lims, indices and float32 score bits identical, no tolerance.  And the
vector path IS the scalar path: for every distinct value of the vector the scalar call with that value returns, for the queries
that carry it, the same bits and the same status.
Shape: Q = 70 (not a multiple of the set-up kernel's four waves per workgroup, more than one wave's worth), N = 5 000 (above the
2 048-entry slot, so a query overflows while its neighbours do not), d = 100 (padded to 128) and d = 384."""
import types

import numpy as np
import pytest
import torch

from oracle.search_ref import _lane_sum, exact_cosine
from text_similarity_amd import ops
from text_similarity_amd.index import GpuFlatIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CAP = ops.RANGE_SLOT_CAP
Q, N = 70, 5000
KINDS = ("selective", "equal", "next_above", "minus_inf", "plus_inf", "nan", "overflow", "below_all")


# ---------------------------------------------------------------------------------------------------------- test-local oracle
def dot_scores(q, c, qblock=16, nblock=4096):
    """[Q, N] float32(q.c): float64 sum in the canonical lane order, one rounding."""
    q = np.asarray(q, dtype=np.float32)
    c = np.asarray(c, dtype=np.float32)
    out = np.empty((q.shape[0], c.shape[0]), dtype=np.float32)
    for a in range(0, q.shape[0], qblock):
        for b in range(0, c.shape[0], nblock):
            out[a:a + qblock, b:b + nblock] = _lane_sum(q[a:a + qblock, None, :], c[None, b:b + nblock, :]).astype(np.float32)
    return out


def range_ref_q(s, tau):
    """the indices of one query's float32 scores s with s >= float32(tau), ordered (score desc, index asc); NaN: none"""
    with np.errstate(invalid="ignore"):
        hit = np.nonzero(s >= np.float32(tau))[0]
    return hit[np.lexsort((hit, -s[hit].astype(np.float64)))]


# ---------------------------------------------------------------------------------------------------------- data, built once
_CASES = {}


def _case(space, d):
    """(q, c, exact [Q, N], tau [Q] float32, kind per query, reference hits per query) — computed once per (space, d), shared"""
    key = (space, d)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(1000 * d + (space == "dot"))
    c = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    base = rng.standard_normal(d).astype(np.float32)
    c[700:760] = base + 1e-3 * rng.standard_normal((60, d)).astype(np.float32)     # a planted cluster ...
    q[:16] = base + 1e-2 * rng.standard_normal((16, d)).astype(np.float32)         # ... around two queries of every kind
    exact = exact_cosine(q, c) if space == "cosine" else dot_scores(q, c)
    tau = np.empty(Q, np.float32)
    kinds = []
    for qi in range(Q):
        kind = KINDS[qi % len(KINDS)]                       # neighbouring queries carry different kinds
        srt = np.sort(exact[qi])[::-1]
        n = 5 + (qi * 7) % 46                               # 5 .. 50 hits
        if kind == "selective":
            t = np.float32((np.float64(srt[n - 1]) + np.float64(srt[n])) / 2)
            if not srt[n] < t <= srt[n - 1]:
                t = srt[n - 1]
        elif kind == "equal":                               # the bits of one exact score of this query: that row is in
            t = srt[n - 1]
        elif kind == "next_above":                          # the next float above it: that row is out
            t = np.nextafter(srt[n - 1], np.float32(np.inf))
        elif kind == "minus_inf":
            t = -np.inf
        elif kind == "plus_inf":
            t = np.inf
        elif kind == "nan":
            t = np.nan
        elif kind == "overflow":                            # more hits than a slot holds
            t = srt[CAP + 300 + qi]
        else:                                               # below every score
            t = np.float32(srt[-1] - (1.0 if space == "cosine" else 100.0))
        tau[qi] = t
        kinds.append(kind)
    ref = [range_ref_q(exact[qi], tau[qi]) for qi in range(Q)]
    _CASES[key] = (q, c, exact, tau, kinds, ref)
    return _CASES[key]


def _operands(space, q, c):
    qf = torch.from_numpy(q).to(DEV)
    cf = torch.from_numpy(c).to(DEV)
    if space == "cosine":
        cn, rho = ops.l2norm_rows(cf, return_rho=True)
        return ops.l2norm_rows(qf), cn, qf, cf, dict(rho_c=rho)
    cn, rho, scale = ops.dot_scaled_rows(cf)
    return ops.l2norm_rows(qf), cn, qf, cf, dict(rho_c=rho, scale_c=scale)


def _call(space, operands, d, threshold, **kw):
    qn, cn, qf, cf, extra = operands
    fn = ops.cosine_range if space == "cosine" else ops.dot_range
    r = fn(qn, cn, d, threshold, eq_f32=qf, ec_f32=cf, return_status=True, **extra, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in r)


def _assert_matches_ref(lims, s, i, exact, ref, idx_offset=0):
    np.testing.assert_array_equal(lims, np.concatenate([[0], np.cumsum([r.size for r in ref])]))
    assert s.shape == (lims[-1],) and i.shape == (lims[-1],)
    for qi, r in enumerate(ref):
        a, b = int(lims[qi]), int(lims[qi + 1])
        np.testing.assert_array_equal(i[a:b], r + idx_offset, err_msg=f"query {qi}: indices")
        np.testing.assert_array_equal(s[a:b].view(np.uint32), exact[qi, r].view(np.uint32), err_msg=f"query {qi}: score bits")


# ---------------------------------------------------------------------------------------------------------- 1. the ops
@pytest.mark.parametrize("space", ["cosine", "dot"])
@pytest.mark.parametrize("d", [100, 384])
def test_threshold_vector_exact_and_equal_to_the_scalar_calls(space, d):
    q, c, exact, tau, kinds, ref = _case(space, d)
    operands = _operands(space, q, c)
    lims, s, i, st = _call(space, operands, d, torch.from_numpy(tau).to(DEV), idx_offset=11)
    _assert_matches_ref(lims, s, i, exact, ref, idx_offset=11)
    sizes = np.diff(lims)
    for qi, kind in enumerate(kinds):
        n = 5 + (qi * 7) % 46
        if kind == "selective":
            assert n <= sizes[qi] <= 64 and st[qi] == 1, (qi, sizes[qi], st[qi])      # (more than n only on a tie of the scores)
        elif kind == "equal":
            assert sizes[qi] >= n and s[lims[qi + 1] - 1].view(np.uint32) == tau[qi].view(np.uint32)    # the row on tau is in
        elif kind == "next_above":
            assert sizes[qi] < n and (sizes[qi] == 0 or s[lims[qi + 1] - 1] > np.sort(exact[qi])[::-1][n - 1])   # ... and out
        elif kind == "minus_inf":
            assert sizes[qi] == N and st[qi] == 2
        elif kind == "plus_inf":
            assert sizes[qi] == 0
        elif kind == "nan":
            assert sizes[qi] == 0 and st[qi] == 2
        elif kind == "overflow":
            assert sizes[qi] > CAP and st[qi] == 2
        else:
            assert sizes[qi] == N
    assert np.isin(st, (1, 2)).all()
    # the vector path is the scalar path: every distinct value as the float of a scalar call, on the same queries
    for v in np.unique(tau.view(np.uint32)):
        value = np.array([v], np.uint32).view(np.float32)[0]
        carriers = np.nonzero(tau.view(np.uint32) == v)[0]
        if value != value:               # the scalar entries refuse a NaN; the vector gave those queries nothing, status 2
            with pytest.raises(ValueError):
                _call(space, operands, d, float(value))
            continue
        l1, s1, i1, st1 = _call(space, operands, d, float(value), idx_offset=11)
        for qi in carriers:
            a, b, a1, b1 = int(lims[qi]), int(lims[qi + 1]), int(l1[qi]), int(l1[qi + 1])
            assert b - a == b1 - a1, (qi, float(value))
            np.testing.assert_array_equal(i[a:b], i1[a1:b1])
            np.testing.assert_array_equal(s[a:b].view(np.uint32), s1[a1:b1].view(np.uint32))
            assert st[qi] == st1[qi], (qi, float(value), st[qi], st1[qi])


def test_threshold_tensor_conversion_and_wrong_length():
    space, d = "cosine", 100
    q, c, exact, tau, kinds, ref = _case(space, d)
    operands = _operands(space, q, c)
    want = _call(space, operands, d, torch.from_numpy(tau).to(DEV))
    # another dtype (float64 holding the same values), the host as device, a numpy array: converted, same bits
    for thr in (torch.from_numpy(tau.astype(np.float64)), torch.from_numpy(tau), tau):
        got = _call(space, operands, d, thr)
        for a, b in zip(want, got):
            np.testing.assert_array_equal(a, b)
    for bad in (torch.zeros(Q - 1), torch.zeros(Q + 1, device=DEV), torch.zeros((Q, 1)), torch.zeros(1), np.zeros(3, np.float32)):
        with pytest.raises(ValueError):
            _call(space, operands, d, bad)
    # a 0-dim tensor is one threshold for the call, as a float is
    one = _call(space, operands, d, torch.tensor(0.3))
    flt = _call(space, operands, d, 0.3)
    for a, b in zip(one, flt):
        np.testing.assert_array_equal(a, b)


def test_threshold_slices_with_the_queries(monkeypatch):
    """query sets above MAX_RANGE_QUERIES_PER_CALL go through in slices: the threshold tensor is sliced with them"""
    space, d = "dot", 100
    q, c, exact, tau, kinds, ref = _case(space, d)
    operands = _operands(space, q, c)
    monkeypatch.setattr(ops, "MAX_RANGE_QUERIES_PER_CALL", 32)      # 32 + 32 + 6
    lims, s, i, st = _call(space, operands, d, torch.from_numpy(tau).to(DEV))
    _assert_matches_ref(lims, s, i, exact, ref)


# ---------------------------------------------------------------------------------------------------------- 2. index, pipeline
@pytest.mark.parametrize("space", ["cosine", "ip"])
def test_flat_index_range_search_with_an_array(space):
    sp, d = ("cosine" if space == "cosine" else "dot"), 100
    q, c, exact, tau, kinds, ref = _case(sp, d)
    labels = np.arange(N) * 3 + 10_000
    idx = GpuFlatIndex(space=space, dim=d, device=DEV)
    idx.init_index(max_elements=N)
    idx.add_items(c, labels)
    for thr in (tau, torch.from_numpy(tau).to(DEV)):
        lims, s, lab = idx.range_search(q, thr)
        _assert_matches_ref(lims.cpu().numpy(), s.cpu().numpy(), (lab.cpu().numpy() - 10_000) // 3, exact, ref)
    lims_n, lab_n, dist_n = idx.range_query(q, tau)
    np.testing.assert_array_equal(lims_n, lims.cpu().numpy())
    np.testing.assert_array_equal(lab_n, lab.cpu().numpy())
    np.testing.assert_array_equal(dist_n, (1.0 - s).cpu().numpy())
    with pytest.raises(ValueError):
        idx.range_search(q, tau[:-1])
    with pytest.raises(ValueError):
        GpuFlatIndex(space=space, dim=d, device=DEV).range_search(q, tau[:-1])      # an empty index checks the length too


class _RowModel:
    """encode_text by table lookup: sentence 'r<i>' is row i of a fixed matrix"""

    def __init__(self, rows):
        self.rows = torch.from_numpy(rows).to(DEV)

    def encode_text(self, texts, output_np=False):
        return self.rows[torch.tensor([int(t[1:]) for t in texts], device=DEV)]


@pytest.mark.parametrize("score_function", ["cosine", "dot"])
def test_mining_pipeline_mine_with_an_array(score_function):
    from text_similarity_amd.pipeline.search_pipeline import SentenceMiningPipeline
    sp, d = score_function, 100
    q, c, exact, tau, kinds, ref = _case(sp, d)
    # (mine builds Python tuples per hit: the three kinds that return thousands of rows are replaced by +inf here)
    heavy = np.array([k in ("minus_inf", "overflow", "below_all") for k in kinds])
    tau_m = np.where(heavy, np.float32(np.inf), tau).astype(np.float32)
    ref_m = [range_ref_q(exact[qi], tau_m[qi]) for qi in range(Q)]
    corpus = [f"r{j}" for j in range(N)]
    params = types.SimpleNamespace(device=torch.device(DEV))
    qt = torch.from_numpy(q).to(DEV)
    results = []
    for chunk in (N, 1700):                                 # one shot, and three chunks joined by ops.range_merge
        pipe = SentenceMiningPipeline(chunk, params, _RowModel(c), corpus=corpus, score_function=score_function)
        res = pipe.mine(qt, tau_m)
        assert sorted(res) == list(range(Q))
        for qi, r in enumerate(ref_m):
            assert [t[0] for t in res[qi]] == r.tolist(), qi
            assert [t[1] for t in res[qi]] == [corpus[j] for j in r]
            np.testing.assert_array_equal(np.array([t[2] for t in res[qi]], np.float32).view(np.uint32), exact[qi, r].view(np.uint32))
        results.append(res)
        # the device-level form with the full vector (whole-corpus queries included)
        lims, s, i = pipe.range_tensors(qt, torch.from_numpy(tau).to(DEV))
        _assert_matches_ref(lims.cpu().numpy(), s.cpu().numpy(), i.cpu().numpy(), exact, ref)
    assert results[0] == results[1]
    with pytest.raises(ValueError):
        pipe.mine(qt, tau[:5])
