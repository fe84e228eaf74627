"""One registry of small cases for the two contracts of include/tsim.h that cut across every entry point:

  1. a call does not depend on what its workspace held on entry (tests/test_workspace_poison_gpu.py), and
  2. all of its work is enqueued on the stream it is given (tests/test_side_stream_gpu.py).

A case names the C entries it must reach, makes seeded host operands for ``which`` in ("real", "decoy", "other"), runs the
Python op on device operands and states the expected output through the numpy restatements the suite already has (no oracle is
written here).  Everything a case computes on the device happens inside ``run`` — the operand preparation included — so that
the stream test can swap the operands' contents on the side stream in front of it.

Operands are a dict name -> numpy array.  Arrays of one or more dimensions become device tensors of the same shape and dtype;
0-d values (a scalar threshold, a row count) are host parameters and are handed to ``run`` as they are.

Decoys.  A decoy has the shapes of the real operands, so the workspace layout is the same, and is built so that whatever a call
on it leaves in the workspace would change the real result if it were read.  ``decoy_rule``:
  "beats"    the top-k searches in which rows can be planted: the real corpus in reversed row order with k rows per query
             (distinct rows for each query) replaced by copies of that query.  In every query the decoy's k-th best score
             strictly beats the real best score and the row ids differ.  Where the real best score is the largest value the
             space can give (the near-tie corpus under cosine: 1.0f), "strictly" is impossible and the scores are equal.
  "looser"   range search: the same data under a looser threshold (more hits in every query that has a finite threshold).
  "other"    other data of the same sizes (mst_prim, the community select, integer tables, inverted lists, whose result sets are
             bounded by the lists and cannot be beaten by planted rows): the decoy's outputs differ from the real ones.
tests/test_contract_cases_cpu.py asserts these conditions on the oracles alone.

Cases that name no workspace entry run in the stream test only: the stream-only entries, the encoder (one handle per slot, so
that two handles can run on two streams), CrossEncoder logits, the composite ops that read back mid-call (community_detection,
hdbscan) and the index classes, each built once on the default stream.  Two index oracles read the built index back (its list
assignment and probes, its graph and seeds), as those indexes' own tests do; the CPU test evaluates no index oracle."""
import functools
import os
import re

import numpy as np
import torch

import community_cases as cc
import graph_cases as gc
import graph_seed_cases as gsc
import hamming_cases as hm
import hdbscan_cases as hc
import int8_cases as i8
import ivf_cases as ivc
import ivfpq_cases as ic
import pq_cases as pc
import refine_cases as rc
from l2_cases import l2_dists, l2_topk_ref
from l2_range_cases import range_ref as l2_range_ref
from list_cases import csr, list_topk_ref
from oracle import encoder_ref, fp8_ref
from oracle.search_ref import _lane_sum, bf16_round, cos_sim, cosine_topk, cosine_topk_f32, exact_cosine, topk_rows, unit_rows
from test_range_search_gpu import dot_scores, range_ref
from test_search_boundary_gpu import _rows as boundary_rows
from text_similarity_amd import _lib, ops

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tsim.h")
WHICH = ("real", "decoy", "other")


def header_entries():
    """(entries with a `void *workspace` parameter, entries with a `void *stream` parameter), parsed from include/tsim.h."""
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    ws, st = [], []
    for m in re.finditer(r"\b(tsim_\w+)\s*\(([^;{}]*?)\)\s*;", text):
        name, params = m.group(1), m.group(2)
        if re.search(r"void\s*\*\s*workspace\b", params):
            ws.append(name)
        if re.search(r"void\s*\*\s*stream\b", params):
            st.append(name)
    return ws, st


class Case:
    """name; entries: the tsim_* functions a run must reach; operands(which) -> dict of host numpy; run(device operands) ->
    tuple of tensors; oracle(host operands) -> tuple of numpy arrays; check(got, want, which): raises unless the outputs (numpy)
    are the oracle's; workspace: None, or a callable giving the bytes the op asks ops._workspace for; host_sync: the Python op
    reads something back from the device mid-call."""

    def __init__(self, name, entries, operands, run, oracle, check=None, workspace=None, host_sync=False, decoy_rule=None,
                 decoy_check=None):
        self.name, self.entries, self._operands, self.run, self._oracle = name, tuple(entries), operands, run, oracle
        self.check = check or check_equal
        self.workspace, self.host_sync, self.decoy_rule, self.decoy_check = workspace, host_sync, decoy_rule, decoy_check
        self._cache = {}

    def operands(self, which):
        assert which in WHICH
        if ("ops", which) not in self._cache:
            o = {k: np.asarray(v) for k, v in self._operands(which).items()}
            for v in o.values():
                v.setflags(write=False)
            self._cache["ops", which] = o
        return self._cache["ops", which]

    def oracle(self, which):
        if ("ref", which) not in self._cache:      # computed once, shared by every test that needs it, never changed
            ref = tuple(np.asarray(a) for a in self._oracle(self.operands(which)))
            for a in ref:
                a.setflags(write=False)
            self._cache["ref", which] = ref
        return self._cache["ref", which]

    def __repr__(self):
        return self.name


def same(a, b):
    """equal bit for bit (floats by their bits, so NaN, the infinities and the zeros count)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype != b.dtype:      # (integers of two widths compare by value: a restatement's int64 against an op's int32)
        return a.dtype.kind in "iub" and b.dtype.kind in "iub" and bool((a.astype(np.int64) == b.astype(np.int64)).all())
    if a.dtype.kind == "f":
        u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return bool((np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)).all())
    return bool((a == b).all())


def check_equal(got, want, which="real"):
    assert len(got) == len(want), (len(got), len(want))
    for j, (g, w) in enumerate(zip(got, want)):
        assert same(g, w), (f"output {j} ({which})", g.shape, g.dtype, w.shape, w.dtype,
                            np.argwhere(np.asarray(g).reshape(-1) != np.asarray(w).reshape(-1))[:5].tolist() if g.shape == w.shape else None)


CASES = []


def _add(*a, **kw):
    c = Case(*a, **kw)
    assert c.name not in {x.name for x in CASES}, c.name
    CASES.append(c)
    return c


def lib():
    return _lib.lib()


def _stream_handle(t):
    return torch.cuda.current_stream(t.device).cuda_stream


# ================================================================================================ decoys of the top-k searches
def plant(q, c, k, rows=None, first=7):
    """The real corpus in reversed row order, with k rows per query (distinct rows for each query) replaced by ``rows[j]``
    (default: copies of query j)."""
    rows = q if rows is None else rows
    c2 = np.ascontiguousarray(c[::-1]).copy()
    assert first + q.shape[0] * k <= c.shape[0], "the corpus is too small to plant k rows per query"
    for j in range(q.shape[0]):
        c2[first + j * k:first + (j + 1) * k] = rows[j]
    return c2


def near_ties(c2, q, at, n=64):
    """Behind the planted copies, n adjacent near-copies of query 0: more near-ties than one partial list holds, so the decoy's
    query 0 is flagged and widened — its run leaves NON-ZERO control words, slot counters and flag lists behind, which is what the
    clear in front of the main pass (the memset, or the pre-pass threshold kernel) must remove.  With exact copies alone the
    decoy resolves in the first pass and a missing clear goes unnoticed."""
    assert at + n <= c2.shape[0]
    c2[at:at + n] = q[0] * (1 + 1e-6 * np.random.default_rng(at).standard_normal((n, q.shape[1]))).astype(np.float32)


def topk_decoy_check(ascending=False, top=None, rows=None):
    """decoy_check of rule "beats" on (scores [Q, k], idx [Q, k], ...) oracles.  top: the largest score the space can give."""
    def chk(real, decoy):
        rs, ri, ds, di = real[0], real[1], decoy[0], decoy[1]
        sel = np.arange(rs.shape[0]) if rows is None else np.asarray(rows)
        for j in sel:
            kth, best = ds[j, -1], rs[j, 0]
            if ascending:
                assert kth < best, (j, kth, best)
            elif top is not None and best == top:
                assert kth == top, (j, kth, best)
            else:
                assert kth > best, (j, kth, best)
            assert (di[j] != ri[j]).any(), j
    return chk


def differs(real, decoy):
    assert not all(same(a, b) for a, b in zip(real, decoy))


# ================================================================================================ flat search
FLAT_D, FLAT_Q = 256, 8


def _flat_operands(corpus, k, plant_k):
    def operands(which):
        q, c = boundary_rows(corpus)
        if which == "decoy":
            c2 = plant(q, c, plant_k)
            if k <= 28:            # (k > 28 flags every query anyway; the small corpus has no room and no k <= 28 case)
                near_ties(c2, q, 7 + q.shape[0] * plant_k)
            return {"q": q, "c": c2}
        if which == "other":       # (query 0 stays where it is: on the near-tie corpus it is the one that takes brute force)
            q2 = q.copy()
            q2[1:] = q[1:][::-1]
            return {"q": q2, "c": np.roll(c, 3, axis=0)}
        return {"q": q, "c": c}
    return operands


def flat_search(space, t, d, k):
    qf, cf = t["q"], t["c"]
    if space == "dot":
        cn, rho, scale = ops.dot_scaled_rows(cf)
        return ops.dot_topk(ops.l2norm_rows(qf), cn, d, k, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale, return_status=True)
    if space == "l2":
        cn, rho, scale = ops.l2_rows(cf)
        return ops.l2_topk(ops.l2_query_rows(qf, scale), cn, d, k, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale, return_status=True)
    cu, rho = ops.l2norm_rows(cf, return_rho=True)
    if space == "unit":
        return ops.cosine_topk(ops.l2norm_rows(qf), cu, d, k, rho_c=rho, return_status=True)
    return ops.cosine_topk(ops.l2norm_rows(qf), cu, d, k, eq_f32=qf, ec_f32=cf, rho_c=rho, return_status=True)


def flat_oracle(space, q, c, k):
    if space == "cosine":
        return cosine_topk_f32(q, c, k)
    if space == "unit":
        return cosine_topk(unit_rows(q), unit_rows(c), k)
    if space == "l2":
        return l2_topk_ref(q, c, k)
    return topk_rows(_lane_sum(q[:, None, :], c[None, :, :]).astype(np.float32), k)      # (test_search_boundary_gpu._oracle_widest)


def _flat_check(route):
    """scores and ids are the oracle's; the status words are those of the route (tests/test_search_boundary_gpu.py) — on the real
    and the other operands; the decoy's planted ties may take another pass."""
    def check(got, want, which="real"):
        check_equal(got[:2], want, which)
        st = got[2]
        if which != "decoy":
            assert route(st), (which, st.tolist())
    return check


FLAT_ROUTES = {
    "list": lambda st: bool((st <= 1).all()),            # k <= 28 on Gaussian rows: the list kernels, some queries widened
    "widen": lambda st: bool((st == 1).all()),           # k > 28 on Gaussian rows: block-maxima bound, widening resolves
    "brute0": lambda st: bool(st[0] == 2),               # query 0 of the near-tie corpus overflows its slot: brute force
    "brute": lambda st: bool((st == 2).all()),           # k > 28 on a shard too small for the bound: every query brute force
}
FLAT_ENTRIES = {
    ("cosine", False): ("tsim_l2norm_rows", "tsim_cosine_topk_ex"), ("cosine", True): ("tsim_l2norm_rows", "tsim_cosine_topk_large"),
    ("unit", False): ("tsim_l2norm_rows", "tsim_cosine_topk_ex"), ("unit", True): ("tsim_l2norm_rows", "tsim_cosine_topk_large"),
    ("dot", False): ("tsim_l2norm_rows", "tsim_max_norm_rows", "tsim_dot_scaled_rows", "tsim_dot_topk_ex"),
    ("dot", True): ("tsim_l2norm_rows", "tsim_max_norm_rows", "tsim_dot_scaled_rows", "tsim_dot_topk_large"),
    ("l2", False): ("tsim_max_norm_rows", "tsim_l2_rows", "tsim_l2_query_rows", "tsim_l2_topk_ex"),
    ("l2", True): ("tsim_max_norm_rows", "tsim_l2_rows", "tsim_l2_query_rows", "tsim_l2_topk_large"),
}


def _flat_case(corpus, space, k, route):
    n = boundary_rows(corpus)[1].shape[0]
    _add(f"flat-{corpus}-{space}-k{k}", FLAT_ENTRIES[space, k > 64], _flat_operands(corpus, k, k),
         lambda t: flat_search(space, t, FLAT_D, k), lambda h: flat_oracle(space, h["q"], h["c"], k), check=_flat_check(FLAT_ROUTES[route]),
         workspace=lambda: (lib().tsim_topk_large_workspace_bytes if k > 64 else lib().tsim_cosine_topk_workspace_bytes)(FLAT_Q, n, k),
         decoy_rule="beats",
         decoy_check=topk_decoy_check(ascending=space == "l2", top=np.float32(1.0) if space == "cosine" else None))


_flat_case("gauss", "cosine", 10, "list")
_flat_case("gauss", "cosine", 29, "widen")
_flat_case("gauss", "cosine", 128, "widen")
_flat_case("near_ties", "cosine", 10, "brute0")
_flat_case("small", "cosine", 65, "brute")
for _space in ("dot", "l2", "unit"):
    _flat_case("gauss", _space, 10, "list")
    _flat_case("gauss", _space, 65, "widen")


def _plain_cosine_topk(t, k=10):
    """tsim_cosine_topk through the C ABI (no Python op calls it): unit rows only, no status, on the stream's cached workspace"""
    L = lib()
    qu, cu = ops.l2norm_rows(t["q"]), ops.l2norm_rows(t["c"])
    dev = qu.device
    Q, N = qu.shape[0], cu.shape[0]
    with torch.cuda.device(dev):
        s = torch.empty((Q, k), dtype=torch.float32, device=dev)
        i = torch.empty((Q, k), dtype=torch.int64, device=dev)
        ws = ops._workspace(dev, L.tsim_cosine_topk_workspace_bytes(Q, N, k))
        _lib.check(L.tsim_cosine_topk(qu.data_ptr(), Q, cu.data_ptr(), N, FLAT_D, qu.shape[1], k, s.data_ptr(), i.data_ptr(), 0,
                                      ws.data_ptr(), ws.numel(), _stream_handle(qu)), "cosine_topk")
    return s, i


_add("flat-gauss-unit-k10-plain", ("tsim_l2norm_rows", "tsim_cosine_topk"), _flat_operands("gauss", 10, 10), _plain_cosine_topk,
     lambda h: flat_oracle("unit", h["q"], h["c"], 10), workspace=lambda: lib().tsim_cosine_topk_workspace_bytes(FLAT_Q, 6000, 10),
     decoy_rule="beats", decoy_check=topk_decoy_check())


# ---------------------------------------------------------------------------------- the two routes only a large shard reaches
BIG_D, BIG_K = 64, 10


@functools.lru_cache(maxsize=None)
def _big_rows(n, nq, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((n, BIG_D), dtype=np.float32)
    q = rng.standard_normal((nq, BIG_D), dtype=np.float32)
    return q, c


def _big_operands(n, nq, seed):
    def operands(which):
        q, c = _big_rows(n, nq, seed)
        if which == "decoy":
            c2 = plant(q, c, BIG_K)
            near_ties(c2, q, 7 + q.shape[0] * BIG_K)
            return {"q": q, "c": c2}
        if which == "other":
            return {"q": np.ascontiguousarray(q[::-1]), "c": np.roll(c, 5, axis=0)}
        return {"q": q, "c": c}
    return operands


def _big_check(sel):
    def check(got, want, which="real"):
        check_equal((got[0][sel], got[1][sel]), want, which)
        assert np.isin(got[2], (0, 1)).all(), got[2]          # Gaussian rows: no query needs brute force
    return check


def _big_oracle(q, c, k):
    """oracle.search_ref.cosine_topk_f32 of every query over the rows that can be in its top-k.  The rows are chosen by a float64
    BLAS cosine with a margin: a row of the float32 top-k scores at least the k-th float32 score, a float32 score differs from
    the float64 value by at most 2^-24 (|s| <= 1) and the BLAS sum from the lane-ordered one by ~1e-15, so every such row has a
    BLAS cosine above (k-th largest BLAS cosine) - 2^-23 - 1e-12; the margin is 1e-6.  The rows keep their order, so ties still go
    to the lower index.  (cosine_topk_f32 over all rows gives the same and takes 17 s a call at these sizes.)"""
    qn = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True)
    cn = c.astype(np.float64) / np.linalg.norm(c.astype(np.float64), axis=1, keepdims=True)
    S, I = np.empty((q.shape[0], k), np.float32), np.empty((q.shape[0], k), np.int64)
    for j in range(q.shape[0]):
        sim = cn @ qn[j]
        rows = np.flatnonzero(sim >= np.partition(sim, -k)[-k] - 1e-6)
        s, i = cosine_topk_f32(q[j:j + 1], c[rows], k)
        S[j], I[j] = s[0], rows[i[0]]
    return S, I


def _big_case(name, n, nq, seed, sel):
    sel = np.asarray(sel)
    _add(name, ("tsim_l2norm_rows", "tsim_cosine_topk_ex"), _big_operands(n, nq, seed), lambda t: flat_search("cosine", t, BIG_D, BIG_K),
         lambda h: _big_oracle(h["q"][sel], h["c"], BIG_K), check=_big_check(sel),
         workspace=lambda: lib().tsim_cosine_topk_workspace_bytes(nq, n, BIG_K), decoy_rule="beats",
         decoy_check=topk_decoy_check())


# plan_prepass needs N >= 262 144: the threshold kernel of the pre-pass clears the control words, not the memset
_big_case("flat-prepass", 262144, 8, 31, np.arange(8))
# plan_two_phase needs N >= 4 x 131 072 and Q > 768: the lists of both phases side by side.  The oracle runs on four queries (as
# tests/test_range_search_gpu.py does at this size); all 769 must be bit-equal across the poison kinds.
_big_case("flat-two-phase", 524288, 769, 32, [0, 255, 256, 768])


# ================================================================================================ range search
RANGE_N, RANGE_D, RANGE_Q = 3000, 128, 8
RANGE_RANK = {"real": 5, "decoy": 60, "other": 20}        # the threshold is query 0's exact score at this rank: '>=' meets a tie


@functools.lru_cache(maxsize=None)
def _range_rows():
    """Gaussian rows; 2 200 rows around one direction v, and query 1 = v: more than TSIM_RANGE_SLOT_CAP hits under any threshold
    that is selective for the Gaussian queries (status 2), while query 0 is selective (status 1)."""
    rng = np.random.default_rng(77)
    c = rng.standard_normal((RANGE_N, RANGE_D)).astype(np.float32)
    q = rng.standard_normal((RANGE_Q, RANGE_D)).astype(np.float32)
    v = rng.standard_normal(RANGE_D).astype(np.float32)
    c[500:2700] = v + 0.05 * rng.standard_normal((2200, RANGE_D)).astype(np.float32)
    q[1] = v
    return q, c


@functools.lru_cache(maxsize=None)
def _range_exact(space, other):
    q, c = _range_rows()
    if other:
        q = np.ascontiguousarray(q[::-1])
    return exact_cosine(q, c) if space == "cosine" else dot_scores(q, c) if space == "dot" else l2_dists(q, c)


def _range_operands(space, per_query):
    def operands(which):
        q, c = _range_rows()
        other = which == "other"
        if other:
            q = np.ascontiguousarray(q[::-1])
        ex = _range_exact(space, other)
        row = ex[7 if other else 0]                            # the selective query the threshold is taken from
        tau = np.sort(row)[RANGE_RANK[which]] if space == "l2" else np.sort(row)[::-1][RANGE_RANK[which]]
        if per_query:
            tau = np.full((RANGE_Q,), tau, dtype=np.float32)
            tau[2] = np.inf if space == "l2" else -np.inf      # every row, through the exact pass
        return {"q": q, "c": c, "tau": np.float32(tau) if not per_query else tau, "other": np.bool_(other)}
    return operands


def _range_run(space):
    def run(t):
        qf, cf, tau = t["q"], t["c"], t["tau"]
        tau = float(tau) if not isinstance(tau, torch.Tensor) else tau
        if space == "cosine":
            cn, rho = ops.l2norm_rows(cf, return_rho=True)
            return ops.cosine_range(ops.l2norm_rows(qf), cn, RANGE_D, tau, eq_f32=qf, ec_f32=cf, rho_c=rho, return_status=True)
        if space == "dot":
            cn, rho, scale = ops.dot_scaled_rows(cf)
            return ops.dot_range(ops.l2norm_rows(qf), cn, RANGE_D, tau, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale, return_status=True)
        cn, rho, scale = ops.l2_rows(cf)
        return ops.l2_range(ops.l2_query_rows(qf, scale), cn, RANGE_D, tau, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale,
                            return_status=True)
    return run


def _range_oracle(space):
    def oracle(h):
        ex = _range_exact(space, bool(h["other"]))
        taus = np.broadcast_to(h["tau"], (RANGE_Q,))
        hits = [l2_range_ref(ex[j], taus[j]) if space == "l2" else range_ref(ex[j:j + 1], taus[j])[0] for j in range(RANGE_Q)]
        lims = np.zeros((RANGE_Q + 1,), np.int64)
        lims[1:] = np.cumsum([len(x) for x in hits])
        # status: 2 where no finite threshold exists or the slot overflows (the hits alone exceed it), else 1 (the Gaussian
        # queries collect a few dozen rows)
        st = np.array([2 if (len(x) > ops.RANGE_SLOT_CAP or np.isinf(taus[j])) else 1 for j, x in enumerate(hits)], np.int32)
        return (lims, np.concatenate([ex[j, x] for j, x in enumerate(hits)]).astype(np.float32),
                np.concatenate(hits).astype(np.int64), st)
    return oracle


def _range_decoy_check(real, decoy):
    rn, dn = np.diff(real[0]), np.diff(decoy[0])
    assert (dn >= rn).all() and dn[0] > rn[0] and dn.sum() > rn.sum()


RANGE_ENTRIES = {
    ("cosine", False): ("tsim_l2norm_rows", "tsim_cosine_range_scan", "tsim_range_fill"),
    ("cosine", True): ("tsim_l2norm_rows", "tsim_cosine_range_scan_tau", "tsim_range_fill_tau"),
    ("dot", False): ("tsim_dot_scaled_rows", "tsim_dot_range_scan", "tsim_range_fill"),
    ("dot", True): ("tsim_dot_scaled_rows", "tsim_dot_range_scan_tau", "tsim_range_fill_tau"),
    ("l2", False): ("tsim_l2_rows", "tsim_l2_query_rows", "tsim_l2_range_scan", "tsim_range_fill"),
    ("l2", True): ("tsim_l2_rows", "tsim_l2_query_rows", "tsim_l2_range_scan_tau", "tsim_range_fill_tau"),
}
for _space in ("cosine", "dot", "l2"):
    for _pq in (False, True):
        (lambda space, per_query: _add(
            f"range-{space}-{'tau_q' if per_query else 'tau'}", RANGE_ENTRIES[space, per_query], _range_operands(space, per_query),
            _range_run(space), _range_oracle(space), workspace=lambda: lib().tsim_range_workspace_bytes(RANGE_Q, RANGE_N),
            host_sync=True, decoy_rule="looser", decoy_check=_range_decoy_check))(_space, _pq)


# ================================================================================================ list search
LIST_N, LIST_D, LIST_LENGTHS = 9000, 65, (0, 1, 1025, 3000, 3000)


@functools.lru_cache(maxsize=None)
def _list_rows(seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((LIST_N, LIST_D)).astype(np.float32)
    q = rng.standard_normal((len(LIST_LENGTHS), LIST_D)).astype(np.float32)
    perm = rng.permutation(LIST_N)                             # disjoint lists of distinct rows
    at = np.concatenate([[0], np.cumsum(LIST_LENGTHS)])
    return q, c, [perm[at[j]:at[j + 1]] for j in range(len(LIST_LENGTHS))]


def _list_operands(k, half):
    def operands(which):
        q, c, lists = _list_rows(41 if which != "other" else 42)
        if which == "decoy":                                   # the first k rows of every list that has k become the query
            c = np.ascontiguousarray(c[::-1]).copy()
            for j, rows in enumerate(lists):
                if len(rows) >= k:
                    c[rows[:k]] = q[j]
        cand, lims = csr(lists)
        if half:                                               # the refine stage's row store: IEEE half rows
            c = c.astype(np.float16)
        return {"q": q, "c": c, "cand": cand, "lims": lims}
    return operands


def _list_run(fn, k):
    return lambda t: fn(t["q"], t["c"], t["cand"], t["lims"], k=k, return_status=True, assume_unique=True)


def _list_oracle(space, k):
    def oracle(h):
        lists = [h["cand"][h["lims"][j]:h["lims"][j + 1]] for j in range(len(LIST_LENGTHS))]
        return list_topk_ref(space, h["q"], h["c"].astype(np.float32), lists, k, unique=False)
    return oracle


def _list_ws(k):
    return lambda: lib().tsim_list_topk_workspace_bytes(len(LIST_LENGTHS), sum(LIST_LENGTHS), k)


for _k in (10, 65):
    _full = [j for j, n in enumerate(LIST_LENGTHS) if n >= _k]
    for _space, _fn, _entry in (("cosine", ops.cosine_list_topk, "tsim_cosine_list_topk"), ("dot", ops.dot_list_topk, "tsim_dot_list_topk"),
                                ("l2", ops.l2_list_topk, "tsim_l2_list_topk")):
        _add(f"list-{_space}-k{_k}", (_entry,), _list_operands(_k, False), _list_run(_fn, _k), _list_oracle(_space, _k),
             workspace=_list_ws(_k), decoy_rule="beats", decoy_check=topk_decoy_check(ascending=_space == "l2", rows=_full))
    _f16 = "cosine" if _k == 10 else "l2"
    _add(f"list-f16-{_f16}-k{_k}", ("tsim_list_topk_f16",), _list_operands(_k, True),
         _list_run(functools.partial(ops.f16_list_topk, _f16), _k), _list_oracle(_f16, _k), workspace=_list_ws(_k), decoy_rule="beats",
         decoy_check=topk_decoy_check(ascending=_f16 == "l2", rows=_full))


# ================================================================================================ code searches
CODE_SHAPES = ((65, 1025, 33, 10), (384, 70000, 3, 10))        # (d, N, Q, k): a short last chunk; many chunks


@functools.lru_cache(maxsize=None)
def _code_rows(d, n, nq, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((nq, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)


def _code_operands(d, n, nq, k, int8):
    def operands(which):
        q, c = _code_rows(d, n, nq, 900 + d + (which == "other"))
        out = {"q": q, "c": c}
        if int8:
            out["ranges"] = i8.ranges_of(c)                    # (the real corpus' calibration, also for the decoy's planted rows)
        if which == "decoy":       # Hamming: copies of the query (distance 0); int8: its signs far out of range (codes +-127 / -128)
            out["c"] = plant(q, c, k, rows=(np.where(q > 0, 1e3, -1e3).astype(np.float32) if int8 else None))
        return out
    return operands


def _hamming_run(d, k):
    return lambda t: ops.hamming_topk(ops.pack_sign_rows(t["q"]), ops.pack_sign_rows(t["c"]), d, k)


def _int8_run(d, k):
    return lambda t: ops.int8_ip_topk(ops.quantize_int8_rows(t["q"], t["ranges"]), ops.quantize_int8_rows(t["c"], t["ranges"]), d, k)


for _d, _n, _q, _k in CODE_SHAPES:
    (lambda d, n, nq, k: (
        _add(f"hamming-d{d}-n{n}", ("tsim_pack_sign_rows", "tsim_hamming_topk"), _code_operands(d, n, nq, k, False), _hamming_run(d, k),
             lambda h: hm.hamming_topk_ref(hm.pack_ref(h["q"]), hm.pack_ref(h["c"]), d, k),
             workspace=lambda: lib().tsim_hamming_topk_workspace_bytes(nq, n, k), decoy_rule="beats",
             decoy_check=topk_decoy_check(ascending=True)),
        _add(f"int8-d{d}-n{n}", ("tsim_quantize_int8_rows", "tsim_int8_ip_topk"), _code_operands(d, n, nq, k, True), _int8_run(d, k),
             lambda h: i8.ip_topk_ref(i8.quantize_ref(h["q"], h["ranges"]), i8.quantize_ref(h["c"], h["ranges"]), d, k),
             workspace=lambda: lib().tsim_int8_ip_topk_workspace_bytes(nq, n, k), decoy_rule="beats",
             decoy_check=topk_decoy_check())))(_d, _n, _q, _k)


# the two smallest ADC_CASES of tests/test_pq_gpu.py (an empty corpus; k > N) and the smallest that fills its lists:
# (N, Q, k, M, space, tables, codes)
ADC_SMALL = ((0, 1, 10, 3, "ip", "random", "uniform"), (1, 5, 10, 16, "l2", "random", "uniform"), (255, 17, 64, 17, "ip", "small", "binary"))


def _adc_operands(i):
    n, nq, k, M, space, tk, ck = ADC_SMALL[i]

    def operands(which):
        rng = np.random.default_rng(50 + i + 100 * WHICH.index(which))
        tables = {"random": pc.random_tables, "small": pc.small_tables}[tk](rng, nq, M, space)
        codes = (pc.uniform_codes if ck == "uniform" else pc.binary_codes)(rng, n, M)
        assert (pc.table_bound(tables) <= 2 ** 24).all()
        return {"tables": tables, "codes": pc.pad_codes(codes)}
    return operands


for _i, (_n, _q, _k, _M, _space, _tk, _ck) in enumerate(ADC_SMALL):
    (lambda i, n, nq, k, M, space: _add(
        f"pq-adc-n{n}", ("tsim_pq_adc_topk",), _adc_operands(i), lambda t: ops.pq_adc_topk_tables(t["tables"], t["codes"], k, space),
        lambda h: pc.adc_topk_ref(h["tables"], h["codes"], k, space), workspace=lambda: lib().tsim_pq_adc_topk_workspace_bytes(nq, n, M, k),
        decoy_rule="other", decoy_check=differs if n else None))(_i, _n, _q, _k, _M, _space)


# ================================================================================================ inverted lists
IVF_LENGTHS = (63, 0, 1, 513, 130)                              # an empty list; one row; a segment and one row (TSIM_IVF_SEG = 512)
IVF_D, IVF_Q, IVF_K = 64, 5, 10
IVF_PROBES = np.array([[1, 0, 3], [3, 4, 2], [1, 1, 1], [2, 1, 4], [0, 3, 4]], np.int64)      # query 2 probes the empty list alone


def _ivf_operands(which):
    rng = np.random.default_rng(60 + WHICH.index(which))
    ln = rng.permutation(np.repeat(np.arange(len(IVF_LENGTHS)), IVF_LENGTHS))
    rows = rng.standard_normal((ln.shape[0], IVF_D)).astype(np.float32)
    q = rng.standard_normal((IVF_Q, IVF_D)).astype(np.float32)
    order, off, ids = ivc.pack_ref(ln, len(IVF_LENGTHS))
    ids = ids.copy()
    ids[::7] = -1 - ids[::7]                                    # tombstones: every seventh position
    return {"q": q, "rows": rows[order], "off": off, "ids": ids, "probes": IVF_PROBES}


def _ivf_oracle(space):
    def oracle(h):
        rows, ln = ivc.arrival_from_packed(h["rows"], h["off"], h["ids"])
        return ivc.ivf_ref(space, h["q"], rows, ln, h["probes"], IVF_K, nlist=len(IVF_LENGTHS))
    return oracle


for _space in ("cosine", "l2"):
    (lambda space: _add(
        f"ivf-scan-{space}", ("tsim_ivf_scan_topk",), _ivf_operands,
        lambda t: ops.ivf_scan_topk(space, t["q"], t["rows"], t["off"], t["ids"], t["probes"], IVF_K, return_status=True,
                                    max_list_len=max(IVF_LENGTHS)),
        _ivf_oracle(space), workspace=lambda: lib().tsim_ivf_scan_workspace_bytes(IVF_Q, IVF_PROBES.shape[1], max(IVF_LENGTHS), IVF_K),
        decoy_rule="other", decoy_check=differs))(_space)

PQL_LENGTHS = (257, 0, 1, 255, 300)
PQL_M, PQL_K = 17, 10
PQL_PROBES = np.array([[1, 0, 3], [3, 4, 2], [1, 1, -1], [2, 1, 4]], np.int64)


def _ivfpq_scan_operands(space):
    def operands(which):
        rng = np.random.default_rng(70 + WHICH.index(which))
        off = np.concatenate([[0], np.cumsum(PQL_LENGTHS)]).astype(np.int64)
        n = int(off[-1])
        nq, nprobe = PQL_PROBES.shape
        tables = (pc.random_tables(rng, nq * nprobe, PQL_M, space) // 2).reshape(nq, nprobe, PQL_M, 256)
        bias = rng.integers(-(1 << 22), (1 << 22) + 1, size=(nq, nprobe))
        bias = (-np.abs(bias) if space == "l2" else bias).astype(np.int32)
        assert (ic.score_bound(tables, bias) < 2 ** 24).all()
        return {"tables": tables, "bias": bias, "codes": pc.pad_codes(pc.uniform_codes(rng, n, PQL_M)), "off": off,
                "ids": ic.ids_with_tombstones(rng, n), "probes": PQL_PROBES}
    return operands


for _space in ("ip", "l2"):
    (lambda space: _add(
        f"ivfpq-scan-{space}", ("tsim_ivfpq_scan_topk",), _ivfpq_scan_operands(space),
        lambda t: ops.ivfpq_scan_topk(space, t["tables"], t["bias"], t["codes"], t["off"], t["ids"], t["probes"], PQL_K,
                                      return_status=True, max_list_len=max(PQL_LENGTHS)),
        lambda h: ic.scan_ref(h["tables"], h["bias"], h["codes"], h["off"], h["ids"], h["probes"], PQL_K, space),
        workspace=lambda: lib().tsim_ivfpq_scan_workspace_bytes(PQL_PROBES.shape[0], PQL_PROBES.shape[1], max(PQL_LENGTHS), PQL_K),
        decoy_rule="other", decoy_check=differs))(_space)

TBL_D, TBL_M, TBL_Q, TBL_NLIST, TBL_NPROBE = 12, 3, 5, 7, 4


def _ivfpq_tables_operands(which):
    rng = np.random.default_rng(80 + WHICH.index(which))
    probes = np.stack([rng.permutation(TBL_NLIST)[:TBL_NPROBE] for _ in range(TBL_Q)]).astype(np.int64)
    probes[0, 1], probes[4, 0] = -1, TBL_NLIST + 3              # padding pairs: their tables are not written
    return {"q": rng.standard_normal((TBL_Q, TBL_D)).astype(np.float32),
            "cent": (3 * rng.standard_normal((TBL_NLIST, TBL_D))).astype(np.float32), "probes": probes,
            "cb": pc.random_codebooks(rng, TBL_D, TBL_M)}


def _ivfpq_tables_run(t):
    tables, _, exps = ops.ivfpq_tables(t["q"], t["cent"], t["probes"], t["cb"], "l2")
    ok = (t["probes"] >= 0) & (t["probes"] < TBL_NLIST)
    return torch.where(ok[:, :, None, None], tables, torch.zeros_like(tables)), exps      # (padding pairs: unwritten memory)


def _ivfpq_tables_oracle(h):
    wt, we = ic.tables_l2_ref(h["q"], h["cent"], h["probes"], h["cb"])
    return np.where(ic.valid_probes(h["probes"], TBL_NLIST)[:, :, None, None], wt, 0).astype(np.int32), we


# l2 is the only space whose tables use the workspace (the per-pair maxima)
_add("ivfpq-tables-l2", ("tsim_ivfpq_tables",), _ivfpq_tables_operands, _ivfpq_tables_run, _ivfpq_tables_oracle,
     workspace=lambda: lib().tsim_ivfpq_tables_workspace_bytes(TBL_Q, TBL_NPROBE), decoy_rule="other", decoy_check=differs)


# ================================================================================================ mst_prim
MST_N, MST_D = 257, 33


def _mst_operands(core):
    def operands(which):
        rows = np.random.default_rng(90 + WHICH.index(which)).standard_normal((MST_N, MST_D)).astype(np.float32)
        return {"rows": rows, "core2": hc.core2_ref(rows, 4)} if core else {"rows": rows}
    return operands


for _core in (False, True):
    _add("mst-prim-core" if _core else "mst-prim", ("tsim_mst_prim",), _mst_operands(_core),
         lambda t: ops.mst_prim(t["rows"], t.get("core2")), lambda h: hc.mst_ref(h["rows"], h.get("core2")),
         workspace=lambda: lib().tsim_mst_prim_workspace_bytes(MST_N), decoy_rule="other", decoy_check=differs)


# ================================================================================================ community select (C ABI)
def _community_lists(kind):
    if kind == "chain":                                         # a chain of 40 needs 40 rounds: three are run, the serial finish decides the rest
        return cc.chain_case(40, 12) + (5,)
    return cc.random_case(np.random.default_rng(7), 2000, 5000, 120), 5000, 10


def _community_operands(kind):
    def operands(which):
        lists, n, min_size = _community_lists(kind)
        if which != "real":                                     # other data of the same sizes: every list keeps its length
            rng = np.random.default_rng(95 + WHICH.index(which))
            lists = [rng.permutation(n)[:len(x)] for x in lists]
        lims, mem = cc.csr(lists)
        return {"lims": np.asarray(lims, np.int64), "members": np.asarray(mem, np.int32), "N": np.int64(n), "min_size": np.int64(min_size)}
    return operands


COMMUNITY_ROUNDS = 3


def _community_run(t):
    """tsim_community_select_rounds then _finish through the C ABI on the cached workspace of the stream (ops.community_select
    allocates a private one, which the cache cannot poison); nothing is read back in between."""
    L = lib()
    lims, mem, n, min_size = t["lims"], t["members"], int(t["N"]), int(t["min_size"])
    dev = lims.device
    C, T = lims.numel() - 1, mem.numel()
    with torch.cuda.device(dev):
        accept = torch.zeros((C,), dtype=torch.int32, device=dev)
        keep = torch.zeros((T,), dtype=torch.uint8, device=dev)
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
        left = torch.zeros((COMMUNITY_ROUNDS,), dtype=torch.int32, device=dev)
        ws = ops._workspace(dev, L.tsim_community_select_workspace_bytes(C, n))
        head = (lims.data_ptr(), mem.data_ptr(), C, T, n, min_size)
        tail = (accept.data_ptr(), keep.data_ptr(), status.data_ptr(), left.data_ptr(), ws.data_ptr(), ws.numel(), _stream_handle(lims))
        _lib.check(L.tsim_community_select_rounds(*head, 0, COMMUNITY_ROUNDS, *tail), "community_select_rounds")
        _lib.check(L.tsim_community_select_finish(*head, *tail), "community_select_finish")
    return accept, keep, status


def _community_oracle(h):
    a, k, st = cc.select_ref(h["lims"], h["members"], int(h["N"]), int(h["min_size"]))
    return np.asarray(a, np.int32), np.asarray(k, np.uint8), np.array([st], np.int32)


def _community_ws(kind):
    def nbytes():
        lists, n, _ = _community_lists(kind)
        return lib().tsim_community_select_workspace_bytes(len(lists), n)
    return nbytes


for _kind in ("chain", "random"):
    _add(f"community-{_kind}", ("tsim_community_select_rounds", "tsim_community_select_finish"), _community_operands(_kind),
         _community_run, _community_oracle, workspace=_community_ws(_kind), decoy_rule="other", decoy_check=differs)


# ================================================================================================ stream-only entries
def _merge_lists(rng, nlists, nq, k, asc=False):
    """nlists sorted top-k lists of the same nq queries over disjoint row sets"""
    s = rng.standard_normal((nlists, nq, k)).astype(np.float32)
    s = np.sort(s, axis=2) if asc else -np.sort(-s, axis=2)
    i = np.stack([rng.permutation(100000)[:nlists * k].reshape(nlists, k) for _ in range(nq)], axis=1).astype(np.int64)
    return s, i


def _topk_merge_case(k_in, k_out):
    def operands(which):
        s, i = _merge_lists(np.random.default_rng(300 + k_out + WHICH.index(which)), 3, 9, k_in)
        return {"s": s, "i": i}

    def oracle(h):      # the union ranked by (score desc, index asc): oracle.search_ref.topk_rows over the concatenated lists
        s = np.concatenate(list(h["s"]), axis=1)
        i = np.concatenate(list(h["i"]), axis=1)
        o = np.lexsort((i, -s.astype(np.float64)), axis=1)[:, :k_out]
        return np.take_along_axis(s, o, 1), np.take_along_axis(i, o, 1)
    _add(f"topk-merge-k{k_out}", ("tsim_topk_merge_strided",), operands, lambda t: ops.topk_merge(t["s"], t["i"], k_out), oracle,
         decoy_rule="other", decoy_check=differs)


_topk_merge_case(40, 40)         # k <= 64: the wave-max kernel
_topk_merge_case(100, 100)       # k > 64: the sort-and-merge kernel


def _range_merge_case(asc):
    nq = 6

    def operands(which):
        rng, shape_rng = np.random.default_rng(320 + asc + 10 * WHICH.index(which)), np.random.default_rng(319)
        out = {}
        for r in range(3):       # three shards of disjoint global indices, segments of any length, also 0
            lens = shape_rng.integers(0, 40, size=nq)
            lens[r] = 0
            lims = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
            s = rng.standard_normal(int(lims[-1])).astype(np.float32)
            for j in range(nq):
                seg = np.sort(s[lims[j]:lims[j + 1]])
                s[lims[j]:lims[j + 1]] = seg if asc else seg[::-1]
            out[f"lims{r}"], out[f"s{r}"], out[f"i{r}"] = lims, s, (rng.permutation(5000)[:s.size] * 3 + r).astype(np.int64)
        return out

    def run(t):
        res = [(t[f"lims{r}"], t[f"s{r}"], t[f"i{r}"]) for r in range(3)]
        return ops.range_merge(res, total=sum(int(r[1].numel()) for r in res), ascending=asc)

    def oracle(h):
        segs_s, segs_i, lims = [], [], [0]
        for j in range(nq):
            s = np.concatenate([h[f"s{r}"][h[f"lims{r}"][j]:h[f"lims{r}"][j + 1]] for r in range(3)])
            i = np.concatenate([h[f"i{r}"][h[f"lims{r}"][j]:h[f"lims{r}"][j + 1]] for r in range(3)])
            o = np.lexsort((i, s.astype(np.float64) if asc else -s.astype(np.float64)))
            segs_s.append(s[o]), segs_i.append(i[o]), lims.append(lims[-1] + s.size)
        return np.asarray(lims, np.int64), np.concatenate(segs_s), np.concatenate(segs_i)
    _add("range-merge-asc" if asc else "range-merge", ("tsim_range_merge_asc" if asc else "tsim_range_merge",), operands, run, oracle,
         decoy_rule="other", decoy_check=differs)


_range_merge_case(False)
_range_merge_case(True)


def _rescore_case(name, entry, op, ref, codes_of, d=65, n=1025, nq=7, m=40, k=10):
    def operands(which):
        rng = np.random.default_rng(340 + WHICH.index(which))
        q, c = rng.standard_normal((nq, d)).astype(np.float32), rng.standard_normal((n, d)).astype(np.float32)
        cand = np.stack([rng.permutation(n)[:m] for _ in range(nq)]).astype(np.int64)
        cand[0, :3] = -1                                        # padding
        return {"q": q, "codes": codes_of(c), "cand": cand}
    _add(name, (entry,), operands, lambda t: op(t["q"], t["codes"], d, t["cand"], k, return_status=True),
         lambda h: ref(h["q"], h["codes"], d, h["cand"], k), decoy_rule="other", decoy_check=differs)


_rescore_case("sign-rescore", "tsim_sign_rescore_topk", ops.sign_rescore_topk, hm.rescore_ref, hm.pack_ref)
_rescore_case("int8-rescore", "tsim_int8_rescore_topk", ops.int8_rescore_topk, i8.rescore_ref, lambda c: i8.quantize_ref(c, i8.ranges_of(c)))

PQ_D, PQ_M = 66, 33


def _pq_operands(which):
    rng = np.random.default_rng(360 + WHICH.index(which))
    cb = pc.random_codebooks(rng, PQ_D, PQ_M)
    return {"x": pc.encoder_rows(rng, 300, cb), "q": rng.standard_normal((5, PQ_D)).astype(np.float32), "cb": cb}


_add("pq-encode-rows", ("tsim_pq_encode_rows",), _pq_operands, lambda t: (ops.pq_encode_rows(t["x"], t["cb"]),),
     lambda h: (pc.encode_ref(h["x"], h["cb"]),), decoy_rule="other", decoy_check=differs)
_add("pq-tables-l2", ("tsim_pq_tables",), _pq_operands, lambda t: ops.pq_tables(t["q"], t["cb"], "l2"),
     lambda h: pc.tables_ref(h["q"], h["cb"], "l2"), decoy_rule="other", decoy_check=differs)


# ------------------------------------------------------------------------------------------------- graph index
G_N, G_R, G_Q, G_K, G_D, G_EF, G_WIDTH, G_ITERS = 2000, 8, 5, 10, 24, 32, 2, 25


def _graph_operands(seeded):
    def operands(which):
        rng = np.random.default_rng(380 + WHICH.index(which))
        c = gc.random_rows(rng, G_N, G_D)
        q = rng.standard_normal((G_Q, G_D)).astype(np.float32)
        g, lost = gc.random_graph(rng, G_N, G_R, island=3)
        ok = np.setdiff1d(np.arange(G_N), lost)
        out = {"q": q, "c": c, "g": np.asarray(g, np.int32)}
        if seeded:
            out["seeds"] = rng.choice(ok, size=(16, 4), replace=True).astype(np.int32)
            out["probes"] = rng.integers(0, 16, size=(G_Q, 3)).astype(np.int32)
        else:
            out["entries"] = rng.choice(ok, size=8, replace=True).astype(np.int32)
        return out
    return operands


_add("graph-search", ("tsim_graph_search",), _graph_operands(False),
     lambda t: ops.graph_search("cosine", t["q"], t["c"], t["g"], t["entries"], G_K, G_EF, width=G_WIDTH, max_iters=G_ITERS, return_status=True),
     lambda h: gc.graph_search_ref("cosine", h["q"], h["c"], h["g"], h["entries"], G_EF, G_WIDTH, G_ITERS, G_K),
     decoy_rule="other", decoy_check=differs)
_add("graph-search-seeded", ("tsim_graph_search_seeded",), _graph_operands(True),
     lambda t: ops.graph_search_seeded("l2", t["q"], t["c"], t["g"], G_K, G_EF, probes=t["probes"], seeds=t["seeds"], width=G_WIDTH,
                                       max_iters=G_ITERS, return_status=True, return_probes=True),
     lambda h: gsc.graph_search_seeded_ref("l2", h["q"], h["c"], h["g"], G_EF, G_WIDTH, G_ITERS, G_K, probes=h["probes"], seeds=h["seeds"]),
     decoy_rule="other", decoy_check=differs)


def _prune_operands(which, n=1000, k0=33):
    rng = np.random.default_rng(390 + WHICH.index(which))
    g0 = rng.integers(-1, n + 2, size=(n, k0)).astype(np.int32)
    near = (np.arange(n)[:, None] + rng.integers(1, 2 * k0 + 2, size=(n, k0))) % n       # mostly local neighbours: detours exist
    return {"g0": np.where(rng.random((n, k0)) < 0.9, near, g0).astype(np.int32)}


def _prune_oracle(h):
    d = gc.detours(h["g0"])
    return gc.forward_lists(h["g0"], d, 16), d


_add("graph-prune", ("tsim_graph_prune",), _prune_operands, lambda t: ops.graph_prune(t["g0"], 16, return_detours=True), _prune_oracle,
     decoy_rule="other", decoy_check=differs)


# ------------------------------------------------------------------------------------------------- dense rows, pooling, fp8
def _within(bound_of):
    """check of a case whose existing test is a bound and not bit-equality: |got - want| <= bound, elementwise"""
    def check(got, want, which="real"):
        assert len(got) + 1 == len(want)
        for g, w, b in zip(got, want[:-1], [want[-1]] * len(got)):
            err = np.abs(g.astype(np.float64) - w.astype(np.float64))
            assert g.shape == w.shape and (err <= b).all(), (which, float(err.max()), float(np.max(b)))
    return check


def _cos_operands(which):
    rng = np.random.default_rng(400 + WHICH.index(which))
    return {"a": rng.standard_normal((70, 100)).astype(np.float32), "b": rng.standard_normal((130, 100)).astype(np.float32)}


# (tests/test_search_gpu.py: atol 1e-6 against oracle.search_ref.cos_sim)
_add("cos-sim-dense", ("tsim_cos_sim",), _cos_operands, lambda t: (ops.cos_sim_dense(t["a"], t["b"]),),
     lambda h: (cos_sim(h["a"], h["b"]), np.float64(1e-6)), check=_within(None), decoy_rule="other")


def _pool_operands(which):
    rng = np.random.default_rng(410 + WHICH.index(which))
    lens = rng.integers(1, 20, size=9)
    lens[3] = 0                                                 # a row without tokens pools to zeros
    return {"hidden": rng.standard_normal((9, 19, 40)).astype(np.float32), "mask": (np.arange(19)[None, :] < lens[:, None]).astype(np.int32)}


def _pool_oracle(mode):
    def oracle(h):      # (tests/test_search_gpu.py: atol 1e-6; tests/test_sentence_head_gpu.py st_pool restates the modes)
        from test_sentence_head_gpu import st_pool
        hid, m = torch.from_numpy(np.array(h["hidden"])), torch.from_numpy(np.array(h["mask"]))
        ref = encoder_ref.mean_pool(hid, m) if mode == "mean" else st_pool(hid, m, mode)
        ref = ref.numpy().astype(np.float32).copy()
        ref[3] = 0
        return ref, np.float64(1e-6)
    return oracle


_add("mean-pool", ("tsim_mean_pool",), _pool_operands, lambda t: (ops.mean_pool(t["hidden"], t["mask"]),), _pool_oracle("mean"),
     check=_within(None), decoy_rule="other")
_add("pool-max", ("tsim_pool",), _pool_operands, lambda t: (ops.pool(t["hidden"], t["mask"], "max"),), _pool_oracle("max"),
     check=_within(None), decoy_rule="other")


def _dense_operands(which, B=77, d_in=392, d_out=1000):
    rng = np.random.default_rng(420 + WHICH.index(which))
    return {"x": (2 * rng.standard_normal((B, d_in))).astype(np.float32),
            "w": (rng.standard_normal((d_out, d_in)) / np.sqrt(d_in)).astype(np.float32), "b": (0.05 * rng.standard_normal(d_out)).astype(np.float32)}


def _dense_oracle(h):   # the float64 value and the bound of tests/test_sentence_head_gpu.py test_dense_rows_accuracy (tanh)
    X, W, Bv = (h[k].astype(np.float64) for k in ("x", "w", "b"))
    z = X @ W.T
    bound = X.shape[1] * 2.0 ** -23 * (np.abs(X) @ np.abs(W).T) + np.abs(z + Bv) * 2.0 ** -24 + 1e-30 + 4 * 2.0 ** -24
    return np.tanh(z + Bv), bound * 1.01


_add("dense-rows", ("tsim_dense_rows",), _dense_operands, lambda t: (ops.dense_rows(t["x"], t["w"], t["b"], "tanh"),), _dense_oracle,
     check=_within(None), decoy_rule="other")


def _mx_operands(which, M=300, N=256, K=768):
    rng = np.random.default_rng(430 + WHICH.index(which))
    x = (rng.standard_normal((M, K)) * np.exp(rng.uniform(-3, 3, (M, 1)))).astype(np.float32)
    w = (rng.standard_normal((N, K)) * 0.05).astype(np.float32)
    xq, xs = fp8_ref.mx_quantize(x)
    wq, ws = fp8_ref.mx_quantize(w)
    return {"x": bf16_round(x), "xq": xq, "xs": xs, "wq": wq, "ws": ws, "bias": rng.standard_normal(N).astype(np.float32)}


def _mx_gemm_oracle(h):  # (tests/test_fp8_gpu.py test_mxfp8_gemm_vs_oracle: 1e-4 (1 + max |ref|))
    ref = fp8_ref.mx_dequantize(h["xq"], h["xs"]).astype(np.float64) @ fp8_ref.mx_dequantize(h["wq"], h["ws"]).astype(np.float64).T + h["bias"]
    return ref, np.float64(1e-4 * (1 + np.abs(ref).max()))


_add("quantize-mxfp8", ("tsim_quantize_mxfp8",), _mx_operands, lambda t: ops.quantize_mxfp8(t["x"].to(torch.bfloat16)),
     lambda h: fp8_ref.mx_quantize(h["x"]), decoy_rule="other", decoy_check=differs)
_add("gemm-mxfp8", ("tsim_gemm_mxfp8",), _mx_operands, lambda t: (ops.gemm_mxfp8(t["xq"], t["xs"], t["wq"], t["ws"], t["bias"]),),
     _mx_gemm_oracle, check=_within(None), decoy_rule="other")


# ------------------------------------------------------------------------------------------------- the encoder
ENC_PRESET = "all-MiniLM-L6-v2"
ENC_POOL_TOL, ENC_COS_MIN = 5e-2, 0.9995                         # the bars of tests/test_encoder_gpu.py against the fp32 golden
_ENCODERS = {}


def encoder():
    """One handle per process, made on first use (tsim_encoder_create synchronises: the tests make it in front of any stream)."""
    if ENC_PRESET not in _ENCODERS:
        from text_similarity_amd.native_encoder import NativeEncoder
        _ENCODERS[ENC_PRESET] = NativeEncoder.from_preset(ENC_PRESET, max_tokens=4096, max_seqs=64)
    return _ENCODERS[ENC_PRESET]


def _enc_golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"encoder_{ENC_PRESET}.npz"), allow_pickle=False)


def _enc_operands(which):
    g = _enc_golden()
    flat, cu = g["flat_ids"].astype(np.int32), g["cu_seqlens"].astype(np.int32)
    if which != "real":      # other token ids inside the vocabulary, the same sequence lengths
        from text_similarity_amd import presets
        flat = ((flat.astype(np.int64) * 7 + 13 + WHICH.index(which)) % presets.PRESETS[ENC_PRESET].vocab).astype(np.int32)
    # (the span table of the spans case: one span per sequence listing every token — its mean is the pooled row)
    tok = np.concatenate([np.arange(n) for n in np.diff(cu)]).astype(np.int32)
    return {"flat": flat, "cu": cu, "span_seq": np.arange(cu.shape[0] - 1, dtype=np.int32), "span_tok": tok}


def _enc_run(kind):
    def run(t):
        enc, g = encoder(), _enc_golden()
        cu_h = g["cu_seqlens"].astype(np.int64)
        max_len = int(np.diff(cu_h).max())                       # known on the host: no read-back in the forward
        if kind == "head":
            from text_similarity_amd.native_encoder import SentenceHead
            return (enc.forward_packed(t["flat"], t["cu"], max_len=max_len, head=SentenceHead("mean"))["pooled"],)
        if kind == "spans":
            return (enc.forward_spans(t["flat"], t["cu"], t["span_seq"], t["cu"], t["span_tok"], max_len=max_len)["spans"],)
        return (enc.forward_packed(t["flat"], t["cu"], max_len=max_len, pooled=True)["pooled"],)
    return run


def _enc_check(got, want, which="real"):
    p, ref = got[0].astype(np.float64), want[0].astype(np.float64)
    err = np.abs(p - ref).max()
    cos = ((p * ref).sum(1) / np.maximum(np.linalg.norm(p, axis=1) * np.linalg.norm(ref, axis=1), 1e-30)).min()
    assert err <= ENC_POOL_TOL and cos >= ENC_COS_MIN, (which, float(err), float(cos))


def _enc_oracle(h):
    g = _enc_golden()
    assert same(h["flat"], g["flat_ids"].astype(np.int32)), "the golden holds the real operands' rows only"
    return (g["pooled"],)


for _kind, _entry in (("packed", "tsim_encoder_forward_ex"), ("head", "tsim_encoder_forward_head"), ("spans", "tsim_encoder_forward_spans")):
    _add(f"encoder-{_kind}", (_entry,), _enc_operands, _enc_run(_kind), _enc_oracle, check=_enc_check, decoy_rule="other")


# ------------------------------------------------------------------------------------------------- the encoder, by its oracle
# tiny-bert, and all-MiniLM-L6-v2 on the 64 sentences of smoke(): the fp32 restatement oracle.encoder_ref.encode_packed under
# the bars of tests/test_encoder_gpu.py.  The oracle exists for every operand set, so these two also run on two streams at
# once, one handle a stream (ENC_SLOT picks the handle, as tools/concurrency_probe.py makes two).
ENC_SLOT = 0
ENC_BATCHES = {"tiny-bert": (40, "contract/tiny", 48), "all-MiniLM-L6-v2": (64, "smoke", 64)}


def encoder_of(preset, slot=None):
    slot = ENC_SLOT if slot is None else slot
    if (preset, slot) not in _ENCODERS:
        from text_similarity_amd.native_encoder import NativeEncoder
        _ENCODERS[preset, slot] = NativeEncoder.from_preset(preset, max_tokens=4096, max_seqs=64)
    return _ENCODERS[preset, slot]


def _enc2_operands(preset):
    def operands(which):
        from text_similarity_amd import presets
        n, seed, max_len = ENC_BATCHES[preset]
        vocab = presets.PRESETS[preset].vocab
        flat, cu = presets.synthetic_token_batch(n, seed=seed, vocab_size=vocab, max_len=max_len)
        flat = flat.astype(np.int32)
        if which != "real":      # other token ids inside the vocabulary, the same sequence lengths
            flat = ((flat.astype(np.int64) * 7 + 13 + WHICH.index(which)) % vocab).astype(np.int32)
        return {"flat": flat, "cu": cu.astype(np.int32), "max_len": np.int64(np.diff(cu).max())}
    return operands


def _enc2_oracle(preset):
    def oracle(h):
        from text_similarity_amd import presets
        ref = encoder_ref.encode_packed(presets.PRESETS[preset], presets.synthetic_weights(preset), h["flat"], h["cu"].astype(np.int64),
                                        batch_size=16)
        return (np.asarray(ref, np.float32),)
    return oracle


for _preset in ENC_BATCHES:
    (lambda preset: _add(
        f"encoder-oracle-{preset}", ("tsim_encoder_forward_ex",), _enc2_operands(preset),
        lambda t: (encoder_of(preset).forward_packed(t["flat"], t["cu"], max_len=int(t["max_len"]), pooled=True)["pooled"],),
        _enc2_oracle(preset), check=_enc_check, decoy_rule="other"))(_preset)
TWO_HANDLE_CASES = [c for c in CASES if c.name.startswith("encoder-oracle-")]

# CrossEncoder logits: the only route to tsim_encoder_forward_ex with token types and the classification head.  tiny-bert, three
# labels, against HF's BertForSequenceClassification on the same synthetic weights under the bars of tests/test_cross_encoder_gpu.py.
CE_PRESET, CE_LABELS, CE_PAIRS = "tiny-bert", 3, 48
_CROSS = {}


def cross_encoder():
    if "ce" not in _CROSS:
        import test_cross_encoder_gpu as tce
        from text_similarity_amd import presets
        from text_similarity_amd.models.cross_encoder import CrossEncoder
        cfg = presets.PRESETS[CE_PRESET]
        _CROSS["ce"] = CrossEncoder(CE_PRESET, num_labels=CE_LABELS, tokenizer=tce._tokenizer(cfg.vocab), max_length=cfg.max_pos,
                                    max_tokens=8192, max_seqs=256)
    return _CROSS["ce"]


def _ce_pairs(which):
    import test_cross_encoder_gpu as tce
    from text_similarity_amd import presets
    return tce._pairs(CE_PAIRS, 12, f"contract/ce/{WHICH.index(which) if which != 'real' else 'real'}", presets.PRESETS[CE_PRESET].vocab)


def _ce_operands(which):
    import test_cross_encoder_gpu as tce
    from text_similarity_amd import presets
    cfg = presets.PRESETS[CE_PRESET]
    tok = tce._tokenizer(cfg.vocab)
    # (one shape for the three operand sets: every pair padded or cut to 40 tokens by the tokenizer, as HF sees it too)
    enc = tok([a for a, _ in _ce_pairs(which)], [b for _, b in _ce_pairs(which)], truncation=True, max_length=40, padding="max_length")
    ids, types = np.asarray(enc["input_ids"], np.int32), np.asarray(enc["token_type_ids"], np.int32)
    cu = (np.arange(ids.shape[0] + 1) * ids.shape[1]).astype(np.int32)
    return {"flat": ids.reshape(-1), "types": types.reshape(-1), "cu": cu}


def _ce_run(t):
    r = cross_encoder().model.forward_packed(t["flat"], t["cu"], types=t["types"], max_len=40, pooled=False, logits=True)
    return (r["logits"],)


def _ce_oracle(h):      # HF on the same padded ids with NO attention mask: the native forward attends to every token it is given
    import test_cross_encoder_gpu as tce
    m = tce._hf_model(CE_PRESET, CE_LABELS)
    ids = torch.from_numpy(h["flat"].reshape(-1, 40).astype(np.int64))
    types = torch.from_numpy(h["types"].reshape(-1, 40).astype(np.int64))
    with torch.no_grad():
        return (m(input_ids=ids, token_type_ids=types).logits.numpy().astype(np.float32),)


def _ce_check(got, want, which="real"):
    import test_cross_encoder_gpu as tce
    err, r = tce._stats(got[0].reshape(want[0].shape), want[0])
    assert err <= tce.LOGIT_TOL and r >= tce.PEARSON_MIN_TINY, (which, err, r)


_add("cross-encoder-logits", ("tsim_encoder_forward_ex",), _ce_operands, _ce_run, _ce_oracle, check=_ce_check, decoy_rule="other")


# ================================================================================================ index classes (stream test only)
# Search only.  Each index is built once, on the default stream (the stream test's first run of a case is on the default stream),
# and synchronised; the operands are the queries.  Expected values: the op-level oracles their own tests use.  They name no C
# entry: what they add is the Python composition around the entries, where a torch helper could leave the current stream.
IDX_N, IDX_D, IDX_Q, IDX_K = 3000, 64, 9, 10
_INDEXES = {}


def _index(name, make):
    if name not in _INDEXES:
        _INDEXES[name] = make()
        torch.cuda.synchronize()
    return _INDEXES[name]


@functools.lru_cache(maxsize=None)
def _idx_rows():
    rng = np.random.default_rng(500)
    return rng.standard_normal((IDX_N, IDX_D)).astype(np.float32), (np.arange(IDX_N) * 3 + 1000).astype(np.int64)


def _idx_queries(nq=IDX_Q, d=IDX_D):
    return lambda which: {"q": np.random.default_rng(510 + WHICH.index(which)).standard_normal((nq, d)).astype(np.float32)}


def _labels_of(labels, i):
    return np.where(i >= 0, labels[np.maximum(i, 0)], -1)


def _make_flat():
    from text_similarity_amd.index import GpuFlatIndex
    x, labels = _idx_rows()
    ix = GpuFlatIndex(space="cosine", dim=IDX_D, device="cuda:0")
    ix.add_items(x, labels)
    return ix


def _flat_index_oracle(h):
    x, labels = _idx_rows()
    s, i = cosine_topk_f32(h["q"], x, IDX_K)
    return labels[i], s


_add("index-flat", (), _idx_queries(), lambda t: _index("flat", _make_flat).search(t["q"], IDX_K), _flat_index_oracle, decoy_rule="other")

IVF_NLIST = 8


def _make_ivf():
    from text_similarity_amd.ivf_index import GpuIVFIndex
    x, labels = _idx_rows()
    ix = GpuIVFIndex("cosine", IDX_D, IVF_NLIST, nprobe=IVF_NLIST, device="cuda:0")
    ix.train(centroids=x[:IVF_NLIST].copy())
    ix.add_items(x, labels)
    return ix


# (every list probed: the flat index's answer, bit for bit — tests/test_ivf_index_gpu.py)
_add("index-ivf", (), _idx_queries(), lambda t: _index("ivf", _make_ivf).search(t["q"], IDX_K), _flat_index_oracle, decoy_rule="other")

PQI_MULT = 3


def _pq_labels():
    return np.random.default_rng(1).permutation(10_000)[:rc.N_ROWS].astype(np.int64) + (1 << 33)


def _make_pq():
    from text_similarity_amd.pq_index import GpuPQIndex
    cent, cb, x, q = rc.small_data()
    ix = GpuPQIndex("ip", rc.D, rc.M, device="cuda:0", refine="float16")
    ix.train(codebooks=cb)
    ix.add_items(x, _pq_labels())
    return ix


def _pq_index_oracle(h):
    cent, cb, x, _ = rc.small_data()
    s, i, _ = rc.pq_refined_ref("ip", h["q"], h["q"], cb, pc.encode_ref(x, cb), rc.store_rows(x, "float16"), IDX_K, PQI_MULT)
    return s, _labels_of(_pq_labels(), i)


_add("index-pq-refine-f16", (), _idx_queries(d=rc.D), lambda t: _index("pq", _make_pq).search(t["q"], IDX_K, rescore_multiplier=PQI_MULT),
     _pq_index_oracle, decoy_rule="other")


def _make_ivfpq():
    from text_similarity_amd.ivfpq_index import GpuIVFPQIndex
    cent, cb, x, q = rc.small_data()
    ix = GpuIVFPQIndex("ip", rc.D, rc.NLIST, 2, rc.M, by_residual=True, device="cuda:0", refine="float16")
    ix.train(centroids=cent, codebooks=cb)
    ix.add_items(x, _pq_labels())
    return ix


def _ivfpq_index_oracle(h):      # (on the index's own list assignment and probes, as tests/test_refine_index_gpu.py takes them)
    cent, cb, x, _ = rc.small_data()
    ix = _index("ivfpq", _make_ivfpq)
    lists = ix._list[:rc.N_ROWS].cpu().numpy()
    probes = ix._coarse(torch.from_numpy(np.array(h["q"])).to("cuda:0"), rc.NLIST).cpu().numpy()[:, :2]
    codes = ic.encode_ref(x, cent, lists, cb, by_residual=True)
    s, i, _ = rc.ivfpq_refined_ref("ip", h["q"], h["q"], cent, cb, codes, lists, probes, rc.store_rows(x, "float16"), IDX_K, PQI_MULT)
    return s, _labels_of(_pq_labels(), i)


_add("index-ivfpq", (), _idx_queries(d=rc.D), lambda t: _index("ivfpq", _make_ivfpq).search(t["q"], IDX_K, rescore_multiplier=PQI_MULT),
     _ivfpq_index_oracle, decoy_rule="other")

GRAPH_IX = dict(M=4, ef=16, width=2, max_iters=32)


def _make_graph():
    from text_similarity_amd.graph_index import GpuGraphIndex
    rows, cent, _ = gsc.island_corpus()
    ix = GpuGraphIndex("cosine", rows.shape[1], device="cuda:0", entry="coarse", nprobe=2, seeds_per_list=2, **GRAPH_IX)
    ix.add_items(rows)
    ix.build(centroids=cent)
    return ix


def _graph_index_operands(which):
    qs = gsc.island_corpus()[2]
    return {"q": np.ascontiguousarray(qs[16 * WHICH.index(which):16 * WHICH.index(which) + 16])}


def _graph_index_oracle(h):      # (the restatement on the index's own graph, centroids and seeds: tests/test_graph_seed_index_gpu.py)
    ix = _index("graph", _make_graph)
    n = ix.get_current_count()
    ef, iters = ix.search_params(5)
    s, i, _, _ = gsc.graph_search_seeded_ref("cosine", h["q"], ix._f32[:n].cpu().numpy(), ix.graph.cpu().numpy(), ef, ix.width, iters, 5,
                                             centroids=ix.centroids.cpu().numpy(), n_probe=min(ix.nprobe, ix.centroids.shape[0]),
                                             seeds=ix.seeds.cpu().numpy())
    return _labels_of(ix._labels[:n].cpu().numpy(), i), s


_add("index-graph-coarse", (), _graph_index_operands, lambda t: _index("graph", _make_graph).search(t["q"], 5), _graph_index_oracle,
     decoy_rule="other")

CODE_IX_D = 200


@functools.lru_cache(maxsize=None)
def _code_ix_rows():
    rng = np.random.default_rng(520)
    return rng.standard_normal((1600, CODE_IX_D)).astype(np.float32), (np.arange(1600) * 7 + 50_000).astype(np.int64)


def _make_binary():
    from text_similarity_amd.binary_index import GpuBinaryIndex
    x, labels = _code_ix_rows()
    ix = GpuBinaryIndex(CODE_IX_D, device="cuda:0")
    ix.add_items(x, labels)
    return ix


def _binary_oracle(h):
    x, labels = _code_ix_rows()
    dist, i = hm.hamming_topk_ref(hm.pack_ref(h["q"]), hm.pack_ref(x), CODE_IX_D, IDX_K)
    return dist, _labels_of(labels, i)


_add("index-binary", (), _idx_queries(5, CODE_IX_D), lambda t: _index("binary", _make_binary).search(t["q"], IDX_K), _binary_oracle,
     decoy_rule="other")


def _make_int8():
    from text_similarity_amd.int8_index import GpuInt8Index
    x, labels = _code_ix_rows()
    ix = GpuInt8Index(CODE_IX_D, device="cuda:0")
    ix.add_items(x, labels)                                    # floats: calibrates on these rows, then quantises
    return ix


def _int8_oracle(h):
    x, labels = _code_ix_rows()
    ranges = i8.ranges_of(x)
    s, i = i8.ip_topk_ref(i8.quantize_ref(h["q"], ranges), i8.quantize_ref(x, ranges), CODE_IX_D, IDX_K)
    return s, _labels_of(labels, i)


_add("index-int8", (), _idx_queries(5, CODE_IX_D), lambda t: _index("int8", _make_int8).search(t["q"], IDX_K), _int8_oracle,
     decoy_rule="other")
INDEX_CASES = [c for c in CASES if c.name.startswith("index-")]

# ================================================================================================ composite ops that read back
# community_detection (the range search's total, the rounds' undecided counts) and hdbscan (the edges, for the host tree stage):
# stream test only, host_sync — the side stream may be idle when they return.
CD_TAU, CD_MIN = 0.75, 10


def _cd_oracle(h):      # the exact range search of the rows against themselves, then tests/community_cases.detect_ref
    x = h["x"]
    ex = exact_cosine(x, x)
    hits = range_ref(ex, CD_TAU)
    lims = np.concatenate([[0], np.cumsum([len(r) for r in hits])]).astype(np.int64)
    return cc.detect_ref(lims, np.concatenate([ex[j, r] for j, r in enumerate(hits)]), np.concatenate(hits), x.shape[0], CD_MIN)[:4]


_add("community-detection", ("tsim_l2norm_rows",), lambda which: {"x": cc.planted_rows(32, seed=5 + WHICH.index(which))[0]},
     lambda t: ops.community_detection(None, t["x"], 32, CD_TAU, CD_MIN)[:4], _cd_oracle, host_sync=True, decoy_rule="other",
     decoy_check=differs)
_add("hdbscan", ("tsim_l2_rows", "tsim_l2_query_rows"),
     lambda which: {"x": hc.blobs(257, 16, 3, 40 + WHICH.index(which))},
     lambda t: (ops.hdbscan(t["x"], 5),), lambda h: (np.asarray(hc.hdbscan_ref(h["x"], 5)[0], np.int64),), host_sync=True,
     decoy_rule="other", decoy_check=differs)



# ================================================================================================ what the two GPU tests share
def to_device(host, device):
    """host operands -> device operands on the CURRENT stream's device: arrays become tensors, 0-d values stay host parameters"""
    def dev(v):
        t = torch.from_numpy(np.array(v))
        # (an empty operand: a fresh allocation, as aligned as any other, where a copy of nothing may point anywhere)
        return t.to(device) if v.size else torch.zeros(t.shape, dtype=t.dtype, device=device)
    return {k: (dev(v) if v.ndim else v) for k, v in host.items()}


def copy_into(dev, staged):
    """overwrite the device operands' contents in place (enqueued on the current stream; device-to-device, so never blocking);
    host parameters are taken from ``staged``"""
    out = {}
    for k, v in staged.items():
        if isinstance(v, torch.Tensor):
            dev[k].copy_(v, non_blocking=True)
            out[k] = dev[k]
        else:
            out[k] = v
    return out


def outputs(result):
    """what run returned, as a tuple of numpy arrays (bf16 widened to float32, which is exact)"""
    result = result if isinstance(result, (tuple, list)) else (result,)
    return tuple((t.float() if t.dtype == torch.bfloat16 else t).cpu().numpy() for t in result)


def count_calls(monkeypatch, names):
    """Thin counting proxies on the attributes of _lib.lib() for the given entries; returns the dict of counts."""
    L, counts = lib(), {}
    for name in names:
        fn = getattr(L, name)
        counts[name] = 0

        def proxy(*a, _fn=fn, _name=name):
            counts[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(L, name, proxy)
    return counts


def by_name(name):
    return next(c for c in CASES if c.name == name)


WORKSPACE_CASES = [c for c in CASES if c.workspace is not None]
# the cases whose Python op reads something back from the device mid-call (pinned literally by the CPU test)
HOST_SYNC_CASES = sorted(c.name for c in CASES if c.host_sync)

# Entries with a `void *stream` (or `void *workspace`) parameter that no case reaches, each with its reason.
EXEMPT = {
    "tsim_encoder_error_flags": "a synchronising call by contract: it reads the handle's flag word back",
    "tsim_encoder_forward": "tsim_encoder_forward_ex with NULL token types and NULL logits, one line in encoder.hip; no Python "
                            "caller",
    "tsim_topk_merge": "tsim_topk_merge_strided with contiguous strides, one line in search.hip; ops.topk_merge calls the strided entry",
}
