"""Test-local oracle of the exact search within candidate lists (include/tsim.h tsim_cosine_list_topk / tsim_dot_list_topk /
tsim_l2_list_topk), shared by tests/test_list_search_cpu.py, tests/test_list_search_gpu.py and tests/test_index_filter_gpu.py.
Scores are the three existing definitions, taken from where they are already restated: the cosine of oracle/search_ref
(exact_cosine_pairs), float32 of the canonical float64 inner product (_lane_sum), and the squared distance of tests/l2_cases.py
(dist2_f64, the pairwise form of l2_dists).  The top-k is (score desc, row asc), Euclidean (distance asc, row asc), padded with
-inf / -1 (Euclidean +inf / -1)."""
import os
import re

import numpy as np

from oracle.search_ref import _lane_sum, exact_cosine_pairs
from l2_cases import dist2_f64

SPACES = ("cosine", "dot", "l2")
HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tsim.h")
ST_ROW, ST_LIMS = 1, 2      # include/tsim.h TSIM_LIST_ST_ROW / TSIM_LIST_ST_LIMS


def header_define(name):
    m = re.search(r"^#define\s+%s\s+(\d+)" % name, open(HDR).read(), re.M)
    assert m, f"{name} is not defined in include/tsim.h"
    return int(m.group(1))


def pair_scores(space, q, c, qi, ci, block=4096):
    """float32 scores of the (query, row) index pairs, bit for bit what the kernels return for them."""
    q = np.asarray(q, dtype=np.float32)
    c = np.asarray(c, dtype=np.float32)
    qi = np.asarray(qi, dtype=np.int64)
    ci = np.asarray(ci, dtype=np.int64)
    out = np.empty(qi.shape, dtype=np.float32)
    for a in range(0, qi.shape[0], block):
        x, y = qi[a:a + block], ci[a:a + block]
        if space == "cosine":
            out[a:a + block] = exact_cosine_pairs(q, c, x, y)
        elif space == "dot":
            out[a:a + block] = _lane_sum(q[x], c[y]).astype(np.float32)
        else:
            out[a:a + block] = dist2_f64(q[x], c[y]).astype(np.float32)
    return out


def rank_list(space, rows, scores, k, idx_offset=0):
    """(scores [k], rows [k]) of ONE list given its usable rows and their scores: ordered and padded as the kernels do.  Rows
    may repeat: equal (score, row) entries stay adjacent."""
    rows = np.asarray(rows, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float32)
    key = scores.astype(np.float64) if space == "l2" else -scores.astype(np.float64)
    order = np.lexsort((rows, key))[:k]
    s = np.full((k,), np.inf if space == "l2" else -np.inf, dtype=np.float32)
    i = np.full((k,), -1, dtype=np.int64)
    s[:order.shape[0]] = scores[order]
    i[:order.shape[0]] = rows[order] + idx_offset
    return s, i


def list_topk_ref(space, q, c, lists, k, idx_offset=0, unique=True):
    """The oracle: ``lists`` is a sequence of Q integer sequences (or ONE 1-D array shared by every query).  Negative entries
    and entries >= N are dropped; ``unique`` drops repeats (what ops does unless assume_unique).  Returns (scores [Q, k], idx
    [Q, k], status [Q]) with status bit ST_ROW where a list held an entry >= N."""
    Q, N = q.shape[0], c.shape[0]
    if isinstance(lists, np.ndarray) and lists.ndim == 1:
        lists = [lists] * Q
    S = np.empty((Q, k), dtype=np.float32)
    I = np.empty((Q, k), dtype=np.int64)
    st = np.zeros((Q,), dtype=np.int32)
    for j in range(Q):
        rows = np.asarray(lists[j], dtype=np.int64).reshape(-1)
        if (rows >= N).any():
            st[j] |= ST_ROW
        rows = rows[(rows >= 0) & (rows < N)]
        if unique:
            rows = np.unique(rows)
        sc = pair_scores(space, q, c, np.full(rows.shape, j, dtype=np.int64), rows)
        S[j], I[j] = rank_list(space, rows, sc, k, idx_offset)
    return S, I, st


def csr(lists):
    """(cand int64 [T], lims int64 [Q+1]) of a sequence of lists."""
    lims = np.zeros((len(lists) + 1,), dtype=np.int64)
    lims[1:] = np.cumsum([len(x) for x in lists])
    cand = np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in lists]) if len(lists) else np.zeros((0,), np.int64)
    return cand.astype(np.int64), lims


def same_bits(a, b):
    """float32 arrays equal bit for bit (so +0 / -0 and the infinities count)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool((a.view(np.int32) == b.view(np.int32)).all())
