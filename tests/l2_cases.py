"""Test-local oracle of the exact Euclidean search (include/tsim.h tsim_l2_topk_ex), shared by tests/test_l2_search_cpu.py and
tests/test_l2_search_gpu.py: the canonical squared distance restated in numpy (float64, no fused multiply-add), the top-k by
(distance asc, index asc), and the augmented half operands of tsim_l2_rows / tsim_l2_query_rows with their residuals."""
import math

import numpy as np

from oracle.search_ref import _LANES, _lane_sum, flush_safe_err, topk_rows


def _lanes(a, d):
    m = -(-d // 64)
    a = np.asarray(a, dtype=np.float64)
    if m * 64 - d:
        a = np.concatenate([a, np.zeros(a.shape[:-1] + (m * 64 - d,))], axis=-1)
    return a.reshape(a.shape[:-1] + (m, 64))


def dist2_f64(x, y):
    """Canonical float64 squared distance along the last axis of two broadcastable float32 arrays: lane l adds diff * diff for
    j = l, l + 64, ... (the difference, the product and the sum each rounded on their own), then the xor butterfly 32 .. 1."""
    d = x.shape[-1]
    xl, yl = _lanes(x, d), _lanes(y, d)
    diff = xl[..., 0, :] - yl[..., 0, :]
    part = diff * diff
    for i in range(1, xl.shape[-2]):
        diff = xl[..., i, :] - yl[..., i, :]
        part = part + diff * diff
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[..., _LANES ^ o]
    return part[..., 0]


def l2_dists(q, c, qblock=4, nblock=4096, dtype=np.float32):
    """[Q, N] squared distances of the float32 rows, rounded once to float32 (dtype=np.float64: before that rounding)."""
    q = np.asarray(q, dtype=np.float32)
    c = np.asarray(c, dtype=np.float32)
    out = np.empty((q.shape[0], c.shape[0]), dtype=dtype)
    for a in range(0, q.shape[0], qblock):
        for b in range(0, c.shape[0], nblock):
            out[a:a + qblock, b:b + nblock] = dist2_f64(q[a:a + qblock, None, :], c[None, b:b + nblock, :]).astype(dtype)
    return out


def l2_topk_ref(q, c, k, idx_offset=0):
    """(distances [Q, min(k, N)] float32 ascending, indices int64): ties go to the lower index."""
    dist = l2_dists(q, c)
    _, i = topk_rows(-dist, k)
    return np.take_along_axis(dist, i, 1), i + idx_offset


def corpus_scale(c):
    """A: the smallest power of two >= the largest row norm (1 for an all-zero corpus) — tsim_dot_scale of the max-norm word,
    for data whose largest norm is not within 1e-6 of a power of two."""
    n = float(np.sqrt(_lane_sum(c, c)).max())
    return 1.0 if n == 0 else 2.0 ** math.ceil(math.log2(n))


def aug_corpus(c, A):
    """(halves [N, d + 1] as float64, rho_c): half((c, -|c|^2 / (2A)) / 2A) and the largest flush-safe residual."""
    c = np.asarray(c, dtype=np.float32)
    inv = 0.5 / A
    v = np.concatenate([c.astype(np.float64) * inv, -(_lane_sum(c, c) * (inv * inv))[:, None]], axis=1)
    h = v.astype(np.float16).astype(np.float64)
    return h, float(np.sqrt((flush_safe_err(h, v) ** 2).sum(1)).max())


def aug_queries(q, A):
    """(halves [Q, d + 1] as float64, rho_q [Q], |q|^2 [Q], nq' [Q]): half((q, A) / nq'), nq' = sqrt(|q|^2 + A^2)."""
    q = np.asarray(q, dtype=np.float32)
    qq = _lane_sum(q, q)
    nq = np.sqrt(qq + A * A)
    v = np.concatenate([q.astype(np.float64), np.full((q.shape[0], 1), A)], axis=1) * (1.0 / nq)[:, None]
    h = v.astype(np.float16).astype(np.float64)
    return h, np.sqrt((flush_safe_err(h, v) ** 2).sum(1)), qq, nq
