"""Numpy restatement of the refine stage of GpuPQIndex and GpuIVFPQIndex (no torch): the float16 row store, the exact re-score of
a candidate list, and the two-stage searches composed from the ADC restatements that exist (tests/pq_cases.py,
tests/ivfpq_cases.py) and the list oracle (tests/list_cases.py).

Two row sets appear everywhere.  ``x`` / ``q`` are the rows and queries AS GIVEN: the store keeps x (rounded to float16 or not)
and the re-score takes q.  ``xs`` / ``qs`` are what the first stage sees: the same, or normalised under 'cosine' — by whoever
calls, with the normalisation of the thing it restates (on the CPU any will do: the theorems hold for all data)."""
import numpy as np

import ivfpq_cases as ic
import pq_cases as pc
from list_cases import list_topk_ref

MAX_K = 1024                                           # include/tsim.h TSIM_TOPK_MAX_K
LIST_SPACE = {"ip": "dot", "l2": "l2", "cosine": "cosine"}
D, M, NLIST, N_ROWS, K = 24, 6, 5, 700, 10             # the small seeded shape of the CPU theorems and their GPU twins
SEED = 11


def to_f16(x):
    with np.errstate(over="ignore"):                   # (beyond +-65 504: inf, which is what the table pins)
        return np.asarray(x).astype(np.float16)


def store_rows(x, refine):
    """what the store holds for the rows ``x`` as given"""
    return to_f16(x) if refine == "float16" else np.asarray(x, np.float32)


def refine_ref(space, q, store, cand, k):
    """(scores [Q, k], rows [Q, k]): the exact top-k of the float32 queries among the candidate rows ``cand`` [Q, m] (negatives
    dropped) of the store widened to float32.  ``space`` in the list search's names: 'cosine', 'dot', 'l2'."""
    s, i, _ = list_topk_ref(space, np.asarray(q, np.float32), np.asarray(store).astype(np.float32),
                            [np.asarray(r)[np.asarray(r) >= 0] for r in np.asarray(cand)], k, unique=False)
    return s, i


def first_stage_width(k, mult, n):
    return min(k * mult, MAX_K, n)


def pq_adc_ref(space, qs, codebooks, codes, m):
    """(values float32 [Q, m], rows int64 [Q, m]) of GpuPQIndex's one-stage search on prepared queries"""
    adc = "l2" if space == "l2" else "ip"
    tables, exps = pc.tables_ref(qs, codebooks, adc)
    v, i = pc.adc_topk_ref(tables, codes, m, adc)
    return pc.values_to_float(v, exps, adc), i


def pq_refined_ref(space, q, qs, codebooks, codes, store, k, mult):
    """GpuPQIndex.search(q, k, rescore_multiplier=mult): (scores, rows, candidates)"""
    _, cand = pq_adc_ref(space, qs, codebooks, codes, first_stage_width(k, mult, codes.shape[0]))
    s, i = refine_ref(LIST_SPACE[space], q, store, cand, k)
    return s, i, cand


def ivfpq_refined_ref(space, q, qs, centroids, codebooks, codes, lists, probes, store, k, mult, by_residual=True):
    """GpuIVFPQIndex.search(q, k, rescore_multiplier=mult) with the given probes: (scores, rows, candidates)"""
    adc = "l2" if space == "l2" else "ip"
    _, cand = ic.search_ref(qs, centroids, codebooks, codes, lists, probes, first_stage_width(k, mult, codes.shape[0]), adc,
                            by_residual=by_residual)
    s, i = refine_ref(LIST_SPACE[space], q, store, cand, k)
    return s, i, cand


def normalise_np(x):
    """a float32 normalisation for the CPU theorems (the GPU tests use the index's own)"""
    x = np.asarray(x, np.float32)
    n = np.sqrt((x.astype(np.float64) ** 2).sum(1, keepdims=True)).astype(np.float32)
    return (x / np.maximum(n, np.float32(1e-12))).astype(np.float32)


def small_data(seed=SEED, n=N_ROWS, nq=9, d=D, nlist=NLIST, m=M):
    """(centroids, codebooks, rows, queries): clustered rows as tests/test_ivfpq_index_gpu.py makes them.  The codebooks are
    random, not trained, so the ADC ranking is poor — recall at multiplier 1 is well below 1 (asserted on the CPU)."""
    rng = np.random.default_rng(seed)
    cent = (2 * rng.standard_normal((nlist, d))).astype(np.float32)
    x = (cent[rng.integers(0, nlist, size=n)] + rng.standard_normal((n, d))).astype(np.float32)
    q = (cent[rng.integers(0, nlist, size=nq)] + rng.standard_normal((nq, d))).astype(np.float32)
    return cent, pc.random_codebooks(rng, d, m), x, q


def nearest_lists_np(space, xs, cent, k):
    """a coarse assignment for the CPU theorems: the k best centroids by float64 score, ties to the lower list"""
    a, c = xs.astype(np.float64), cent.astype(np.float64)
    if space == "l2":
        s = -((a[:, None, :] - c[None]) ** 2).sum(-1)
    else:
        s = a @ c.T
        if space == "cosine":
            s = s / np.maximum(np.sqrt((c * c).sum(1)), 1e-12)[None]
    return np.argsort(-s, axis=1, kind="stable")[:, :k]


def recall(ids, exact_ids):
    """mean over queries of |ids ∩ exact_ids| / |exact_ids| (negatives are padding)"""
    hit = [len(set(a[a >= 0].tolist()) & set(b[b >= 0].tolist())) / max(1, int((b >= 0).sum())) for a, b in zip(ids, exact_ids)]
    return float(np.mean(hit))


# to_f16 at the rounding boundaries: (float32 value, the float16 bits it must give).  Ties go to the even mantissa.
F16_TABLE = (
    (1.0, 0x3C00),
    (1.0 + 2.0 ** -11, 0x3C00),                 # halfway between 1 and 1 + 2^-10: to even (down)
    (1.0 + 3 * 2.0 ** -11, 0x3C02),             # halfway between 1 + 2^-10 and 1 + 2^-9: to even (up)
    (1.0 + 2.0 ** -11 + 2.0 ** -23, 0x3C01),    # just above the tie: up
    (65504.0, 0x7BFF),                          # the largest finite half
    (65520.0 - 2.0 ** -7, 0x7BFF),              # the float32 below the tie at 65 520: still finite
    (65520.0, 0x7C00),                          # the smallest overflow: the tie goes to even, which is inf
    (-65520.0, 0xFC00),
    (2.0 ** -24, 0x0001),                       # the smallest subnormal
    (2.0 ** -25, 0x0000),                       # halfway to zero: to even (zero)
    (2.0 ** -25 + 2.0 ** -40, 0x0001),          # just above: the smallest subnormal
    (3 * 2.0 ** -25, 0x0002),                   # halfway between subnormals 1 and 2: to even
    (2.0 ** -14, 0x0400),                       # the smallest normal
    (2.0 ** -14 - 2.0 ** -25, 0x0400),          # halfway between the largest subnormal (odd) and the smallest normal: to even
    (1023 * 2.0 ** -24, 0x03FF),                # the largest subnormal
    (0.0, 0x0000),
    (-0.0, 0x8000),
    (-2.0 ** -24, 0x8001),
)
