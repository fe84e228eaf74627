"""Test-local oracle of the exact Euclidean range search (include/tsim.h tsim_l2_range_scan), shared by tests/test_l2_range_cpu.py
and tests/test_l2_range_gpu.py, on top of tests/l2_cases.py: the hits of a radius in (distance asc, index asc) order, the host
mirror of the set-up kernel's eps and nqs, the width of the band the collect pass gathers around the radius (which decides the
status a query must have), and the data sets both files use."""
from fractions import Fraction

import numpy as np

from l2_cases import aug_corpus, aug_queries, corpus_scale
from oracle import search_ref

SLOT_CAP = 2048          # include/tsim.h TSIM_RANGE_SLOT_CAP (the tests assert ops.RANGE_SLOT_CAP == this)


def range_ref(dist_f32, radius):
    """The rows of one query with float32 distance <= float32(radius), ordered by (distance asc, index asc).  NaN hits nothing."""
    dist_f32 = np.asarray(dist_f32, dtype=np.float32)
    hit = np.nonzero(dist_f32 <= np.float32(radius))[0]
    return hit[np.argsort(dist_f32[hit], kind="stable")]


def dist_up(r):
    """csrc/search.hip l2_dist_up: above every float64 distance that rounds to a float32 <= r."""
    return float(np.float32(r)) * (1.0 + 1.1921e-7) + 1e-44


def mirror(q, c, ld):
    """(A, eps [Q] float64 of the float32 bound, nqs [Q], qq [Q]) as range_setup_kernel<SM_L2> derives them: A from the corpus'
    largest norm, eps = guard_eps(rho_q, rho_c, ld) over the d + 1 elements of the augmented rows, nqs = nq' 2A."""
    A = corpus_scale(c)
    _, rho_c = aug_corpus(c, A)
    _, rho_q, qq, nq = aug_queries(q, A)
    eps = np.array([float(np.float32(search_ref.guard_eps(r, rho_c, ld))) for r in rho_q])
    return A, eps, nq * 2.0 * A, qq


def band(eps, nqs):
    """W: a collected row has an MFMA score above thr ~ (|q|^2 - up(r)) / (2 nqs) - eps, and its score is within eps of
    (|q|^2 - dist^2) / (2 nqs), so dist^2 < up(r) + 4 eps nqs; the factor 2 is slack for the 1e-13 / 1e-14 terms and the float32
    steps of the threshold."""
    return 2.0 * (4.0 * eps * nqs)


def must_be_collected(dist_f64, radius, eps, nqs):
    """True when the query must have status 1: every row the collect pass can gather (dist^2 < up(r) + W) fits the slot."""
    return int((np.asarray(dist_f64) < dist_up(radius) + band(eps, nqs)).sum()) <= SLOT_CAP


def unit_norm_rows(rng, n, d, lo=0.5, hi=2.0):
    """Gaussian directions with norms uniform in lo .. hi"""
    x = rng.standard_normal((n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return (x * rng.uniform(lo, hi, (n, 1))).astype(np.float32)


GAUSS_DIMS = (127, 128, 300, 384, 767)      # the widths around the padding steps of d + 1, the 512-wide case, the maximum
# One radius (query 0's) serves all 8 queries, whose norms differ: the seeds are those at which every query's band around that
# radius fits the collect slot (found, and re-checked by tests/test_l2_range_cpu.py, with the oracle alone).
GAUSS_SEEDS = {127: 0, 128: 1, 300: 3, 384: 3, 767: 0}


def gauss_case(d, n=3000, nq=8):
    """(q, c): the Gaussian case of the GPU test for one width; tests/test_l2_range_cpu.py checks with the oracle alone that
    every query must have status 1 at the selective radius."""
    rng = np.random.default_rng(1000 * d + GAUSS_SEEDS[d])
    return unit_norm_rows(rng, nq, d), unit_norm_rows(rng, n, d)


def selective_radii(dist_f32_q0):
    """The 10th-smallest distance of query 0 (a real tie on the radius) and its float32 predecessor."""
    r = np.sort(np.asarray(dist_f32_q0, dtype=np.float32))[9]
    return r, np.nextafter(r, np.float32(-np.inf))


def fused_pair(d=65):
    """tests/test_l2_search_gpu.py test_square_and_sum_are_rounded_separately: elements 0 and 64 of a pair of rows whose other
    differences are zero, such that the canonical sum round(round(d0^2) + round(d1^2)) and a fused fma(d1, d1, d0^2) round to
    different float32 distances.  Returns (q0, q1, c1, unfused, fused): q[0] = q0, q[64] = q1, c[0] = 0, c[64] = c1."""
    q0, q1, c1 = (float.fromhex(h) for h in ("0x1.a763c4p+0", "0x1.fa8492p-3", "-0x1.f8326ap-28"))
    assert all(float(np.float32(v)) == v for v in (q0, q1, c1))
    d0, d1 = q0 - 0.0, q1 - c1
    unfused = np.float32(d0 * d0 + d1 * d1)                  # (d0^2 is exact; Python rounds the product and the sum separately)
    fused = np.float32(float(Fraction(d1) * Fraction(d1) + Fraction(d0 * d0)))
    assert unfused != fused and unfused == np.float32(2.7964415550231934)
    return q0, q1, c1, unfused, fused
