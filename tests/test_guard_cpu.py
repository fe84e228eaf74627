"""CPU checks of the search's exactness guard (oracle/search_ref.guard_eps == csrc/common.h guard_eps): the BOUND it rests on
holds on random, anisotropic and adversarially rounded rows, and the adversarial fixture of VERDICT r2 defeats a sampled-error
guard while the bound-based guard flags it.

Subnormal halves (last item): the cosine guard's residual rho = ||half(u) - u|| assumes that the f16 MFMA KEEPS
subnormal half inputs.  The spiky cases of tests/adversary.py (unit rows with 767 subnormal halves) are replayed here on both
models of the MFMA: kept — the bound holds and the replayed call returns the oracle's list; flushed with the shipped
residuals — the bound fails and the replayed call returns a WRONG list (what tests/test_search_subnormal_gpu.py guards
against on the hardware); flushed with the flush-safe residuals (common.h flush_safe_err, as the inner-product path
measures them) — exact again."""
import functools

import numpy as np
import pytest

from adversary import adversarial_case, aligned_rounding_row, spiky_case, spiky_query_case
from oracle import search_ref as sr


def _max_violation(q, c, order, flush=False, flush_safe=False):
    m = sr.mfma_model_scores(q, c, order, flush=flush).astype(np.float64)
    ex = sr.exact_cosine(q, c).astype(np.float64)
    eps = sr.guard_eps(sr.rho_rows(q, flush_safe=flush_safe)[:, None], sr.rho_rows(c, flush_safe=flush_safe)[None, :], c.shape[1])
    return float((np.abs(m - ex) - eps).max()), float((np.abs(m - ex) / eps).max())


def test_bound_holds_on_random_and_anisotropic_rows():
    rng = np.random.default_rng(0)
    for d in (64, 384, 768):
        q = (rng.standard_normal((8, d)) * np.exp(rng.uniform(-3, 3, (8, 1)))).astype(np.float32)
        c = (rng.standard_normal((500, d)) * np.exp(rng.uniform(-3, 3, (500, 1)))).astype(np.float32)
        base = rng.standard_normal(d).astype(np.float32) * 20
        c[250:] = base + rng.standard_normal((250, d)).astype(np.float32)       # cosines ~0.9975 among themselves
        q[4:] = base + rng.standard_normal((4, d)).astype(np.float32)
        c[7] = 0.0                                                              # zero row: unit image 0, cosine 0
        c[8] = 1e-30                                                            # norm below eps: clamped scale
        for order in ("f64", "f32seq"):
            viol, ratio = _max_violation(q, c, order)
            assert viol <= 0.0, (d, order, viol)
        assert sr.rho_rows(c).max() <= sr.rho_apriori(d) and sr.rho_rows(q).max() <= sr.rho_apriori(d)


def test_bound_is_nearly_attained_by_aligned_rounding():
    """The adversarial row errs by ~0.49 sum|q_i| ulp_i ~ 3e-4 at d = 384: 7-10x the typical error, and still inside eps."""
    rng = np.random.default_rng(1)
    d = 384
    q = rng.standard_normal(d).astype(np.float32)
    row, exact, sel = aligned_rounding_row(q, 0.9496, rng)
    ex = float(sr.exact_cosine(q[None], row[None])[0, 0])
    m = float(sr.mfma_model_scores(q[None], row[None])[0, 0])
    assert abs(ex - exact) < 1e-6 and abs(ex - 0.9496) < 5e-5
    assert 2.0e-4 < ex - m < 4.5e-4                                  # the selection score is far too low ...
    eps = float(sr.guard_eps(sr.rho_rows(q[None])[0], sr.rho_rows(row[None])[0], d))
    assert ex - m <= eps <= 8e-4                                     # ... but inside the bound, which is not vacuous


def test_adversarial_row_defeats_a_sampled_guard_and_is_flagged_by_the_bound():
    q, c = adversarial_case()
    truth = sr.cosine_topk_f32(q[None], c, 10)[1][0]
    assert truth.tolist() == list(range(100, 109)) + [5000]
    top, safe, eps, cut, sk = sr.guard_replay(q, c, 10, 16, mode="sampled")
    assert 5000 not in top and top.tolist() == list(range(100, 110))          # first pass misses the row ...
    assert safe                                                               # ... and the sampled-error guard accepts it
    top, safe, eps, cut, sk = sr.guard_replay(q, c, 10, 16, mode="bound")
    assert not safe and 3e-4 < eps < 8e-4                                     # the bound-based guard flags the query
    m = sr.mfma_model_scores(q[None], c)[0]
    assert m[5000] > sk - eps                                                 # and the widening threshold collects the row
    # with the a-priori rho (no measured maximum) the guard is looser, never unsafe
    _, safe2, eps2, _, _ = sr.guard_replay(q, c, 10, 16, mode="bound", rho_c=sr.rho_apriori(384))
    assert not safe2 and eps2 > eps


def test_duplicates_with_a_better_near_duplicate():
    """>= KL exact duplicates of one row fill the candidate list with identical errors; a near-duplicate with a
    HIGHER exact cosine can score lower on the half rows.  The bound-based guard must flag (cut ~ k-th exact score)."""
    rng = np.random.default_rng(3)
    d, N = 384, 4000
    for KL, k in ((16, 10), (32, 20)):
        hit = 0
        for trial in range(40):
            q = rng.standard_normal(d).astype(np.float32)
            c = rng.standard_normal((N, d)).astype(np.float32)
            c0 = (q + 0.35 * rng.standard_normal(d)).astype(np.float32)
            c[200:200 + KL + 4] = c0
            c[3000] = (c0 + 1e-3 * rng.standard_normal(d)).astype(np.float32)
            top, safe, *_ = sr.guard_replay(q, c, k, KL, mode="bound")
            assert not safe                       # KL identical candidates: cut == their score, nothing separates the rest
            ex = sr.exact_cosine(q[None], c[[200, 3000]])[0]
            m = sr.mfma_model_scores(q[None], c[[200, 3000]])[0]
            hit += int(ex[1] > ex[0] and m[1] < m[0])
        assert hit > 0      # the scenario does occur: the better row is ranked below the duplicates by the half rows


# ---------------------------------------------------------------------------------------------------------- subnormal halves
@functools.lru_cache(maxsize=None)
def _spiky(k, KL):
    q, c, info = spiky_case(d=768, k=k, KL=KL)
    return q, c, info, sr.cosine_topk_f32(q[None], c, k)[1][0]


@pytest.mark.parametrize("k,KL", [(10, 16), (20, 32), (100, None)])
def test_spiky_row_kept_is_exact_flushed_is_wrong_flush_safe_is_exact(k, KL):
    """d = 768, the smallest padded width at which the drop (t sum|q_j| ~ 1.5e-3) exceeds what the widening pass forgives."""
    q, c, info, truth = _spiky(k, KL)
    spiky = info["spiky"]
    print(f"k={k} KL={KL}: exact {info['exact']:.6f} kept {info['kept']:.6f} flushed {info['flushed']:.6f} "
          f"drop {info['drop']:.3e} eps {info['eps']:.3e} neighbours {info['neighbours']} over {info['span']:.3e}, "
          f"flushed score {info['margin']:.3e} below (k-th score - 2 eps)")
    assert truth[k - 1] == spiky and info["drop"] > 2.0 * info["eps"]
    # kept model, shipped residuals: the replayed call returns the oracle's list, and the spiky row is why it had to widen
    got, st = sr.search_replay(q, c, k, KL)
    assert got.tolist() == truth.tolist() and st == 1
    # flushed model, shipped residuals: the first pass misses the row, the widening threshold does not collect it, the
    # re-check of the widened list passes: a flushing MFMA would return a wrong list with status 1
    got, st = sr.search_replay(q, c, k, KL, flush=True)
    assert spiky not in got and st == 1 and got.tolist() != truth.tolist()
    mf = sr.mfma_model_scores(q[None], c, flush=True)[0]
    if KL is not None:
        top, safe, eps, cut, sk = sr.guard_replay(q, c, k, KL, flush=True)
        assert spiky not in top and not safe
        assert mf[spiky] < sr.guard_tau(sk, eps) and mf[spiky] < sk - 2.0 * eps
    # flushed model, flush-safe residuals: the row is collected (or everything is: brute force) and the list is exact
    got, st = sr.search_replay(q, c, k, KL, flush=True, flush_safe=True)
    assert got.tolist() == truth.tolist() and st in (1, 2)
    if KL is not None:
        top, safe, eps, cut, sk = sr.guard_replay(q, c, k, KL, flush=True, flush_safe=True)
        assert not safe and mf[spiky] > sr.guard_tau(sk, eps)


def test_spiky_row_bound_on_every_pair():
    q, c, info, _ = _spiky(10, 16)
    for order in ("f64", "f32seq"):
        assert _max_violation(q[None], c, order)[0] <= 0.0                                     # kept: the shipped bound holds
        assert _max_violation(q[None], c, order, flush=True, flush_safe=True)[0] <= 0.0        # flushed: the flush-safe one
        viol, ratio = _max_violation(q[None], c, order, flush=True)                            # flushed, shipped: it fails
        assert viol > 0.0 and ratio > 2.0, (viol, ratio)
    # the flush-safe residual of a Gaussian unit row at d = 768 is the shipped one to within a few percent: ~one subnormal
    # element of at most 6.1e-5 in quadrature with ~2.3e-4
    g = np.delete(np.arange(c.shape[0]), np.concatenate([info["slots"], [info["spiky"]]]))
    kept, safe = sr.rho_rows(c[g]), sr.rho_rows(c[g], flush_safe=True)
    assert (safe >= kept).all() and safe.max() <= np.sqrt(kept.max() ** 2 + 6 * sr.HALF_MIN_NORMAL ** 2)


def test_spiky_query_bound_and_replay():
    """Query-side: the spiky rows are the queries.  Query 0's best rows are all aligned with its signs: flushed, every
    candidate misses the bound and the check on the candidates sends the query to brute force (status 2 — the signature
    the GPU test records).  Query 1's aligned rows sit between unaligned neighbours: flushed, the candidates are honest
    neighbours, the check passes and the list is wrong."""
    q, c, info = spiky_query_case()
    truth = sr.cosine_topk_f32(q, c, 10)[1]
    print(f"eps {info['eps']}, drop of the aligned rows under the flushed model: query 0 {info['drop0']}, query 1 {info['drop1']}")
    for order in ("f64", "f32seq"):
        assert _max_violation(q, c, order)[0] <= 0.0
        assert _max_violation(q, c, order, flush=True, flush_safe=True)[0] <= 0.0
        assert _max_violation(q, c, order, flush=True)[1] > 2.0
    for qi in (0, 1):
        got, st = sr.search_replay(q[qi], c, 10, 16)
        assert got.tolist() == truth[qi].tolist() and st in (0, 1)
        got, st = sr.search_replay(q[qi], c, 10, 16, flush=True, flush_safe=True)
        assert got.tolist() == truth[qi].tolist()
    got, st = sr.search_replay(q[0], c, 10, 16, flush=True)
    assert st == 2 and got.tolist() == truth[0].tolist()
    got, st = sr.search_replay(q[1], c, 10, 16, flush=True)
    assert st == 1 and got.tolist() != truth[1].tolist() and not set(info["aligned1"]) & set(got)
