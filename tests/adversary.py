"""Adversarial corpora for the search's exactness guard (test data builders; numpy only).

``aligned_rounding_row``: a float32 row whose unit image sits ``frac`` of a half-precision ulp past a grid point in EVERY
element, on the side that makes the rounding LOWER q.c — the worst case of the half-row selection error (~3e-4 at d = 384,
7-10x the typical error).  ``neighbours``: rows at prescribed exact cosines.  VERDICT r2 "What's weak 1".

``spiky_row`` / ``spiky_case`` / ``spiky_query_case``: unit rows made of one large element and d - 1 elements that are
SUBNORMAL as halves (|u_j| = t < 2^-14).  The guard's residual rho = ||half(u) - u|| is nearly zero for such a row, which is
right only while the f16 MFMA keeps subnormal inputs; if it flushed them the row's selection score would lose
t sum|q_j| ~ 1.6e-3 at d = 768, three times the guard's eps.  ADVICE r3, last item."""
import numpy as np

from oracle import search_ref as sr


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum())


def row_at_cosine(q, cos_t, rng):
    """float64 unit vector with cosine cos_t to q."""
    uq = _unit(q)
    r = rng.standard_normal(uq.size)
    r -= (r @ uq) * uq
    return cos_t * uq + np.sqrt(1.0 - cos_t * cos_t) * _unit(r)


def neighbours(q, cosines, rng, scale=1.0):
    return np.stack([row_at_cosine(q, float(ct), rng) * scale for ct in cosines]).astype(np.float32)


def aligned_rounding_row(q, cos_target, rng, frac=0.49, scale=3.7):
    """Returns (row float32 [d], exact cosine with q, selection score = dot of the half images).  The row's exact cosine is
    within ~1e-5 of cos_target; its half image scores ~0.49 sum|q_i| ulp_i lower."""
    uq = _unit(q)
    sgn = np.where(uq >= 0, 1.0, -1.0)
    uqh = uq.astype(np.float16).astype(np.float64)
    cos_t = cos_target - 3e-4
    best = None
    for _ in range(8):
        v = row_at_cosine(q, cos_t, rng)
        beta = 1.0
        for _ in range(60):
            g16 = (beta * v).astype(np.float16)
            g = g16.astype(np.float64)
            ulp = np.spacing(np.abs(g16)).astype(np.float64)            # spacing towards larger magnitude
            toward_zero = (sgn * np.sign(g)) < 0
            pow2 = np.frexp(np.abs(g))[0] == 0.5
            step = np.where(toward_zero & pow2, 0.5 * ulp, ulp)         # below a power of two the grid is twice as fine
            w = g + frac * step * sgn
            n = np.sqrt((w * w).sum())
            if abs(n - 1.0) < 2e-6:
                break
            beta /= n
        j = int(np.argmax(np.abs(w)))                                    # absorb the remaining norm defect in one element
        rest = (w * w).sum() - w[j] * w[j]
        w[j] = np.sign(w[j]) * np.sqrt(max(1.0 - rest, 0.0))
        assert np.array_equal(w.astype(np.float16)[np.arange(w.size) != j], g16[np.arange(w.size) != j])
        exact = float(w @ uq)
        sel = float(w.astype(np.float16).astype(np.float64) @ uqh)
        best = ((w * scale).astype(np.float32), exact, sel)
        if abs(exact - cos_target) < 1e-5:
            break
        cos_t += cos_target - exact
    return best


def adversarial_case(seed=0, N=20000, d=384, spacing=4.2e-5):
    """30 neighbours c[100+j] spaced `spacing` apart in exact cosine and one aligned-rounding row (5000)
    whose exact cosine sits between the 9th and the 10th of them (rank 10) while its selection score falls below the 16th.
    Returns (q [d], c [N, d]) float32."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(d).astype(np.float32)
    c = rng.standard_normal((N, d)).astype(np.float32)
    row, s_star, _ = aligned_rounding_row(q, 0.9496, rng)
    c[5000] = row
    c[100:130] = neighbours(q, s_star + (8.5 - np.arange(30)) * spacing, rng, scale=2.0)
    return q, c


# ---------------------------------------------------------------------------------------------------------------------
# Subnormal halves: what a flushing f16 MFMA would get wrong
# ---------------------------------------------------------------------------------------------------------------------
def uniform_bulk_query(d, rng, first=0.3, jitter=0.1):
    """Dense query whose unit image is ~(first, +-b, ..): a bulk of nearly uniform magnitude (+- jitter, so that the half
    rounding errors of its elements are spread like a generic row's) gives the largest sum|q_j| for its norm, hence the
    largest drop of a spiky row under the flushed model: ~sqrt(d - 1) t |q_bulk|, against 0.8 of that for a Gaussian bulk."""
    b = np.sqrt((1.0 - first * first) / (d - 1))
    q = np.empty(d)
    q[0] = first
    q[1:] = b * (1.0 + jitter * rng.uniform(-1, 1, d - 1)) * rng.choice([-1.0, 1.0], d - 1)
    return (q * 1.7).astype(np.float32)


def spiky_unit(signs, t):
    """float64 unit vector (sign_0 a, sign_1 t, .., sign_{d-1} t)."""
    w = np.where(np.asarray(signs) >= 0, 1.0, -1.0) * t
    w[0] = np.sign(w[0]) * np.sqrt(1.0 - (w.size - 1) * t * t)
    return w


def spiky_row(q, t=6.0e-5, scale=2.3):
    """Returns (row float32 [d], exact cosine with q, selection score with subnormal halves kept, the same with them flushed).
    The row's unit image has one large element (the first) and d - 1 elements sign(q_j) t that are subnormal as halves
    (t < 2^-14): kept, the half image scores within ~1e-6 of the exact cosine; flushed, t sum_j>0 |uq_j| lower."""
    assert 2.0 ** -24 < t < sr.HALF_MIN_NORMAL
    q = np.asarray(q, dtype=np.float32)
    row = (spiky_unit(q, t) * scale).astype(np.float32)
    exact = float(sr.exact_cosine(q[None], row[None])[0, 0])
    kept = float(sr.mfma_model_scores(q[None], row[None])[0, 0])
    flushed = float(sr.mfma_model_scores(q[None], row[None], flush=True)[0, 0])
    h = sr.unit_rows(row[None])[0]
    assert (np.abs(h[1:]) < sr.HALF_MIN_NORMAL).all() and (h[1:] != 0).all() and abs(h[0]) > 0.99
    return row, exact, kept, flushed


def fullmax_slots(N, k, count, skip=()):
    """`count` corpus rows in pairwise different partitions of the k > 28 block-maxima pass (sr.fullmax_partition), none in
    `skip`: the k-th largest block maximum then is the k-th best of the rows placed there."""
    rows, seen = [], set(int(p) for p in sr.fullmax_partition(np.asarray(list(skip), dtype=np.int64), N, k))
    for r in range(17, N, 4):
        p = int(sr.fullmax_partition(np.asarray([r]), N, k)[0])
        if p not in seen:
            seen.add(p)
            rows.append(r)
            if len(rows) == count:
                return np.asarray(rows)
    raise AssertionError(f"N = {N} has fewer than {count} free partitions at k = {k}")


def spiky_case(d=768, k=10, KL=16, N=5000, seed=0, t=6.0e-5, below=None, spacing=None, margin=5e-5):
    """Row-side case.  Returns (q [d], c [N, d], info): Gaussian corpus, the spiky row at c[info['spiky']] with exact rank k
    for q, k - 1 dense neighbours above it and `below` under it, `spacing` apart in exact cosine, each in a partition of its
    own.  KL = 16 / 32: the list path of k (k1_topk.h plan_topk); KL = None: the k > 28 path.
    The builder asserts what makes the case adversarial, on the model of a FLUSHING MFMA and with the guard's shipped
    (kept-assuming) residuals: the rows the first pass keeps do not include the spiky row, and its flushed selection score
    lies more than `margin` below the collection threshold even in its widest form (k-th score - 2 eps) — so the widening
    pass would not collect it either — while on the kept model it is collected."""
    rng = np.random.default_rng(seed)
    q = uniform_bulk_query(d, rng)
    c = rng.standard_normal((N, d)).astype(np.float32)
    row, s_star, kept, flushed = spiky_row(q, t)
    if below is None:
        below = 36 if KL is not None else 24
    if spacing is None:
        spacing = 4.2e-5 if KL is not None else 4.0e-6
    spiky = N - 1000
    slots = fullmax_slots(N, max(k, 29), k - 1 + below, skip=(spiky,))
    c[spiky] = row
    # k - 1 above (the nearest half a step away), `below` under
    c[slots] = neighbours(q, s_star + (k - 1.5 - np.arange(k - 1 + below)) * spacing, rng, scale=2.0)
    ex = sr.exact_cosine(q[None], c)[0]
    order = np.lexsort((np.arange(N), -ex.astype(np.float64)))
    assert order[k - 1] == spiky and set(order[:k - 1]) == set(slots[:k - 1])
    rho_c = float(sr.rho_rows(c).max())                       # what l2norm_rows reports: the shipped, kept-assuming residual
    eps = float(sr.guard_eps(sr.rho_rows(q[None])[0], rho_c, d))
    mk = sr.mfma_model_scores(q[None], c)[0]
    mf = sr.mfma_model_scores(q[None], c, flush=True)[0]
    assert abs(float(mk[spiky]) - kept) == 0 and abs(float(mf[spiky]) - flushed) == 0
    above = int((mf > mf[spiky]).sum())
    if KL is not None:
        top, safe, _, cut, sk = sr.guard_replay(q, c, k, KL, flush=True)
        assert above >= KL and spiky not in top, (above, KL)
        base = sk                                             # the first pass's k-th exact score
    else:
        part = sr.fullmax_partition(np.arange(N), N, k)
        bmax = np.full(int(part.max()) + 1, -np.inf)
        np.maximum.at(bmax, part, mf.astype(np.float64))
        base = float(np.sort(bmax)[::-1][k - 1])              # B: the k-th largest block maximum
        assert above >= k
    assert flushed < base - 2.0 * eps - margin, (flushed, base, eps)      # flushed: out of reach of the widening pass
    assert kept > s_star - 0.1 * eps                                      # kept: nearly exact, collected with room
    info = dict(spiky=spiky, slots=slots, exact=s_star, kept=kept, flushed=flushed, drop=s_star - flushed, eps=eps, rho_c=rho_c,
                span=(k - 1 + below - 1) * spacing, neighbours=k - 1 + below, above_flushed=above, base=base,
                margin=base - 2.0 * eps - flushed)
    return q, c, info


def aligned_row_at_cosine(uq_spiky, cos_t, rng):
    """float64 unit row (x, s_j b_j ..) with cosine cos_t to the spiky unit query: a dense bulk whose signs follow the
    query's, so that the query's d - 1 subnormal elements contribute t sum|c_j| ~ 1.3e-3 to the score."""
    d = uq_spiky.size
    g = np.abs(rng.standard_normal(d - 1))
    g /= np.sqrt((g * g).sum())
    t, a = abs(uq_spiky[1]), abs(uq_spiky[0])
    x = cos_t / a
    for _ in range(50):
        x = (cos_t - t * g.sum() * np.sqrt(1.0 - x * x)) / a
    v = np.empty(d)
    v[0] = x * np.sign(uq_spiky[0])
    v[1:] = np.sqrt(1.0 - x * x) * g * np.sign(uq_spiky[1:])
    return v


def spiky_query_case(d=768, N=4000, seed=0, t=6.0e-5, spacing=4.2e-5):
    """Query-side case.  Returns (q [2, d], c [N, d], info): both queries are spiky (one large element, d - 1 subnormal halves,
    independent sign patterns); the corpus is Gaussian plus, per query, dense rows near exact cosine 0.3.
    Query 0: its 40 best rows are all ALIGNED with its sign pattern.  A flushing MFMA scores every one of them ~1.3e-3 low
    (the score collapses to the one product of the large element), which the bound check on the candidates sees: brute
    force, status 2.  A keeping MFMA scores them within eps: status 0 or 1.
    Query 1: aligned rows at exact ranks 2, 4, .., 10 between 30 unaligned neighbours.  A flushing MFMA ranks the aligned rows
    below every neighbour, the candidates are neighbours with honest errors, the check passes — and the list is wrong."""
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((N, d)).astype(np.float32)
    uq = np.stack([spiky_unit(rng.choice([-1.0, 1.0], d), t) for _ in range(2)])
    q = (uq * np.array([[3.1], [0.7]])).astype(np.float32)
    rows0 = 100 + 7 * np.arange(40)
    c[rows0] = np.stack([aligned_row_at_cosine(uq[0], 0.3 - j * spacing, rng) * 1.9 for j in range(40)]).astype(np.float32)
    rows1 = 2000 + 11 * np.arange(30)
    c[rows1] = neighbours(q[1], 0.3 - np.arange(30) * spacing, rng, scale=2.0)
    al1 = 3000 + 13 * np.arange(5)
    c[al1] = np.stack([aligned_row_at_cosine(uq[1], 0.3 - (j + 0.5) * spacing, rng) * 0.8 for j in range(5)]).astype(np.float32)
    h = sr.unit_rows(q)
    assert (np.abs(h[:, 1:]) < sr.HALF_MIN_NORMAL).all() and (h[:, 1:] != 0).all()
    ex = sr.exact_cosine(q, c)
    o0 = np.lexsort((np.arange(N), -ex[0].astype(np.float64)))
    o1 = np.lexsort((np.arange(N), -ex[1].astype(np.float64)))
    assert o0[:40].tolist() == rows0.tolist()
    assert o1[1:10:2].tolist() == al1.tolist() and set(o1[:35]) == set(rows1) | set(al1)
    mf = sr.mfma_model_scores(q, c, flush=True)
    rho_c = float(sr.rho_rows(c).max())
    eps = sr.guard_eps(sr.rho_rows(q), rho_c, d)
    drop0 = ex[0][rows0].astype(np.float64) - mf[0][rows0]
    drop1 = ex[1][al1].astype(np.float64) - mf[1][al1]
    assert drop0.min() > 2.0 * eps[0] and drop1.min() > 2.0 * eps[1] + 10 * spacing
    info = dict(rows0=rows0, rows1=rows1, aligned1=al1, eps=eps, rho_c=rho_c, drop0=(float(drop0.min()), float(drop0.max())),
                drop1=(float(drop1.min()), float(drop1.max())))
    return q, c, info
