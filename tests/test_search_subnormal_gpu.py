"""Does the f16 MFMA of the search's selection pass KEEP subnormal half inputs?  The cosine guard (csrc/common.h guard_eps,
l2norm_rows_kernel, query_rho<false>) is proven under that assumption only.  The spiky cases of tests/adversary.py hold unit
rows with 767 subnormal halves at d = 768; tests/test_guard_cpu.py shows on a model of a FLUSHING MFMA that the shipped guard
would then return wrong lists for them (the spiky row's selection score drops ~1.5e-3 = 2.5 eps: out of the first pass's
candidates and below the widening pass's threshold, status 1 all the same).  Here the same data go through the real kernels:
every list must be the oracle's, bit for bit.

Every search goes through ops with the float32 rows and the measured rho_c, d = 768, N <= 6 000.

Measured on MI355X (gfx950): the MFMA keeps them — every list exact, spiky-query status [1, 1] (printed and recorded, not
asserted, by test_spiky_queries_are_exact_and_the_status_is_recorded)."""
import functools

import numpy as np
import pytest
import torch

from adversary import spiky_case, spiky_query_case
from oracle import search_ref as sr
from text_similarity_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 768


@functools.lru_cache(maxsize=None)
def _case(k, KL):
    q, c, info = spiky_case(d=D, k=k, KL=KL)
    return q, c, info, sr.cosine_topk_f32(q[None], c, k)


def _topk(q, c, k):
    qf, cf = torch.from_numpy(np.atleast_2d(q)).to(DEV), torch.from_numpy(c).to(DEV)
    cu, rho = ops.l2norm_rows(cf, return_rho=True)
    s, i, st = ops.cosine_topk(ops.l2norm_rows(qf), cu, D, k, eq_f32=qf, ec_f32=cf, rho_c=rho, return_status=True)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy(), st.cpu().numpy(), float(rho.item())


@pytest.mark.parametrize("k,KL", [(10, 16), (20, 32), (100, None)])
def test_spiky_row_is_found(k, KL):
    """The spiky row has exact rank k.  k = 10: lists of 16; k = 20: lists of 32; k = 100: tsim_cosine_topk_large, whose
    collection threshold is (k-th largest block maximum) - 2 eps.  On a flushing MFMA the row would be missing (status 1)."""
    q, c, info, (rs, ri) = _case(k, KL)
    s, i, st, rho = _topk(q, c, k)
    print(f"k={k}: status {st.tolist()} rho_c {rho:.4e}; spiky row {info['spiky']} exact {info['exact']:.6f}, model selection "
          f"score kept {info['kept']:.6f} / flushed {info['flushed']:.6f} (drop {info['drop']:.3e}), eps {info['eps']:.3e}, "
          f"{info['neighbours']} neighbours over {info['span']:.3e}; flushed score {info['margin']:.3e} below k-th - 2 eps")
    assert ri[0, k - 1] == info["spiky"]
    np.testing.assert_array_equal(i, ri)
    np.testing.assert_array_equal(s, rs)
    assert rho >= info["rho_c"] and rho <= info["rho_c"] * (1 + 3e-6)     # the builder's eps is the kernel's


def test_spiky_row_is_in_the_range_result():
    """tau one float below the spiky row's exact cosine: the hits are the nine neighbours above it and the row itself.  The
    collect threshold is tau - eps; flushed, the row's selection score would sit ~0.9e-3 below that."""
    q, c, info, _ = _case(10, 16)
    exact = sr.exact_cosine(q[None], c)
    tau = np.nextafter(exact[0, info["spiky"]], np.float32(-np.inf))
    qf, cf = torch.from_numpy(q[None]).to(DEV), torch.from_numpy(c).to(DEV)
    cu, rho = ops.l2norm_rows(cf, return_rho=True)
    lims, s, i, st = ops.cosine_range(ops.l2norm_rows(qf), cu, D, float(tau), eq_f32=qf, ec_f32=cf, rho_c=rho, return_status=True)
    torch.cuda.synchronize()
    lims, s, i, st = lims.cpu().numpy(), s.cpu().numpy(), i.cpu().numpy(), st.cpu().numpy()
    hit = np.nonzero(exact[0] >= tau)[0]                                   # tests/test_range_search_gpu.py range_ref
    ref = hit[np.lexsort((hit, -exact[0][hit].astype(np.float64)))]
    print(f"range: status {st.tolist()}, {ref.size} hits, tau {tau:.7f}")
    assert ref.size == 10 and ref[-1] == info["spiky"]
    assert lims.tolist() == [0, 10]
    np.testing.assert_array_equal(i, ref)
    np.testing.assert_array_equal(s.view(np.uint32), exact[0, ref].view(np.uint32))


def test_spiky_queries_are_exact_and_the_status_is_recorded():
    """Query-side: both queries are spiky rows.  The lists must be exact.  The status of query 0 is a MEASUREMENT of the
    hardware, printed and not asserted: all its candidates are aligned with its subnormal elements, so a flushing MFMA
    scores each ~1.3e-3 = 4 eps low, the bound check on the candidates fails and the query goes to brute force (status 2); a
    keeping MFMA gives 0 or 1.  Query 1 is the case such a check cannot see (tests/test_guard_cpu.py): flushed, its list
    would be wrong with status 1.
    Recorded on MI355X (gfx950): status [1, 1], both lists exact — the f16 MFMA KEEPS subnormal half operands (DESIGN.md
    section 7, "Subnormal halves and strided rows")."""
    q, c, info = spiky_query_case(d=D)
    rs, ri = sr.cosine_topk_f32(q, c, 10)
    s, i, st, rho = _topk(q, c, 10)
    print(f"spiky queries: status {st.tolist()} (query 0: 2 = the MFMA flushes subnormal halves, 0 / 1 = it keeps them); "
          f"eps {info['eps'].tolist()}, model drop of the aligned rows when flushed {info['drop0']} / {info['drop1']}")
    np.testing.assert_array_equal(i, ri)
    np.testing.assert_array_equal(s, rs)


def test_l2norm_rows_reports_the_residual_of_spiky_rows():
    """rho of rows that are almost entirely subnormal halves, against the oracle's (kept) residual, in the band of
    test_l2norm_rows_reports_the_residual_maximum — one row at a time and accumulated."""
    rng = np.random.default_rng(5)
    rows = []
    for t in (6.0e-5, 3.1e-5, 1.0e-6, 2.0e-8):          # the last one rounds to zero halves: residual = the elements
        w = np.where(rng.standard_normal(D) >= 0, 1.0, -1.0) * t
        w[rng.integers(D)] = np.sqrt(1.0 - (D - 1) * t * t)
        rows.append(w * 10.0 ** rng.uniform(-2, 2))
    x = np.stack(rows).astype(np.float32)
    want = sr.rho_rows(x)
    xt = torch.from_numpy(x).to(DEV)
    acc = ops.new_rho(DEV)
    for r in range(x.shape[0]):
        _, rho = ops.l2norm_rows(xt[r:r + 1], return_rho=True)
        ops.l2norm_rows(xt[r:r + 1], rho=acc)
        got = float(rho.item())
        print(f"row {r}: rho {got:.6e} oracle {want[r]:.6e} (flush-safe {sr.rho_rows(x[r:r + 1], flush_safe=True)[0]:.6e})")
        assert got >= want[r] and got <= want[r] * (1 + 3e-6)
    assert float(acc.item()) >= want.max() and float(acc.item()) <= want.max() * (1 + 3e-6)
    assert float(acc.item()) <= sr.rho_apriori(D)
