"""Every entry point that takes a row stride, on rows placed FAR APART (tests/far_cases.py): 6 000 rows whose offsets from the
pointer the kernel is handed cross 2^31 and 2^32 bytes (the code rows, Layout B, 4.72 GB) and 2^31, 2^32, 2^33 and 2^34 bytes —
2^31 and 2^32 elements — (the float32 rows, Layout F, 17.26 GB), one row straddling 2^32 bytes.  The buffer around the rows is
0xFF: a kernel that drops one (int64_t), or builds a 32-bit byte offset, reads NaN, -1 or all-ones codes, or another row.

Two bars in every test, both array_equal on values, indices, statuses and counts: the result on the far view equals the result
of the same call on a compact .contiguous() copy, and it equals the existing oracle or numpy restatement.  tests/
test_far_cases_cpu.py shows on the CPU that the oracles see every modelled truncation on exactly these inputs.

Findings — operands ops forces contiguous, so that no far view reaches their kernels (they are left out here; ops is not
loosened): the input of l2norm_rows, max_norm_rows, dot_scaled_rows, l2_rows and l2_query_rows (``x.contiguous()`` /
``_rows_operand``: a strided view is copied by torch first; the C entries take ld_in and tests/test_search_strided_gpu.py reaches
them only through that copy); the half rows of every MFMA search and the graph adjacency (tests/test_large_corpus_gpu.py
covers those with truly large operands); row_ids, list_off, probes of the IVF entries, seeds and entries of the graph search.
pack_sign_rows, quantize_int8_rows and pq_encode_rows read a strided view in place and are tested with a far input.

Needs 18.5 GB of free device memory for the Layout F tests and 6 GB for the Layout B ones (one buffer lives at a time)."""
import gc

import numpy as np
import pytest
import torch

import far_cases as fc
import graph_cases as gcs
import graph_seed_cases as gsc
import hamming_cases as hc
import int8_cases as i8
import ivf_cases as ivc
import ivfpq_cases as ipc
import pq_cases as pc
from list_cases import list_topk_ref, csr
from oracle.search_ref import cosine_topk_f32
from l2_cases import l2_topk_ref
from text_similarity_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KS = (10, 29, 100)
SPACES = ("cosine", "dot", "l2")
NEED = {"F": fc.LAYOUT_F.nbytes + (5 << 28), "B": fc.LAYOUT_B.nbytes + (5 << 28)}


class _Far:
    """the far buffer of one layout at a time"""

    def __init__(self):
        self.fb = None

    def get(self, name):
        if self.fb is None or self.fb.layout.name != name:
            self.release()
            free = torch.cuda.mem_get_info()[0]
            if free < NEED[name]:
                pytest.skip(f"layout {name} needs {NEED[name] / 1e9:.1f} GB of device memory, {free / 1e9:.1f} GB are free")
            self.fb = fc.FarBuffer(fc.LAYOUTS[name], DEV)
        return self.fb

    def release(self):
        self.fb = None
        gc.collect()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def far():
    torch.cuda.reset_peak_memory_stats()
    holder = _Far()
    yield holder
    holder.release()
    print(f"\ntests/test_far_rows_gpu.py: peak device memory allocated {torch.cuda.max_memory_allocated() / 1e9:.2f} GB")


def _dev(x, dtype=None):
    return torch.from_numpy(np.array(x, dtype=dtype, order="C")).to(DEV)


def _np(out):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (out if isinstance(out, (tuple, list)) else (out,)))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    assert len(got) == len(want)
    for n, (g, w) in enumerate(zip(got, want)):
        np.testing.assert_array_equal(_bits(g), _bits(np.asarray(w, dtype=g.dtype)), err_msg=f"{what}: output {n}")


def _far_and_compact(far, layout, x, stride=None):
    v = far.get(layout).place(x, stride)
    c = v.contiguous()
    assert c.is_contiguous() and c.data_ptr() != v.data_ptr()
    return v, c


# ------------------------------------------------------------------------------------------------- Layout F: float32 rows far
def _operands(space, qf, cf):
    """the half rows, made from the float32 rows by the row kernels (which copy a view first): they stay compact"""
    if space == "dot":
        cn, rho, scale = ops.dot_scaled_rows(cf)
        return ops.l2norm_rows(qf), cn, dict(rho_c=rho, scale_c=scale)
    if space == "l2":
        cn, rho, scale = ops.l2_rows(cf)
        return ops.l2_query_rows(qf, scale), cn, dict(rho_c=rho, scale_c=scale)
    cn, rho = ops.l2norm_rows(cf, return_rho=True)
    return ops.l2norm_rows(qf), cn, dict(rho_c=rho)


_TOPK = {"cosine": ops.cosine_topk, "dot": ops.dot_topk, "l2": ops.l2_topk}
_RANGE = {"cosine": ops.cosine_range, "dot": ops.dot_range, "l2": ops.l2_range}
_LIST = {"cosine": ops.cosine_list_topk, "dot": ops.dot_list_topk, "l2": ops.l2_list_topk}


@pytest.mark.parametrize("d", fc.DIMS)
@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("space", SPACES)
def test_topk_far_corpus(far, space, kind, d):
    """cosine_topk / dot_topk / l2_topk with ec_f32 far, k <= 64 and k > 64; the near-ties send query 0 to brute force, which
    then reads every far row"""
    q, c = fc.rows("F", kind, d)
    cv, cc = _far_and_compact(far, "F", c)
    qf = _dev(q)
    rs, ri = fc.oracle_topk("F", kind, d, space)
    os_, oi = (cosine_topk_f32(q, c, max(KS)) if space == "cosine" else l2_topk_ref(q, c, max(KS)) if space == "l2" else (rs, ri))
    np.testing.assert_array_equal(oi, ri)
    np.testing.assert_array_equal(_bits(os_), _bits(rs))
    ops_v, ops_c = _operands(space, qf, cv), _operands(space, qf, cc)
    for k in KS:
        got = _np(_TOPK[space](ops_v[0], ops_v[1], d, k, eq_f32=qf, ec_f32=cv, return_status=True, **ops_v[2]))
        want = _np(_TOPK[space](ops_c[0], ops_c[1], d, k, eq_f32=qf, ec_f32=cc, return_status=True, **ops_c[2]))
        print(f"{space} {kind} d={d} k={k}: status {got[2].tolist()}")
        _same(got, want, f"{space} k={k} far vs compact")
        _same(got[:2], (rs[:, :k], ri[:, :k]), f"{space} k={k} far vs oracle")
        if kind == "near_ties":
            assert got[2][0] == 2, got[2]


@pytest.mark.parametrize("d", fc.DIMS)
@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("space", SPACES)
def test_range_far_corpus(far, space, kind, d):
    """cosine_range / dot_range / l2_range with ec_f32 far: one threshold (query 1's exact score at rank 5: six hits there, 1 494
    for query 0 of the near-ties) and one threshold per query (query j's exact score at rank 3 + j; the last query's
    lets every row in, which the exact pass over the far float32 rows answers: status 2)"""
    q, c = fc.rows("F", kind, d)
    cv, cc = _far_and_compact(far, "F", c)
    qf = _dev(q)
    ex = fc.exact("F", kind, d, space)
    ranked = np.sort(ex, axis=1) if space == "l2" else -np.sort(-ex, axis=1)
    ops_v, ops_c = _operands(space, qf, cv), _operands(space, qf, cc)
    per_query = ranked[np.arange(fc.Q), 3 + np.arange(fc.Q)].astype(np.float32)
    per_query[fc.Q - 1] = np.inf if space == "l2" else -np.inf
    for taus in (float(ranked[1, 5]), per_query):
        arg = taus if isinstance(taus, float) else _dev(taus)
        got = _np(_RANGE[space](ops_v[0], ops_v[1], d, arg, eq_f32=qf, ec_f32=cv, return_status=True, **ops_v[2]))
        want = _np(_RANGE[space](ops_c[0], ops_c[1], d, arg, eq_f32=qf, ec_f32=cc, return_status=True, **ops_c[2]))
        lims, s, i, st = got
        print(f"{space} {kind} d={d} tau {'scalar' if isinstance(taus, float) else 'per query'}: hits {np.diff(lims).tolist()} "
              f"status {st.tolist()}")
        _same(got, want, f"{space} range far vs compact")
        ref = fc.range_ref(space, ex, taus)
        np.testing.assert_array_equal(np.diff(lims), [r.size for r in ref])
        for j, r in enumerate(ref):
            a, b = int(lims[j]), int(lims[j + 1])
            np.testing.assert_array_equal(i[a:b], r)
            np.testing.assert_array_equal(_bits(s[a:b]), _bits(ex[j, r]))
        if isinstance(taus, float):
            assert lims[2] - lims[1] == 6 and (kind != "near_ties" or lims[1] - lims[0] >= 1490)     # (six near-ties are sentinels)
        else:
            np.testing.assert_array_equal(np.diff(lims)[1:], (4 + np.arange(1, fc.Q - 1)).tolist() + [fc.N])
            assert st[fc.Q - 1] == 2, st
        assert np.isin(st, (1, 2)).all(), st


def _lists(seed):
    """per query 700 random rows and every sentinel of Layout F: rows on both sides of every boundary in every list"""
    rng = np.random.default_rng(seed)
    return [np.unique(np.concatenate([rng.choice(fc.N, 700, replace=False), fc.LAYOUT_F.sentinels()])) for _ in range(fc.Q)]


@pytest.mark.parametrize("d", fc.DIMS)
@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("space", SPACES)
def test_list_topk_far_corpus(far, space, kind, d):
    q, c = fc.rows("F", kind, d)
    cv, cc = _far_and_compact(far, "F", c)
    qf = _dev(q)
    lists = _lists(d)
    cand, lims = (_dev(x) for x in csr(lists))
    for k in (10, 100):
        got = _np(_LIST[space](qf, cv, cand, lims, k, return_status=True))
        want = _np(_LIST[space](qf, cc, cand, lims, k, return_status=True))
        _same(got, want, f"{space} list k={k} far vs compact")
        _same(got, list_topk_ref(space, q, c, lists, k), f"{space} list k={k} far vs oracle")


IVF_OFF = np.array([0, 300, 1200, 1800, 2500, 3400, 5600, fc.N], dtype=np.int64)      # lists 1, 2, 4 and 6 hold rows on both sides


@pytest.mark.parametrize("d", fc.DIMS)
@pytest.mark.parametrize("space", SPACES)
def test_ivf_scan_far_rows(far, space, d):
    """ivf_scan_topk with rows_f32 far: seven lists, of which four hold the rows beside a boundary (2^31, 2^32, 2^33, 2^34 bytes),
    three probed by every query"""
    q, c = fc.rows("F", "gauss", d)
    for b, l in zip(fc.LAYOUT_F.boundaries, (1, 2, 4, 6)):
        rb = b // fc.LAYOUT_F.row_bytes
        assert IVF_OFF[l] < rb - 1 and rb + 1 < IVF_OFF[l + 1]
    cv, cc = _far_and_compact(far, "F", c)
    qf = _dev(q)
    nlist = IVF_OFF.size - 1
    ln = np.searchsorted(IVF_OFF, np.arange(fc.N), side="right") - 1
    probes = np.array([[j % nlist, (j + 2) % nlist, (j + 4) % nlist] for j in range(fc.Q)], dtype=np.int64)
    assert all(np.isin(l, probes).any() for l in (1, 2, 4, 6))
    off, ids, pr = _dev(IVF_OFF), _dev(np.arange(fc.N, dtype=np.int32)), _dev(probes)
    for k in (10, 100):
        got = _np(ops.ivf_scan_topk(space, qf, cv, off, ids, pr, k, return_status=True, max_list_len=2200))
        want = _np(ops.ivf_scan_topk(space, qf, cc, off, ids, pr, k, return_status=True, max_list_len=2200))
        _same(got, want, f"ivf {space} k={k} far vs compact")
        _same(got, ivc.ivf_ref(space, q, c, ln, probes, k, nlist=nlist, scores=fc.exact("F", "gauss", d, space)),
              f"ivf {space} k={k} far vs oracle")


def _strided(x, pad=37):
    """x as a view of a buffer pad columns wider, NaN elsewhere"""
    buf = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), dtype=torch.float32, device=DEV)
    buf[:, 1:1 + x.shape[1]] = _dev(x)
    return buf[:, 1:1 + x.shape[1]]


@pytest.mark.parametrize("d", fc.DIMS)
@pytest.mark.parametrize("space", SPACES)
def test_graph_search_far_rows(far, space, d):
    """graph_search and graph_search_seeded with rows_f32 far; the graph, the seeds and the entry points come from the existing
    case helpers (a random graph with repeats, padding and ids >= N), the entry points and seeds include the rows beside every
    boundary, and the centroids are a strided view too"""
    q, c = fc.rows("F", "gauss", d)
    cv, cc = _far_and_compact(far, "F", c)
    qf = _dev(q)
    rng = np.random.default_rng(300 + d)
    g, _ = gcs.random_graph(rng, fc.N, 16)
    gd = _dev(g, np.int32)
    ef, width, iters, k = 64, 4, 30, 10
    ent = np.concatenate([fc.LAYOUT_F.sentinels(), rng.choice(fc.N, 6), [-1, fc.N + 1]])
    ref = gcs.graph_search_ref(space, q, c, g, ent, ef, width, iters, k, return_visits=True)
    assert ref[3].min() > ent.size                       # every query went beyond its entry points
    for rows_f32, what in ((cv, "far"), (cc, "compact")):
        got = _np(ops.graph_search(space, qf, rows_f32, gd, _dev(ent, np.int32), k, ef, width=width, max_iters=iters, return_status=True))
        _same(got, ref[:3], f"graph_search {space} {what} vs restatement")
    cent = (c[rng.choice(fc.N, 32, replace=False)] + 0.1 * rng.standard_normal((32, d))).astype(np.float32)
    seeds = gsc.seed_table_ref(space, cent, c, 4)
    seeds[:len(fc.LAYOUT_F.sentinels()), 3] = fc.LAYOUT_F.sentinels()
    refs = gsc.graph_search_seeded_ref(space, q, c, g, ef, width, iters, k, centroids=cent, n_probe=3, seeds=seeds)
    cent_v = _strided(cent)
    for rows_f32, what in ((cv, "far"), (cc, "compact")):
        got = _np(ops.graph_search_seeded(space, qf, rows_f32, gd, k, ef, centroids=cent_v, n_probe=3, seeds=_dev(seeds, np.int32),
                                          width=width, max_iters=iters, return_status=True, return_probes=True))
        _same(got, refs, f"graph_search_seeded {space} {what} vs restatement")


@pytest.mark.parametrize("d", fc.DIMS)
@pytest.mark.parametrize("kind", fc.KINDS)
def test_row_kernels_far_input(far, kind, d):
    """pack_sign_rows, quantize_int8_rows and pq_encode_rows read a far float32 input in place: bit-equal to the compact copy and
    to the restatements.  (l2norm_rows, max_norm_rows, dot_scaled_rows, l2_rows: see the findings above — ops copies their
    input, so a far view never reaches those kernels; their results on the view are what every top-k test here starts from.)"""
    q, c = fc.rows("F", kind, d)
    cv, cc = _far_and_compact(far, "F", c)
    _same(_np(ops.pack_sign_rows(cv)), _np(ops.pack_sign_rows(cc)), "pack_sign_rows far vs compact")
    _same(_np(ops.pack_sign_rows(cv)), (hc.pack_ref(c),), "pack_sign_rows far vs restatement")
    ranges = i8.ranges_of(c)
    _same(_np(ops.quantize_int8_rows(cv, _dev(ranges))), _np(ops.quantize_int8_rows(cc, _dev(ranges))), "quantize_int8_rows far vs compact")
    _same(_np(ops.quantize_int8_rows(cv, _dev(ranges))), (i8.quantize_ref(c, ranges),), "quantize_int8_rows far vs restatement")
    M, _ = fc.pq_shape(d)
    cb = pc.random_codebooks(np.random.default_rng(5 + d), d, M)
    _same(_np(ops.pq_encode_rows(cv, _dev(cb))), _np(ops.pq_encode_rows(cc, _dev(cb))), "pq_encode_rows far vs compact")
    _same(_np(ops.pq_encode_rows(cv, _dev(cb))), (pc.encode_ref(c, cb),), "pq_encode_rows far vs restatement")
    for fn in (ops.l2norm_rows, lambda x: ops.dot_scaled_rows(x)[0], lambda x: ops.l2_rows(x)[0]):     # through ops' copy
        assert torch.equal(fn(cv), fn(cc))
    assert torch.equal(ops.max_norm_rows(cv), ops.max_norm_rows(cc))


@pytest.mark.parametrize("d", fc.DIMS)
@pytest.mark.parametrize("family", ["sign", "int8"])
def test_rescore_far_queries(far, family, d):
    """the float32 QUERY operand of sign_rescore_topk / int8_rescore_topk far: eight rows 2.45 GB apart, the last one straddling
    2^32 elements (the code rows are compact here)"""
    q, c = fc.rows("F", "gauss", d)
    qv, qc = _far_and_compact(far, "F", q, fc.QUERY_STRIDE_F)
    assert qv.stride(0) == fc.QUERY_STRIDE_F
    cand = np.random.default_rng(d).integers(0, fc.N, size=(fc.Q, 64))
    cand[:, 0], cand[:, 1] = -1, fc.N + 3
    if family == "sign":
        codes, fn, ref = hc.pack_ref(c), ops.sign_rescore_topk, hc.rescore_ref
    else:
        codes, fn, ref = i8.quantize_ref(c, i8.ranges_of(c)), ops.int8_rescore_topk, i8.rescore_ref
    for k in (10, 100):
        got = _np(fn(qv, _dev(codes), d, _dev(cand), k, return_status=True))
        _same(got, _np(fn(qc, _dev(codes), d, _dev(cand), k, return_status=True)), f"{family} rescore k={k} far vs compact queries")
        _same(got, ref(q, codes, d, cand, k), f"{family} rescore k={k} far queries vs restatement")


# ------------------------------------------------------------------------------------------------- Layout B: code rows far
@pytest.mark.parametrize("d", fc.DIMS)
@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("family", ["hamming", "int8"])
def test_code_topk_and_rescore_far_codes(far, family, kind, d):
    """hamming_topk / int8_ip_topk with the corpus codes far, then sign_rescore_topk / int8_rescore_topk on candidate lists that
    name the rows beside every boundary (and 57 more, padding and a row >= N)"""
    q = fc.rows("B", kind, d)[0]
    q_codes, c_codes = fc.codes(kind, d, family)[:2]
    cv, cc = _far_and_compact(far, "B", c_codes)
    assert cv.stride(0) % 16 == 0 and cv.data_ptr() % 16 == 0
    first, first_ref, second, second_ref = ((ops.hamming_topk, hc.hamming_topk_ref, ops.sign_rescore_topk, hc.rescore_ref)
                                            if family == "hamming" else
                                            (ops.int8_ip_topk, i8.ip_topk_ref, ops.int8_rescore_topk, i8.rescore_ref))
    for k in (10, 100):
        got = _np(first(_dev(q_codes), cv, d, k))
        _same(got, _np(first(_dev(q_codes), cc, d, k)), f"{family} top-{k} far vs compact")
        _same(got, first_ref(q_codes, c_codes, d, k), f"{family} top-{k} far vs restatement")
    rng = np.random.default_rng(d)
    cand = np.concatenate([np.tile(fc.LAYOUT_B.sentinels(), (fc.Q, 1)), rng.integers(0, fc.N, size=(fc.Q, 55)),
                           np.full((fc.Q, 1), -1), np.full((fc.Q, 1), fc.N)], axis=1)
    qf = _dev(q)
    for k in (10, 29):
        got = _np(second(qf, cv, d, _dev(cand), k, return_status=True))
        _same(got, _np(second(qf, cc, d, _dev(cand), k, return_status=True)), f"{family} rescore k={k} far vs compact")
        _same(got, second_ref(q, c_codes, d, cand, k), f"{family} rescore k={k} far vs restatement")


@pytest.mark.parametrize("d", fc.DIMS)
@pytest.mark.parametrize("kind", fc.KINDS)
@pytest.mark.parametrize("adc", ["ip", "l2"])
def test_pq_adc_far_codes(far, adc, kind, d):
    """pq_adc_topk with the PQ code rows far (32 bytes a row: 32 x 8 and 30 x 10 sub-spaces)"""
    q = fc.rows("B", kind, d)[0]
    cb, c_codes = fc.codes(kind, d, "pq")
    cv, cc = _far_and_compact(far, "B", c_codes)
    tables, exps = pc.tables_ref(q, cb, adc)
    for k in (10, 100):
        got = _np(ops.pq_adc_topk(_dev(q), _dev(cb), cv, k, adc, raw=True))
        _same(got, _np(ops.pq_adc_topk(_dev(q), _dev(cb), cc, k, adc, raw=True)), f"pq {adc} top-{k} far vs compact")
        _same(got, pc.adc_topk_ref(tables, c_codes, k, adc) + (exps,), f"pq {adc} top-{k} far vs restatement")


IVFPQ_OFF = np.array([0, 300, 1200, 2000, 3400, 5000, 5700, fc.N], dtype=np.int64)    # lists 3 and 5 hold rows on both sides


@pytest.mark.parametrize("d", fc.DIMS)
@pytest.mark.parametrize("adc", ["ip", "l2"])
def test_ivfpq_search_far_codes(far, adc, d):
    """ivfpq_search (tables, then ivfpq_scan_topk) with the PQ code rows far, in list order, residual tables"""
    q = fc.rows("B", "gauss", d)[0]
    cb, c_codes = fc.codes("gauss", d, "pq")
    for b, l in zip(fc.LAYOUT_B.boundaries, (3, 5)):
        rb = b // fc.LAYOUT_B.row_bytes
        assert IVFPQ_OFF[l] < rb - 1 and rb + 1 < IVFPQ_OFF[l + 1]
    cv, cc = _far_and_compact(far, "B", c_codes)
    nlist = IVFPQ_OFF.size - 1
    lists = np.searchsorted(IVFPQ_OFF, np.arange(fc.N), side="right") - 1
    cent = (0.3 * np.random.default_rng(9 + d).standard_normal((nlist, d))).astype(np.float32)
    probes = np.array([[(j + 3) % nlist, (j + 5) % nlist, j % nlist] for j in range(fc.Q)], dtype=np.int64)
    args = (_dev(q), _dev(cent), _dev(cb))
    tail = (_dev(IVFPQ_OFF), _dev(np.arange(fc.N, dtype=np.int32)), _dev(probes))
    for k in (10, 100):
        got = _np(ops.ivfpq_search(*args, cv, *tail, k, adc, max_list_len=1600))
        _same(got, _np(ops.ivfpq_search(*args, cc, *tail, k, adc, max_list_len=1600)), f"ivfpq {adc} top-{k} far vs compact")
        _same(got, ipc.search_ref(q, cent, cb, c_codes, lists, probes, k, adc), f"ivfpq {adc} top-{k} far vs restatement")
