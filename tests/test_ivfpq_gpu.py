"""The IVF-PQ ops on the GPU against the numpy restatement in tests/ivfpq_cases.py: every comparison is for equality.

The list lengths of the scan cases follow TSIM_IVFPQ_SEG in the header (0, 1, 255, 256, 257, SEG - 1, SEG, SEG + 1, 2 SEG + 1: at
SEG = 4096 that is N = 21 250 rows)."""
import numpy as np
import pytest
import torch

import ivfpq_cases as ic
import pq_cases as pc
from text_similarity_amd import _lib, ops
from text_similarity_amd.pq_index import GpuPQIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEG = ic.header_seg()
KS = (1, 10, 100, 1024)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _np(t):
    return t.cpu().numpy()


# ------------------------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("d,M", [(8, 1), (12, 3), (66, 33), (1024, 64)])      # NW = 1, 1, 3, 4; dsub = 8, 4, 2, 16
@pytest.mark.parametrize("space", ("ip", "l2"))
def test_tables(space, d, M):
    rng = np.random.default_rng(d + (space == "l2"))
    Q, nlist, nprobe = 5, 7, 4
    cb = pc.random_codebooks(rng, d, M)
    cent = (3 * rng.standard_normal((nlist, d))).astype(np.float32)           # three times the codebook entries: the bias sets e
    q = rng.standard_normal((Q, d)).astype(np.float32)
    probes = np.stack([rng.permutation(nlist)[:nprobe] for _ in range(Q)]).astype(np.int64)
    probes[0, 1], probes[0, 3], probes[4, 0] = -1, nlist + 3, -1
    q[1] = 0
    q[2, d // 2] = np.nan
    q[3, d - 1], cent[probes[3, 2], d - 1] = 3e38, -3e38                       # only this pair's residual is infinite
    for l in probes[3, [0, 1, 3]]:
        assert cent[l, d - 1] > -1e38
    t, b, e = ops.ivfpq_tables(_dev(q), _dev(cent), _dev(probes), _dev(cb), space)
    if space == "ip":
        wt, wb, we = ic.tables_ip_ref(q, cent, probes, cb)
        assert t.shape == (Q, M, 256) and np.array_equal(_np(t), wt) and np.array_equal(_np(b), wb)
        assert not wt[1:3].any() and not wb[1:3].any() and wb[3].any()
        above = np.abs(wb).max(axis=1) > np.abs(wt).max(axis=(1, 2))         # the bias set the exponent
        assert above[3] and (we[above] < pc.tables_ref(q, cb, "ip")[1][above]).all()
    else:
        wt, we = ic.tables_l2_ref(q, cent, probes, cb)
        ok = ic.valid_probes(probes, nlist)
        assert b is None and t.shape == (Q, nprobe, M, 256) and np.array_equal(_np(t)[ok], wt[ok])
        assert wt[0].any() and wt[1].any() and not wt[2:4].any() and wt[4].any()
    assert np.array_equal(_np(e), we) and we[0] != 0 and we[2] == 0


# ------------------------------------------------------------------------------------------------- the scan, given integer tables
class Lists:
    """nine lists of the lengths around a step and a segment, in a shuffled list order; ids a permutation with tombstones; a code
    row of the longest list repeated in two other lists"""

    def __init__(self, M, binary):
        rng = np.random.default_rng(M + binary)
        lengths = ic.seg_lengths(SEG)
        self.M, self.nlist = M, len(lengths)
        self.list_off, which = ic.lists_of_lengths(rng, lengths)
        self.N = int(self.list_off[-1])
        at = {n: int(which[i]) for i, n in enumerate(lengths)}                # length -> list number
        raw = (pc.binary_codes if binary else pc.uniform_codes)(rng, self.N, M)
        for n in (SEG, 257):
            raw[self.list_off[at[n]] + 3] = raw[self.list_off[at[2 * SEG + 1]] + 2 * SEG]
        self.codes = pc.pad_codes(raw, junk_rng=rng)
        self.wide = pc.pad_codes(raw, stride=pc.code_bytes(M) + 16, junk_rng=rng)
        self.ids = ic.ids_with_tombstones(rng, self.N)
        self.probes = np.array([[at[0], at[1], at[255], -1],
                                [at[256], at[257], at[SEG - 1], at[2 * SEG + 1]],
                                [at[SEG], at[SEG + 1], self.nlist + 3, at[SEG - 1]],
                                [at[2 * SEG + 1], at[SEG + 1], at[SEG], at[257]],
                                [-1, -1, -1, -1]], np.int64)
        self.Q, self.nprobe = self.probes.shape
        self.dev = {k: _dev(getattr(self, k)) for k in ("codes", "list_off", "ids", "probes")}
        self.dev["wide"] = _dev(self.wide)

    def tables(self, kind, space, per_pair, rng):
        n = self.Q * self.nprobe if per_pair else self.Q
        if kind == "random":
            t = pc.random_tables(rng, n, self.M, space) // 2                 # half the room is the bias's
        elif kind == "small":
            t = pc.small_tables(rng, n, self.M, space)
        else:
            t = pc.one_hot_tables(n, self.M, space)
        return t.reshape(self.Q, self.nprobe, self.M, 256) if per_pair else t

    def bias(self, kind, space, rng):
        hi = (1 << 22) if kind == "random" else 3
        b = rng.integers(-hi, hi + 1, size=(self.Q, self.nprobe))
        return (-np.abs(b) if space == "l2" else b).astype(np.int32)

    def scan(self, space, t, b, k, codes="codes", list_off=None, **kw):
        return ops.ivfpq_scan_topk(space, _dev(t), None if b is None else _dev(b), self.dev[codes],
                                   self.dev["list_off"] if list_off is None else _dev(list_off), self.dev["ids"], self.dev["probes"], k,
                                   **kw)

    def ref(self, space, t, b, k, list_off=None, **kw):
        return ic.scan_ref(t, b, self.codes, self.list_off if list_off is None else list_off, self.ids, self.probes, k, space, **kw)


_LISTS = {}


def _lists(M, binary=False):
    if (M, binary) not in _LISTS:
        _LISTS[M, binary] = Lists(M, binary)
    return _LISTS[M, binary]


@pytest.mark.parametrize("kind", ("random", "small", "one_hot"))
@pytest.mark.parametrize("M", (48, 33))                                       # NW = 3 both; 33 is no multiple of 16
@pytest.mark.parametrize("space", ("ip", "l2"))
def test_scan(space, M, kind):
    ls = _lists(M, binary=kind == "small")                                    # small tables on binary codes: ties decide
    rng = np.random.default_rng(7)
    assert ls.N == sum(ic.seg_lengths(SEG))
    for per_pair in (False, True):
        t = ls.tables(kind, space, per_pair, rng)
        for b in (None, ls.bias(kind, space, rng)):
            assert (ic.score_bound(t, b) < 2 ** 24).all()
            for k in KS:
                v, i, st = ls.scan(space, t, b, k, return_status=True)
                wv, wi, wst = ls.ref(space, t, b, k)
                assert np.array_equal(_np(v), wv), (per_pair, b is not None, k)
                assert np.array_equal(_np(i), wi), (per_pair, b is not None, k)
                assert np.array_equal(_np(st), wst) and wst.tolist() == [0, 0, ic.ST_LIST, 0, 0]
            assert (wi[0] == -1).any() and (wi[4] == -1).all() and (wi[1:4] >= 0).all()      # k = 1024: padding where rows run out


@pytest.mark.parametrize("M", (3, 20, 64))                                    # NW = 1, 2, 4
def test_scan_other_widths(M):
    ls = _lists(M)
    rng = np.random.default_rng(M)
    for space, per_pair in (("ip", True), ("l2", False)):
        t, b = ls.tables("random", space, per_pair, rng), ls.bias("random", space, rng)
        for k in (10, 1024):
            v, i = ls.scan(space, t, b, k)
            wv, wi, _ = ls.ref(space, t, b, k)
            assert np.array_equal(_np(v), wv) and np.array_equal(_np(i), wi), (space, k)


def test_scan_ties_between_lists_go_to_the_lower_id():
    ls = _lists(48)
    t = pc.one_hot_tables(ls.Q, 48, "ip")
    lo = int(ls.list_off[ls.probes[3, 0]]) + 2 * SEG                          # the repeated row, in the longest list
    t[3] = 0
    t[3, 5, ls.codes[lo, 5]] = 77
    v, i = ls.scan("ip", t, None, 10)
    wv, wi, _ = ls.ref("ip", t, None, 10)
    assert np.array_equal(_np(v), wv) and np.array_equal(_np(i), wi)
    assert (wv[3] == 77).all() and (np.diff(wi[3]) > 0).all()               # some 60 rows of the probed lists share that byte


@pytest.mark.parametrize("space", ("ip", "l2"))
def test_scan_hint_offset_and_stride(space):
    ls = _lists(33)
    rng = np.random.default_rng(8)
    t, b = ls.tables("random", space, True, rng), ls.bias("random", space, rng)
    for k in (10, 1024):
        wv, wi, _ = ls.ref(space, t, b, k)
        for hint in (1, SEG, 10 * SEG, 10 ** 7):                             # a list longer than the hint is still complete
            v, i = ls.scan(space, t, b, k, max_list_len=hint)
            assert np.array_equal(_np(v), wv) and np.array_equal(_np(i), wi), hint
        v, i = ls.scan(space, t, b, k, codes="wide", idx_offset=1 << 33)      # rows 16 junk bytes further apart
        wv2, wi2, _ = ls.ref(space, t, b, k, idx_offset=1 << 33)
        assert np.array_equal(_np(v), wv2) and np.array_equal(_np(i), wi2)
        assert np.array_equal(wv, wv2) and (wi2[wi2 >= 0] >= 1 << 33).all() and (wi2[wi == -1] == -1).all()
    view = ls.dev["wide"][:, :pc.code_bytes(33)]
    assert view.stride(0) == pc.code_bytes(33) + 16


def test_scan_status_bits_and_cleaned_offsets():
    ls = _lists(48)
    rng = np.random.default_rng(9)
    t = ls.tables("random", "ip", False, rng)
    bad = ls.list_off.copy()
    l = int(ls.probes[1, 1])
    bad[l + 1] = bad[l] - 5 if bad[l] >= 5 else ls.N + 9                      # a decreasing pair (or beyond N): cleaned
    bad[-1] = ls.N + 100
    v, i, st = ls.scan("ip", t, None, 100, list_off=bad, return_status=True)
    wv, wi, wst = ls.ref("ip", t, None, 100, list_off=bad)
    assert np.array_equal(_np(v), wv) and np.array_equal(_np(i), wi) and np.array_equal(_np(st), wst)
    assert wst[1] & ic.ST_OFF and wst[2] & ic.ST_LIST and wst[4] == 0
    v2, i2 = ls.scan("ip", t, None, 100, list_off=bad)                        # without a status tensor
    assert np.array_equal(_np(v2), wv) and np.array_equal(_np(i2), wi)


def test_scan_refusals():
    ls = _lists(48)
    t = pc.one_hot_tables(ls.Q, 48, "ip")
    with pytest.raises(ValueError):
        ls.scan("cosine", t, None, 5)
    with pytest.raises(ValueError):
        ls.scan("ip", t, None, 1025)
    with pytest.raises(ValueError):
        ls.scan("ip", t[:3], None, 5)
    with pytest.raises(ValueError):
        ops.ivfpq_scan_topk("ip", _dev(t), None, ls.dev["codes"][:, :32], ls.dev["list_off"], ls.dev["ids"], ls.dev["probes"], 5)


# ------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(11)
    d, M, nlist, N, Q = 384, 48, 16, 3000, 4
    cent = (2 * rng.standard_normal((nlist, d))).astype(np.float32)
    lists = rng.integers(0, nlist, size=N)
    x = (cent[lists] + rng.standard_normal((N, d))).astype(np.float32)
    q = (cent[rng.integers(0, nlist, size=Q)] + rng.standard_normal((Q, d))).astype(np.float32)
    cb = pc.random_codebooks(rng, d, M)
    return dict(d=d, M=M, nlist=nlist, nprobe=5, N=N, Q=Q, cent=cent, lists=lists, x=x, q=q, cb=cb)


@pytest.mark.parametrize("by_residual", (True, False))
@pytest.mark.parametrize("space", ("ip", "l2", "cosine"))
def test_search_end_to_end(corpus, space, by_residual):
    c = corpus
    x, q, cent = c["x"], c["q"], c["cent"]
    if space == "cosine":
        x, q = _np(GpuPQIndex.normalise(_dev(x))), _np(GpuPQIndex.normalise(_dev(q)))
        cent = cent / np.linalg.norm(cent, axis=1, keepdims=True).astype(np.float32)
    adc = "l2" if space == "l2" else "ip"
    dist = ((q[:, None, :].astype(np.float64) - cent[None]) ** 2).sum(-1)
    probes = np.argsort(dist, axis=1, kind="stable")[:, :c["nprobe"]].astype(np.int64)
    xd, cd, ld = _dev(x), _dev(cent), _dev(c["lists"])
    codes = ops.pq_encode_rows(xd - cd[ld] if by_residual else xd, _dev(c["cb"]))      # the subtraction in torch, as the index does
    want_codes = ic.encode_ref(x, cent, c["lists"], c["cb"], by_residual)
    assert np.array_equal(_np(codes), want_codes)
    order, list_off, row_ids = ic.pack(c["lists"], c["nlist"])
    args = (_dev(q), cd, _dev(c["cb"]), codes[_dev(order)], _dev(list_off), _dev(row_ids), _dev(probes))
    for k in (10, 1024):
        s, i = ops.ivfpq_search(*args, k, adc, by_residual=by_residual)
        ws, wi = ic.search_ref(q, cent, c["cb"], want_codes, c["lists"], probes, k, adc, by_residual)
        assert np.array_equal(_np(s).view(np.uint32), ws.view(np.uint32)) and np.array_equal(_np(i), wi)
        one = c["M"] * 1024 * (c["nprobe"] if by_residual and adc == "l2" else 1)
        s1, i1 = ops.ivfpq_search(*args, k, adc, by_residual=by_residual, table_budget=one)       # one query a slice
        assert torch.equal(s1.view(torch.int32), s.view(torch.int32)) and torch.equal(i1, i)
    v, i2, e = ops.ivfpq_search(*args, 10, adc, by_residual=by_residual, raw=True)
    assert v.dtype == torch.int32 and e.shape == (c["Q"],) and torch.equal(i2, ops.ivfpq_search(*args, 10, adc, by_residual=by_residual)[1])
    assert (wi[:, :50] >= 0).all() and np.isfinite(ws[:, :50]).all()
