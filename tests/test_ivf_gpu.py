"""The inverted-list scan on the GPU (ops.ivf_scan_topk): every result — scores and ids — is compared bit for bit with the numpy
oracle of tests/ivf_cases.py.  No tolerance anywhere.  The assignment of rows to lists is crafted directly; no k-means here.

Shapes.  The length test holds one list of every length of ivf_cases.list_lengths (around a wave, a block of the running list,
one and two segments of TSIM_IVF_SEG rows, read from the header) at d = 64, in a shuffled order, and scores its 5 queries against
all rows ONCE per space; every case of the test ranks from that matrix."""
import functools

import numpy as np
import pytest
import torch

from ivf_cases import SL_NB, ST_LIST, ST_OFF, arrival_from_packed, clean_offsets, ivf_ref, list_lengths, pack_ref
from list_cases import header_define, pair_scores, same_bits
from text_similarity_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEG = header_define("TSIM_IVF_SEG")
SPACES = ("cosine", "dot", "l2")
KS = (1, 10, 64, 65, 1024)
WIDTHS = (1, 63, 64, 65, 300, 384, 385, 768)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _scan(space, q, packed, off, ids, probes, k, **kw):
    out = ops.ivf_scan_topk(space, q if isinstance(q, torch.Tensor) else _dev(q), packed if isinstance(packed, torch.Tensor) else
                            _dev(packed), _dev(np.asarray(off, dtype=np.int64)), _dev(np.asarray(ids, dtype=np.int32)),
                            _dev(np.asarray(probes, dtype=np.int64)), k, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _assert_same(got, ref, what):
    assert (got[1] == ref[1]).all(), (what, np.argwhere(got[1] != ref[1])[:5])
    assert same_bits(got[0], ref[0]), (what, np.argwhere(got[0].view(np.int32) != ref[0].view(np.int32))[:5])


def _layout(lengths, d, nq, seed):
    """rows [N, d] in ARRIVAL order with a shuffled assignment that gives list l exactly lengths[l] rows, and its packed form."""
    rng = np.random.default_rng(seed)
    ln = rng.permutation(np.repeat(np.arange(len(lengths)), lengths))
    rows = rng.standard_normal((ln.shape[0], d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    order, off, ids = pack_ref(ln, len(lengths))
    return q, rows, ln, rows[order], off, ids


@functools.lru_cache(maxsize=None)
def _length_case():
    lengths = list_lengths(SEG)
    lengths = [lengths[i] for i in np.random.default_rng(5).permutation(len(lengths))]      # (the empty list somewhere inside)
    return (lengths,) + _layout(lengths, 64, 5, 21)


@functools.lru_cache(maxsize=None)
def _length_scores(space):
    _, q, rows, *_ = _length_case()
    n = rows.shape[0]
    return np.stack([pair_scores(space, q, rows, np.full((n,), j), np.arange(n)) for j in range(q.shape[0])])


@pytest.mark.parametrize("space", SPACES)
def test_list_lengths_and_k(space):
    """Every list length alone, all together and three with the empty one among them; one query and five queries that probe
    DIFFERENT lists; every k regime of the LDS list.  k above the candidates pads (k = 1 024 against a list of 63 rows)."""
    lengths, q, rows, ln, packed, off, ids = _length_case()
    sc = _length_scores(space)
    nlist = len(lengths)
    empty = lengths.index(0)
    qd, pd = _dev(q), _dev(packed)
    rng = np.random.default_rng(8)
    for k in KS:
        for Q in (1, 5):
            cases = [np.array([[(c * Q + j) % nlist] for j in range(Q)]) for c in range(-(-nlist // Q))]         # each list alone
            cases.append(np.stack([rng.permutation(nlist) for _ in range(Q)]))                               # all together
            cases.append(np.stack([rng.permutation([empty, (empty + 1 + j) % nlist, (empty + 3 + j) % nlist]) for j in range(Q)]))
            for probes in cases:
                ref = ivf_ref(space, q[:Q], rows, ln, probes, k, nlist=nlist, scores=sc[:Q])
                got = _scan(space, qd[:Q], pd, off, ids, probes, k, max_list_len=max(lengths), return_status=True)
                _assert_same(got, ref, (space, k, Q, probes.tolist()))
                assert (got[2] == 0).all()
                pad = ref[1] < 0
                assert np.isinf(got[0][pad]).all() and (got[1][pad] == -1).all()
    assert (ivf_ref(space, q[:1], rows, ln, [[lengths.index(63)]], 1024, nlist=nlist, scores=sc[:1])[1][0, 63:] == -1).all()


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("space", SPACES)
def test_widths(space, d):
    """The lane tail and both NI paths of the exact scores: Q = 5, three of four lists per query."""
    if space == "l2" and d == 768:
        d = 767
    lengths = [65, SL_NB + 1, 300, 130]
    q, rows, ln, packed, off, ids = _layout(lengths, d, 5, 300 + d)
    probes = np.array([[0, 1, 2], [3, 1, 0], [2, 3, 1], [1, 0, 3], [2, 0, 3]])
    qd, pd = _dev(q), _dev(packed)
    for k in (10, 65):
        ref = ivf_ref(space, q, rows, ln, probes, k, nlist=4)
        _assert_same(_scan(space, qd, pd, off, ids, probes, k, max_list_len=SL_NB + 1), ref, (space, d, k))


@pytest.mark.parametrize("space", SPACES)
def test_ties_rank_by_id_not_by_position(space):
    """Identical rows in different lists and within one list, ids a random permutation of the positions: equal scores are ordered
    by id, as the flat search orders equal rows by row number."""
    rng = np.random.default_rng(31)
    base = rng.integers(-3, 4, size=(40, 48)).astype(np.float32)
    packed = np.repeat(base, 8, axis=0)[rng.permutation(320)]
    off = np.array([0, 70, 70, 200, 320])
    ids = rng.permutation(320).astype(np.int32)
    q = rng.integers(-3, 4, size=(3, 48)).astype(np.float32)
    rows, ln = arrival_from_packed(packed, off, ids)
    for probes in ([[0, 1, 2, 3]] * 3, [[3, 0], [2, 3], [0, 2]]):
        for k in (20, 65, 320):
            ref = ivf_ref(space, q, rows, ln, probes, k, nlist=4)
            got = _scan(space, q, packed, off, ids, probes, k, max_list_len=130)
            _assert_same(got, ref, (space, probes, k))
            for j in range(3):      # inside a run of equal scores the ids ascend, although the positions do not
                run = np.flatnonzero((got[0][j][1:] == got[0][j][:-1]) & (got[1][j][1:] >= 0))
                assert run.size and (got[1][j][run + 1] > got[1][j][run]).all()


def test_probe_padding_duplicates_and_list_numbers_out_of_range():
    q, rows, ln, packed, off, ids = _layout([100, 40, 0, 700, 90], 64, 3, 41)
    probes = np.array([[3, -1, 3, 5, 2], [-1, -1, -1, -1, -1], [4, 0, 1, -7, 1 << 40]])
    for space in SPACES:
        ref = ivf_ref(space, q, rows, ln, probes, 30, nlist=5)
        assert ref[2].tolist() == [ST_LIST, 0, ST_LIST]
        got = _scan(space, q, packed, off, ids, probes, 30, return_status=True)
        _assert_same(got, ref, space)
        assert got[2].tolist() == [ST_LIST, 0, ST_LIST]
        assert (got[1][1] == -1).all()                                        # nothing probed: padding
        assert (got[1][0, 0:20:2] == got[1][0, 1:20:2]).all()                 # list 3 twice: its rows twice, adjacent
        # the status is written, not accumulated; NULL is fine
        again = _scan(space, q, packed, off, ids, np.abs(probes) % 5, 30, return_status=True)
        assert (again[2] == 0).all()
        _assert_same(_scan(space, q, packed, off, ids, probes, 30), ref, space)


def test_negative_row_ids_are_tombstones():
    q, rows, ln, packed, off, ids = _layout([300, 0, SEG + 7, 64], 64, 4, 42)
    dead = np.random.default_rng(1).random(ids.shape[0]) < 0.4
    ids = np.where(dead, -1 - ids, ids).astype(np.int32)
    arr_rows, arr_ln = arrival_from_packed(packed, off, ids)
    probes = np.array([[0, 2], [2, 3], [3, 1], [0, 3]])
    for space in SPACES:
        for k in (10, 200):
            ref = ivf_ref(space, q, arr_rows, arr_ln, probes, k, nlist=4)
            got = _scan(space, q, packed, off, ids, probes, k)
            _assert_same(got, ref, (space, k))
            assert not np.isin(got[1], np.flatnonzero(arr_ln < 0)).any()


def test_bad_list_offsets_are_clamped_and_reported():
    """list_off decreasing, negative and beyond N: read as its running maximum clamped to [0, N]; the queries that probed a list
    whose pair changed get TSIM_IVF_ST_OFF.  The rows tensor holds exactly N rows."""
    N = 1500
    rng = np.random.default_rng(43)
    packed = rng.standard_normal((N, 64)).astype(np.float32)
    ids = rng.permutation(N).astype(np.int32)
    q = rng.standard_normal((6, 64)).astype(np.float32)
    pd = torch.empty((N, 64), dtype=torch.float32, device=DEV)
    pd.copy_(_dev(packed))
    for off in ([0, 300, 200, 900, N + 50, N], [-5, 300, 600, 2 ** 40, 100, -(2 ** 40)], [40, 40, 30, 20, 10, 0]):
        clean = clean_offsets(off, N)
        changed = [bool(clean[l] != off[l] or clean[l + 1] != off[l + 1]) for l in range(5)]
        rows, ln = arrival_from_packed(packed, clean, ids)
        probes = np.array([[0, -1], [1, 2], [3, 0], [4, 1], [2, 4], [0, 0]])
        want = [ST_OFF if any(changed[l] for l in p if l >= 0) else 0 for p in probes]
        for space in SPACES:
            ref = ivf_ref(space, q, rows, ln, probes, 50, nlist=5)
            got = _scan(space, q, pd, off, ids, probes, 50, return_status=True, max_list_len=600)
            _assert_same(got, ref, (space, off))
            assert got[2].tolist() == want, (off, got[2].tolist(), want)


def test_sizing_hint_never_changes_the_result():
    lengths, q, rows, ln, packed, off, ids = _length_case()
    nlist = len(lengths)
    probes = np.stack([np.random.default_rng(9).permutation(nlist)[:4] for _ in range(5)])
    probes[0, 0] = lengths.index(2 * SEG + 1)
    for space in SPACES:
        sc = _length_scores(space)
        for k in (10, 100):
            ref = ivf_ref(space, q, rows, ln, probes, k, nlist=nlist, scores=sc)
            for hint in (0, 1, SEG, SEG + 1, None, 10 ** 6, 10 ** 9):
                _assert_same(_scan(space, q, packed, off, ids, probes, k, max_list_len=hint), ref, (space, k, hint))


def test_strided_rows_offsets_many_queries_and_the_largest_k():
    lengths, q5, rows, ln, packed, off, ids = _length_case()
    nlist = len(lengths)
    rng = np.random.default_rng(10)
    q = rng.standard_normal((70, 64)).astype(np.float32)
    small = [l for l in range(nlist) if lengths[l] <= 65]
    probes = np.stack([rng.choice(small, size=3, replace=False) for _ in range(70)])
    probes[::7, 1] = lengths.index(SEG + 1)
    wide_q = torch.zeros((70, 64 + 37), dtype=torch.float32, device=DEV)
    wide_q[:, :64] = _dev(q)
    wide_r = torch.full((packed.shape[0], 64 + 5), float("nan"), dtype=torch.float32, device=DEV)
    wide_r[:, :64] = _dev(packed)
    for space in SPACES:
        ref = ivf_ref(space, q, rows, ln, probes, 10, idx_offset=1 << 33, nlist=nlist)
        got = _scan(space, wide_q[:, :64], wide_r[:, :64], off, ids, probes, 10, idx_offset=1 << 33)
        _assert_same(got, ref, space)
        # k = 1 024, nprobe = nlist = 12
        allp = np.stack([rng.permutation(nlist) for _ in range(2)])
        ref = ivf_ref(space, q5[:2], rows, ln, allp, 1024, nlist=nlist, scores=_length_scores(space)[:2])
        _assert_same(_scan(space, q5[:2], packed, off, ids, allp, 1024, max_list_len=max(lengths)), ref, (space, 1024))


def test_ops_refuses_bad_operands():
    lengths, q, rows, ln, packed, off, ids = _length_case()
    a = dict(q=_dev(q), r=_dev(packed), off=_dev(off), ids=_dev(ids), p=_dev(np.zeros((5, 2), np.int64)))
    call = lambda **kw: ops.ivf_scan_topk(kw.get("space", "dot"), kw.get("q", a["q"]), kw.get("r", a["r"]), kw.get("off", a["off"]),
                                          kw.get("ids", a["ids"]), kw.get("p", a["p"]), kw.get("k", 5))
    for bad in (dict(space="ip"), dict(k=0), dict(k=1025), dict(ids=a["ids"].long()), dict(p=a["p"].int()), dict(p=a["p"][:4]),
                dict(off=a["off"].int()), dict(r=a["r"][:, :32]), dict(q=a["q"].double()), dict(ids=a["ids"][:-1])):
        with pytest.raises(ValueError):
            call(**bad)
    from text_similarity_amd import _lib
    with pytest.raises(_lib.TsimError):
        call(q=a["q"].cpu())
