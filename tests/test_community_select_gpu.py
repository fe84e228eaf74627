"""ops.community_select against the literal loop of the definition (tests/community_cases.select_ref), bit for bit, on crafted
CSRs: the serial form alone (max_rounds=0), one round and then the serial finish (1), and the default budget must all give the
restatement's accept and keep."""
import numpy as np
import pytest
import torch

from community_cases import ST_LIMS, ST_ROW, chain_case, csr, random_case, select_ref
from text_similarity_amd import ops

pytestmark = pytest.mark.gpu
BUDGETS = (0, 1, None)


def _run(lims, mem, N, min_size, max_rounds):
    dev = torch.device("cuda:0")
    a, k, rounds, st = ops.community_select(torch.from_numpy(np.asarray(lims, np.int64)).to(dev),
                                            torch.from_numpy(np.asarray(mem, np.int32)).to(dev), N, min_size, max_rounds)
    assert a.dtype == torch.int32 and k.dtype == torch.uint8
    return a.cpu().numpy(), k.cpu().numpy(), rounds, st


def _check(lists, N, min_size, lims=None):
    l0, mem = csr(lists)
    lims = l0 if lims is None else lims
    ra, rk, rst = select_ref(lims, mem, N, min_size)
    used = {}
    for b in BUDGETS:
        a, k, rounds, st = _run(lims, mem, N, min_size, b)
        assert np.array_equal(a, ra) and np.array_equal(k, rk) and st == rst, (b, min_size)
        used[b] = rounds
    assert used[0] == 0 and used[1] <= 1
    return ra, rk, used


SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1025)


@pytest.mark.parametrize("min_size", [1, 2, 1026])
def test_sizes_across_wave_and_workgroup_edges(min_size):
    """Communities of every edge size over overlapping windows of rows (each shares about a third of its rows with the next
    one), N = 3001, no multiple of 64; 1026 is one above the largest."""
    lists, at = [], 0
    for n in SIZES + SIZES[::-1]:
        lists.append(np.arange(at, at + n) % 3001)
        at += (2 * n) // 3
    a, k, _ = _check(lists, 3001, min_size)
    assert a.any() == (min_size <= 1025)


def test_chain_needs_rounds_and_reaches_the_serial_finish():
    lists, N = chain_case(40, 12)
    a, k, used = _check(lists, N, 5)
    assert a.all() and k.sum() == N
    lims, mem = csr(lists)
    assert used[None] >= 2
    # a cap below the chain's length: the rounds decide a prefix, the serial finish the rest — same result (checked above for 1)
    for cap in (3, 8):
        a2, k2, rounds, _ = _run(lims, mem, N, 5, cap)
        assert rounds == cap and np.array_equal(a2, a) and np.array_equal(k2, k)
    a3, _, rounds, _ = _run(lims, mem, N, 5, 64)
    assert rounds == 40 and a3.all()                         # one round per link, no finish needed


def test_disjoint_and_identical_communities():
    disjoint = [np.arange(i * 70, (i + 1) * 70) for i in range(50)]
    a, k, used = _check(disjoint, 3500, 10)
    assert a.all() and k.all() and used[None] == 1           # nothing to wait for: one round
    same = [np.arange(100)] * 30
    a, k, _ = _check(same, 100, 10)
    assert a.tolist() == [1] + [0] * 29 and k[:100].all() and not k[100:].any()


def test_member_listed_twice_counts_twice():
    lists = [[5, 5, 6], [5, 7, 7], [8, 8], [9]]
    a, k, _ = _check(lists, 10, 2)
    assert a.tolist() == [1, 1, 1, 0] and k.tolist() == [1, 1, 1, 0, 1, 1, 1, 1, 0]
    _check(lists, 10, 3)
    _check(lists, 10, 1)


def test_padding_and_rows_beyond_n_are_never_kept():
    rng = np.random.default_rng(4)
    lists = [rng.integers(-3, 140, size=n).astype(np.int32) for n in (70, 5, 300, 64, 129)]
    N = 100                                                  # members 100 .. 139 are beyond the rows, -3 .. -1 padding
    _, mem = csr(lists)
    a, k, _ = _check(lists, N, 3)
    assert not k[(mem < 0) | (mem >= N)].any() and k.any()
    lims, mem = csr([[1, 2, 3], [4, 5]])
    assert _run(lims, mem, 6, 1, None)[3] == 0 and _run(lims, mem, 5, 1, None)[3] == ST_ROW and _run(lims, mem, 5, 1, 0)[3] == ST_ROW


def test_decreasing_lims_pair_is_an_empty_community():
    lists = [np.arange(0, 40), np.arange(30, 70), np.arange(60, 100), np.arange(90, 130)]
    lims, _ = csr(lists)
    bad = lims.copy()
    bad[2] = 10                                              # [0, 40, 10, 120, 160]: community 1 empty, 2 = entries [40, 120)
    a, k, _ = _check(lists, 130, 5, lims=bad)
    assert a[1] == 0 and select_ref(bad, csr(lists)[1], 130, 5)[2] == ST_LIMS
    beyond = lims.copy()
    beyond[-1] = 10_000                                      # past the payload: clamped
    _check(lists, 130, 5, lims=beyond)


def test_one_community_and_odd_row_counts():
    for N in (1, 63, 65, 1000):
        _check([np.arange(N)], N, 1)
        _check([np.arange(N)], N, N + 1)
    _check([[]], 7, 1)


def test_ops_argument_errors_and_no_community():
    dev = torch.device("cuda:0")
    lims = torch.tensor([0, 2], dtype=torch.int64, device=dev)
    mem = torch.tensor([1, 2], dtype=torch.int32, device=dev)
    for kw in (dict(N=0), dict(min_size=0), dict(max_rounds=-1)):
        a = dict(N=4, min_size=1, max_rounds=None)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.community_select(lims, mem, a["N"], a["min_size"], a["max_rounds"])
    with pytest.raises(ValueError):
        ops.community_select(lims, mem.long(), 4, 1)
    with pytest.raises(ValueError):
        ops.community_select(lims.int(), mem, 4, 1)
    a, k, rounds, st = ops.community_select(lims[:1], mem[:0], 4, 1)      # C = 0
    assert a.numel() == 0 and k.numel() == 0 and (rounds, st) == (0, 0)


def test_random_communities():
    rng = np.random.default_rng(7)
    lists = random_case(rng, 2000, 5000, 120)
    for min_size in (1, 10):
        a, _, used = _check(lists, 5000, min_size)
        assert 0 < a.sum() < 2000
    lists = random_case(rng, 300, 200, 40, dup=True)         # dense overlap and repeated members
    _check(lists, 200, 3)
