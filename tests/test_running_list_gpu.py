"""The kernels that keep a running sorted list in LDS (csrc/search.hip SlList: bf_partial / bf_merge, topk_merge_large,
list_partial / list_merge), each compared twice: with the oracle (oracle/search_ref.py and the test-local oracles built on it)
on order and float32 score bits, and with the sha256 of the raw output bytes recorded in tests/golden/running_list_parent.json
by tools/hash_running_list.py on the commit BEFORE the kernels were rewritten over one list type.  Cases: tests/running_list_cases.py.

Brute force: shards of 600 and 2 500 rows are too small for the block-maxima bound, so every k > 28 is served by
the brute-force pass, status 2: k around the list lengths (64 | 65, 1 000 -> 1 024), k > N padding at N = 600, several chunks
and a last block that is not full at N = 2 500."""
import json
import os

import numpy as np
import pytest

import running_list_cases as rl
from list_cases import ST_ROW, same_bits

pytestmark = pytest.mark.gpu
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "running_list_parent.json")) as f:
    PARENT = json.load(f)


def _same(got_s, got_i, ref_s, ref_i, what):
    assert (got_i == ref_i).all(), (what, np.argwhere(got_i != ref_i)[:5])
    assert same_bits(got_s, ref_s), (what, np.argwhere(got_s.view(np.int32) != ref_s.view(np.int32))[:5])


@pytest.mark.parametrize("k", rl.BF_K)
@pytest.mark.parametrize("n", rl.BF_N)
@pytest.mark.parametrize("space", rl.SPACES)
def test_brute_force(space, n, k):
    s, i, st = rl.bf_run(space, n, k)
    rs, ri = rl.bf_oracle(space, n)
    kk = min(k, n)
    _same(s[:, :kk], i[:, :kk], rs[:, :kk], ri[:, :kk], (space, n, k))
    assert (i[:, kk:] == -1).all() and (np.isposinf(s[:, kk:]) if space == "l2" else np.isneginf(s[:, kk:])).all()
    if k > 28:
        assert (st == 2).all(), st
    assert rl.digest(s, i, st) == PARENT[rl.bf_id(space, n, k)]


@pytest.mark.parametrize("k_out", rl.MERGE_K_OUT)
def test_merge_with_duplicates_and_an_empty_list(k_out):
    s, i = rl.merge_run(k_out)
    rs, ri = rl.merge_oracle(k_out)
    _same(s, i, rs, ri, k_out)
    assert rl.digest(s, i) == PARENT[rl.merge_id(k_out)]


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("k", rl.LIST_K)
@pytest.mark.parametrize("space", rl.SPACES)
def test_csr_lists_across_slice_boundaries(space, k, dtype):
    s, i, st = rl.list_run(space, k, dtype)
    rs, ri, rst = rl.list_oracle(space, k)
    _same(s, i, rs, ri, (space, k, dtype))
    assert (st == rst).all() and st.tolist() == [0, 0, 0, 0, ST_ROW, 0], st
    assert rl.digest(s, i, st) == PARENT[rl.list_id(space, k, dtype)]


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("space", rl.SPACES)
def test_shared_list(space, dtype):
    s, i, st = rl.shared_run(space, dtype)
    rs, ri, rst = rl.shared_oracle(space)
    _same(s, i, rs, ri, (space, dtype))
    assert not st.any() and not rst.any()
    assert rl.digest(s, i, st) == PARENT[rl.shared_id(space, dtype)]
