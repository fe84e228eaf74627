"""CPU checks of the community de-overlap (include/tsim.h tsim_community_select_*): the symbols exist, every bad argument is
refused before any launch, the workspace function is host arithmetic, and the parallel form — restated round by round in
tests/community_cases.py — decides exactly what the sequential loop of the definition decides."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from community_cases import (ST_LIMS, ST_ROW, chain_case, clean_lims, csr, detect_ref, planted_rows, random_case, rounds_model,
                             select_ref)
from list_cases import header_define
from text_similarity_amd import _lib

EINVAL, ENOMEM = 1, 3
SYMBOLS = {"tsim_community_select_workspace_bytes", "tsim_community_select_rounds", "tsim_community_select_finish"}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from text_similarity_amd.build import build
        build(verbose=False)
    return _lib.lib()


def test_symbols_and_constants(lib):
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(cdll, s) for s in SYMBOLS) and SYMBOLS <= set(_lib.DECLARED_SYMBOLS)
    assert (header_define("TSIM_COMMUNITY_ST_ROW"), header_define("TSIM_COMMUNITY_ST_LIMS")) == \
        (_lib.COMMUNITY_ST_ROW, _lib.COMMUNITY_ST_LIMS) == (ST_ROW, ST_LIMS)


def _rounds(lib, p, **kw):
    a = dict(lims=p, members=p, C=4, T=16, N=100, min_size=2, first=0, rounds=1, accept=p, keep=p, status=p, undecided=p, ws=p,
             ws_bytes=1 << 30, stream=None)
    a.update(kw)
    return lib.tsim_community_select_rounds(a["lims"], a["members"], a["C"], a["T"], a["N"], a["min_size"], a["first"], a["rounds"],
                                            a["accept"], a["keep"], a["status"], a["undecided"], a["ws"], a["ws_bytes"], a["stream"])


def _finish(lib, p, **kw):
    a = dict(lims=p, members=p, C=4, T=16, N=100, min_size=2, accept=p, keep=p, status=p, undecided=p, ws=p, ws_bytes=1 << 30,
             stream=None)
    a.update(kw)
    return lib.tsim_community_select_finish(a["lims"], a["members"], a["C"], a["T"], a["N"], a["min_size"], a["accept"], a["keep"],
                                            a["status"], a["undecided"], a["ws"], a["ws_bytes"], a["stream"])


@pytest.mark.parametrize("call", [_rounds, _finish])
def test_argument_validation_before_any_launch(lib, call):
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    for name in ("lims", "members", "accept", "keep", "status", "undecided"):
        assert call(lib, p, **{name: None}) == EINVAL, name
    assert b"null pointer" in lib.tsim_last_error()
    assert call(lib, p, C=-1) == EINVAL
    assert call(lib, p, T=-1) == EINVAL
    assert call(lib, p, N=0) == EINVAL and call(lib, p, N=-5) == EINVAL
    assert call(lib, p, min_size=0) == EINVAL and call(lib, p, min_size=-1) == EINVAL
    assert call(lib, p, C=1 << 31) == EINVAL and call(lib, p, N=1 << 31) == EINVAL
    if call is _rounds:
        assert call(lib, p, rounds=-1) == EINVAL
        assert call(lib, p, first=-1) == EINVAL
        assert call(lib, p, first=1 << 30, rounds=1) == EINVAL
    # a short (or missing) workspace: every argument was accepted, nothing was launched
    need = lib.tsim_community_select_workspace_bytes(4, 100)
    assert need > 0
    assert call(lib, p, ws_bytes=need - 1) == ENOMEM
    assert call(lib, p, ws=None) == ENOMEM
    assert call(lib, p, T=0, members=None, keep=None, ws_bytes=need - 1) == ENOMEM      # an empty CSR needs no payload


def test_workspace_function(lib):
    f = lib.tsim_community_select_workspace_bytes
    assert f(-1, 10) == 0 and f(4, 0) == 0 and f(4, -1) == 0
    assert f(1 << 31, 10) == 0 and f(4, 1 << 31) == 0
    assert f(0, 1) > 0                                       # no community at all is legal
    Cs = (0, 1, 2, 63, 64, 65, 4096, 1 << 20, 1 << 30)
    Ns = (1, 2, 63, 64, 65, 5000, 1 << 20, 1 << 30)
    val = {c: f(*c) for c in itertools.product(Cs, Ns)}
    assert all(v > 0 for v in val.values())
    for axis, grid in enumerate((Cs, Ns)):
        for c in val:
            i = grid.index(c[axis])
            if i + 1 < len(grid):
                up = c[:axis] + (grid[i + 1],) + c[axis + 1:]
                assert val[up] >= val[c], (c, up)
    for (C, N), v in val.items():                           # cleaned lims, a state word per community, owner and claim per row
        assert (C + 1) * 8 + C * 4 + N * 12 <= v <= (C + 1) * 8 + C * 4 + N * 12 + 4 * 256


def test_ops_have_no_cpu_path():
    import torch
    from text_similarity_amd import ops
    with pytest.raises(_lib.TsimError):
        ops.community_select(torch.zeros(2, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), 4, 1)
    with pytest.raises(_lib.TsimError):
        ops.community_detection(None, torch.zeros(4, 8), 8, 0.5, 2)
    assert ops.COMMUNITY_MAX_ROUNDS > 0 and ops.COMMUNITY_ROUND_BATCH > 0


def test_clustering_pipeline_accepts_the_community_method():
    from types import SimpleNamespace
    from text_similarity_amd.pipeline.clustering import ClusteringPipeline
    params = SimpleNamespace(device="cpu")
    p = ClusteringPipeline(None, params, None, method="community", threshold=0.75)       # n_clusters is ignored
    assert (p.method, p.threshold, p.min_community_size) == ("community", 0.75, 10)
    assert ClusteringPipeline(7, params, None).method == "k-means"
    for kw in (dict(method="community"), dict(method="dbscan")):                         # no threshold; unknown method
        with pytest.raises(ValueError):
            ClusteringPipeline(3, params, None, **kw)


def _same(lists, N, min_size):
    lims, mem = csr(lists)
    a, k, _ = select_ref(lims, mem, N, min_size)
    ra, rk, rounds, left = rounds_model(lims, mem, N, min_size)
    assert left.size == 0 and (ra == a).all() and (rk == k).all()
    return a, k, rounds


def test_rounds_model_equals_the_sequential_loop_on_random_csrs():
    rng = np.random.default_rng(20)
    most = 0
    for trial in range(60):
        N = int(rng.integers(1, 120))
        lists = random_case(rng, int(rng.integers(1, 40)), N, int(rng.integers(1, 30)), dup=trial % 3 == 0)
        for min_size in (1, 2, 5):
            most = max(most, _same(lists, N, min_size)[2])
    assert most >= 3                                         # the cases do make communities wait for one another


def test_rounds_model_on_a_chain_needs_one_round_per_link():
    lists, N = chain_case(40, 12)
    a, k, rounds = _same(lists, N, 5)
    assert a.all() and rounds == 40 and k.sum() == N         # every row once: the shared row goes to the earlier community
    # a budget below the chain's length leaves the tail undecided, decided so far = the loop's prefix
    lims, mem = csr(lists)
    ra, rk, r, left = rounds_model(lims, mem, N, 5, max_rounds=7)
    assert r == 7 and left.tolist() == list(range(7, 40)) and (ra[:7] == 1).all() and (ra[7:] == 0).all()
    # min_size above what is left once the neighbour took the shared row: every second community falls
    a, _, _ = _same(lists, N, 12)
    assert a.tolist() == [1, 0] * 20


def test_id_rules_of_the_restatement():
    lists = [[0, 1, 2, -1, 7], [2, 3, 3], [9, 1], []]
    lims, mem = csr(lists)
    a, k, st = select_ref(lims, mem, 8, 2)
    assert st == ST_ROW                                      # 9 >= N = 8: dropped and flagged
    assert a.tolist() == [1, 1, 0, 0] and k.tolist() == [1, 1, 1, 0, 1, 0, 1, 1, 0, 0]      # 3 listed twice counts twice
    bad = lims.copy()
    bad[2] = 1                                               # a decreasing pair: community 1 comes out empty, 2 takes [8, 10)
    assert clean_lims(bad, len(mem)).tolist() == [0, 5, 5, 10, 10]
    a, k, st = select_ref(bad, mem, 8, 1)
    assert st == (ST_ROW | ST_LIMS) and a.tolist() == [1, 0, 1, 0]
    ra, rk, _, _ = rounds_model(bad, mem, 8, 1)
    assert (ra == a).all() and (rk == k).all()


def test_detect_ref_on_the_planted_rows():
    x, planted = planted_rows(32)
    N = len(x)
    s = (x.astype(np.float64) @ x.astype(np.float64).T).astype(np.float32)
    lims, sc, ix = [0], [], []
    for i in range(N):
        hit = np.nonzero(s[i] >= 0.75)[0]
        hit = hit[np.lexsort((hit, -s[i, hit]))]
        lims.append(lims[-1] + len(hit))
        sc.append(s[i, hit])
        ix.append(hit)
    ol, mem, cen, lab, _ = detect_ref(np.array(lims), np.concatenate(sc), np.concatenate(ix), N, 10)
    assert len(cen) == 6 and (np.diff(ol) == [120, 95, 70, 50, 35, 20]).all()
    for k in range(6):
        assert len(set(planted[mem[ol[k]:ol[k + 1]]])) == 1
    assert ((lab >= 0) == (planted >= 0)).all()
