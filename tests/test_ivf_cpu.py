"""CPU checks of the inverted-list scan (include/tsim.h tsim_ivf_scan_topk, tsim_ivf_scan_workspace_bytes) and of the packing
of GpuIVFIndex: the entry validates its arguments before any launch, the workspace function is host arithmetic, the packing is a
pure function that runs on CPU tensors, and the oracle of tests/ivf_cases.py agrees with the list oracle it is built on."""
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

from ivf_cases import ST_LIST, ivf_ref, pack_ref
from list_cases import header_define, list_topk_ref, same_bits
from text_similarity_amd import _lib

EINVAL, ENOMEM = 1, 3
COS, DOT, L2 = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from text_similarity_amd.build import build
        build(verbose=False)
    return _lib.lib()


def test_symbols_and_constants(lib):
    cdll = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(cdll, "tsim_ivf_scan_topk") and hasattr(cdll, "tsim_ivf_scan_workspace_bytes")
    assert {"tsim_ivf_scan_topk", "tsim_ivf_scan_workspace_bytes"} <= set(_lib.DECLARED_SYMBOLS)
    assert header_define("TSIM_IVF_SEG") == _lib.IVF_SEG and _lib.IVF_SEG % 64 == 0
    assert (header_define("TSIM_IVF_ST_LIST"), header_define("TSIM_IVF_ST_OFF")) == (_lib.IVF_ST_LIST, _lib.IVF_ST_OFF) == (1, 2)


def _call(lib, p, **kw):
    a = dict(space=COS, eq=p, ldq=64, Q=4, rows=p, ldr=64, N=100, d=64, off=p, nlist=4, ids=p, probes=p, nprobe=2, hint=50, k=10,
             out_s=p, out_i=p, idx_offset=0, status=None, ws=p, ws_bytes=1 << 30, stream=None)
    a.update(kw)
    return lib.tsim_ivf_scan_topk(a["space"], a["eq"], a["ldq"], a["Q"], a["rows"], a["ldr"], a["N"], a["d"], a["off"], a["nlist"],
                                  a["ids"], a["probes"], a["nprobe"], a["hint"], a["k"], a["out_s"], a["out_i"], a["idx_offset"],
                                  a["status"], a["ws"], a["ws_bytes"], a["stream"])


def test_argument_validation_before_any_launch(lib):
    buf = (ctypes.c_char * 4096)()
    p = ctypes.addressof(buf)
    for name in ("eq", "rows", "off", "ids", "probes", "out_s", "out_i"):
        assert _call(lib, p, **{name: None}) == EINVAL, name
    assert b"null pointer" in lib.tsim_last_error()
    for k in (0, 1025):
        assert _call(lib, p, k=k) == EINVAL
    for d in (0, 769):
        assert _call(lib, p, d=d, ldq=1024, ldr=1024) == EINVAL
    assert _call(lib, p, space=L2, d=768, ldq=768, ldr=768) == EINVAL
    assert b"Euclidean" in lib.tsim_last_error()
    assert _call(lib, p, ldq=63) == EINVAL and _call(lib, p, ldr=63) == EINVAL
    assert _call(lib, p, space=3) == EINVAL and _call(lib, p, space=-1) == EINVAL
    assert _call(lib, p, nprobe=0) == EINVAL
    assert _call(lib, p, Q=0) == EINVAL and _call(lib, p, N=0) == EINVAL and _call(lib, p, nlist=0) == EINVAL
    assert _call(lib, p, hint=-1) == EINVAL
    # a short (or missing) workspace: every argument was accepted, nothing was launched
    need = lib.tsim_ivf_scan_workspace_bytes(4, 2, 50, 10)
    assert need > 0
    assert _call(lib, p, ws_bytes=need - 1) == ENOMEM
    assert _call(lib, p, ws=None) == ENOMEM
    for space, d in ((DOT, 768), (L2, 767), (COS, 1)):
        assert _call(lib, p, space=space, d=d, ldq=768, ldr=768, ws_bytes=need - 1) == ENOMEM


def test_workspace_function(lib):
    f = lib.tsim_ivf_scan_workspace_bytes
    assert f(0, 2, 50, 10) == 0 and f(-1, 2, 50, 10) == 0
    assert f(4, 0, 50, 10) == 0 and f(4, -3, 50, 10) == 0
    assert f(4, 2, -1, 10) == 0
    assert f(4, 2, 50, 0) == 0 and f(4, 2, 50, 1025) == 0
    assert f(1, 1, 0, 1) > 0                      # an index of empty lists is legal
    seg = header_define("TSIM_IVF_SEG")
    Qs = (1, 2, 16, 255, 256, 4096, 16384)
    Ps = (1, 2, 8, 32, 1024)
    Ls = (0, 1, seg - 1, seg, seg + 1, 8 * seg, 256 * seg, 257 * seg, 1 << 24)
    Ks = (1, 10, 64, 65, 1024)
    val = {c: f(*c) for c in itertools.product(Qs, Ps, Ls, Ks)}
    assert all(v > 0 for v in val.values())
    for axis, grid in enumerate((Qs, Ps, Ls, Ks)):
        for c in val:
            i = grid.index(c[axis])
            if i + 1 < len(grid):
                up = c[:axis] + (grid[i + 1],) + c[axis + 1:]
                assert val[up] >= val[c], (c, up)
    # the slots hold the first k of every (query, probe, segment slot), 8 B an entry; within the budget unless one slot per pair
    # already exceeds it
    assert val[(1, 8, 8 * seg, 10)] >= 1 * 8 * 8 * 10 * 8
    for c, v in val.items():
        Q, P, _, k = c
        assert v <= max(64 << 20, Q * P * k * 8) + 1024, c


def test_pack_lists_on_cpu_tensors():
    from text_similarity_amd.ivf_index import pack_lists
    rng = np.random.default_rng(3)
    nlist = 9
    ln = rng.integers(0, nlist, size=500)
    ln[ln == 4] = 5                                # list 4 is empty
    ln[ln == 8] = 0                                # ... and so is the last one
    order, off, ids = pack_lists(torch.from_numpy(ln), nlist)
    assert order.dtype == torch.int64 and off.dtype == torch.int64 and ids.dtype == torch.int32 and not order.is_cuda
    order, off, ids = order.numpy(), off.numpy(), ids.numpy()
    ro, roff, rids = pack_ref(ln, nlist)
    assert (order == ro).all() and (off == roff).all() and (ids == rids).all()
    counts = np.bincount(ln, minlength=nlist)
    assert off[0] == 0 and (np.diff(off) == counts).all() and off[-1] == 500      # the exclusive cumulative count
    assert off[4] == off[5] and off[8] == off[9]                                  # empty lists: equal offsets
    assert sorted(order.tolist()) == list(range(500))                             # a permutation
    for l in range(nlist):
        seg = ids[off[l]:off[l + 1]]
        assert (ln[seg] == l).all() and (np.diff(seg) > 0).all()                  # arrival order survives within a list
    # a pure function: the same input again, and an int32 input, give the same output
    o2, f2, i2 = pack_lists(torch.from_numpy(ln.astype(np.int32)), nlist)
    assert (o2.numpy() == order).all() and (f2.numpy() == off).all() and (i2.numpy() == ids).all()
    e = pack_lists(torch.zeros((0,), dtype=torch.int64), 3)
    assert e[0].numel() == 0 and e[1].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("space", ["cosine", "dot", "l2"])
def test_oracle_equals_the_list_oracle_when_every_list_is_probed(space):
    rng = np.random.default_rng(11)
    N, d, nlist, Q, k = 300, 24, 7, 4, 20
    c = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    ln = rng.integers(0, nlist, size=N)
    probes = np.stack([rng.permutation(nlist) for _ in range(Q)])
    s, i, st = ivf_ref(space, q, c, ln, probes, k, nlist=nlist)
    rs, ri, _ = list_topk_ref(space, q, c, np.arange(N), k)
    assert (i == ri).all() and same_bits(s, rs) and (st == 0).all()
    # a probe >= nlist and a negative one change nothing but the status
    probes2 = np.concatenate([probes, np.full((Q, 1), nlist), np.full((Q, 1), -1)], axis=1)
    probes2[0, -2] = -1
    s2, i2, st2 = ivf_ref(space, q, c, ln, probes2, k, nlist=nlist)
    assert (i2 == ri).all() and same_bits(s2, rs) and st2.tolist() == [0] + [ST_LIST] * (Q - 1)


@pytest.mark.parametrize("space", ["cosine", "dot", "l2"])
def test_oracle_orders_duplicate_vectors_in_different_lists_by_row(space):
    rng = np.random.default_rng(12)
    base = rng.standard_normal((10, 16)).astype(np.float32)
    c = np.concatenate([base, base, base])               # rows r, r + 10, r + 20 are the same vector
    ln = np.concatenate([np.full(10, 2), np.full(10, 0), np.full(10, 1)])       # ... in three different lists
    q = rng.standard_normal((3, 16)).astype(np.float32)
    s, i, _ = ivf_ref(space, q, c, ln, np.tile(np.array([1, 2, 0]), (3, 1)), 30, nlist=3)
    for j in range(3):
        for t in range(0, 30, 3):
            assert i[j, t] + 10 == i[j, t + 1] and i[j, t] + 20 == i[j, t + 2] and i[j, t] < 10
            assert s[j, t] == s[j, t + 1] == s[j, t + 2]
    # a list probed twice: its rows twice, adjacent
    s, i, _ = ivf_ref(space, q, c, ln, np.tile(np.array([1, 1]), (3, 1)), 20, nlist=3)
    assert (i[:, 0::2] == i[:, 1::2]).all() and (i >= 20).all()
