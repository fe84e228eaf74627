"""Exact search within candidate lists, on the host: the C ABI (symbols, argument checks before any launch, the workspace
function), GpuFlatIndex.filter_plan, and the tie between the new tests' oracle (tests/list_cases.py) and the existing one."""
import os

import numpy as np
import pytest

from list_cases import HDR, SPACES, header_define, list_topk_ref, same_bits
from oracle import search_ref
from text_similarity_amd import _lib

NEW = ("tsim_cosine_list_topk", "tsim_dot_list_topk", "tsim_l2_list_topk", "tsim_list_topk_workspace_bytes")
ENTRY = {"cosine": "tsim_cosine_list_topk", "dot": "tsim_dot_list_topk", "l2": "tsim_l2_list_topk"}


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtsim.so is not built")
    return _lib.lib()


def test_header_symbols_exported_and_bound():
    hdr = open(HDR).read()
    for name in NEW:
        assert f"{name}(" in hdr, name
        assert name in _lib.DECLARED_SYMBOLS, name
    L = _lib_or_skip()
    assert L.tsim_version() == 104
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name


def test_list_slice_in_header():
    S = header_define("TSIM_LIST_SLICE")
    assert S >= 64
    assert header_define("TSIM_LIST_ST_ROW") == 1 and header_define("TSIM_LIST_ST_LIMS") == 2
    assert (header_define("TSIM_I32"), header_define("TSIM_I64")) == (_lib.TSIM_I32, _lib.TSIM_I64)


@pytest.mark.parametrize("space", SPACES)
def test_argument_errors_before_any_launch(space):
    """Fake (never dereferenced) 16-byte aligned device pointers: every refusal comes back before a launch, as TSIM_EINVAL, with
    the entry's name in the message."""
    L = _lib_or_skip()
    p = 1 << 20
    ws = L.tsim_list_topk_workspace_bytes(4, 100, 10)
    base = dict(eq=p, ldq=384, Q=4, ec=p, ldc=384, N=1000, d=384, cand=p, dt=_lib.TSIM_I64, T=100, lims=p, shared=0, k=10,
                out_s=p, out_i=p)
    fn = getattr(L, ENTRY[space])
    name = ENTRY[space][len("tsim_"):].encode()

    def call(**kw):
        a = {**base, **kw}
        return fn(a["eq"], a["ldq"], a["Q"], a["ec"], a["ldc"], a["N"], a["d"], a["cand"], a["dt"], a["T"], a["lims"], a["shared"],
                  a["k"], a["out_s"], a["out_i"], 0, None, p, ws, None)

    bad = [{"eq": None}, {"ec": None}, {"cand": None}, {"out_s": None}, {"out_i": None},      # null pointers
           {"k": 0}, {"k": 1025}, {"k": -3},                                                  # k outside 1..1024
           {"d": 0}, {"d": 769, "ldq": 769, "ldc": 769},                                      # d outside 1..768
           {"ldq": 383}, {"ldc": 383},                                                        # strides < d
           {"lims": None, "shared": 0},                                                       # neither lims nor shared
           {"dt": 0}, {"dt": 7}]                                                              # unknown index dtype
    if space == "l2":
        bad.append({"d": 768, "ldq": 768, "ldc": 768})                                        # as tsim_l2_topk_ex
    for kw in bad:
        assert call(**kw) == 1, kw                                                            # TSIM_EINVAL
        assert name in L.tsim_last_error(), (kw, L.tsim_last_error())
    assert call(lims=p, shared=1) == 1 and name in L.tsim_last_error()                        # (both given: ambiguous)


def test_workspace_function():
    L = _lib_or_skip()
    f = L.tsim_list_topk_workspace_bytes
    assert f(1, 0, 1) > 0 and f(4, 100, 10) > 0
    assert f(4, 100, 1025) == 0 and f(4, 100, 0) == 0 and f(0, 100, 10) == 0
    Qs = (1, 2, 5, 64, 70, 255, 256, 1000, 4096, 16384, 100000)
    Ts = (0, 1, 1023, 1024, 1025, 5000, 10 ** 5, 10 ** 6, 41 * 10 ** 6)
    ks = (1, 2, 10, 64, 65, 100, 1000, 1024)
    for T in Ts:
        for k in ks:
            v = [f(Q, T, k) for Q in Qs]
            assert all(x > 0 for x in v) and v == sorted(v), ("Q", T, k, v)
    for Q in Qs:
        for k in ks:
            v = [f(Q, T, k) for T in Ts]
            assert v == sorted(v), ("T", Q, k, v)
        for T in Ts:
            v = [f(Q, T, k) for k in ks]
            assert v == sorted(v), ("k", Q, T, v)


@pytest.mark.parametrize("space", ["cosine", "ip", "euclidean"])
def test_filter_plan(space):
    from text_similarity_amd.index import GpuFlatIndex
    _lib_or_skip()      # (pad_dim is a host function of the library)
    ix = GpuFlatIndex(space=space, dim=384, device="cpu")
    assert ix.filter_plan(1, 10) == "list"
    assert ix.filter_plan(4096, 500000) == "compact"
    rank = {"list": 0, "compact": 1}
    Qs = (1, 2, 3, 4, 5, 8, 16, 64, 256, 1024, 4096, 65536)
    ns = (1, 3, 10, 100, 500, 1000, 10 ** 4, 10 ** 5, 5 * 10 ** 5, 10 ** 6, 10 ** 7)
    for n in ns:
        v = [rank[ix.filter_plan(Q, n)] for Q in Qs]
        assert v == sorted(v), ("Q", n, v)
    for Q in Qs:
        v = [rank[ix.filter_plan(Q, n)] for n in ns]
        assert v == sorted(v), ("n", Q, v)


def test_oracle_on_a_full_list_is_the_existing_oracle():
    rng = np.random.default_rng(3)
    d, N, Q, k = 70, 300, 6, 12
    c = rng.standard_normal((N, d)).astype(np.float32)
    c[7] = 0.0
    c[20:25] = c[19]
    q = rng.standard_normal((Q, d)).astype(np.float32)
    q[1] = c[19]
    s, i, st = list_topk_ref("cosine", q, c, np.arange(N), k, idx_offset=5)
    rs, ri = search_ref.cosine_topk_f32(q, c, k, idx_offset=5)
    assert same_bits(s, rs) and (i == ri).all() and not st.any()
    assert (i[1, :6] == np.arange(19, 25) + 5).all()        # the tie rule: the copies in row order
    # a shuffled list with repeats, padding and rows out of range ranks the same rows
    lst = np.concatenate([rng.permutation(N), [-1, -1, 3, 3, N, N + 10 ** 9]])
    s2, i2, st2 = list_topk_ref("cosine", q, c, [lst] * Q, k, idx_offset=5)
    assert same_bits(s2, rs) and (i2 == ri).all() and (st2 == 1).all()
    # dot and l2 on a full list: the matrices the existing tests restate
    sd, idd, _ = list_topk_ref("dot", q, c, np.arange(N), k)
    vd, jd = search_ref.topk_rows(search_ref._lane_sum(q[:, None, :], c[None, :, :]).astype(np.float32), k)
    assert same_bits(sd, vd) and (idd == jd).all()
    from l2_cases import l2_topk_ref
    sl, il, _ = list_topk_ref("l2", q, c, np.arange(N), k)
    vl, jl = l2_topk_ref(q, c, k)
    assert same_bits(sl, vl) and (il == jl).all()
    # fewer usable rows than k: padding
    s3, i3, _ = list_topk_ref("l2", q, c, [[4, 2, -1]] * Q, 5)
    assert (i3[:, 2:] == -1).all() and np.isposinf(s3[:, 2:]).all() and (np.sort(i3[:, :2], 1) == [2, 4]).all()
