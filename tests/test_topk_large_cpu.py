"""Host side of top-k for k up to 1024 (include/tsim.h tsim_cosine_topk_large / tsim_dot_topk_large /
tsim_topk_large_workspace_bytes): symbols, workspace sizes and the argument checks that run before any launch."""
import os

import pytest

from text_similarity_amd import _lib, ops

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tsim.h")
NEW = ("tsim_topk_large_workspace_bytes", "tsim_cosine_topk_large", "tsim_dot_topk_large")


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtsim.so is not built")
    return _lib.lib()


def test_symbols_declared_bound_and_exported():
    hdr = open(HDR).read()
    assert "#define TSIM_TOPK_MAX_K 1024" in hdr
    for name in NEW:
        assert f"{name}(" in hdr, name
        assert name in _lib.DECLARED_SYMBOLS, name
    L = _lib_or_skip()
    assert L.tsim_version() == 104
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name
    assert ops.MAX_K == 1024


def test_workspace_bytes():
    L = _lib_or_skip()
    Q, N = 256, 1_000_000
    assert L.tsim_topk_large_workspace_bytes(Q, N, 65) > 0
    assert L.tsim_topk_large_workspace_bytes(Q, N, 1024) > 0
    assert L.tsim_topk_large_workspace_bytes(Q, N, 1025) == 0
    assert L.tsim_topk_large_workspace_bytes(Q, N, 0) == 0
    assert L.tsim_topk_large_workspace_bytes(0, N, 100) == 0
    assert L.tsim_topk_large_workspace_bytes(Q, 0, 100) == 0
    for k in (1, 10, 28, 29, 64):
        for q, n in ((256, 1_000_000), (3, 70), (5000, 20_000)):
            assert L.tsim_topk_large_workspace_bytes(q, n, k) == L.tsim_cosine_topk_workspace_bytes(q, n, k), (q, n, k)
    # the brute-force chunk lists are held to a fixed budget: the workspace grows about linearly in Q, not as Q x 64 chunks x k
    big = L.tsim_topk_large_workspace_bytes(4096, N, 1024)
    assert big < (1 << 30)
    assert L.tsim_topk_large_workspace_bytes(4096, N, 1000) <= big


def _args(p, k, ws, dot):
    eq = dict(eq=p, eq_f32=p, ldq=384, Q=4, ec=p, ec_f32=p, ldc=384)
    tail = (100, 384, 384, k, p, p, None, 0, p, ws, None)
    if dot:
        return (eq["eq"], eq["eq_f32"], eq["ldq"], eq["Q"], eq["ec"], eq["ec_f32"], eq["ldc"], p, p) + tail
    return (eq["eq"], eq["eq_f32"], eq["ldq"], eq["Q"], eq["ec"], eq["ec_f32"], eq["ldc"], p) + tail


@pytest.mark.parametrize("dot", [False, True])
def test_argument_checks_before_any_launch(dot):
    """Fake (never dereferenced) 16-byte aligned device pointers: every refusal happens on the host."""
    L = _lib_or_skip()
    fn = L.tsim_dot_topk_large if dot else L.tsim_cosine_topk_large
    p = 1 << 20
    big = 1 << 40
    assert fn(*_args(p, 1025, big, dot)) == 1            # TSIM_EINVAL: k > TSIM_TOPK_MAX_K
    assert b"1..1024" in L.tsim_last_error()
    assert fn(*_args(p, 0, big, dot)) == 1
    for k in (65, 100, 1024, 10):
        need = L.tsim_topk_large_workspace_bytes(4, 100, k)
        assert fn(*_args(p, k, need - 1, dot)) == 3, k     # TSIM_ENOMEM: short workspace
    a = list(_args(p, 100, big, dot))
    a[1] = None                                          # float32 matrices: both or neither (cosine) / required (dot)
    assert fn(*a) == 1
