"""tsim_mst_prim on the GPU: (from, to, w2) bit for bit the literal Prim loop of tests/hdbscan_cases.mst_ref.

Sizes around a wave's 64 rows and a workgroup's 256 (the step kernel's grid is one workgroup per 256 rows and is never capped, so
there is no further threshold), every width class of the exact scores (one register set up to 384, two beyond, odd widths, the
largest), a row stride above the width, core distances absent and given, core-dominated weights (most w equal a core value:
both tie rules decide), duplicate rows, integer grids, rows of large norm, and the argument checks."""
import functools

import numpy as np
import pytest
import torch

import hdbscan_cases as hc
from list_cases import same_bits
from text_similarity_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _rows(kind, n, d):
    rng = np.random.default_rng(1000 * n + d)
    if kind == "gauss":
        x = rng.standard_normal((n, d))
    elif kind == "large_norm":        # a norm-expansion shortcut (|a|^2 + |b|^2 - 2 a.b) loses the difference here
        x = 1e4 * rng.standard_normal((n, d))
    elif kind == "grid":              # integer coordinates: many equal distances
        x = rng.integers(0, 4, size=(n, d)).astype(np.float64)
    elif kind == "duplicates":        # groups of identical rows: weight 0, ties everywhere
        x = np.repeat(rng.standard_normal((-(-n // 7), d)), 7, axis=0)[rng.permutation(-(-n // 7) * 7)[:n]]
    else:
        raise ValueError(kind)
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _ref(kind, n, d, min_samples):
    rows = _rows(kind, n, d)
    core2 = hc.core2_ref(rows, min_samples) if min_samples else None
    # (the blocked form gives the literal loop's results, tests/test_hdbscan_cpu.py, in a fraction of its time)
    return core2, (hc.mst_ref_blocked if n > 1000 else hc.mst_ref)(rows, core2)


def _check(kind, n, d, min_samples, pad=0):
    rows = _rows(kind, n, d)
    core2, (frm, to, w2) = _ref(kind, n, d, min_samples)
    if pad:                            # ld_rows > d: the rows are a view of a wider buffer filled with NaN
        buf = torch.full((n, d + pad), float("nan"), dtype=torch.float32, device=DEV)
        buf[:, :d] = torch.from_numpy(np.array(rows))
        x = buf[:, :d]
        assert x.stride(0) == d + pad or n == 1
    else:
        x = torch.from_numpy(np.array(rows)).to(DEV)
    c = torch.from_numpy(core2).to(DEV) if core2 is not None else None
    gf, gt, gw = ops.mst_prim(x, c)
    torch.cuda.synchronize()
    assert gf.dtype == gt.dtype == torch.int32 and gw.dtype == torch.float32 and gf.shape == gt.shape == gw.shape == (n - 1,)
    gf, gt, gw = gf.cpu().numpy(), gt.cpu().numpy(), gw.cpu().numpy()
    first = np.flatnonzero((gf != frm) | (gt != to) | (gw.view(np.uint32) != w2.view(np.uint32)))
    assert first.size == 0, (kind, n, d, min_samples, "first differing step", int(first[0]), (gf[first[0]], gt[first[0]], gw[first[0]]),
                             (frm[first[0]], to[first[0]], w2[first[0]]))
    assert same_bits(gw, w2)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1025])
@pytest.mark.parametrize("min_samples", [0, 4])
def test_sizes_around_a_wave_and_a_workgroup(n, min_samples):
    _check("gauss", n, 33, min(min_samples, n))


@pytest.mark.parametrize("d", [1, 33, 64, 384, 385, 767])
@pytest.mark.parametrize("min_samples", [0, 5])
def test_widths_and_a_row_stride_above_the_width(d, min_samples):
    _check("gauss", 130, d, min_samples, pad=0 if d == 64 else 3)


@pytest.mark.parametrize("kind,d,min_samples", [("gauss", 8, 60), ("grid", 3, 40)])
def test_core_dominated_weights_pin_both_tie_rules(kind, d, min_samples):
    n = 300
    core2, (frm, to, w2) = _ref(kind, n, d, min_samples)
    assert (w2 == np.maximum(core2[frm], core2[to])).mean() > 0.8      # most weights are a core value ...
    if kind == "grid":                      # ... and on the grid equal ones meet: the earlier endpoint and the lower row decide
        assert np.unique(core2).size <= 4 and np.unique(w2).size <= 4
    _check(kind, n, d, min_samples)


@pytest.mark.parametrize("kind,n,d,min_samples", [("duplicates", 200, 12, 0), ("duplicates", 200, 12, 5), ("grid", 260, 3, 0),
                                                  ("grid", 260, 3, 6), ("large_norm", 150, 40, 0), ("large_norm", 150, 40, 4)])
def test_ties_and_large_norms(kind, n, d, min_samples):
    if kind != "large_norm":
        _, (_, _, w2) = _ref(kind, n, d, min_samples)
        assert np.unique(w2).size < (n - 1) // 4
    _check(kind, n, d, min_samples)


def test_argument_checks():
    L = _lib.lib()
    x = torch.zeros((10, 8), dtype=torch.float32, device=DEV)
    out = torch.zeros((9,), dtype=torch.int32, device=DEV)
    w = torch.zeros((9,), dtype=torch.float32, device=DEV)
    need = L.tsim_mst_prim_workspace_bytes(10)
    ws = torch.zeros((need,), dtype=torch.uint8, device=DEV)
    p, o, wp, wsp = x.data_ptr(), out.data_ptr(), w.data_ptr(), ws.data_ptr()
    for n, d, ld in ((0, 8, 8), (10, 0, 8), (10, 768, 768), (10, 8, 7), ((1 << 31) - 64, 8, 8)):
        assert L.tsim_mst_prim(p, ld, n, d, None, o, o, wp, wsp, need, None) == 1
    assert L.tsim_mst_prim(p, 8, 10, 8, None, o, o, wp, wsp, need - 1, None) == 3          # a workspace that is too small
    assert L.tsim_mst_prim(p, 8, 10, 8, None, o, o, wp, None, need, None) == 3
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0 and int(ws.sum()) == 0                                 # nothing was launched
    for bad in (x.double(), x[0], x.cpu()):
        with pytest.raises((ValueError, _lib.TsimError)):
            ops.mst_prim(bad)
    with pytest.raises(ValueError):
        ops.mst_prim(torch.zeros((4, 768), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        ops.mst_prim(x, torch.zeros((9,), dtype=torch.float32, device=DEV))
    f, t, w2 = ops.mst_prim(x[:1])
    assert f.numel() == t.numel() == w2.numel() == 0
    f, t, w2 = ops.mst_prim(x)              # ten equal rows: every weight 0, the rows join in order from row 0
    assert f.tolist() == [0] * 9 and t.tolist() == list(range(1, 10)) and w2.tolist() == [0.0] * 9
