"""tsim_mst_prim on rows placed FAR APART (tests/far_cases.py, Layout F): the 6 000 float32 rows lie 719 184 elements apart, so
their offsets from the pointer the kernel is handed cross 2^31, 2^32, 2^33 and 2^34 bytes — 2^31 and 2^32 elements — and row 1 493
straddles 2^32 bytes.  The buffer around the rows is 0xFF: a step kernel that drops one (int64_t) in ``row * ld_rows`` reads NaN
or another row, and the tree changes (tests/test_far_cases_cpu.py shows that every modelled truncation misreads rows of exactly
these corpora).  Two bars, both exact: the tree on the far view equals the tree of the same call on a compact copy, and it
equals the Prim restatement on the dense rows (hdbscan_cases.mst_ref_blocked: mst_ref's loop on distances made in blocks, the
same bits — the literal loop would take two minutes at this size).

Needs 18.5 GB of free device memory."""
import gc

import numpy as np
import pytest
import torch

import far_cases as fc
import hdbscan_cases as hc
from text_similarity_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEED = fc.LAYOUT_F.nbytes + (5 << 28)


@pytest.fixture(scope="module")
def far_f():
    free = torch.cuda.mem_get_info()[0]
    if free < NEED:
        pytest.skip(f"layout F needs {NEED / 1e9:.1f} GB of device memory, {free / 1e9:.1f} GB are free")
    fb = fc.FarBuffer(fc.LAYOUT_F, DEV)
    yield fb
    del fb
    gc.collect()
    torch.cuda.empty_cache()


def _np(out):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _same(got, want, what):
    for name, g, w in zip(("from", "to", "w2"), got, want):
        g, w = (np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a for a in (g, w))
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (what, name, "first differing step", int(bad[0]), bad.size)


@pytest.mark.parametrize("kind,d,with_core", [("gauss", 256, True), ("near_ties", 300, False)])
def test_mst_far_rows(far_f, kind, d, with_core):
    _, c = fc.rows("F", kind, d)
    assert c.shape == (fc.N, d) and d > 112                 # (row 1 493 starts 112 elements below 2^32 bytes: it straddles)
    core2 = None
    if with_core:                                           # any non-negative float32 [N] is a legal core2; this one binds often
        core2 = np.sort(hc.d2_upper(c[:64])[0])[8] * np.random.default_rng(6).uniform(0.8, 1.2, fc.N).astype(np.float32)
    want = hc.mst_ref_blocked(c, core2)
    view = far_f.place(c)
    assert view.stride(0) == fc.LAYOUT_F.stride and (fc.N - 1) * view.stride(0) * 4 > 1 << 34
    core_dev = torch.from_numpy(core2).to(DEV) if with_core else None
    got = _np(ops.mst_prim(view, core_dev))
    compact = _np(ops.mst_prim(view.contiguous(), core_dev))
    _same(got, compact, "far view against the compact copy")
    _same(got, want, "far view against the restatement")
    if with_core:
        assert 0.05 < (want[2] == np.maximum(core2[want[0]], core2[want[1]])).mean() < 0.95      # both kinds of weight occur
