"""The encoder kernels on the accepted configurations that no other test reaches (tests/config_cases.py: its docstring holds the
route table and says which kernel each case runs first), against the float64 probe oracle under the tolerance rule of
tests/encoder_cases.py: TOL = 2 x floor, floor = the probe's bf16 emulation against the exact probe on the same inputs,
computed at test time.  tests/test_encoder_power_cpu.py proves for every case here that the named defects, among them a
dropped partial head group and a dropped feature tail of FFN1, lie at >= 4 x TOL.

Every case is one forward of ~1 300 tokens per handle; the route tests are one large forward and four small ones.  These
routes ran for the first time with this file: run a new case alone and under a time limit of its own first, for instance
``timeout -k 10 300 python -m pytest "tests/test_encoder_config_gpu.py::test_hidden_states_after_every_layer[bert-64-h2-f64]" -m gpu -s``."""
from dataclasses import replace

import numpy as np
import pytest
import torch

import config_cases as cc
import encoder_cases as ec
from test_encoder_sharp_gpu import compare
from text_similarity_amd import presets
from text_similarity_amd.native_encoder import NativeEncoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", list(cc.CASES))
def test_hidden_states_after_every_layer(name):
    cfg, wdtype = cc.CASES[name]
    ids, cu, notes = cc.inputs(name)
    w = cc.weights(name)
    exact, floor, tol = cc.tolerances(name)
    fd, cd = torch.from_numpy(ids.copy()).to(DEV), torch.from_numpy(cu.astype(np.int32)).to(DEV)
    empty = np.diff(cu) == 0
    assert empty.any()
    for l in range(1, cfg.num_layers + 1):      # the first boundary that misses is the layer that is wrong
        enc = NativeEncoder(replace(cfg, num_layers=l), w, max_tokens=ids.size, max_seqs=cu.size - 1, weight_dtype=wdtype)
        r = enc.forward_packed(fd, cd, pooled=True, unit=cfg.hidden <= 768, hidden=True)
        torch.cuda.synchronize()
        enc.check()
        h = r["hidden"].float().cpu().numpy()
        p = r["pooled"].cpu().numpy()
        assert (p[empty] == 0).all()
        if cfg.hidden <= 768:               # (unit rows stop at width 768)
            assert (r["unit"].float().cpu().numpy()[empty] == 0).all()
        compare(f"{name} boundary {l}", h, exact[l], floor[l], tol[l], cu)
        if l == cfg.num_layers:
            compare(f"{name} pooled", p, ec.pooled_rows(exact[l], cu), floor["pooled"], tol["pooled"])
        del enc


def _big_and_slices(name, n, seed):
    """One call of n sentences and the same sentences 48 at a time: yields (first row, token range, cu of the slice, hidden and
    pooled rows of the large call, of the small call) for four slices; the last one holds the rows the remainder launches compute."""
    cfg, wdtype = cc.CASES[name]
    flat, cu = presets.synthetic_token_batch(n, seed=seed, vocab_size=ec.VOCAB, max_len=64)
    cu = cu.astype(np.int64)
    enc = NativeEncoder(cfg, cc.weights(name), max_tokens=int(cu[-1]), max_seqs=n, weight_dtype=wdtype)
    big = enc.forward_packed(torch.from_numpy(flat).to(DEV), torch.from_numpy(cu.astype(np.int32)).to(DEV), pooled=True, hidden=True)
    torch.cuda.synchronize()
    enc.check()
    assert torch.isfinite(big["hidden"].float()).all() and torch.isfinite(big["pooled"]).all()
    for s in sorted({0, 480, 1452, n - 48}):
        a, b = int(cu[s]), int(cu[s + 48])
        c = cu[s:s + 49] - cu[s]
        small = enc.forward_packed(torch.from_numpy(flat[a:b]).to(DEV), torch.from_numpy(c.astype(np.int32)).to(DEV), pooled=True, hidden=True)
        torch.cuda.synchronize()
        yield s, flat[a:b], c, (big["hidden"][a:b], big["pooled"][s:s + 48]), (small["hidden"], small["pooled"])


@pytest.mark.parametrize("name,n", [("bert-384-h6-f768", 2300), ("bert-384-h6-f768", 4700), ("bert-384-h24-f1920", 4700),
                                    ("bert-384-f1024", 2300)])
def test_hidden_384_token_count_routes(name, n):
    """The token-count routes of the hidden-384 layer (tests/test_encoder_gpu.py::test_large_batch_equals_small_batches_bitwise
    names them) at ffn widths other than 1536: 2300 sentences = ln_rows_gemm + tail, 4700 = one whole round, chained launches where
    ffn <= 1536 and packed, + the 64-token remainder launch; bert-384-f1024 is the row-major form, whose K = 1024 has no ln_tail.
    48-sentence slices of ONE large call equal the same sentences encoded alone bit for bit, and meet the probe under the TOL of
    the case."""
    cfg, _ = cc.CASES[name]
    _, floor, tol = cc.tolerances(name)
    L = cfg.num_layers
    for s, ids, c, big, small in _big_and_slices(name, n, "config/route"):
        assert torch.equal(big[0], small[0]), f"{name} n={n}: hidden states of rows {s}.. differ between batch sizes"
        assert torch.equal(big[1], small[1]), f"{name} n={n}: pooled rows {s}.. differ between batch sizes"
        ref = cc.probe(name, ids=ids, cu=c)[L]
        compare(f"{name} n={n} rows {s}..{s + 47} hidden", big[0].float().cpu().numpy(), ref, floor[L], tol[L], c)
        compare(f"{name} n={n} rows {s}..{s + 47} pooled", big[1].cpu().numpy(), ec.pooled_rows(ref, c), floor["pooled"], tol["pooled"])


@pytest.mark.parametrize("name", ["bert-768-h24-f1920", "bert-768-h48-f1984", "bert-768-h24-f2048-mxfp8"])
def test_many_tiles_per_workgroup(name):
    """1500 sentences (~24 k tokens) in one call: every projection has more than 256 output tiles, so the persistent workgroups of
    the ping-pong GEMM cross a tile boundary with the 128-wide feature tile, on row-major W, with an odd number of k-tiles
    (slot parity carried across tiles) and with the MXFP8 epilogue at 8 feature tiles.  Bit for bit the same sentences 48 at a time."""
    for s, ids, c, big, small in _big_and_slices(name, 1500, "config/tiles"):
        assert torch.equal(big[0], small[0]), f"{name}: hidden states of rows {s}.. differ between batch sizes"
        assert torch.equal(big[1], small[1]), f"{name}: pooled rows {s}.. differ between batch sizes"


@pytest.mark.parametrize("name", list(cc.REFUSED))
def test_refused_configurations(name):
    """ffn = 64 above hidden 64: FFN2 would run with K = 64, for which hidden 1024 has no kernel, hidden 768 had one that no
    shipped shape ever ran (removed with the encoder's plan: no accepted configuration reaches it) and hidden 384 one that fails at the first large batch.  MXFP8 with an ffn that is no multiple of 256:
    no tile of the block-scaled GEMM.  Both refused in tsim_encoder_create (TSIM_EUNSUPPORTED, a ValueError here), before any
    allocation or launch, with the accepted values in the message."""
    cfg, wdtype, text = cc.REFUSED[name]
    with pytest.raises(ValueError, match=text):
        NativeEncoder(cfg, presets.synthetic_weights("config/" + name, cfg), max_tokens=256, max_seqs=4, weight_dtype=wdtype)
