"""The chained launches of the hidden-384 BERT path (ln_rows_xres2): wherever the LayerNorm GEMM has whole 256-token blocks for
ln_rows_gemm in whole rounds of 256 (65 536 .. 65 536 + 127 x 256 tokens, 131 072 .., ...: the projection keeps the 256 workgroups
it has on its own), those blocks' workgroups keep the normalised rows in registers and run the next
projection themselves — O-projection -> FFN1 and FFN2 -> the next layer's QKV — and share out the projection items of the
rows behind the whole blocks.  No arithmetic changed, so every row must carry the bits the stand-alone kernels give it: the
reference is the same sentences encoded in sub-batches of at most 48 sentences (ln_split + gemm_xres2), whose bits
tests/test_residual_packed_gpu.py ties to the parent.  Compared with torch.equal, hidden rows and pooled rows, for the sentences
around every block boundary of each case."""
import numpy as np
import pytest
import torch

import residual_cases as rc
from text_similarity_amd import presets
from text_similarity_amd.native_encoder import NativeEncoder

pytestmark = pytest.mark.gpu
N_SENT = 9000
MAX_T = 131072 + 40
# T -> the whole blocks that go to ln_rows_gemm / the chained kernel (ln_rows_blocks), for the boundaries below
CASES = {
    32768: 128,                 # half a round of whole blocks: stand-alone kernels (a chained launch would halve the projection's grid)
    32768 + 255: 128,
    98304 + 40: 384,            # a round and a half: stand-alone kernels
    65536: 256,                 # chained, no remainder: R = 0
    65536 + 255: 256,           # chained, one partial remainder block
    65536 + 300: 256,           # chained, two remainder blocks, the second with 44 rows: items spread over the workgroups
    131072 + 40: 512,           # 512 chained workgroups: more than one round of CUs
}


@pytest.fixture(scope="module")
def sentences():
    flat, cu = presets.synthetic_token_batch(N_SENT, seed="chain-fused", vocab_size=1000, max_len=64)
    assert int(cu[-1]) >= MAX_T
    return flat, cu.astype(np.int64)


@pytest.fixture(scope="module")
def enc2():
    return NativeEncoder(rc.config(2), rc.weights(2), max_tokens=MAX_T, max_seqs=N_SENT)


def _groups(c, T, blocks):
    """Runs of at most 48 sentences around the first and the last row, the 256-row boundaries of the first blocks, of the last
    chained blocks, of every CU round (256 blocks) and of the remainder blocks, and the 32-row boundary inside the last block."""
    B = len(c) - 1
    rows = {0, T - 1, 256, 512, 32 * 256, 128 * 256, 255 * 256, 256 * 256, 257 * 256, 383 * 256, (blocks - 1) * 256, blocks * 256,
            (blocks + 1) * 256, 511 * 256, (T - 1) // 256 * 256, (T - 1) // 32 * 32}
    sel = sorted({int(np.searchsorted(c, t, side="right")) - 1 for t in rows if 0 < t < T} | {0, B - 1})
    out = []
    for s in sel:
        a = max(min(s - 24, B - 48), 0)
        if not out or a >= out[-1][1]:
            out.append((a, min(a + 48, B)))
    return out


def _check(enc, flat, cu, T, blocks):
    f, c = rc.cut(flat, cu, T)
    big_p, big_h = rc.encode(enc, f, c)
    big_p, big_h = big_p.clone(), big_h.clone()
    assert torch.isfinite(big_p).all() and torch.isfinite(big_h.float()).all()
    groups = _groups(c, T, blocks)
    assert len(groups) >= 3
    for s, e in groups:
        t0, t1 = int(c[s]), int(c[e])
        assert t1 - t0 < 8192                 # a small batch: the stand-alone kernels
        p, h = rc.encode(enc, f[t0:t1], c[s:e + 1] - t0)
        assert torch.equal(h, big_h[t0:t1]), f"T={T}: hidden rows {t0}..{t1 - 1} (sentences {s}..{e - 1}) differ"
        assert torch.equal(p, big_p[s:e]), f"T={T}: pooled rows of sentences {s}..{e - 1} differ"


@pytest.mark.parametrize("T", sorted(CASES), ids=[f"T{t}" for t in sorted(CASES)])
def test_rows_equal_sub_batches_bitwise(enc2, sentences, T):
    _check(enc2, *sentences, T, CASES[T])


def test_one_layer_only_ffn1_is_chained(sentences):
    """One layer: only O-projection -> FFN1 is chained, with the embedding kernel's row-major x0 as the residual; the FFN2 of
    the last layer keeps its own launches.  (32 768 + 33: the same model on the stand-alone kernels.)"""
    enc = NativeEncoder(rc.config(1), rc.weights(1), max_tokens=65536 + 33, max_seqs=N_SENT)
    _check(enc, *sentences, 32768 + 33, 128)
    _check(enc, *sentences, 65536 + 33, 256)


def test_twenty_forwards_give_one_digest(enc2, sentences):
    """A missing barrier between the LayerNorm ring and the W ring, or a ring wait that counts the epilogue's stores wrongly, is
    a race: it does not give the same bytes twenty times."""
    f, c = rc.cut(*sentences, 65536 + 300)
    seen = {tuple(sorted(rc.digests(*rc.encode(enc2, f, c)).items())) for _ in range(20)}
    assert len(seen) == 1, f"{len(seen)} different results in 20 forwards"


def test_stale_blocks_are_not_read(enc2, sentences):
    """33 tokens after 131 072 + 40 (chained) and after 98 304 + 40 on the same encoder against the same 33 tokens on an encoder that has run nothing else."""
    flat, cu = sentences
    rc.encode(enc2, *rc.cut(flat, cu, 98304 + 40))
    rc.encode(enc2, *rc.cut(flat, cu, 131072 + 40))
    f, c = rc.cut(flat, cu, 33)
    p, h = rc.encode(enc2, f, c)
    fresh = NativeEncoder(rc.config(2), rc.weights(2), max_tokens=256, max_seqs=16)
    p0, h0 = rc.encode(fresh, f, c)
    assert torch.equal(h, h0) and torch.equal(p, p0)
