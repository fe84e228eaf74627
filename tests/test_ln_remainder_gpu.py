"""The hidden-384 LayerNorm GEMMs (O-projection, FFN2) for few rows: ln_rows_gemm's remainder and small batches go through
ln_tail_gemm, which splits the 384 output features over 4 or 2 workgroups per 32-row block (ln_split) when the row blocks
leave most CUs idle, and keeps one workgroup per block (ln_tail) otherwise.  Every form must give a row the same bits, so the
hidden rows and pooled rows of a batch are compared, bit for bit, with the same sentences encoded in smaller batches that take
other forms: 48 sentences at a time (a few hundred tokens: ln_split, 4 slices) and a group of >= 4 200 tokens (more than 128
row blocks: ln_tail)."""
import numpy as np
import pytest
import torch

from text_similarity_amd import presets
from text_similarity_amd.native_encoder import NativeEncoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRESET = "all-MiniLM-L6-v2"
N_SENT = 5000          # ~80 k tokens of synthetic sentences (16 per sentence on average)
MAX_T = 65536 + 8000


@pytest.fixture(scope="module")
def setup():
    cfg = presets.PRESETS[PRESET]
    flat, cu = presets.synthetic_token_batch(N_SENT, seed="ln-remainder", vocab_size=cfg.vocab, max_len=64)
    assert int(cu[-1]) >= MAX_T
    enc = NativeEncoder.from_preset(PRESET, max_tokens=MAX_T, max_seqs=N_SENT)
    return enc, flat, cu.astype(np.int64)


def _cut(flat, cu, T):
    """The first sentences of the list holding exactly T tokens (the last one shortened)."""
    n = int(np.searchsorted(cu, T, side="left"))
    c = cu[:n + 1].copy()
    c[n] = T
    assert c[n] > c[n - 1]
    return flat[:T], c


def _encode(enc, f, c):
    r = enc.forward_packed(torch.from_numpy(np.ascontiguousarray(f)).to(DEV), torch.from_numpy(c.astype(np.int32)).to(DEV),
                           hidden=True)
    torch.cuda.synchronize()
    return r["pooled"], r["hidden"]


def _check_group(enc, f, c, big_p, big_h, s, e, what):
    """Sentences s .. e - 1 of the batch (f, c), encoded on their own, against their rows of the whole batch."""
    t0, t1 = int(c[s]), int(c[e])
    p, h = _encode(enc, f[t0:t1], (c[s:e + 1] - t0))
    assert torch.equal(h, big_h[t0:t1]), f"{what}: hidden rows of sentences {s}..{e - 1} differ"
    assert torch.equal(p, big_p[s:e]), f"{what}: pooled rows of sentences {s}..{e - 1} differ"


# T = whole 256-token tiles of ln_rows_gemm + the remainder; ln_rows takes all of a last round that is at least half full
# (32 768 = 128 tiles) and whole rounds otherwise (65 536 = 256 tiles)
@pytest.mark.parametrize("T, rows_main, slices", [
    pytest.param(32768 + 1, 32768, 4, id="rem1-S4"),
    pytest.param(32768 + 31, 32768, 4, id="rem31-S4"),
    pytest.param(32768 + 33, 32768, 4, id="rem33-S4"),
    pytest.param(65536 + 1650, 65536, 4, id="rem1650-S4"),     # the benchmark's shape: 52 row blocks
    pytest.param(65536 + 2080, 65536, 2, id="rem2080-S2"),     # 65 row blocks: the first with two slices
    pytest.param(65536 + 3000, 65536, 2, id="rem3000-S2"),
    pytest.param(65536 + 4100, 65536, 1, id="rem4100-S1"),     # 129 row blocks: ln_tail
    pytest.param(65536 + 8000, 65536, 1, id="rem8000-S1"),
])
def test_remainder_rows_equal_smaller_batches_bitwise(setup, T, rows_main, slices):
    enc, flat, cu = setup
    f, c = _cut(flat, cu, T)
    big_p, big_h = _encode(enc, f, c)
    assert torch.isfinite(big_p).all() and torch.isfinite(big_h.float()).all()
    B = len(c) - 1
    rem = T - rows_main
    nb = (rem + 31) // 32
    assert {4: nb <= 64, 2: 64 < nb <= 128, 1: 128 < nb <= 256}[slices]
    first_rem = int(np.searchsorted(c, rows_main, side="right")) - 1     # the sentence holding the first remainder row
    groups = {0, max(first_rem - 24, 0), max(first_rem, 0), B - 48}
    for s in sorted(groups):
        _check_group(enc, f, c, big_p, big_h, s, min(s + 48, B), f"T={T}")
    # the last sentences of >= 4 200 tokens at once: more than 128 row blocks without ln_rows, i.e. ln_tail
    s = int(np.searchsorted(c, T - 4200, side="right")) - 1
    assert (T - int(c[s]) + 31) // 32 > 128
    _check_group(enc, f, c, big_p, big_h, s, B, f"T={T} (ln_tail group)")


@pytest.mark.parametrize("T", [1, 20, 100, 127, 2048, 2049, 4096, 4097])
def test_small_batches_equal_large_batch_bitwise(setup, T):
    """Batches with no ln_rows round at all: fewer tokens than 32 x 4 (one row block, four slices), and on both sides of the
    4- / 2- / 1-slice thresholds (64 and 128 row blocks).  Their rows against the same sentences inside a batch of 65 536 +
    1 650 tokens, where ln_rows_gemm computes them."""
    enc, flat, cu = setup
    fb, cb = _cut(flat, cu, 65536 + 1650)
    big_p, big_h = _encode(enc, fb, cb)
    f, c = _cut(flat, cu, T) if T > 1 else (flat[:1], np.array([0, 1], dtype=np.int64))
    p, h = _encode(enc, f, c)
    B = len(c) - 1
    last = int(c[B]) < int(cb[B])          # the last sentence was shortened: its rows differ from the big batch's
    n_full = B - 1 if last else B
    assert torch.equal(h[:int(c[n_full])], big_h[:int(c[n_full])]), f"T={T}: hidden rows differ"
    assert torch.equal(p[:n_full], big_p[:n_full]), f"T={T}: pooled rows differ"
    assert torch.isfinite(p).all() and torch.isfinite(h.float()).all()
