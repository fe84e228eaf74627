"""The hidden-384 BERT path keeps its residual stream x0 / x1 block-packed between layers: the LayerNorm GEMMs (ln_rows_gemm,
ln_tail / ln_split, gemm_bf16's EPI_RES_LN form) write and read it through group_off, gemm_xres2 loads its resident fragments
from it.  Layer 0 still reads the embedding kernel's row-major rows and the last layer still writes row-major ones, so models
of 1, 2 and 3 layers cover every combination.  Only addresses changed: every bit must be what the row-major stream gave
(tests/golden/residual_stream_parent.json, written by tools/hash_forward.py on the parent commit), rows must not depend on
the batch they were encoded in, and nothing may be read from the padding rows a longer forward left behind.

Bars of the oracle check: those of test_encoder_gpu.py (max |err| <= 8e-2 on hidden rows, <= 5e-2 on pooled rows, row cosine
>= 0.9995), which cover 12-layer encoders; these have at most three."""
import json
import os

import numpy as np
import pytest
import torch

import residual_cases as rc
from oracle import encoder_ref
from text_similarity_amd import presets
from text_similarity_amd.native_encoder import NativeEncoder

pytestmark = pytest.mark.gpu
HID_TOL, POOL_TOL, COS_MIN = 8e-2, 5e-2, 0.9995
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "residual_stream_parent.json")


@pytest.fixture(scope="module")
def sentences():
    return rc.sentences()


@pytest.fixture(scope="module")
def parent_digests():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module", params=rc.LAYERS, ids=[f"L{n}" for n in rc.LAYERS])
def model(request, sentences):
    """(layers, weights, encoder, {T: (flat, cu, pooled, hidden)}): every token count encoded once, shared by the tests."""
    L = request.param
    w = rc.weights(L)
    enc = NativeEncoder(rc.config(L), w, max_tokens=rc.MAX_T, max_seqs=rc.N_SENT)
    flat, cu = sentences
    runs = {}
    for T in rc.TOKENS:
        f, c = rc.cut(flat, cu, T)
        p, h = rc.encode(enc, f, c)
        runs[T] = (f, c, p.clone(), h.clone())
    return L, w, enc, runs


def _sample(c, T):
    """The first and the last sentence and those holding the rows on both sides of the 32-row / 256-row block boundaries and of
    the last round of ln_rows_gemm."""
    B = len(c) - 1
    rows = {0, T - 1}
    for b in (32, 256, 8192, 9984, 32768):
        rows |= {b - 1, b}
    rows |= {(T - 1) // 32 * 32, (T - 1) // 256 * 256}
    sel = {int(np.searchsorted(c, t, side="right")) - 1 for t in rows if 0 <= t < T}
    return sorted(s for s in sel if 0 <= s < B)


def _cos_rows(a, b):
    num = (a * b).sum(1)
    return num / np.maximum(np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1), 1e-30)


def test_rows_match_fp32_oracle(model):
    L, w, enc, runs = model
    cfg = rc.config(L)
    for T, (f, c, p, h) in runs.items():
        sel = _sample(c, T)
        ids, mask = encoder_ref.pad_batch(f, c, sel)
        with torch.no_grad():
            ref_h = encoder_ref.encoder_forward(cfg, w, ids, mask)
            ref_p = encoder_ref.mean_pool(ref_h, mask).numpy()
        ref_h = ref_h.numpy()
        got_p = p[sel].cpu().numpy()
        hid_err = 0.0
        for i, s in enumerate(sel):
            n = int(c[s + 1] - c[s])
            got = h[int(c[s]):int(c[s + 1])].float().cpu().numpy()
            hid_err = max(hid_err, float(np.abs(got - ref_h[i, :n]).max()))
        pool_err = float(np.abs(got_p - ref_p).max())
        cos = float(_cos_rows(got_p, ref_p).min())
        print(f"L={L} T={T}: {len(sel)} sentences, hidden max|err|={hid_err:.4f} pooled max|err|={pool_err:.4f} min cos={cos:.6f}")
        assert hid_err <= HID_TOL and pool_err <= POOL_TOL and cos >= COS_MIN, (T, hid_err, pool_err, cos)


def test_rows_equal_sub_batches_bitwise(model):
    """Sentences of the two large batches (gemm_bf16's form at 10 000 tokens; ln_rows_gemm and its remainder at 32 768 + 33)
    encoded again in sub-batches that take ln_split (48 sentences) and ln_tail (>= 4 200 tokens), and the small batches
    against the rows of the large one."""
    L, w, enc, runs = model
    for T in (10000, 32768 + 33):
        f, c, big_p, big_h = runs[T]
        B = len(c) - 1
        first_rem = int(np.searchsorted(c, T // 256 * 256, side="right")) - 1
        groups = [(s, min(s + 48, B)) for s in sorted({0, max(first_rem - 24, 0), B - 48})]
        s = int(np.searchsorted(c, T - 4200, side="right")) - 1
        groups.append((s, B))
        for s, e in groups:
            t0, t1 = int(c[s]), int(c[e])
            p, h = rc.encode(enc, f[t0:t1], c[s:e + 1] - t0)
            assert torch.equal(h, big_h[t0:t1]), f"L={L} T={T}: hidden rows of sentences {s}..{e - 1} differ"
            assert torch.equal(p, big_p[s:e]), f"L={L} T={T}: pooled rows of sentences {s}..{e - 1} differ"
    _, cb, big_p, big_h = runs[32768 + 33]
    for T in rc.TOKENS[:-1]:
        f, c, p, h = runs[T]
        B = len(c) - 1
        n_full = B - 1 if int(c[B]) < int(cb[B]) else B     # a shortened last sentence differs from the big batch's
        assert torch.equal(h[:int(c[n_full])], big_h[:int(c[n_full])]), f"L={L} T={T}: hidden rows differ"
        assert torch.equal(p[:n_full], big_p[:n_full]), f"L={L} T={T}: pooled rows differ"
        assert torch.isfinite(p).all() and torch.isfinite(h.float()).all()


def test_stale_padding_is_not_read(model, sentences):
    """33 tokens after 10 000 on the same encoder (its buffers hold the longer forward's rows behind row 33) against the same
    33 tokens on an encoder that has run nothing else."""
    L, w, enc, runs = model
    flat, cu = sentences
    rc.encode(enc, *rc.cut(flat, cu, 10000))
    f, c = rc.cut(flat, cu, 33)
    p, h = rc.encode(enc, f, c)
    fresh = NativeEncoder(rc.config(L), w, max_tokens=256, max_seqs=16)
    p0, h0 = rc.encode(fresh, f, c)
    assert torch.equal(h, h0) and torch.equal(p, p0)


def test_bits_of_the_row_major_parent(model, parent_digests):
    L, w, enc, runs = model
    for T, (f, c, p, h) in runs.items():
        assert rc.digests(p, h) == parent_digests[rc.case_id(L, T)], f"L={L} T={T}"


def test_minilm_bench_shape_bits_of_the_row_major_parent(parent_digests):
    f, c = rc.minilm_sentences()
    enc = NativeEncoder.from_preset("all-MiniLM-L6-v2", max_tokens=rc.MINILM_T, max_seqs=rc.MINILM_SENT)
    assert rc.digests(*rc.encode(enc, f, c)) == parent_digests[f"all-MiniLM-L6-v2-T{rc.MINILM_T}"]
