"""Binary embeddings on the GPU (ops.pack_sign_rows / hamming_topk / sign_rescore_topk, GpuBinaryIndex, encode_text(precision=
"ubinary")): every result is compared for equality with the numpy restatement of tests/hamming_cases.py.  No tolerance anywhere.

Shapes are the smallest at which each kernel can go wrong: widths around the 8-, 64- and 128-element boundaries of the code
layout, row counts around one block of the running list (1 024) and more than one chunk (70 000), k around 64 (the list length
changes) and at 1 024, more queries than one group (33 > 8)."""
import functools

import numpy as np
import pytest
import torch

import hamming_cases as hc
from text_similarity_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


# ------------------------------------------------------------------------------------------------- pack
@pytest.mark.parametrize("d", (1, 7, 8, 9, 64, 65, 384, 1000, 1024))
@pytest.mark.parametrize("rows", (3, 257))
def test_pack_sign_rows(d, rows):
    x = hc.special_rows(rows, d, seed=1000 * rows + d)
    xb = hc.to_bf16_f32(x)                                             # (the float32 subnormals became +-0)
    xb.reshape(-1)[-2:] = np.array([0x00010000, 0x80010000], np.uint32).view(np.float32)   # +- the smallest bf16 subnormal
    for src, to_dev in ((x, lambda a: a), (xb, lambda a: a.to(torch.bfloat16))):
        want = hc.pack_ref(src)
        got = ops.pack_sign_rows(to_dev(_dev(src)))
        assert got.dtype == torch.uint8 and tuple(got.shape) == (rows, hc.code_bytes(d))
        assert np.array_equal(got.cpu().numpy(), want)
        wide = np.full((rows, d + 5), np.float32(1.0))                                       # ld_in = d + 5
        wide[:, :d] = src
        got = ops.pack_sign_rows(to_dev(_dev(wide))[:, :d])
        assert np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(ops.codes_from_packbits(np.packbits(x > 0, axis=1), d).cpu().numpy(), hc.pack_ref(x))


# ------------------------------------------------------------------------------------------------- Hamming top-k
#        d     N      Q   k
CASES = ((1, 9, 3, 10),            # N < k: padding
         (1, 1, 1, 1),
         (8, 5000, 3, 65),         # nine distinct distances: ties across every block and chunk boundary
         (8, 5000, 1, 1024),
         (65, 1025, 33, 10),
         (65, 9, 33, 64),
         (384, 70000, 3, 10),
         (384, 1023, 33, 64),
         (384, 5000, 33, 1),
         (768, 1024, 1, 1),
         (768, 70000, 1, 65),
         (1024, 5000, 3, 1024),
         (1024, 1025, 33, 65),
         (1024, 1023, 1, 10))


@functools.lru_cache(maxsize=None)
def _codes(d, N, Q):
    """(q_codes, c_codes) in the padded layout; one row — query 0 with a few elements flipped — copied to rows 0, 1 023, 1 024
    and N - 1 where they exist"""
    rng = np.random.default_rng(d * 1_000_003 + N * 101 + Q)
    q, c = hc.random_rows(rng, Q, d), hc.random_rows(rng, N, d)
    near = q[0].copy()
    near[:min(2, d - 1)] *= -1
    for r in (0, 1023, 1024, N - 1):
        if 0 <= r < N:
            c[r] = near
    return hc.pack_ref(q), hc.pack_ref(c)


@functools.lru_cache(maxsize=None)
def _topk_want(d, N, Q, k):
    qc, cc = _codes(d, N, Q)
    return hc.hamming_topk_ref(qc, cc, d, k)


@pytest.mark.parametrize("d,N,Q,k", CASES)
def test_hamming_topk(d, N, Q, k):
    qc, cc = _codes(d, N, Q)
    wd, wi = _topk_want(d, N, Q, k)
    gd, gi = ops.hamming_topk(_dev(qc), _dev(cc), d, k)
    assert gd.dtype == torch.int32 and gi.dtype == torch.int64
    assert np.array_equal(gd.cpu().numpy(), wd) and np.array_equal(gi.cpu().numpy(), wi)
    if N >= 1025 and d >= 65 and k >= 4:   # the copies lead query 0's list, tied, in row order
        copies = sorted({0, 1023, 1024, N - 1})
        assert wi[0, :len(copies)].tolist() == copies and len(set(wd[0, :len(copies)].tolist())) == 1


@pytest.mark.parametrize("d,N,Q,k", ((384, 70000, 3, 10), (65, 1025, 33, 10), (8, 5000, 3, 65)))
def test_hamming_topk_strided_rows_and_offset(d, N, Q, k):
    """ldc = code_bytes + 16 (a view into wider rows whose extra bytes hold junk), idx_offset = 10**9, preallocated outputs"""
    qc, cc = _codes(d, N, Q)
    wd, wi = _topk_want(d, N, Q, k)
    cb = hc.code_bytes(d)
    wide = np.full((N, cb + 16), 0xA5, np.uint8)
    wide[:, :cb] = cc
    out = (torch.empty((Q, k), dtype=torch.int32, device=DEV), torch.empty((Q, k), dtype=torch.int64, device=DEV))
    gd, gi = ops.hamming_topk(_dev(qc), _dev(wide)[:, :cb], d, k, idx_offset=10 ** 9, out=out)
    assert gd is out[0] and gi is out[1]
    assert np.array_equal(gd.cpu().numpy(), wd) and np.array_equal(gi.cpu().numpy(), np.where(wi >= 0, wi + 10 ** 9, -1))


def test_hamming_topk_ignores_bits_beyond_d():
    d, N, Q, k = 65, 1025, 33, 10
    qc, cc = _codes(d, N, Q)
    wd, wi = _topk_want(d, N, Q, k)
    rng = np.random.default_rng(3)
    jq, jc = qc.copy(), cc.copy()
    for a in (jq, jc):
        a[:, 8] |= rng.integers(0, 128, size=a.shape[0], dtype=np.uint8)            # bits 65 .. 71
        a[:, 9:] = rng.integers(0, 256, size=(a.shape[0], a.shape[1] - 9), dtype=np.uint8)
    assert not np.array_equal(jc, cc)
    gd, gi = ops.hamming_topk(_dev(jq), _dev(jc), d, k)
    assert np.array_equal(gd.cpu().numpy(), wd) and np.array_equal(gi.cpu().numpy(), wi)


@pytest.mark.parametrize("d,N,k", ((65, 1025, 10), (384, 1023, 64), (1024, 1025, 65)))
def test_hamming_topk_groups_do_not_leak(d, N, k):
    """the result for 33 queries is the 33 single-query results stacked"""
    qc, cc = _codes(d, N, 33)
    q_d, c_d = _dev(qc), _dev(cc)
    gd, gi = ops.hamming_topk(q_d, c_d, d, k)
    one = [ops.hamming_topk(q_d[i:i + 1], c_d, d, k) for i in range(33)]
    assert torch.equal(gd, torch.cat([o[0] for o in one])) and torch.equal(gi, torch.cat([o[1] for o in one]))


def test_hamming_topk_query_slices(monkeypatch):
    """more queries than one call takes: slices of 5, 5 and 2 strided query rows, each written to its own rows of the outputs"""
    monkeypatch.setattr(ops, "MAX_QUERIES_PER_CALL", 5)
    d, N, Q, k = 65, 300, 12, 3
    qc, cc = _codes(d, N, Q)
    cb = hc.code_bytes(d)
    wide = np.full((Q, cb + 16), 0xA5, np.uint8)
    wide[:, :cb] = qc
    wd, wi = hc.hamming_topk_ref(qc, cc, d, k)
    assert len({tuple(row) for row in wi.tolist()}) > 1
    gd, gi = ops.hamming_topk(_dev(wide)[:, :cb], _dev(cc), d, k)
    assert np.array_equal(gd.cpu().numpy(), wd) and np.array_equal(gi.cpu().numpy(), wi)


def test_hamming_topk_empty_sides():
    qc, cc = _codes(65, 9, 33)
    gd, gi = ops.hamming_topk(_dev(qc), _dev(cc)[:0], 65, 5)                      # N = 0: all padding
    assert (gd.cpu().numpy() == hc.INT32_MAX).all() and (gi.cpu().numpy() == -1).all()
    gd, gi = ops.hamming_topk(_dev(qc)[:0], _dev(cc), 65, 5)                      # Q = 0
    assert tuple(gd.shape) == (0, 5) and tuple(gi.shape) == (0, 5)
    with pytest.raises(ValueError):
        ops.hamming_topk(_dev(qc), _dev(cc), 65, 1025)
    with pytest.raises(ValueError):
        ops.hamming_topk(_dev(qc)[:, :8], _dev(cc), 65, 5)


# ------------------------------------------------------------------------------------------------- re-score
RS_N = 3000


@functools.lru_cache(maxsize=None)
def _rescore_rows(d):
    rng = np.random.default_rng(77 + d)
    q, c = hc.random_rows(rng, 5, d), hc.random_rows(rng, RS_N, d)
    c[11] = c[7]                                                                   # two equal code rows
    return q, hc.pack_ref(c)


def _cand(d, m):
    rng = np.random.default_rng(d + 13 * m)
    cand = np.stack([rng.permutation(RS_N)[:m] if m <= RS_N else rng.integers(0, RS_N, m) for _ in range(5)]).astype(np.int64)
    cand[0, 0] = -1                                                                # padding
    if m >= 3:
        cand[1, m // 2] = RS_N                                                     # beyond the corpus: the status bit
        cand[2, m - 1] = cand[2, 0]                                                # a row listed twice
        cand[3, :2] = (11, 7)                                                      # equal code rows: the lower row first
    return cand


@pytest.mark.parametrize("d", (65, 384, 768, 1000, 1024))
@pytest.mark.parametrize("m,k", ((1, 1), (100, 10), (100, 65), (1025, 10), (2500, 65), (2500, 1)))
def test_sign_rescore_topk(d, m, k):
    q, cc = _rescore_rows(d)
    cand = _cand(d, m)
    ws, wi, wst = hc.rescore_ref(q, cc, d, cand, k, idx_offset=5)
    gs, gi, gst = ops.sign_rescore_topk(_dev(q), _dev(cc), d, _dev(cand), k, idx_offset=5, return_status=True)
    assert np.array_equal(gs.cpu().numpy().view(np.uint32), ws.view(np.uint32))
    assert np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(gst.cpu().numpy(), wst * _lib.LIST_ST_ROW)
    if m >= 3:
        assert wst.tolist() == [0, 1, 0, 0, 0]
    if d <= 768:   # the same bits as the float32 list search over the unpacked +-1 matrix
        signs = (2.0 * hc.bits_of(cc, d).astype(np.float32) - 1.0)
        ls, li, lst = ops.dot_list_topk(_dev(q), _dev(signs), _dev(cand), k=k, idx_offset=5, return_status=True, assume_unique=True)
        assert torch.equal(ls.view(torch.int32), gs.view(torch.int32)) and torch.equal(li, gi) and torch.equal(lst, gst)


def test_sign_rescore_after_hamming_topk():
    """the out_idx of hamming_topk — padding included — passes straight into the re-score"""
    d, N, Q = 65, 9, 33
    rng = np.random.default_rng(9)
    q, c = hc.random_rows(rng, Q, d), hc.random_rows(rng, N, d)
    cc = hc.pack_ref(c)
    _, idx = ops.hamming_topk(ops.pack_sign_rows(_dev(q)), _dev(cc), d, 64)
    gs, gi = ops.sign_rescore_topk(_dev(q), _dev(cc), d, idx, 10)
    ws, wi, _ = hc.rescore_ref(q, cc, d, idx.cpu().numpy(), 10)
    assert np.array_equal(gs.cpu().numpy().view(np.uint32), ws.view(np.uint32)) and np.array_equal(gi.cpu().numpy(), wi)
    assert (wi[:, 9:] == -1).all() and (wi[:, :9] >= 0).all()


# ------------------------------------------------------------------------------------------------- index
def test_binary_index_matches_the_ops(tmp_path):
    from text_similarity_amd.binary_index import GpuBinaryIndex
    d = 1000
    rng = np.random.default_rng(21)
    a, b, q = hc.random_rows(rng, 700, d), hc.random_rows(rng, 900, d), hc.random_rows(rng, 5, d)
    la, lb = np.arange(700) * 3 + 10_000, np.arange(900) * 7 + 50_000
    index = GpuBinaryIndex(d, device=DEV)
    assert index.get_current_count() == 0
    index.add_items(a, la)                                                         # floats, packed on the device
    index.add_items(np.packbits(b > 0, axis=1), lb)                                # packbits codes
    assert index.get_current_count() == 1600
    labels = np.concatenate([la, lb])
    cc = _dev(hc.pack_ref(np.concatenate([a, b])))
    qc = ops.pack_sign_rows(_dev(q))
    wd, wi = ops.hamming_topk(qc, cc, d, 10)
    gd, gl = index.search(q, 10)
    assert torch.equal(gd, wd) and np.array_equal(gl.cpu().numpy(), labels[wi.cpu().numpy()])
    gd2, gl2 = index.search(np.packbits(q > 0, axis=1), 10)                        # uint8 queries
    assert torch.equal(gd2, gd) and torch.equal(gl2, gl)
    _, cand = ops.hamming_topk(qc, cc, d, 40)
    ws, wi = ops.sign_rescore_topk(_dev(q), cc, d, cand, 10)
    gs, gl = index.search(q, 10, rescore_multiplier=4)
    assert torch.equal(gs, ws) and np.array_equal(gl.cpu().numpy(), labels[wi.cpu().numpy()])
    nl, nd = index.knn_query(q, 10)
    assert np.array_equal(nl, index.search(q, 10)[1].cpu().numpy()) and np.array_equal(nd, gd.cpu().numpy())
    # k > count pads; Q = 0
    gd, gl = index.search(q, 1024)
    assert (gd[:, 1600:] == hc.INT32_MAX).all() and (gl[:, 1600:] == -1).all() and (gl[:, :1600] >= 0).all()
    gs, gl = index.search(q, 1024, rescore_multiplier=2)
    assert torch.isinf(gs[:, 1024:]).all() if gs.shape[1] > 1024 else True
    assert (gl[:, :1024] >= 0).all()
    gd, gl = index.search(np.zeros((0, d), np.float32), 3)
    assert tuple(gd.shape) == (0, 3) and tuple(gl.shape) == (0, 3)
    empty = GpuBinaryIndex(d, device=DEV)
    gd, gl = empty.search(q, 3)
    assert (gd == hc.INT32_MAX).all() and (gl == -1).all()
    gs, gl = empty.search(q, 3, rescore_multiplier=2)
    assert torch.isinf(gs).all() and (gl == -1).all()
    # save / load
    path = str(tmp_path / "bin.npz")
    index.save_index(path)
    again = GpuBinaryIndex(d, device=DEV)
    again.load_index(path)
    assert again.get_current_count() == 1600
    for mult in (None, 4):
        x, y = index.search(q, 10, rescore_multiplier=mult), again.search(q, 10, rescore_multiplier=mult)
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    with pytest.raises(ValueError):
        GpuBinaryIndex(384, device=DEV).load_index(path)
    with pytest.raises(ValueError):
        GpuBinaryIndex(1025)


def test_encode_text_ubinary():
    transformers = pytest.importorskip("transformers")
    from text_similarity_amd import presets
    from text_similarity_amd.configurations.config import Configuration, ModelParameters
    from text_similarity_amd.models.sentence_encoder import SentenceTransformerWrapper
    preset = "tiny-bert"
    cfg = presets.PRESETS[preset]
    tok = transformers.BertTokenizer(vocab=presets.synthetic_vocab(cfg.vocab), do_lower_case=True)
    params = Configuration(model_parameters=ModelParameters(preset, hidden_size=cfg.hidden), model=preset, save_path="", tokenizer=tok,
                           device=torch.device(DEV), max_tokens_per_batch=1024, max_seqs_per_batch=64, sequence_max_len=48)
    model = SentenceTransformerWrapper.from_preset(preset, params, parallel_mode=False)
    sents = presets.synthetic_sentences(21, seed="ubinary", vocab_size=cfg.vocab)
    f32 = model.encode_text(sents, output_np=True)
    codes = model.encode_text(sents, output_np=True, precision="ubinary")
    assert f32.shape == (21, cfg.hidden) and codes.dtype == np.uint8 and codes.shape == (21, (cfg.hidden + 7) // 8)
    assert np.array_equal(codes, np.packbits(f32 > 0, axis=1))
    dev_codes = model.encode_text(sents, precision="ubinary")
    assert dev_codes.is_cuda and np.array_equal(dev_codes.cpu().numpy(), codes)
    with pytest.raises(ValueError):
        model.encode_text(sents, precision="int8")
