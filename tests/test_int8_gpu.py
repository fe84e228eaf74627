"""int8 embeddings on the GPU (ops.quantize_int8_rows / int8_ip_topk / int8_rescore_topk, GpuInt8Index, encode_text(precision=
"int8")): every result is compared for equality with the numpy restatement of tests/int8_cases.py.  No tolerance anywhere.

Shapes are the smallest at which each kernel can go wrong: widths around the 16-byte word and the 64-byte k-step of the MFMA
tile, row counts around one block of the running list (1 024) and more than one chunk (70 000), k around 64 (the list length and
the queries per workgroup change: 16 -> 8) and at 1 024, more queries than one group (17, 33 > 16)."""
import functools

import numpy as np
import pytest
import torch

import int8_cases as ic
from text_similarity_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _eq(t, a):
    return np.array_equal(t.cpu().numpy(), a)


# ------------------------------------------------------------------------------------------------- the quantiser
@pytest.mark.parametrize("d", (1, 15, 16, 17, 64, 65, 384, 1000, 1024))
@pytest.mark.parametrize("rows", (3, 257))
def test_quantize_int8_rows(d, rows):
    x, ranges = ic.quantiser_rows(rows, d, seed=1000 * rows + d)
    want = ic.quantize_ref(x, ranges)
    cb = ic.int8_bytes(d)
    got = ops.quantize_int8_rows(_dev(x), _dev(ranges))
    assert got.dtype == torch.int8 and tuple(got.shape) == (rows, cb)
    g = got.cpu().numpy()
    bad = np.argwhere(g != want)
    assert bad.size == 0, (bad[:5], [(x[r, c], ranges[:, c], g[r, c], want[r, c]) for r, c in bad[:5] if c < d])
    assert (g[:, d:] == 0).all()
    wide = np.full((rows, d + 5), np.float32(1.0))                                         # ld_in = d + 5
    wide[:, :d] = x
    assert _eq(ops.quantize_int8_rows(_dev(wide)[:, :d], _dev(ranges)), want)
    out = torch.full((rows, cb + 16), 0xA5 - 256, dtype=torch.int8, device=DEV)            # ld_code = stride + 16
    ops.quantize_int8_rows(_dev(x), _dev(ranges), out=out[:, :cb])
    o = out.cpu().numpy()
    assert np.array_equal(o[:, :cb], want) and (o[:, cb:].view(np.uint8) == 0xA5).all()
    assert _eq(ops.int8_ranges(_dev(np.nan_to_num(x, nan=0.0, posinf=9.0, neginf=-9.0))),
               ic.ranges_of(np.nan_to_num(x, nan=0.0, posinf=9.0, neginf=-9.0)))
    assert _eq(ops.int8_codes_from_numpy(want[:, :d], d, device=DEV), want)


# ------------------------------------------------------------------------------------------------- the MFMA operand and C/D maps
@functools.lru_cache(maxsize=None)
def _layout_codes(d):
    Q, N = 33, 1000
    c = np.zeros((N, d), np.int64)
    for r in range(N):
        c[r, (7 * r + 3) % d] += (r % 127) + 1
        c[r, (11 * r) % d] += -((r % 5) + 1)
    q = np.zeros((Q, d), np.int64)
    for i in range(Q):
        q[i, (13 * i) % d] += i + 1
        q[i, (5 * i + 1) % d] += -(i + 2)
    assert np.abs(c).max() <= 127 and np.abs(q).max() <= 127
    return ic.pad_codes(q.astype(np.int8)), ic.pad_codes(c.astype(np.int8))


@pytest.mark.parametrize("d", (64, 128, 1024))
def test_int8_ip_layout(d):
    """k = N: the call returns the whole score matrix of asymmetric one-hot rows — a row/column swap, a wrong k slice or a
    dropped k-step cannot pass"""
    qc, cc = _layout_codes(d)
    ws, wi = ic.ip_topk_ref(qc, cc, d, 1000)
    assert len(np.unique(ic.ip_ref(qc, cc, d))) > 20
    gs, gi = ops.int8_ip_topk(_dev(qc), _dev(cc), d, 1000)
    assert _eq(gs, ws) and _eq(gi, wi)


# ------------------------------------------------------------------------------------------------- top-k parity
#        d     N      Q   k
CASES = ((1, 5, 1, 10),            # N < k: padding
         (16, 1000, 1, 1),
         (63, 1025, 17, 10),
         (65, 1025, 33, 10),
         (384, 70000, 3, 10),      # several chunks
         (384, 5000, 16, 64),
         (1000, 3000, 5, 65),      # the 8-query group form
         (1024, 2049, 9, 1024))
KINDS = ("uniform", "ternary")


@functools.lru_cache(maxsize=None)
def _codes(kind, d, N, Q):
    rng = np.random.default_rng(d * 1_000_003 + N * 101 + Q + (7 if kind == "ternary" else 0))
    make = ic.uniform_codes if kind == "uniform" else ic.ternary_codes
    q, c = make(rng, Q, d), make(rng, N, d)
    for r in (0, 1023, 1024, N - 1):          # one row copied across the block and chunk boundaries: tied scores, row order decides
        if 0 <= r < N:
            c[r] = c[0]
    return q, c


@functools.lru_cache(maxsize=None)
def _topk_want(kind, d, N, Q, k):
    qc, cc = _codes(kind, d, N, Q)
    return ic.ip_topk_ref(qc, cc, d, k)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("d,N,Q,k", CASES)
def test_int8_ip_topk(kind, d, N, Q, k):
    qc, cc = _codes(kind, d, N, Q)
    ws, wi = _topk_want(kind, d, N, Q, k)
    gs, gi = ops.int8_ip_topk(_dev(qc), _dev(cc), d, k)
    assert gs.dtype == torch.int32 and gi.dtype == torch.int64
    assert _eq(gs, ws) and _eq(gi, wi)


def test_int8_ip_topk_extremes():
    """d = 1024: all -128 against all -128 is 2^24, against all 127 the minimum; mixed with random rows the order is exact"""
    d, N = 1024, 1500
    rng = np.random.default_rng(4)
    cc = ic.uniform_codes(rng, N, d)
    cc[7], cc[1030], cc[1499] = -128, -128, -128
    cc[3], cc[1024] = 127, 127
    qc = ic.uniform_codes(rng, 3, d)
    qc[0], qc[1] = -128, 127
    ws, wi = ic.ip_topk_ref(qc, cc, d, N)
    assert ws[0, :3].tolist() == [2 ** 24] * 3 and wi[0, :3].tolist() == [7, 1030, 1499]
    assert ws[0, -2:].tolist() == [-128 * 127 * 1024] * 2 and wi[0, -2:].tolist() == [3, 1024]
    assert ws[1, :2].tolist() == [127 * 127 * 1024] * 2
    for k in (N, 10):
        gs, gi = ops.int8_ip_topk(_dev(qc), _dev(cc), d, min(k, 1024))
        assert _eq(gs, ws[:, :min(k, 1024)]) and _eq(gi, wi[:, :min(k, 1024)])
    # the minimum itself as a best score: a corpus of all-127 rows only
    only = ic.pad_codes(np.full((20, d), 127, np.int8))
    gs, gi = ops.int8_ip_topk(_dev(qc[:1]), _dev(only), d, 5)
    assert gs.cpu().numpy().tolist() == [[-128 * 127 * 1024] * 5] and gi.cpu().numpy().tolist() == [[0, 1, 2, 3, 4]]


@pytest.mark.parametrize("d", (65, 1000))
def test_int8_ip_topk_ignores_bytes_beyond_d(d):
    N, Q, k = 1025, 33, 10
    qc, cc = _codes("uniform", d, N, Q)
    ws, wi = _topk_want("uniform", d, N, Q, k)
    rng = np.random.default_rng(3)
    jq, jc = qc.copy(), cc.copy()
    for a in (jq, jc):
        a[:, d:] = rng.integers(-128, 128, size=(a.shape[0], a.shape[1] - d)).astype(np.int8)
    assert not np.array_equal(jc, cc) and not np.array_equal(jq, qc)
    gs, gi = ops.int8_ip_topk(_dev(jq), _dev(jc), d, k)
    assert _eq(gs, ws) and _eq(gi, wi)


@pytest.mark.parametrize("d,N,Q,k", ((384, 70000, 3, 10), (65, 1025, 33, 10)))
def test_int8_ip_topk_strided_rows_and_offset(d, N, Q, k):
    """ldc = int8_bytes + 16 (a view into wider rows whose extra bytes hold junk), idx_offset = 10**9, preallocated outputs"""
    qc, cc = _codes("uniform", d, N, Q)
    ws, wi = _topk_want("uniform", d, N, Q, k)
    cb = ic.int8_bytes(d)
    wide = np.full((N, cb + 16), 0xA5 - 256, np.int8)
    wide[:, :cb] = cc
    out = (torch.empty((Q, k), dtype=torch.int32, device=DEV), torch.empty((Q, k), dtype=torch.int64, device=DEV))
    gs, gi = ops.int8_ip_topk(_dev(qc), _dev(wide)[:, :cb], d, k, idx_offset=10 ** 9, out=out)
    assert gs is out[0] and gi is out[1]
    assert _eq(gs, ws) and _eq(gi, np.where(wi >= 0, wi + 10 ** 9, -1))


@pytest.mark.parametrize("d,N,k", ((65, 1025, 10), (384, 1023, 64), (1024, 1025, 65)))
def test_int8_ip_topk_groups_do_not_leak(d, N, k):
    """the result for 19 queries is the 19 single-query results stacked"""
    qc, cc = _codes("ternary", d, N, 19)
    q_d, c_d = _dev(qc), _dev(cc)
    gs, gi = ops.int8_ip_topk(q_d, c_d, d, k)
    one = [ops.int8_ip_topk(q_d[i:i + 1], c_d, d, k) for i in range(19)]
    assert torch.equal(gs, torch.cat([o[0] for o in one])) and torch.equal(gi, torch.cat([o[1] for o in one]))
    ws, wi = ic.ip_topk_ref(qc, cc, d, k)
    assert _eq(gs, ws) and _eq(gi, wi)


@pytest.mark.parametrize("Q", (1, 5))
def test_int8_ip_topk_every_row_improves(Q):
    """The in-between flush of a 512-entry block.  Row r scores exactly r - 1024 against the all-ones query, so every row beats
    all before it and no bound spares an offer: one query (one group, two chunks of 1 024 rows, four steps each) has 512 > 512 -
    256 entries in its block after a chunk's third step, which is neither its first nor its last.  Q = 5: groups of 2, 2, 1."""
    d, N, k = 16, 2048, 10
    r = np.arange(N)
    cc = np.repeat((r // 16 - 64)[:, None], d, axis=1)
    cc += np.arange(d)[None, :] < (r % 16)[:, None]
    assert cc.min() == -64 and cc.max() == 64
    cc, qc = ic.pad_codes(cc.astype(np.int8)), ic.pad_codes(np.ones((Q, d), np.int8))
    ws, wi = ic.ip_topk_ref(qc, cc, d, k)
    assert wi.tolist() == [list(range(N - 1, N - 1 - k, -1))] * Q and ws.tolist() == [list(range(1023, 1023 - k, -1))] * Q
    gs, gi = ops.int8_ip_topk(_dev(qc), _dev(cc), d, k)
    assert _eq(gs, ws) and _eq(gi, wi)


def test_int8_ip_topk_query_slices(monkeypatch):
    """more queries than one call takes: slices of 5, 5 and 2 strided query rows, each written to its own rows of the outputs"""
    monkeypatch.setattr(ops, "MAX_QUERIES_PER_CALL", 5)
    d, N, Q, k = 65, 300, 12, 3
    qc, cc = _codes("uniform", d, N, Q)
    cb = ic.int8_bytes(d)
    wide = np.full((Q, cb + 16), 0xA5 - 256, np.int8)
    wide[:, :cb] = qc
    ws, wi = ic.ip_topk_ref(qc, cc, d, k)
    assert len({tuple(row) for row in wi.tolist()}) > 1
    gs, gi = ops.int8_ip_topk(_dev(wide)[:, :cb], _dev(cc), d, k)
    assert _eq(gs, ws) and _eq(gi, wi)


def test_int8_ip_topk_empty_sides():
    qc, cc = _codes("uniform", 65, 9, 5)
    gs, gi = ops.int8_ip_topk(_dev(qc), _dev(cc)[:0], 65, 5)                      # N = 0: all padding
    assert (gs.cpu().numpy() == ic.INT32_MIN).all() and (gi.cpu().numpy() == -1).all()
    gs, gi = ops.int8_ip_topk(_dev(qc), _dev(cc), 65, 12)                         # N < k: a padded tail
    ws, wi = ic.ip_topk_ref(qc, cc, 65, 12)
    assert _eq(gs, ws) and _eq(gi, wi) and (wi[:, 9:] == -1).all() and (ws[:, 9:] == ic.INT32_MIN).all()
    gs, gi = ops.int8_ip_topk(_dev(qc)[:0], _dev(cc), 65, 5)                      # Q = 0
    assert tuple(gs.shape) == (0, 5) and tuple(gi.shape) == (0, 5)
    with pytest.raises(ValueError):
        ops.int8_ip_topk(_dev(qc), _dev(cc), 65, 1025)
    with pytest.raises(ValueError):
        ops.int8_ip_topk(_dev(qc)[:, :64], _dev(cc), 65, 5)
    with pytest.raises(ValueError):
        ops.int8_ip_topk(_dev(qc).view(torch.uint8), _dev(cc), 65, 5)


# ------------------------------------------------------------------------------------------------- re-score
RS_N = 3000


@functools.lru_cache(maxsize=None)
def _rescore_rows(d):
    rng = np.random.default_rng(77 + d)
    q, c = ic.random_rows(rng, 5, d), ic.uniform_codes(rng, RS_N, d)
    c[11] = c[7]                                                                   # two equal code rows
    return q, c


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
def test_int8_rescore_topk(d, m, k):
    q, cc = _rescore_rows(d)
    cand = _cand(d, m)
    ws, wi, wst = ic.rescore_ref(q, cc, d, cand, k, idx_offset=5)
    gs, gi, gst = ops.int8_rescore_topk(_dev(q), _dev(cc), d, _dev(cand), k, idx_offset=5, return_status=True)
    assert np.array_equal(gs.cpu().numpy().view(np.uint32), ws.view(np.uint32))
    assert _eq(gi, wi) and _eq(gst, wst * _lib.LIST_ST_ROW)
    if m >= 3:
        assert wst.tolist() == [0, 1, 0, 0, 0]
    if d <= 768:   # the same bits as the float32 list search over the codes as a float32 matrix
        vals = _dev(cc)[:, :d].float().contiguous()
        ls, li, lst = ops.dot_list_topk(_dev(q), vals, _dev(cand), k=k, idx_offset=5, return_status=True, assume_unique=True)
        assert torch.equal(ls.view(torch.int32), gs.view(torch.int32)) and torch.equal(li, gi) and torch.equal(lst, gst)


def test_int8_rescore_after_ip_topk():
    """random float data: quantise, search the codes (padding included in idx), re-score with the float queries"""
    d, N, Q = 65, 9, 33
    rng = np.random.default_rng(9)
    q, c = ic.random_rows(rng, Q, d), ic.random_rows(rng, N, d)
    ranges = ic.ranges_of(c)
    cc = ic.quantize_ref(c, ranges)
    c_d = ops.quantize_int8_rows(_dev(c), _dev(ranges))
    q_d = ops.quantize_int8_rows(_dev(q), _dev(ranges))
    assert _eq(c_d, cc) and _eq(q_d, ic.quantize_ref(q, ranges))
    _, idx = ops.int8_ip_topk(q_d, c_d, d, 64)
    assert _eq(idx, ic.ip_topk_ref(ic.quantize_ref(q, ranges), cc, d, 64)[1])
    gs, gi = ops.int8_rescore_topk(_dev(q), c_d, d, idx, 10)
    ws, wi, _ = ic.rescore_ref(q, cc, d, idx.cpu().numpy(), 10)
    assert np.array_equal(gs.cpu().numpy().view(np.uint32), ws.view(np.uint32)) and _eq(gi, wi)
    assert (wi[:, 9:] == -1).all() and (wi[:, :9] >= 0).all()


# ------------------------------------------------------------------------------------------------- index
def test_int8_index_matches_the_ops(tmp_path):
    from text_similarity_amd.int8_index import GpuInt8Index
    d = 1000
    rng = np.random.default_rng(21)
    a, b, q = ic.random_rows(rng, 700, d), ic.random_rows(rng, 900, d), ic.random_rows(rng, 5, d)
    la, lb = np.arange(700) * 3 + 10_000, np.arange(900) * 7 + 50_000
    index = GpuInt8Index(d, device=DEV)
    assert index.get_current_count() == 0 and index.ranges is None
    with pytest.raises(ValueError):
        index.search(q, 3)                                                         # float queries, no ranges yet
    index.add_items(a, la)                                                         # floats: calibrates, then quantises
    ranges = ic.ranges_of(a)
    assert _eq(index.ranges, ranges)
    index.add_items(ic.quantize_ref(b, ranges)[:, :d], lb)                         # int8 codes; 1 600 > the first reservation
    assert index.get_current_count() == 1600 and _eq(index.ranges, ranges)
    labels = np.concatenate([la, lb])
    cc = _dev(ic.quantize_ref(np.concatenate([a, b]), ranges))
    qc = ops.quantize_int8_rows(_dev(q), _dev(ranges))
    ws, wi = ops.int8_ip_topk(qc, cc, d, 10)
    gs, gl = index.search(q, 10)
    assert gs.dtype == torch.int32 and torch.equal(gs, ws) and np.array_equal(gl.cpu().numpy(), labels[wi.cpu().numpy()])
    gs2, gl2 = index.search(ic.quantize_ref(q, ranges)[:, :d], 10)                 # int8 queries
    assert torch.equal(gs2, gs) and torch.equal(gl2, gl)
    _, cand = ops.int8_ip_topk(qc, cc, d, 40)
    ws, wi = ops.int8_rescore_topk(_dev(q), cc, d, cand, 10)
    gf, gl = index.search(q, 10, rescore_multiplier=4)
    assert gf.dtype == torch.float32 and torch.equal(gf, ws) and np.array_equal(gl.cpu().numpy(), labels[wi.cpu().numpy()])
    with pytest.raises(ValueError):
        index.search(ic.quantize_ref(q, ranges)[:, :d], 10, rescore_multiplier=4)
    nl, nd = index.knn_query(q, 10)
    assert np.array_equal(nl, index.search(q, 10)[1].cpu().numpy()) and np.array_equal(nd, gs.cpu().numpy())
    # k > count pads; Q = 0
    gs, gl = index.search(q, 1024)
    assert (gs[:, :1600] > ic.INT32_MIN).all() and (gl[:, :1024] >= 0).all()
    small = GpuInt8Index(d, ranges=ranges, device=DEV)
    small.add_items(a[:7])
    gs, gl = small.search(q, 9)
    assert (gs[:, 7:] == ic.INT32_MIN).all() and (gl[:, 7:] == -1).all() and (gl[:, :7] >= 0).all()
    gf, gl = small.search(q, 9, rescore_multiplier=2)
    assert torch.isinf(gf[:, 7:]).all() and (gl[:, 7:] == -1).all() and (gl[:, :7] >= 0).all()
    gs, gl = index.search(np.zeros((0, d), np.float32), 3)
    assert tuple(gs.shape) == (0, 3) and tuple(gl.shape) == (0, 3)
    empty = GpuInt8Index(d, ranges=ranges, device=DEV)
    gs, gl = empty.search(q, 3)
    assert (gs == ic.INT32_MIN).all() and (gl == -1).all()
    gf, gl = empty.search(q, 3, rescore_multiplier=2)
    assert torch.isinf(gf).all() and (gl == -1).all()
    # save / load
    path = str(tmp_path / "i8.npz")
    index.save_index(path)
    again = GpuInt8Index(d, device=DEV)
    again.load_index(path)
    assert again.get_current_count() == 1600 and torch.equal(again.ranges, index.ranges)
    for mult in (None, 4):
        x, y = index.search(q, 10, rescore_multiplier=mult), again.search(q, 10, rescore_multiplier=mult)
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1])
    with pytest.raises(ValueError):
        GpuInt8Index(384, device=DEV).load_index(path)
    with pytest.raises(ValueError):
        GpuInt8Index(1025)


def test_encode_text_int8():
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
    sents = presets.synthetic_sentences(21, seed="int8", vocab_size=cfg.vocab)
    f32 = model.encode_text(sents, output_np=True)
    ranges = ic.ranges_of(f32[:12])                                               # calibrated on a part: the rest saturates
    codes = model.encode_text(sents, output_np=True, precision="int8", ranges=ranges)
    assert f32.shape == (21, cfg.hidden) and codes.dtype == np.int8 and codes.shape == (21, cfg.hidden)
    assert np.array_equal(codes, ic.quantize_ref(f32, ranges)[:, :cfg.hidden])
    dev_codes = model.encode_text(sents, precision="int8", ranges=_dev(ranges))
    assert dev_codes.is_cuda and dev_codes.dtype == torch.int8 and np.array_equal(dev_codes.cpu().numpy(), codes)
    with pytest.raises(ValueError, match="ranges"):
        model.encode_text(sents, precision="int8")
    with pytest.raises(ValueError):
        model.encode_text(sents, precision="int8", ranges=ranges, output_value="token_embeddings")
