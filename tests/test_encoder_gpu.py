"""GPU parity of the encoder half of the hot path.  The encoder computes in bf16 (MFMA, fp32 accumulate;
LayerNorm / softmax / GELU in fp32) as BASELINE.json's north_star prescribes, so it is compared with the fp32
reference goldens and the fp32 oracle under a stated tolerance:

    max |err| <= 8e-2 on LayerNorm-scale hidden states (|x| up to ~4) and <= 5e-2 on pooled rows,
    cosine(native row, reference row) >= 0.9995   (measured: 0.012-0.036 and >= 0.99996).

bf16 has 8 significand bits (rel. 2^-9 per rounding); a 12-layer encoder rounds the residual stream 25 times and the
attention probabilities once per layer.  The row cosine is the figure that matters to similarity search."""
import numpy as np
import pytest
import torch

from conftest import golden
from oracle import encoder_ref
from text_similarity_amd import presets
from text_similarity_amd.native_encoder import NativeEncoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HID_TOL, POOL_TOL, COS_MIN = 8e-2, 5e-2, 0.9995


def _cos_rows(a, b):
    num = (a * b).sum(1)
    return num / np.maximum(np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1), 1e-30)


@pytest.mark.parametrize("preset", ["tiny-bert", "tiny-mpnet"])
def test_tiny_encoder_hidden_and_pooled(preset):
    g = golden(f"encoder_{preset}.npz")
    enc = NativeEncoder.from_preset(preset, max_tokens=1024, max_seqs=64)
    ids = torch.from_numpy(g["input_ids"]).to(DEV)
    mask = torch.from_numpy(g["attention_mask"]).to(DEV)
    hidden = enc(input_ids=ids, attention_mask=mask)[0]
    torch.cuda.synchronize()
    h = hidden.cpu().numpy()
    m = g["attention_mask"].astype(bool)
    err = np.abs(h[m] - g["last_hidden_state"][m]).max()
    assert err <= HID_TOL, err
    assert (h[~m] == 0).all()
    # pooled through the reference-named modules
    from text_similarity_amd.configurations.config import Configuration, ModelParameters
    from text_similarity_amd.dataset.dataset import EmbeddingsFeatures
    from text_similarity_amd.models.sentence_encoder import OnnxSentenceTransformerWrapper
    from text_similarity_amd.modules.modules import AvgPoolingStrategy
    params = Configuration(model_parameters=ModelParameters(preset), model=preset, save_path="", device=torch.device(DEV))
    wrap = OnnxSentenceTransformerWrapper(params=params, context_embedder=enc)
    pooled = wrap.forward(ids, mask)
    pooled2 = AvgPoolingStrategy(params).forward(hidden, EmbeddingsFeatures(ids, mask))
    assert torch.equal(pooled, pooled2)
    p = pooled.cpu().numpy()
    assert np.abs(p - g["pooled"]).max() <= POOL_TOL
    assert (p[3] == 0).all()                      # all-zero mask row
    live = g["attention_mask"].sum(1) > 0
    assert _cos_rows(p[live], g["pooled"][live]).min() >= COS_MIN
    # the same numbers against the oracle (fp32 restatement) — proves oracle and fixture agree on this input
    w = presets.synthetic_weights(preset)
    ref = encoder_ref.encode(presets.PRESETS[preset], w, g["input_ids"], g["attention_mask"]).numpy()
    assert np.abs(p - ref).max() <= POOL_TOL


@pytest.mark.parametrize("preset", ["all-MiniLM-L6-v2", "all-mpnet-base-v2", "bert-base-uncased"])
def test_preset_encoder_pooled_rows(preset):
    g = golden(f"encoder_{preset}.npz")
    enc = NativeEncoder.from_preset(preset, max_tokens=4096, max_seqs=64)
    flat = torch.from_numpy(g["flat_ids"]).to(DEV)
    cu = torch.from_numpy(g["cu_seqlens"].astype(np.int32)).to(DEV)
    r = enc.forward_packed(flat, cu, pooled=True, unit=True)
    torch.cuda.synchronize()
    p = r["pooled"].cpu().numpy()
    err = np.abs(p - g["pooled"]).max()
    cos = _cos_rows(p, g["pooled"]).min()
    print(f"{preset}: max|err|={err:.4f} min cos={cos:.6f}")
    assert err <= POOL_TOL and cos >= COS_MIN
    # fused unit rows == tsim_l2norm_rows(pooled) == oracle canonical normalisation, bit for bit
    from oracle import search_ref
    from text_similarity_amd import ops
    assert torch.equal(r["unit"], ops.l2norm_rows(r["pooled"]))
    np.testing.assert_array_equal(r["unit"][:, :enc.cfg.hidden].float().cpu().numpy(),
                                  search_ref.unit_rows(p))
    assert (r["unit"][:, enc.cfg.hidden:] == 0).all()


def test_batch_composition_invariance():
    """Packed rows are independent: encoding a sentence alone or inside any batch gives identical bits."""
    preset = "all-MiniLM-L6-v2"
    g = golden(f"encoder_{preset}.npz")
    enc = NativeEncoder.from_preset(preset, max_tokens=4096, max_seqs=64)
    flat, cu = g["flat_ids"], g["cu_seqlens"].astype(np.int64)
    full = enc.forward_packed(torch.from_numpy(flat).to(DEV), torch.from_numpy(cu.astype(np.int32)).to(DEV))["pooled"]
    for r in (0, 13, 31):
        one = enc.forward_packed(torch.from_numpy(flat[cu[r]:cu[r + 1]]).to(DEV),
                                 torch.tensor([0, cu[r + 1] - cu[r]], dtype=torch.int32, device=DEV))["pooled"]
        assert torch.equal(one[0], full[r])


def test_empty_and_degenerate_inputs():
    enc = NativeEncoder.from_preset("tiny-bert", max_tokens=256, max_seqs=16)
    # a batch containing an empty sequence
    flat = torch.tensor([5, 6, 7], dtype=torch.int32, device=DEV)
    cu = torch.tensor([0, 0, 3, 3], dtype=torch.int32, device=DEV)
    p = enc.forward_packed(flat, cu)["pooled"]
    assert (p[0] == 0).all() and (p[2] == 0).all() and p[1].abs().sum() > 0
    # a batch of ONLY empty sequences (no tokens at all): zero rows, no error
    p0 = enc.forward_packed(torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV),
                            pooled=True, unit=True)
    assert p0["pooled"].shape == (3, enc.cfg.hidden) and (p0["pooled"] == 0).all() and (p0["unit"] == 0).all()
    with pytest.raises(ValueError):
        enc.forward_packed(torch.zeros(300, dtype=torch.int32, device=DEV),
                           torch.tensor([0, 300], dtype=torch.int32, device=DEV))


def test_e2e_config1_encode_text_and_mining_pipeline():
    """BASELINE.json configs[0] shape: 1k synthetic sentences, MiniLM preset, encode + top-10, through the
    reference-named API (Configuration -> SentenceTransformerWrapper.encode_text -> SentenceMiningPipeline)."""
    from transformers import BertTokenizer
    from text_similarity_amd.configurations.config import Configuration, ModelParameters
    from text_similarity_amd.models.sentence_encoder import SentenceTransformerWrapper
    from text_similarity_amd.pipeline.search_pipeline import SentenceMiningPipeline
    g = golden("e2e_config1.npz")
    preset = "all-MiniLM-L6-v2"
    tok = BertTokenizer(vocab=presets.synthetic_vocab(30522), do_lower_case=True)
    params = Configuration(model_parameters=ModelParameters(preset, hidden_size=384), model=preset, save_path="",
                           tokenizer=tok, device=torch.device(DEV), batch_size=16, max_tokens_per_batch=8192,
                           max_seqs_per_batch=512)
    model = SentenceTransformerWrapper.from_preset(preset, params, parallel_mode=False)
    sents = presets.synthetic_sentences(1000, seed="sent1234", vocab_size=30522)
    assert sents[:4] == [str(s) for s in g["first_sentences"]]
    emb = model.encode_text(sents)
    assert emb.shape == (1000, 384) and emb.dtype == torch.float32 and emb.is_cuda
    e = emb.cpu().numpy()
    err = np.abs(e - g["embeddings"]).max()
    cos = _cos_rows(e, g["embeddings"]).min()
    print(f"e2e encode: max|err|={err:.4f} min cos={cos:.6f}")
    assert err <= POOL_TOL and cos >= COS_MIN
    assert model.encode_text(sents[:3], output_np=True).shape == (3, 384)
    assert model.get_sentence_embedding_dimension() == 384
    # search: 100 queries against the 1000-sentence corpus in 3 chunks (exercises chunk merge)
    pipe = SentenceMiningPipeline(400, params, model, corpus=sents)
    res = pipe(sents[:100], 10)
    assert set(res.keys()) == set(range(100)) and all(len(v) == 10 for v in res.values())
    assert all(res[q][0][0] == q and res[q][0][1] == sents[q] for q in range(100))   # a sentence finds itself first
    # identical result when the corpus is passed pre-encoded in one chunk
    pipe1 = SentenceMiningPipeline(1000, params, model, corpus=emb)
    s1, i1 = pipe1.search_tensors(emb[:100], None, 10)
    assert torch.equal(i1, pipe.last_indices) and torch.equal(s1, pipe.last_scores)
    # the reference's own integration metric (eval_sentence_mining.py:11-34): top-k overlap with the fp32 reference
    from oracle import search_ref
    ref_idx = g["top10_indices"][:100]
    got = pipe.last_indices.cpu().numpy()
    overlap = np.mean([len(set(a) & set(b)) / 10 for a, b in zip(got.tolist(), ref_idx.tolist())])
    print(f"top-10 overlap with the fp32 reference: {overlap:.3f}")
    assert overlap >= 0.90
    # north_star's score tolerance, end to end through OUR bf16 encoder: the score returned for a (query, row) pair is
    # within 1e-3 of the reference's float32 cosine of ITS embeddings of the same two sentences
    qi = np.repeat(np.arange(100), 10)
    ref_pair = search_ref.exact_cosine_pairs(g["embeddings"], g["embeddings"], qi, got.reshape(-1)).reshape(100, 10)
    score_err = np.abs(pipe.last_scores.cpu().numpy() - ref_pair).max()
    print(f"max |score - reference cosine of the same pair| = {score_err:.2e}")
    assert score_err <= 1e-3
    # and exact agreement with the oracle search on OUR embeddings (same inputs -> same indices and scores, bit for bit)
    rv, ri = search_ref.mining_search(e[:100], e, 10, chunk=400)
    np.testing.assert_array_equal(got, ri)
    np.testing.assert_array_equal(pipe.last_scores.cpu().numpy(), rv)
    # searching the REFERENCE's float32 embeddings reproduces the reference's lists (BASELINE configs[0], all 1 000 queries)
    E = torch.from_numpy(g["embeddings"]).to(DEV)
    sr, ir = SentenceMiningPipeline(1000, params, model, corpus=E).search_tensors(E, None, 10)
    assert np.abs(sr.cpu().numpy() - g["top10_values"]).max() <= 1e-6
    same = (ir.cpu().numpy() == g["top10_indices"]).all(1)
    print(f"lists identical to the reference's: {same.sum()} / 1000")
    assert same.sum() >= 998


@pytest.mark.parametrize("preset", ["all-MiniLM-L6-v2", "all-mpnet-base-v2"])
def test_long_sequences_online_softmax_and_bias_buckets(preset):
    """Sequences of 1..max length (256 / 384 tokens): many key blocks per query block, so the online-softmax rescale and
    MPNet's log-spaced relative-position buckets (|distance| up to 383) are exercised; one sequence has a single huge
    score spike late in the sequence (a key identical to the query token far away), which forces a max jump at a late tile."""
    cfg = presets.PRESETS[preset]
    w = presets.synthetic_weights(preset)
    maxlen = 256 if cfg.arch == "bert" else 384
    lens = [1, 2, 31, 32, 33, 64, 65, 100, maxlen - 1, maxlen]
    ids = presets.randint(preset + "/long", sum(lens), 5, cfg.vocab).astype(np.int32)
    cu = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=cu[1:])
    ids[cu[-2] + 3] = ids[cu[-1] - 2]          # repeated token far apart in the longest sequence
    enc = NativeEncoder.from_preset(preset, max_tokens=int(cu[-1]), max_seqs=len(lens))
    r = enc.forward_packed(torch.from_numpy(ids).to(DEV), torch.from_numpy(cu.astype(np.int32)).to(DEV), pooled=True)
    torch.cuda.synchronize()
    p = r["pooled"].cpu().numpy()
    ref = encoder_ref.encode_packed(cfg, w, ids, cu, batch_size=4)
    err = np.abs(p - ref).max()
    cos = _cos_rows(p, ref).min()
    print(f"{preset} long: max|err|={err:.4f} min cos={cos:.6f}")
    assert err <= POOL_TOL and cos >= COS_MIN


def test_from_pretrained_local_directory(tmp_path):
    """sentence_encoder.py:187-217: weights come from a local HF directory (config.json + model.safetensors)."""
    from text_similarity_amd.configurations.config import Configuration, ModelParameters
    from text_similarity_amd.models.sentence_encoder import OnnxSentenceTransformerWrapper, SentenceTransformerWrapper
    from text_similarity_amd.weights import load_hf_dir, save_hf_dir
    preset = "tiny-mpnet"
    cfg = presets.PRESETS[preset]
    w = presets.synthetic_weights(preset)
    save_hf_dir(str(tmp_path), cfg, w)
    cfg2, w2 = load_hf_dir(str(tmp_path))
    assert cfg2 == cfg and set(w2) == set(w) and all(np.array_equal(w[k], w2[k]) for k in w)
    params = Configuration(model_parameters=ModelParameters(preset, hidden_size=64), model=preset, save_path="",
                           device=torch.device(DEV), max_tokens_per_batch=512, max_seqs_per_batch=32)
    g = golden(f"encoder_{preset}.npz")
    ids, mask = torch.from_numpy(g["input_ids"]).to(DEV), torch.from_numpy(g["attention_mask"]).to(DEV)
    for cls in (OnnxSentenceTransformerWrapper, SentenceTransformerWrapper):
        m = cls.from_pretrained(str(tmp_path), params=params)
        from text_similarity_amd.dataset.dataset import EmbeddingsFeatures
        out = m.encode(EmbeddingsFeatures(ids, mask))
        assert np.abs(out.cpu().numpy() - g["pooled"]).max() <= POOL_TOL


@pytest.mark.parametrize("preset,wdtype,n", [
    pytest.param("bert-base-uncased", "bf16", 1500, id="bert-base-uncased-bf16"),
    pytest.param("bert-base-uncased", "mxfp8", 1500, id="bert-base-uncased-mxfp8"),
    pytest.param("all-mpnet-base-v2", "bf16", 1500, id="all-mpnet-base-v2-bf16"),
    # MiniLM, hidden-384 LayerNorm GEMM dispatch: 2300 sentences (36 986 tokens) = ln_rows_gemm + ln_tail_gemm; 1500 (24 201
    # tokens) = the 128-token gemm_bf16_kernel form alone; 4700 (76 072 tokens) = one ln_rows_gemm round + the 64-token
    # remainder launch for 10 536 rows
    pytest.param("all-MiniLM-L6-v2", "bf16", 2300, id="all-MiniLM-L6-v2-bf16"),
    pytest.param("all-MiniLM-L6-v2", "bf16", 1500, id="all-MiniLM-L6-v2-bf16-1500"),
    pytest.param("all-MiniLM-L6-v2", "bf16", 4700, id="all-MiniLM-L6-v2-bf16-4700"),
])
def test_large_batch_equals_small_batches_bitwise(preset, wdtype, n):
    """~24 k tokens in one call: every projection launch has more output tiles than CUs, so the persistent workgroups of
    the ping-pong kernel walk several tiles each (next tile's first k-tile fetched during the epilogue, slot parity and
    source offsets carried across tiles) and the LayerNorm GEMMs take their main + tail launches.  Rows are independent
    and every kernel sums over k in the same order whatever the tile, so the result must equal — bit for bit — the same
    sentences encoded 48 at a time (one tile per workgroup, no tail)."""
    cfg = presets.PRESETS[preset]
    flat, cu = presets.synthetic_token_batch(n, seed="big/" + preset, vocab_size=cfg.vocab, max_len=64)
    cu = cu.astype(np.int64)
    enc = NativeEncoder.from_preset(preset, max_tokens=int(cu[-1]), max_seqs=n, weight_dtype=wdtype)
    big = enc.forward_packed(torch.from_numpy(flat).to(DEV), torch.from_numpy(cu.astype(np.int32)).to(DEV))["pooled"]
    torch.cuda.synchronize()
    assert torch.isfinite(big).all()
    for s in sorted({0, 480, 1452, n - 48}):     # n - 48: the last rows, which the LayerNorm GEMMs' tail launches compute
        rows = slice(s, s + 48)
        f = flat[cu[s]:cu[s + 48]]
        c = (cu[s:s + 49] - cu[s]).astype(np.int32)
        small = enc.forward_packed(torch.from_numpy(f).to(DEV), torch.from_numpy(c).to(DEV))["pooled"]
        assert torch.equal(small, big[rows]), f"{preset}/{wdtype}: rows {s}.. differ between batch sizes"


@pytest.mark.parametrize("preset", ["all-MiniLM-L6-v2", "bert-base-uncased"])
def test_repeated_forwards_are_bit_stable(preset):
    """The same batch 60 times through fresh launches: every result equals the first, bit for bit, and is finite.  (Round 3: an
    inline-asm 16-byte global store without the wait state the ISA wants before its data registers are overwritten corrupted one
    8-feature group in roughly every fourth forward on some boxes and never on others; a single forward per test let it
    through.)"""
    cfg = presets.PRESETS[preset]
    n = 2300 if cfg.hidden == 384 else 900
    flat, cu = presets.synthetic_token_batch(n, seed="big/" + preset, vocab_size=cfg.vocab, max_len=64)
    enc = NativeEncoder.from_preset(preset, max_tokens=int(cu[-1]), max_seqs=n)
    fd, cd = torch.from_numpy(flat).to(DEV), torch.from_numpy(cu.astype(np.int32)).to(DEV)
    first = enc.forward_packed(fd, cd, hidden=True)
    ref_p, ref_h = first["pooled"].clone(), first["hidden"].clone()
    assert torch.isfinite(ref_p).all() and torch.isfinite(ref_h.float()).all()
    for rep in range(60):
        out = enc.forward_packed(fd, cd, hidden=True)
        assert torch.equal(out["hidden"], ref_h), f"{preset}: hidden states of forward {rep + 1} differ from the first"
        assert torch.equal(out["pooled"], ref_p), f"{preset}: pooled rows of forward {rep + 1} differ from the first"


def test_out_of_range_inputs_are_clamped_flagged_and_refused():
    """HF raises IndexError for a token id / position id outside its table; the kernels clamp the index (no read outside
    the tables, no fault) and NativeEncoder.check() reports it.  Sequences that need position rows beyond the table are
    refused before any launch (MPNet: 513 tokens)."""
    preset = "tiny-mpnet"
    cfg = presets.PRESETS[preset]
    enc = NativeEncoder.from_preset(preset, max_tokens=4096, max_seqs=8)
    ids = presets.randint("oob/ids", 40, 5, cfg.vocab).astype(np.int32)
    cu = torch.tensor([0, 17, 40], dtype=torch.int32, device=DEV)
    good = enc.forward_packed(torch.from_numpy(ids).to(DEV), cu)["pooled"]
    enc.check()                                                    # clean input: nothing flagged
    bad = ids.copy()
    bad[5] = cfg.vocab + 1000                                      # tokenizer / vocabulary mismatch
    bad[20] = -3
    out = enc.forward_packed(torch.from_numpy(bad).to(DEV), cu)["pooled"]
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    with pytest.raises(IndexError, match="token id"):
        enc.check()
    enc.check()                                                    # the flag word was cleared by the failed check
    # a caller-supplied max_len smaller than the longest sequence would leave attention blocks unvisited: flagged
    enc.forward_packed(torch.from_numpy(ids).to(DEV), cu, max_len=10)
    with pytest.raises(IndexError, match="max_len"):
        enc.check()
    # position rows beyond the table: refused on the host
    n = cfg.max_pos - cfg.pad_id       # one token more than the table holds for MPNet
    long_ids = torch.from_numpy(presets.randint("oob/long", n, 5, cfg.vocab).astype(np.int32)).to(DEV)
    big = NativeEncoder.from_preset(preset, max_tokens=n, max_seqs=1)
    with pytest.raises(ValueError, match="position rows"):
        big.forward_packed(long_ids, torch.tensor([0, n], dtype=torch.int32, device=DEV))
    ok = big.forward_packed(long_ids[:n - 1], torch.tensor([0, n - 1], dtype=torch.int32, device=DEV))["pooled"]
    big.check()
    assert torch.isfinite(ok).all() and torch.equal(good, enc.forward_packed(torch.from_numpy(ids).to(DEV), cu)["pooled"])


def test_save_pretrained_round_trip(tmp_path):
    """modeling.py:52-59: save_pretrained writes the encoder weights (+ tokenizer + parameters); from_pretrained on that
    directory gives a model with bit-identical outputs."""
    from transformers import BertTokenizer
    from text_similarity_amd.configurations.config import Configuration, ModelParameters
    from text_similarity_amd.models.sentence_encoder import SentenceTransformerWrapper
    preset = "tiny-bert"
    tok = BertTokenizer(vocab=presets.synthetic_vocab(1000), do_lower_case=True)
    params = Configuration(model_parameters=ModelParameters(preset, hidden_size=64), model=preset, save_path="",
                           tokenizer=tok, device=torch.device(DEV), batch_size=4, max_tokens_per_batch=2048,
                           max_seqs_per_batch=64, sequence_max_len=48)      # tiny-bert has 64 position rows
    model = SentenceTransformerWrapper.from_preset(preset, params, parallel_mode=False)
    sents = presets.synthetic_sentences(40, seed="save/s", vocab_size=1000)
    a = model.encode_text(sents)
    model.save_pretrained(str(tmp_path))
    for f in ("config.json", "model.safetensors", "model_config.bin"):
        assert (tmp_path / f).exists(), f
    assert any((tmp_path / f).exists() for f in ("vocab.txt", "tokenizer.json", "tokenizer_config.json"))   # tokenizer files
    cfgd = torch.load(str(tmp_path / "model_config.bin"), weights_only=True)
    assert cfgd["batch_size"] == 4 and cfgd["model_parameters"]["hidden_size"] == 64
    again = SentenceTransformerWrapper.from_pretrained(str(tmp_path), params=params, parallel_mode=False)
    assert torch.equal(a, again.encode_text(sents))
    assert model.last_encode_stats["sentences"] == 40 and model.last_encode_stats["wall_s"] > 0
