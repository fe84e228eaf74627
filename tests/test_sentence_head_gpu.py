"""GPU checks of the sentence-embedding heads (include/tsim.h tsim_encoder_forward_head, tsim_pool, tsim_dense_rows):
every pooling mode against a float32 restatement of sentence-transformers' Pooling on oracle hidden states (the encoder
bars of test_encoder_gpu.py), BertPoolingStrategy against HF's BertModel pooler, bit-identity of the default path, batch
composition invariance, unit rows, Dense accuracy, padded against packed, and a sentence-transformers directory end to end."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import encoder_ref, search_ref
from text_similarity_amd import ops, presets
from text_similarity_amd.native_encoder import NativeEncoder, SentenceHead

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POOL_TOL, COS_MIN = 5e-2, 0.9995
MODES = ["mean", "cls", "max", "mean_sqrt_len"]


def _cos_rows(a, b):
    return (a * b).sum(1) / np.maximum(np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1), 1e-30)


def _batch(preset, n, seed, max_len=48):
    cfg = presets.PRESETS[preset]
    flat, cu = presets.synthetic_token_batch(n, seed=seed, vocab_size=cfg.vocab, max_len=max_len)
    return cfg, flat, cu


def _dev(flat, cu):
    return torch.from_numpy(flat).to(DEV), torch.from_numpy(cu.astype(np.int32)).to(DEV)


def _dense(d_in, d_out, seed):
    w = presets.normal(seed + "/w", d_out * d_in).reshape(d_out, d_in) / np.sqrt(d_in)
    b = presets.normal(seed + "/b", d_out) * 0.05
    return torch.from_numpy(w).float().to(DEV), torch.from_numpy(b).float().to(DEV)


def st_pool(hidden, mask, mode):
    """sentence-transformers' Pooling (float32 torch) on [B, S, H] hidden states."""
    m = mask.unsqueeze(-1).float()
    if mode == "cls":
        return hidden[:, 0]
    if mode == "max":
        return torch.where(m > 0, hidden, torch.full_like(hidden, -1e9)).max(1).values
    s = (hidden * m).sum(1)
    n = torch.clamp(m.sum(1), min=1e-9)
    return s / n if mode == "mean" else s / torch.sqrt(n)


_ENC = {}


def _encoder(preset):
    if preset not in _ENC:
        _ENC[preset] = NativeEncoder.from_preset(preset, max_tokens=8192, max_seqs=512, device=DEV)
    return _ENC[preset]


@pytest.mark.parametrize("preset", ["tiny-bert", "tiny-mpnet", "all-MiniLM-L6-v2"])
def test_each_mode_against_restatement(preset):
    cfg, flat, cu = _batch(preset, 24, "head/modes/" + preset)
    enc = _encoder(preset)
    fd, cd = _dev(flat, cu)
    ids, mask = encoder_ref.pad_batch(flat, cu, range(len(cu) - 1), cfg.pad_id)
    with torch.no_grad():
        hidden = encoder_ref.encoder_forward(cfg, presets.synthetic_weights(preset), ids, mask)
    for mode in MODES:
        got = enc.forward_packed(fd, cd, head=SentenceHead(mode))["pooled"].cpu().numpy()
        ref = st_pool(hidden, torch.from_numpy(mask), mode).numpy()
        err = float(np.abs(got - ref).max())
        assert err <= POOL_TOL and _cos_rows(got, ref).min() >= COS_MIN, (mode, err)


def test_bert_pooling_strategy_against_hf_pooler():
    transformers = pytest.importorskip("transformers")
    from text_similarity_amd.configurations.config import Configuration, ModelParameters
    from text_similarity_amd.models.sentence_encoder import SentenceTransformerWrapper
    from text_similarity_amd.modules.modules import BertPoolingStrategy
    preset = "tiny-bert"
    cfg, flat, cu = _batch(preset, 32, "head/bertpool")
    hc = transformers.BertConfig(vocab_size=cfg.vocab, hidden_size=cfg.hidden, num_hidden_layers=cfg.num_layers,
                                 num_attention_heads=cfg.heads, intermediate_size=cfg.ffn, max_position_embeddings=cfg.max_pos,
                                 type_vocab_size=cfg.type_vocab, layer_norm_eps=cfg.ln_eps, hidden_act="gelu",
                                 attn_implementation="eager")
    hf = transformers.BertModel(hc, add_pooling_layer=True).eval()
    w = presets.synthetic_weights(preset)
    pw, pb = _dense(cfg.hidden, cfg.hidden, "head/pooler")
    sd = {k: torch.from_numpy(v) for k, v in w.items()}
    sd.update({"pooler.dense.weight": pw.cpu(), "pooler.dense.bias": pb.cpu()})
    missing = hf.load_state_dict(sd, strict=False).missing_keys
    assert not [k for k in missing if "position_ids" not in k], missing
    params = Configuration(model_parameters=ModelParameters(preset, hidden_size=cfg.hidden), model=preset, save_path="",
                           device=torch.device(DEV))
    bp = BertPoolingStrategy(params)
    bp.load_state_dict({"linear.weight": pw.cpu(), "linear.bias": pb.cpu()})
    wrap = SentenceTransformerWrapper(pooler=bp, params=params, context_embedder=_encoder(preset), parallel_mode=False)
    fd, cd = _dev(flat, cu)
    got = wrap.encode_packed(fd, cd).cpu().numpy()
    ids, mask = encoder_ref.pad_batch(flat, cu, range(len(cu) - 1), cfg.pad_id)
    with torch.no_grad():
        ref = hf(input_ids=torch.from_numpy(ids), attention_mask=torch.from_numpy(mask)).pooler_output.numpy()
    assert np.abs(got - ref).max() <= POOL_TOL and _cos_rows(got, ref).min() >= COS_MIN
    # the padded form (wrapper.forward path) gives the same rows
    feats_hidden = _encoder(preset)(input_ids=torch.from_numpy(ids).to(DEV), attention_mask=torch.from_numpy(mask).to(DEV))[0]
    from text_similarity_amd.dataset.dataset import EmbeddingsFeatures
    pad = bp(feats_hidden, EmbeddingsFeatures(torch.from_numpy(ids).to(DEV), torch.from_numpy(mask).to(DEV)))
    assert torch.equal(pad.cpu(), torch.from_numpy(got))


@pytest.mark.parametrize("preset", ["tiny-bert", "all-MiniLM-L6-v2"])
def test_mean_head_is_the_default_forward_bit_for_bit(preset):
    cfg, flat, cu = _batch(preset, 40, "head/nochange")
    enc = _encoder(preset)
    fd, cd = _dev(flat, cu)
    r0, r1 = ops.new_rho(DEV), ops.new_rho(DEV)
    a = enc.forward_packed(fd, cd, unit=True, rho=r0)
    b = enc.forward_packed(fd, cd, unit=True, rho=r1, head=SentenceHead("mean"))
    assert torch.equal(a["pooled"], b["pooled"]) and torch.equal(a["unit"], b["unit"]) and torch.equal(r0, r1)
    ids, mask = encoder_ref.pad_batch(flat, cu, range(len(cu) - 1), cfg.pad_id)
    hidden = enc(input_ids=torch.from_numpy(ids).to(DEV), attention_mask=torch.from_numpy(mask).to(DEV))[0]
    m = torch.from_numpy(mask).to(DEV)
    assert torch.equal(ops.pool(hidden, m, "mean"), ops.mean_pool(hidden, m))
    assert torch.equal(ops.pool(hidden.bfloat16(), m, "mean"), ops.mean_pool(hidden.bfloat16(), m))


def _shuffled(flat, cu, perm):
    lens = np.diff(cu)
    parts = [flat[cu[i]:cu[i + 1]] for i in perm]
    cu2 = np.zeros(len(perm) + 1, np.int64)
    cu2[1:] = np.cumsum(lens[perm])
    return np.concatenate(parts).astype(np.int32), cu2


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dense", [False, True])
def test_batch_composition_invariance(mode, dense):
    preset = "all-MiniLM-L6-v2"
    cfg, flat, cu = _batch(preset, 150, "head/compose")
    enc = _encoder(preset)
    w, b = _dense(cfg.hidden, 256, "head/compose") if dense else (None, None)
    head = SentenceHead(mode, w, b, "tanh" if dense else "identity", normalize=dense)
    fd, cd = _dev(flat, cu)
    whole = enc.forward_packed(fd, cd, head=head, unit=True)
    parts = []
    for lo, hi in ((0, 7), (7, 100), (100, 150)):
        f2, c2 = flat[cu[lo]:cu[hi]], (cu[lo:hi + 1] - cu[lo])
        parts.append(enc.forward_packed(*_dev(f2, c2), head=head, unit=True))
    assert torch.equal(whole["pooled"], torch.cat([p["pooled"] for p in parts]))
    assert torch.equal(whole["unit"], torch.cat([p["unit"] for p in parts]))
    perm = np.random.default_rng(5).permutation(len(cu) - 1)
    sh = enc.forward_packed(*_dev(*_shuffled(flat, cu, perm)), head=head, unit=True)
    assert torch.equal(sh["pooled"], whole["pooled"][torch.from_numpy(perm).to(DEV)])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dense", [None, 256, 768])
def test_unit_rows_are_l2norm_of_final_rows(mode, dense):
    preset = "all-MiniLM-L6-v2"
    cfg, flat, cu = _batch(preset, 70, "head/unit")
    # two empty sequences (zero rows in every mode)
    cu = np.concatenate([cu[:5], cu[4:5], cu[5:], cu[-1:]])
    enc = _encoder(preset)
    w, b = _dense(cfg.hidden, dense, "head/unit") if dense else (None, None)
    for norm in (False, True):
        head = SentenceHead(mode, w, b, "tanh" if dense else "identity", normalize=norm)
        rho = ops.new_rho(DEV)
        r = enc.forward_packed(*_dev(flat, cu), head=head, unit=True, rho=rho)
        u, rho2 = ops.l2norm_rows(r["pooled"], return_rho=True)
        assert torch.equal(r["unit"], u) and torch.equal(rho, rho2) and float(rho) > 0
        assert (r["pooled"][4] == 0).all() and (r["pooled"][-1] == 0).all() or dense
        if norm:
            n = torch.linalg.vector_norm(r["pooled"].double(), dim=1)
            live = n > 0
            assert torch.allclose(n[live], torch.ones_like(n[live]), atol=1e-6, rtol=0)


def test_head_refusals():
    enc = _encoder("tiny-bert")
    cfg, flat, cu = _batch("tiny-bert", 4, "head/bad")
    fd, cd = _dev(flat, cu)
    w, b = _dense(cfg.hidden, 1024, "head/bad")
    with pytest.raises(ValueError, match="768"):
        enc.forward_packed(fd, cd, head=SentenceHead("cls", w, b), unit=True)
    w2, b2 = _dense(cfg.hidden, 20, "head/bad2")
    with pytest.raises(ValueError, match="d_out"):
        enc.forward_packed(fd, cd, head=SentenceHead("cls", w2, b2))
    h = SentenceHead("cls")
    h.mode = 7
    with pytest.raises(ValueError, match="pool_mode"):
        enc.forward_packed(fd, cd, head=h)
    h = SentenceHead("cls", *_dense(cfg.hidden, 64, "head/bad3"))
    h.act = 5
    with pytest.raises(ValueError, match="activation"):
        enc.forward_packed(fd, cd, head=h)
    with pytest.raises(ValueError):
        ops.dense_rows(torch.zeros(3, 64, device=DEV), torch.zeros(64, 2048, device=DEV))
    with pytest.raises(ValueError):
        ops.pool(torch.zeros(2, 3, 8, device=DEV), torch.ones(2, 3, device=DEV), "lasttoken")


@pytest.mark.parametrize("d_in,d_out", [(8, 8), (64, 24), (384, 384), (384, 256), (768, 768), (1024, 1024), (392, 1000)])
def test_dense_rows_accuracy(d_in, d_out):
    B = 77
    x = torch.from_numpy(presets.normal(f"dense/x/{d_in}", B * d_in).reshape(B, d_in) * 2).float().to(DEV)
    w, b = _dense(d_in, d_out, f"dense/{d_in}/{d_out}")
    for act in ("identity", "tanh"):
        y = ops.dense_rows(x, w, b, act).cpu().numpy().astype(np.float64)
        X, W, Bv = (t.cpu().numpy().astype(np.float64) for t in (x, w, b))
        z = X @ W.T
        bound = d_in * 2.0 ** -23 * (np.abs(X) @ np.abs(W).T) + np.abs(z + Bv) * 2.0 ** -24 + 1e-30
        ref = z + Bv
        if act == "tanh":
            ref = np.tanh(ref)       # |tanh'| <= 1: the same bound, plus the library tanh's few ulp
            bound = bound + 4 * 2.0 ** -24
        assert (np.abs(y - ref) <= bound * 1.01).all(), float((np.abs(y - ref) / bound).max())
    yn = ops.dense_rows(x, w, b, "tanh", normalize=True).double()
    assert torch.allclose(torch.linalg.vector_norm(yn, dim=1), torch.ones(B, dtype=torch.float64, device=DEV), atol=1e-6, rtol=0)
    # Normalize alone (no projection): F.normalize
    xn = ops.dense_rows(x, None, None, "identity", normalize=True)
    assert torch.allclose(xn, F.normalize(x, dim=1), atol=1e-6, rtol=0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dense", [False, True])
def test_padded_matches_packed(mode, dense):
    from text_similarity_amd.dataset.dataset import EmbeddingsFeatures
    from text_similarity_amd.modules.modules import SentenceEmbeddingHead
    preset = "all-MiniLM-L6-v2"
    cfg, flat, cu = _batch(preset, 40, "head/padded")
    enc = _encoder(preset)
    lin = None
    if dense:
        lin = torch.nn.Linear(cfg.hidden, 128)
        w, b = _dense(cfg.hidden, 128, "head/padded")
        lin.load_state_dict({"weight": w.cpu(), "bias": b.cpu()})
    mod = SentenceEmbeddingHead(pooling_mode=mode, dense=lin, activation="tanh" if dense else "identity", normalize=dense)
    packed = enc.forward_packed(*_dev(flat, cu), head=mod.native_head(torch.device(DEV)))["pooled"]
    ids, mask = encoder_ref.pad_batch(flat, cu, range(len(cu) - 1), cfg.pad_id)
    ids_d, mask_d = torch.from_numpy(ids).to(DEV), torch.from_numpy(mask).to(DEV)
    padded = mod(enc(input_ids=ids_d, attention_mask=mask_d)[0], EmbeddingsFeatures(ids_d, mask_d))
    if mode in ("cls", "max"):
        assert torch.equal(padded, packed)
    else:
        assert (padded - packed).abs().max().item() <= 1e-6


def test_sentence_transformers_directory_end_to_end(tmp_path):
    transformers = pytest.importorskip("transformers")
    from text_similarity_amd.configurations.config import SearchConfiguration, ModelParameters
    from text_similarity_amd.models.sentence_encoder import SentenceTransformerWrapper
    from text_similarity_amd.models.st_format import DenseSpec, write_sentence_transformers_modules
    from text_similarity_amd.pipeline.search_pipeline import SemanticSearchPipeline
    from text_similarity_amd.weights import save_hf_dir
    preset = "all-MiniLM-L6-v2"
    cfg = presets.PRESETS[preset]
    w = presets.synthetic_weights(preset)
    path = str(tmp_path / "st")
    save_hf_dir(path, cfg, w)
    dw, db = _dense(cfg.hidden, 256, "head/e2e")
    write_sentence_transformers_modules(path, cfg.hidden, "cls", DenseSpec(cfg.hidden, 256, "tanh", dw.cpu().numpy(),
                                                                            db.cpu().numpy()), True)
    tok = transformers.BertTokenizer(vocab=presets.synthetic_vocab(cfg.vocab), do_lower_case=True)
    params = SearchConfiguration(model_parameters=ModelParameters(preset, hidden_size=None), model=preset, save_path="", tokenizer=tok,
                                 device=torch.device(DEV), max_tokens_per_batch=8192, max_seqs_per_batch=512,
                                 sequence_max_len=64)
    model = SentenceTransformerWrapper.from_sentence_transformers(path, params, parallel_mode=False)
    assert model.get_sentence_embedding_dimension() == 256
    sents = presets.synthetic_sentences(160, seed="head/e2e", vocab_size=cfg.vocab, max_words=40)
    emb = model.encode_text(sents, output_np=True)
    assert emb.shape == (160, 256)
    # HF BertModel float32 + a torch restatement of Pooling(cls) -> Dense(tanh) -> Normalize
    hc = transformers.BertConfig(vocab_size=cfg.vocab, hidden_size=cfg.hidden, num_hidden_layers=cfg.num_layers,
                                 num_attention_heads=cfg.heads, intermediate_size=cfg.ffn, max_position_embeddings=cfg.max_pos,
                                 type_vocab_size=cfg.type_vocab, layer_norm_eps=cfg.ln_eps, hidden_act="gelu",
                                 attn_implementation="eager")
    hf = transformers.BertModel(hc, add_pooling_layer=False).eval()
    missing = hf.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=False).missing_keys
    assert not [k for k in missing if "position_ids" not in k], missing
    ref = []
    with torch.no_grad():
        for s in range(0, len(sents), 32):
            bt = tok(sents[s:s + 32], padding=True, truncation=True, max_length=64, return_tensors="pt")
            h = hf(input_ids=bt["input_ids"], attention_mask=bt["attention_mask"]).last_hidden_state
            ref.append(F.normalize(torch.tanh(F.linear(h[:, 0], dw.cpu(), db.cpu())), dim=1))
    ref = torch.cat(ref).numpy()
    assert _cos_rows(emb, ref).min() >= COS_MIN
    # a 256-wide index on those embeddings returns the oracle's exact lists
    corpus, queries = sents[:120], sents[120:]
    pipe = SemanticSearchPipeline(str(tmp_path / "index"), params, model, corpus=list(corpus))
    res = pipe(list(queries), 5)
    rs, ri = search_ref.cosine_topk_f32(emb[120:], emb[:120], 5)
    assert np.array_equal(pipe.last_labels.cpu().numpy(), ri) and np.array_equal(pipe.last_scores.cpu().numpy(), rs)
    assert res[0] == [corpus[i] for i in ri[0]]
    # save_pretrained -> from_sentence_transformers round-trips bit for bit
    out = str(tmp_path / "saved")
    model.save_pretrained(out)
    again = SentenceTransformerWrapper.from_sentence_transformers(out, params, parallel_mode=False)
    assert np.array_equal(again.encode_text(sents, output_np=True), emb)


def test_default_and_foreign_poolers():
    import warnings
    from text_similarity_amd.configurations.config import Configuration, ModelParameters
    from text_similarity_amd.models.sentence_encoder import SentenceTransformerWrapper
    from text_similarity_amd.modules.modules import PoolingStrategy
    preset = "tiny-bert"
    cfg, flat, cu = _batch(preset, 12, "head/foreign")
    params = Configuration(model_parameters=ModelParameters(preset), model=preset, save_path="", device=torch.device(DEV))
    enc = _encoder(preset)
    fd, cd = _dev(flat, cu)
    base = enc.forward_packed(fd, cd)["pooled"]
    default = SentenceTransformerWrapper(params=params, context_embedder=enc, parallel_mode=False)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert torch.equal(default.encode_packed(fd, cd), base)

    class Foreign(PoolingStrategy):
        pass

    foreign = SentenceTransformerWrapper(pooler=Foreign(params), params=params, context_embedder=enc, parallel_mode=False)
    with pytest.warns(UserWarning, match="Foreign"):
        assert torch.equal(foreign.encode_packed(fd, cd), base)
