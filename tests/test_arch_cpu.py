"""DistilBERT, RoBERTa, XLM-R and CamemBERT checkpoints on the BERT graph, and the hidden-1024 test weights (CPU).

The mapping is checked against HF's own models, built locally (no download) with ``presets.synthetic_weights`` and written
with HF ``save_pretrained``: ``weights.load_hf_dir`` plus ``oracle.encoder_ref.encoder_forward`` on the mapped weights (as a
plain BERT configuration, arch_cases.canonical_bert) must equal the HF forward within the bars the oracle meets against its
fixtures (tests/test_oracle_golden.py: hidden 2e-5, pooled 1e-5).  A wrong position offset or a dropped token-type row moves
the output by more than 1e-3, so those bars can tell."""
import json
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

import arch_cases as ac
import encoder_cases as ec
from conftest import golden
from oracle import encoder_probe, encoder_ref
from text_similarity_amd import presets
from text_similarity_amd.native_encoder import NativeEncoder
from text_similarity_amd.weights import config_from_hf, load_hf_dir, save_hf_dir

HID_ATOL, POOL_ATOL = 2e-5, 1e-5          # tests/test_oracle_golden.py
WRONG_MIN = 1e-3
TYPES = list(ac.ARCHS)


def _batch():
    g = golden("encoder_tiny-bert.npz")
    return g["input_ids"], g["attention_mask"]


def _oracle(cfg, w, ids, mask, **kw):
    c, cw = ac.canonical_bert(cfg, w, **kw)
    with torch.no_grad():
        h = encoder_ref.encoder_forward(c, cw, ids, mask)
        return h.numpy(), encoder_ref.mean_pool(h, mask).numpy()


def _hf_pooled(h, mask):
    return encoder_ref.mean_pool(torch.from_numpy(h), mask).numpy()


@pytest.mark.parametrize("mt", TYPES)
def test_config_from_hf_reads_the_new_model_types(mt):
    cfg, _ = ac.ARCHS[mt]
    d = ac.hf_config(cfg).to_dict()
    assert d["model_type"] == mt
    got = config_from_hf(d)
    assert got == cfg
    assert got.arch == "bert" and got.model_type == mt and got.source_type == mt
    if mt == "distilbert":
        assert (got.type_vocab, got.pos_offset, got.first_pos, got.ln_eps, got.pad_id) == (0, 0, 0, 1e-12, 0)
        assert (got.num_layers, got.hidden, got.heads, got.ffn, got.vocab, got.max_pos) == (2, 64, 4, 128, 1000, 64)
    else:
        assert (got.type_vocab, got.pos_offset, got.first_pos, got.pad_id) == (1, 2, 2, 1)
        assert (got.num_layers, got.hidden, got.heads, got.ffn, got.vocab, got.max_pos) == (2, 64, 4, 128, 1000, 66)


def test_config_from_hf_keeps_refusing():
    rob = ac.hf_config(ac.ARCHS["roberta"][0]).to_dict()
    dis = ac.hf_config(ac.ARCHS["distilbert"][0]).to_dict()
    for bad in ({"model_type": "albert"}, {"model_type": "electra"}, {"model_type": "deberta-v2"}, {"model_type": "gpt2"},
                dict(rob, hidden_act="relu"), dict(dis, activation="relu"),
                dict(rob, position_embedding_type="relative_key"), dict(rob, type_vocab_size=2)):
        with pytest.raises(ValueError):
            config_from_hf(bad)
    # existing presets compare equal to what their configuration files give, with the new fields at their defaults
    for preset in ("tiny-bert", "tiny-mpnet", "bert-base-uncased", "all-mpnet-base-v2"):
        cfg = presets.PRESETS[preset]
        assert (cfg.pos_offset, cfg.model_type, cfg.source_type) == (0, "", cfg.arch)
    assert presets.PRESETS["tiny-bert"] == presets.EncoderConfig("bert", 2, 64, 4, 128, 1000, 64, 1e-12)


def test_new_presets_and_weight_names():
    P = presets.PRESETS
    assert (P["distilbert-base-multilingual-cased"].num_layers, P["distilbert-base-multilingual-cased"].hidden,
            P["distilbert-base-multilingual-cased"].vocab) == (6, 768, 119547)
    x = P["xlm-roberta-base"]
    assert (x.num_layers, x.hidden, x.vocab, x.max_pos, x.first_pos) == (12, 768, 250002, 514, 2)
    for name in ("bert-large", "xlm-roberta-large"):
        assert (P[name].num_layers, P[name].hidden, P[name].heads, P[name].ffn, P[name].head_dim) == (24, 1024, 16, 4096, 64)
    for mt in TYPES:
        cfg, w = ac.arch_weights(mt)
        hf_names = set(ac.hf_model(cfg, w).state_dict())
        ours = {n for n, _, _ in presets.weight_names(cfg, source=True)}
        assert ours <= hf_names, sorted(ours - hf_names)
        assert {presets.bert_name(mt, n) for n in ours} == set(w)
        assert (ac.TYPE in w) == (mt != "distilbert")
    assert ac.TYPE not in presets.synthetic_weights("tiny-distilbert")
    assert presets.synthetic_weights("tiny-roberta")[ac.TYPE].shape == (1, 64)


@pytest.mark.parametrize("mt", TYPES)
def test_mapping_equals_the_hf_model(mt, tmp_path):
    cfg, w = ac.arch_weights(mt)
    model = ac.hf_model(cfg, w)
    model.save_pretrained(str(tmp_path))
    cfg2, w2 = load_hf_dir(str(tmp_path))
    assert cfg2 == cfg
    assert set(w2) == set(w) and all(np.array_equal(w[k], w2[k]) for k in w)
    ids, mask = _batch()
    live = mask.astype(bool)
    ref = ac.hf_hidden(model, ids, mask)
    h, p = _oracle(cfg2, w2, ids, mask)
    eh, ep = float(np.abs(h[live] - ref[live]).max()), float(np.abs(p - _hf_pooled(ref, mask)).max())
    print(f"{mt}: oracle on the mapped weights vs HF: hidden {eh:.2e} pooled {ep:.2e}")
    assert eh <= HID_ATOL and ep <= POOL_ATOL
    if mt != "distilbert":       # the bar can tell: the two ways to get the mapping wrong stand far above it
        for what, kw in (("position offset 0", {"pos_offset": 0}), ("no token-type row", {"type_row": False})):
            hw, _ = _oracle(cfg2, w2, ids, mask, **kw)
            ew = float(np.abs(hw[live] - ref[live]).max())
            print(f"{mt}: with {what}: hidden {ew:.2e}")
            assert ew > WRONG_MIN
    else:                        # DistilBERT with BERT's token-type row added would be as wrong
        wt = dict(w2)
        wt[ac.TYPE] = presets.synthetic_weights("tiny-bert")[ac.TYPE]
        with torch.no_grad():
            hw = encoder_ref.encoder_forward(replace(cfg2, type_vocab=2, model_type=""), wt, ids, mask).numpy()
        assert float(np.abs(hw[live] - ref[live]).max()) > WRONG_MIN


@pytest.mark.parametrize("preset", ["tiny-distilbert", "tiny-roberta"])
def test_fixtures_equal_the_oracle(preset):
    g = golden(f"encoder_{preset}.npz")
    gb = golden("encoder_tiny-bert.npz")
    assert set(g.files) == set(gb.files)
    np.testing.assert_array_equal(g["input_ids"], gb["input_ids"])
    np.testing.assert_array_equal(g["attention_mask"], gb["attention_mask"])
    cfg, w = presets.PRESETS[preset], presets.synthetic_weights(preset)
    h, p = _oracle(cfg, w, g["input_ids"], g["attention_mask"])
    live = g["attention_mask"].astype(bool)
    np.testing.assert_allclose(h[live], g["last_hidden_state"][live], rtol=0, atol=HID_ATOL)
    np.testing.assert_allclose(p, g["pooled"], rtol=0, atol=POOL_ATOL)


@pytest.mark.parametrize("mt", TYPES)
def test_save_hf_dir_is_read_by_automodel(mt, tmp_path):
    cfg, w = ac.arch_weights(mt)
    save_hf_dir(str(tmp_path), cfg, w)
    with open(os.path.join(str(tmp_path), "config.json")) as f:
        assert json.load(f)["model_type"] == mt
    transformers = pytest.importorskip("transformers")
    auto = transformers.AutoModel.from_pretrained(str(tmp_path)).eval()
    assert auto.config.model_type == mt
    ids, mask = _batch()
    live = mask.astype(bool)
    ref = ac.hf_hidden(ac.hf_model(cfg, w), ids, mask)
    got = ac.hf_hidden(auto, ids, mask)
    np.testing.assert_allclose(got[live], ref[live], rtol=0, atol=HID_ATOL)
    cfg2, w2 = load_hf_dir(str(tmp_path))
    assert cfg2 == cfg and set(w2) == set(w) and all(np.array_equal(w[k], w2[k]) for k in w)


def test_length_guard_of_a_514_row_roberta_table():
    cfg = presets.PRESETS["xlm-roberta-base"]
    assert (cfg.max_pos, cfg.first_pos) == (514, 2)
    NativeEncoder.check_lengths(cfg, 512)
    for n in (513, 514):
        with pytest.raises(ValueError, match="position rows"):
            NativeEncoder.check_lengths(cfg, n)
    NativeEncoder.check_lengths(presets.PRESETS["distilbert-base-multilingual-cased"], 512)
    with pytest.raises(ValueError, match="position rows"):
        NativeEncoder.check_lengths(presets.PRESETS["distilbert-base-multilingual-cased"], 513)


@pytest.mark.parametrize("name", list(ac.CASES_1024))
def test_hidden_1024_weights_make_every_stage_matter(name):
    """The criteria tests/test_encoder_power_cpu.py bounds for hidden 64 / 384 / 768, at hidden 1024.  The Q/K scale starts from
    encoder_cases' law (a ~ 1 / sqrt(H)) and ends at the scale of hidden 768, for the reason arch_cases.QK_A_1024 gives."""
    cfg = ac.CFG_1024
    assert abs(ac.QK_A_LAW_1024 - ec._QK_A[768] * np.sqrt(768 / 1024)) < 1e-6 and 1024 not in ec._QK_A
    assert ac.QK_A_LAW_1024 <= ac.QK_A_1024 <= ec._QK_A[768] and ac.VO_A_1024 == ec._VO_A[768]
    ids, cu, notes = ac.inputs_1024(name)
    w = ac.weights_1024(name)
    assert all(np.array_equal(v, presets.bf16_round(v)) for k, v in w.items() if "word_embeddings" not in k)
    st = {}
    encoder_probe.probe_forward(cfg, w, ids, cu, linear=ec.fp8_ref.mx_linear if name.endswith("mxfp8") else None, stats=st)
    live = int((np.diff(cu) > 0).sum())
    for l in range(cfg.num_layers):
        per_seq = st["softmax_max"][l * live:(l + 1) * live]
        med = float(np.median(np.concatenate([v for S, v in per_seq if S >= 16])))
        print(f"{name} layer {l + 1}: median largest probability {med:.3f}, max |FFN1 pre-activation| {st['ffn1_absmax'][l]:.1f}")
        assert 0.2 <= med <= 0.9
        assert st["ffn1_absmax"][l] >= 3.0
    s = notes["lowvar"]
    tok = ids[cu[s]:cu[s + 1]].astype(np.int64)
    x = (w["embeddings.word_embeddings.weight"][tok].astype(np.float64) + w[ac.POS][:len(tok)] + w[ac.TYPE][0])
    assert (x.var(1) < 2e-6).all() and (x.var(1) > 5e-7).all()
    assert 1024 not in ec._QK_A and not set(ac.CASES_1024) & set(ec.CASES)      # the borrowed registry is clean again
