"""Test data for the source architectures that run on the BERT graph (DistilBERT, RoBERTa, XLM-R, CamemBERT) and for
hidden-1024 encoders (builders only; no GPU).  Used by tests/test_arch_cpu.py and tests/test_arch_gpu.py.

* ``hf_model`` builds HF's own model of an architecture locally (no download) and loads ``presets.synthetic_weights`` into it
  under the architecture's own state_dict names.
* ``canonical_bert`` restates such a model as a plain BERT configuration for ``oracle.encoder_ref``: the position table shifted
  by the position offset, and an all-zero token-type row where the architecture has none.  It holds for inputs in which the
  pad id does not occur (position = offset + column), which is true of the fixtures' batch (every id >= 5).
* ``CASES_1024``: the hidden-1024 shape of the issue under ``encoder_cases.sharp_weights`` with the Q/K scale its documented
  law starts from (see ``QK_A_1024``), and the inputs, probe and tolerance rule of ``encoder_cases`` (borrowed through ``registered``).
"""
import contextlib
import functools
from dataclasses import replace

import numpy as np
import pytest
import torch

import encoder_cases as ec
from text_similarity_amd import presets
from text_similarity_amd.presets import EncoderConfig

POS, TYPE = "embeddings.position_embeddings.weight", "embeddings.token_type_embeddings.weight"

# model_type -> (configuration, stream name of its synthetic weights)
ARCHS = {
    "distilbert": (presets.PRESETS["tiny-distilbert"], "tiny-distilbert"),
    "roberta": (presets.PRESETS["tiny-roberta"], "tiny-roberta"),
    "xlm-roberta": (replace(presets.PRESETS["tiny-roberta"], model_type="xlm-roberta"), "tiny-xlm-roberta"),
    "camembert": (replace(presets.PRESETS["tiny-roberta"], model_type="camembert"), "tiny-camembert"),
}


def arch_weights(model_type):
    cfg, stream = ARCHS[model_type]
    return cfg, presets.synthetic_weights(stream, cfg)


def hf_config(cfg, **extra):
    transformers = pytest.importorskip("transformers")
    if cfg.model_type == "distilbert":
        return transformers.DistilBertConfig(vocab_size=cfg.vocab, dim=cfg.hidden, n_layers=cfg.num_layers, n_heads=cfg.heads,
                                             hidden_dim=cfg.ffn, max_position_embeddings=cfg.max_pos, activation="gelu",
                                             pad_token_id=cfg.pad_id, dropout=0.0, attention_dropout=0.0, seq_classif_dropout=0.0,
                                             **extra)
    cls = {"roberta": transformers.RobertaConfig, "xlm-roberta": transformers.XLMRobertaConfig,
           "camembert": transformers.CamembertConfig, "bert": transformers.BertConfig}[cfg.source_type]
    return cls(vocab_size=cfg.vocab, hidden_size=cfg.hidden, num_hidden_layers=cfg.num_layers, num_attention_heads=cfg.heads,
               intermediate_size=cfg.ffn, max_position_embeddings=cfg.max_pos, layer_norm_eps=cfg.ln_eps,
               type_vocab_size=cfg.type_vocab, pad_token_id=cfg.pad_id, hidden_act="gelu", **extra)


def hf_model(cfg, w):
    """HF's base model of ``cfg.model_type`` (no pooler) holding the weights ``w`` (in-memory BERT names)."""
    transformers = pytest.importorskip("transformers")
    hc = hf_config(cfg)
    if cfg.model_type == "distilbert":
        m = transformers.DistilBertModel(hc)
    else:
        cls = {"roberta": transformers.RobertaModel, "xlm-roberta": transformers.XLMRobertaModel,
               "camembert": transformers.CamembertModel}[cfg.model_type]
        m = cls(hc, add_pooling_layer=False)
    sd = {presets.source_name(cfg.model_type, k): torch.from_numpy(v.copy()) for k, v in w.items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    missing = [k for k in missing if "position_ids" not in k and "token_type_ids" not in k]
    assert not missing and not unexpected, (missing, unexpected)
    return m.eval()


def hf_hidden(model, ids, mask):
    with torch.no_grad():
        return model(input_ids=torch.from_numpy(np.asarray(ids)), attention_mask=torch.from_numpy(np.asarray(mask)))[0].numpy()


def canonical_bert(cfg, w, pos_offset=None, type_row=True):
    """(BERT configuration, weights) computing the same function as (cfg, w) on inputs without the pad id.  ``pos_offset``
    and ``type_row`` override what the architecture prescribes (the tests' deliberately wrong mappings)."""
    off = cfg.pos_offset if pos_offset is None else pos_offset
    w2 = dict(w)
    w2[POS] = np.ascontiguousarray(w[POS][off:])
    if cfg.type_vocab == 0 or not type_row:
        w2[TYPE] = np.zeros((1, cfg.hidden), np.float32)
    return replace(cfg, arch="bert", max_pos=cfg.max_pos - off, pos_offset=0, model_type="", type_vocab=w2[TYPE].shape[0]), w2


def sharp_arch_weights(preset):
    """(configuration with encoder_cases' vocabulary, ``encoder_cases.sharp_weights``) of a tiny preset of this file's
    architectures.  Under ``presets.synthetic_weights`` attention is almost uniform and a sequence's first-token row hardly
    depends on its text: the classifier logits of 200 pairs then spread by 0.0013 (one label), about as much as the bf16
    encoder's error moves them, and a correlation bound measures noise.  Under these weights the float64 probe puts the
    spread per label at 0.009 - 0.064 and its own bf16-rounded run at most 0.004 away (Pearson >= 0.9994)."""
    cfg = replace(presets.PRESETS[preset], vocab=ec.VOCAB)
    w = dict(ec.sharp_weights(replace(cfg, type_vocab=max(cfg.type_vocab, 1)), "arch/" + preset))
    if cfg.type_vocab == 0:          # (sharp_weights wants a token-type row to build its LayerNorm-eps tokens; DistilBERT has none)
        del w[TYPE]
    return cfg, w


# --------------------------------------------------------------------------- hidden 1024
# encoder_cases documents the law: the logits' standard deviation grows like H a^2 / 3 times the mean square of a LayerNorm
# output, so a ~ 1 / sqrt(H); from hidden 768 that gives a(1024) = 0.085 sqrt(768 / 1024) = 0.0736.  Measured with the
# float64 probe on the case's inputs, that value reproduces hidden 768 in layer 1 (median largest probability 0.293 against
# 0.292) but leaves layer 2 at 0.153 (hidden 768: 0.241), below the 0.2 that the criteria ask for: the law holds the first
# layer's logits, not what a wider layer 1 hands to layer 2 (scaling V and O by the same law gives 0.176).  The criteria are
# the aim and the law a first estimate, so hidden 1024 keeps the scales of hidden 768, the nearest documented size: measured
# 0.425 / 0.268 (bf16 case), inside [0.2, 0.9] in both layers.  tests/test_arch_cpu.py prints and bounds these figures.
QK_A_LAW_1024 = float(np.float32(0.085 * np.sqrt(768.0 / 1024.0)))
QK_A_1024 = 0.085
VO_A_1024 = 0.10
CFG_1024 = EncoderConfig("bert", 2, 1024, 16, 4096, ec.VOCAB, 260, 1e-12)
CASES_1024 = {"bert-1024": (CFG_1024, "bf16"), "bert-1024-mxfp8": (CFG_1024, "mxfp8")}


@contextlib.contextmanager
def registered():
    """encoder_cases' builders look a case up by name: inside this block they know the hidden-1024 cases and scales too
    (removed again afterwards, so the parametrised tests over ``encoder_cases.CASES`` keep their cases)."""
    ec.CASES.update(CASES_1024)
    ec._QK_A[1024], ec._VO_A[1024] = QK_A_1024, VO_A_1024
    try:
        yield
    finally:
        for k in CASES_1024:
            ec.CASES.pop(k, None)
        ec._QK_A.pop(1024, None)
        ec._VO_A.pop(1024, None)


def weights_1024(name):
    with registered():
        return ec.sharp_weights(CFG_1024, name)


def inputs_1024(name):
    with registered():
        return ec.case_inputs(name)


@functools.lru_cache(maxsize=None)
def tolerances_1024(name):
    """(exact, floor, tol) by the rule of ``encoder_cases.tolerances``: floor = the probe's bf16-rounded run against its
    float64 run, tol = TOL_FACTOR x floor, computed here."""
    with registered():
        return ec.tolerances(name)
