"""Strings to embeddings, end to end, for a tokenizer with user-added tokens: token ids are the only input of the encoder, so
the native tokenizer path and the library path must give the same BITS from ``encode_text``, ``CrossEncoder.predict`` and
``WordEncoder.encode_words``.  The tokenizer is variant H of tests/tokenizer_cases.py (normalized=True and =False tokens, a
content with a blank, one with punctuation, a single_word one, an additional special token) on a vocabulary small enough for
the tiny-bert shape; the library path is the same call with TSIM_NATIVE_TOKENIZER=0 and a fresh tokenizer object.  Both runs
sort and batch alike (same strings, same ids), so the comparison is ``torch.equal``."""
import dataclasses

import numpy as np
import pytest
import torch

from text_similarity_amd import presets
from text_similarity_amd.native_encoder import NativeEncoder

transformers = pytest.importorskip("transformers")

import tokenizer_cases as tc    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PRESET = "tiny-bert"
SEQ_MAX = 32          # tiny-bert has 64 position rows
LATE = "prezz"        # the token added to the live tokenizer in the stale-cache test


def _tokenizer(late=False):
    vocab, _ = tc.matrix_vocab(300, 150)
    tok = tc.make_tokenizer("H", True, vocab)
    if late:
        assert tok.add_tokens([LATE]) == 1
    return tok


def _config():
    """tiny-bert with a word-embedding table for every id of the tokenizer, the late token's included."""
    return dataclasses.replace(presets.PRESETS[PRESET], vocab=len(_tokenizer(late=True)))


def _model(cls, tok):
    from text_similarity_amd.configurations.config import Configuration, ModelParameters
    cfg = _config()
    enc = NativeEncoder(cfg, presets.synthetic_weights(PRESET, cfg), max_tokens=4096, max_seqs=128, device=torch.device(DEV))
    params = Configuration(model_parameters=ModelParameters(PRESET, hidden_size=cfg.hidden), model=PRESET, save_path="",
                           tokenizer=tok, device=torch.device(DEV), batch_size=4, max_tokens_per_batch=4096,
                           max_seqs_per_batch=128, sequence_max_len=SEQ_MAX)
    return cls(params=params, context_embedder=enc, parallel_mode=False)


def _changed_case(content):
    """The case forms of a content other than the content as written."""
    return [f for f in tc.case_forms(content) if f != content]


def _sentences():
    """32 sentences that hold an added content in a letter case other than the one it was added in (or cut by a control
    character, with a tab for its blank, next to punctuation, or straddling the truncation point), then 32 clean ones."""
    tok = _tokenizer()
    _, syll = tc.matrix_vocab(300, 150)
    per_content = []
    for i, c in enumerate(tc.CONTENTS["H"]):
        forms = _changed_case(c)
        f, g = forms[0], forms[-1]
        per_content.append([f"the {f} and", "the " * (SEQ_MAX - 4 + i % 3) + f + " and", f"{g} {'the ' * (i + 1)}and {f}",
                            f"un{g}s the", f"the {c[:2]}\x01{c[2:]} and the", "and " + f.replace(" ", "\t") + ", " + g, f"({g})"])
    with_added = [row[k] for k in range(7) for row in per_content]      # round robin: every content in the first five placements
    with_added = list(dict.fromkeys(with_added))[:32]
    clean = [s for s in tc.clean_sentences(tok, syll, 200, seed=41) if 0 < len(s) < 150][:32]
    assert len(with_added) == 32 and len(clean) == 32
    return with_added + clean


def _library_tokenizer(monkeypatch, late=False):
    monkeypatch.setenv("TSIM_NATIVE_TOKENIZER", "0")
    return _tokenizer(late)


def test_encode_text_native_equals_library(monkeypatch):
    from text_similarity_amd.models.sentence_encoder import SentenceTransformerWrapper
    sents = _sentences()
    tok = _tokenizer()
    ids = tok(sents[:32], truncation=True, max_length=SEQ_MAX)["input_ids"]
    added = tc.user_added_ids(tok)
    # at least 16 of them hold a MATCHED token (a normalized=False content in another case is text, as it must be) ...
    assert sum(bool(added & set(r)) for r in ids) >= 16, "the sentences hardly hold an added token: the case tests nothing"
    assert max(len(r) for r in tok(sents)["input_ids"]) > SEQ_MAX         # ... and some are cut at SEQ_MAX
    model = _model(SentenceTransformerWrapper, tok)
    native = model.encode_text(sents)
    assert tok._tsim_native_wordpiece, "the native tokenizer was not in use"
    model.params.tokenizer = _library_tokenizer(monkeypatch)
    library = model.encode_text(sents)
    assert model.params.tokenizer._tsim_native_wordpiece is False
    assert native.shape == (64, 64) and torch.isfinite(native).all()
    differ = [s for s, a, b in zip(sents, native, library) if not torch.equal(a, b)]
    assert not differ, differ[:5]
    assert torch.equal(native, library)


def test_token_added_to_a_live_tokenizer_reaches_encode_text(monkeypatch):
    from text_similarity_amd.models.sentence_encoder import SentenceTransformerWrapper
    tok = _tokenizer()
    model = _model(SentenceTransformerWrapper, tok)
    holding = ["the PREZZ and", "Prezz", "the and pre\x01zz the", "unprezz"]
    sents = holding + ["the and", "prequ the", "the QQFOO and"]
    before = model.encode_text(sents)
    assert tok._tsim_native_wordpiece
    assert tok.add_tokens([LATE]) == 1
    after = model.encode_text(sents)
    model.params.tokenizer = _library_tokenizer(monkeypatch, late=True)
    library = model.encode_text(sents)
    assert torch.equal(after, library)
    for i in range(len(holding)):
        assert not torch.equal(after[i], before[i]), sents[i]
    assert torch.equal(after[len(holding):], before[len(holding):])


def _pairs():
    sents = _sentences()
    a, b = sents[:32], sents[32:]
    return [[a[i], b[i]] if i % 2 else [b[i], a[(i * 7) % 32]] for i in range(32)]


def test_cross_encoder_predict_native_equals_library(monkeypatch):
    from text_similarity_amd.models.cross_encoder import CrossEncoder
    tok = _tokenizer()
    assert len(tok) <= presets.PRESETS[PRESET].vocab      # the preset's own word-embedding table holds every id
    pairs = _pairs()
    kw = dict(max_length=SEQ_MAX, max_tokens=4096, max_seqs=128)
    ident = torch.nn.Identity()
    native = CrossEncoder(PRESET, tokenizer=tok, **kw).predict(pairs, activation_fct=ident, convert_to_tensor=True)
    assert tok._tsim_native_wordpiece, "the native tokenizer was not in use"
    lib_tok = _library_tokenizer(monkeypatch)
    library = CrossEncoder(PRESET, tokenizer=lib_tok, **kw).predict(pairs, activation_fct=ident, convert_to_tensor=True)
    assert lib_tok._tsim_native_wordpiece is False
    assert native.shape == (32,) and torch.isfinite(native).all()
    assert torch.equal(native, library), [p for p, x, y in zip(pairs, native, library) if x != y][:5]


def test_word_encoder_spans_of_added_tokens_native_equals_library(monkeypatch):
    from text_similarity_amd.models import WordEncoder
    sents, words = [], []
    for c in tc.CONTENTS["H"]:
        for f in _changed_case(c) or [c]:
            sents += [f"the {f} and the", f"and {f} the {f}"]
            words += [[f], ["and", f, f]]
    tok = _tokenizer()
    added = tc.user_added_ids(tok)
    target_is_added = [bool(added & set(tok.encode(w, add_special_tokens=False))) for ws in words for w in ws]
    # the library's rule: a normalized=True content in another case IS its token, a normalized=False one ("ZZtop", "<ent>") is text
    flat_words = [w for ws in words for w in ws]
    assert target_is_added == [w != "and" and w.lower() not in ("zztop", "<ent>") for w in flat_words]
    assert sum(target_is_added) > len(flat_words) // 3
    model = _model(WordEncoder, tok)
    native, owner = model.encode_words(sents, words)
    assert tok._tsim_native_wordpiece, "the native tokenizer was not in use"
    model.params.tokenizer = _library_tokenizer(monkeypatch)
    library, owner_l = model.encode_words(sents, words)
    assert torch.equal(owner, owner_l) and native.shape == (len(target_is_added), 64)
    # a word that is in its sentence has a span: an empty span pools to a zero row
    empty = [i for i in range(len(native)) if not native[i].abs().sum() > 0]
    assert not empty, [(sents[int(owner[i])], i) for i in empty[:5]]
    assert torch.equal(native, library)
    np.testing.assert_array_equal(owner.cpu().numpy(), np.repeat(np.arange(len(sents)), [len(w) for w in words]))
