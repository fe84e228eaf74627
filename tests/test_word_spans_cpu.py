"""Word-to-token alignment and the span table of the word-in-context path (text_similarity_amd/word_spans.py), and the
declaration of its C entry point.  Host code only: runs without a GPU.

The expected positions are written down by hand from the tokenisation (every sentence is `[CLS] tokens [SEP]`, so the first
word's first token is position 1); nothing here is computed by the code under test."""
import os
import re

import numpy as np
import pytest

from text_similarity_amd import _lib, presets, word_spans

transformers = pytest.importorskip("transformers")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(REPO, "include", "tsim.h")


def _piece_vocab():
    """A small hand-written vocabulary with '##' pieces."""
    vocab = {"[PAD]": 0, "[UNK]": 1, "[CLS]": 2, "[SEP]": 3, "[MASK]": 4}
    for k in ("the", "river", "bank", "was", "flab", "##berg", "##ast", "##ed", "em", "##bed", "##ding", "##s", "by", "a",
              "play", "##ing", "we", "saw", "near"):
        vocab[k] = len(vocab)
    return vocab


@pytest.fixture(scope="module")
def tok():
    return transformers.BertTokenizer(vocab=_piece_vocab(), do_lower_case=True)


@pytest.fixture(scope="module")
def syn_tok():
    return transformers.BertTokenizer(vocab=presets.synthetic_vocab(2000), do_lower_case=True)


def _ids(tokenizer, sentence, max_length=None):
    if max_length is None:
        return tokenizer.encode(sentence, add_special_tokens=True)
    return tokenizer.encode(sentence, add_special_tokens=True, truncation=True, max_length=max_length)


def test_special_layout_and_word_ids(tok, syn_tok):
    assert word_spans.special_layout(tok) == (1, 1)
    assert word_spans.special_layout(syn_tok) == (1, 1)
    v = _piece_vocab()
    assert word_spans.word_ids(tok, "embeddings") == [v["em"], v["##bed"], v["##ding"], v["##s"]]
    assert word_spans.word_ids(tok, "bank") == [v["bank"]]
    assert word_spans.word_ids(tok, "") == []
    assert word_spans.word_ids(syn_tok, "w00500") == [500]


def test_words_at_start_middle_and_end_synthetic_vocabulary(syn_tok):
    sent = "w00200 w00300 w00400 w00500 w00600"
    ids = _ids(syn_tok, sent)
    assert ids == [101, 200, 300, 400, 500, 600, 102]
    assert word_spans.spans_for_sentence(syn_tok, ids, ["w00200"]) == [[1]]
    assert word_spans.spans_for_sentence(syn_tok, ids, ["w00400"]) == [[3]]
    assert word_spans.spans_for_sentence(syn_tok, ids, ["w00600"]) == [[5]]
    assert word_spans.spans_for_sentence(syn_tok, ids, ["w00200", "w00400", "w00600"]) == [[1], [3], [5]]
    # the running position: a word in front of the previous match is not found any more (empty span), the next one still is
    assert word_spans.spans_for_sentence(syn_tok, ids, ["w00400", "w00200", "w00600"]) == [[3], [], [5]]


def test_second_request_finds_the_second_occurrence(tok):
    ids = _ids(tok, "the bank by the river bank")          # [CLS] the bank by the river bank [SEP]
    assert word_spans.spans_for_sentence(tok, ids, ["bank", "bank"]) == [[2], [6]]
    assert word_spans.spans_for_sentence(tok, ids, ["the", "the", "the"]) == [[1], [4], []]
    assert word_spans.spans_for_sentence(tok, ids, ["river", "bank"]) == [[5], [6]]


def test_multi_piece_words(tok):
    ids = _ids(tok, "the embeddings flabbergasted a bank")
    # [CLS] the em ##bed ##ding ##s flab ##berg ##ast ##ed a bank [SEP]
    assert len(ids) == 13
    assert word_spans.spans_for_sentence(tok, ids, ["embeddings"]) == [[2, 3, 4, 5]]
    assert word_spans.spans_for_sentence(tok, ids, ["flabbergasted", "bank"]) == [[6, 7, 8, 9], [11]]
    # the word alone is what is searched: "bed" is not a token of this sentence although "##bed" is
    assert word_spans.spans_for_sentence(tok, ids, ["the", "embeddings", "flabbergasted", "a", "bank"]) == \
        [[1], [2, 3, 4, 5], [6, 7, 8, 9], [10], [11]]


def test_absent_and_empty_words_give_empty_spans(tok):
    ids = _ids(tok, "the river was near")
    assert word_spans.spans_for_sentence(tok, ids, ["bank"]) == [[]]
    assert word_spans.spans_for_sentence(tok, ids, ["", "river"]) == [[], [2]]         # tokenises to nothing: no TypeError
    assert word_spans.spans_for_sentence(tok, ids, ["bank", "river", "zzz"]) == [[], [2], []]   # an absent word does not move the cursor
    assert word_spans.align_words(ids, [[]]) == [[]]
    assert word_spans.align_words([], [[5]]) == [[]]


def test_word_cut_by_truncation_keeps_the_surviving_positions(tok):
    full = _ids(tok, "we saw the embeddings")               # [CLS] we saw the em ##bed ##ding ##s [SEP]
    assert len(full) == 9
    cut = _ids(tok, "we saw the embeddings", max_length=7)   # [CLS] we saw the em ##bed [SEP]
    v = _piece_vocab()
    assert cut == [2, v["we"], v["saw"], v["the"], v["em"], v["##bed"], 3]
    assert word_spans.spans_for_sentence(tok, cut, ["embeddings"], max_length=7) == [[4, 5]]
    assert word_spans.spans_for_sentence(tok, cut, ["the", "embeddings"], max_length=7) == [[3], [4, 5]]
    # not truncated (no max_length, or a longer one): a partial match is not a match
    assert word_spans.spans_for_sentence(tok, cut, ["embeddings"]) == [[]]
    assert word_spans.spans_for_sentence(tok, cut, ["embeddings"], max_length=8) == [[]]
    # a word that was cut off entirely is absent; the whole word in a truncated sentence is found as usual
    cut4 = _ids(tok, "we saw the embeddings", max_length=5)  # [CLS] we saw the [SEP]
    assert word_spans.spans_for_sentence(tok, cut4, ["embeddings"], max_length=5) == [[]]
    assert word_spans.spans_for_sentence(tok, cut4, ["saw"], max_length=5) == [[2]]
    # the surviving prefix must end where the content ends: "em ##bed" in the middle of a truncated sentence is not the word
    mid = [2, v["em"], v["##bed"], v["the"], v["we"], v["saw"], 3]
    assert word_spans.align_words(mid, [[v["em"], v["##bed"], v["##ding"], v["##s"]]], truncated=True) == [[]]


def test_native_wordpiece_tokenizer_gives_the_same_alignment():
    """The native ASCII WordPiece tokenizer (NativeWordPiece) as the tokenizer object: same ids, same positions."""
    from text_similarity_amd.wordpiece import NativeWordPiece
    if not os.path.exists(_lib.LIB_PATH):
        from text_similarity_amd.build import build
        build(verbose=False)
    wp = NativeWordPiece.from_tokenizer(transformers.BertTokenizer(vocab=_piece_vocab(), do_lower_case=True))
    assert wp is not None
    assert word_spans.special_layout(wp) == (1, 1)
    v = _piece_vocab()
    assert word_spans.word_ids(wp, "embeddings") == [v["em"], v["##bed"], v["##ding"], v["##s"]]
    ids, lens, handled = wp.encode_ascii(["the embeddings flabbergasted a bank"], 64)
    assert handled.all() and lens[0] == 13
    assert word_spans.spans_for_sentence(wp, ids, ["embeddings", "bank"]) == [[2, 3, 4, 5], [11]]


def test_explicit_positions_pass_through_unchanged():
    import torch
    given = [[3, 1, 1], np.array([7, 2]), torch.tensor([0]), [], (5, 4), 9]
    assert word_spans.explicit_positions(given) == [[3, 1, 1], [7, 2], [0], [], [5, 4], [9]]
    # no range check on the host: the device clamps and flags
    assert word_spans.explicit_positions([[-1, 10 ** 6]]) == [[-1, 10 ** 6]]


def test_span_table_csr_assembly():
    batch = [
        [[1], [2, 3]],                                  # two spans
        [],                                             # a sentence without a span
        [[4, 4, 1], [], [0], [9, 2], [5, 6, 7, 8]],     # five spans: a repeat, an empty one, CLS, out of order, a run
        [[2]],
    ]
    seq, cu, tok = word_spans.span_table(batch)
    assert seq.dtype == cu.dtype == tok.dtype == np.int32
    assert seq.tolist() == [0, 0, 2, 2, 2, 2, 2, 3]
    assert cu.tolist() == [0, 1, 3, 6, 6, 7, 9, 13, 14]
    assert tok.tolist() == [1, 2, 3, 4, 4, 1, 0, 9, 2, 5, 6, 7, 8, 2]
    for s in range(len(seq)):      # every span reads back as it was given
        flat = [sp for spans in batch for sp in spans]
        assert tok[cu[s]:cu[s + 1]].tolist() == flat[s]
    seq0, cu0, tok0 = word_spans.span_table([[], []])
    assert seq0.shape == (0,) and cu0.tolist() == [0] and tok0.shape == (0,)
    # a position beyond int32 stays out of range instead of wrapping into it
    assert word_spans.span_table([[[2 ** 32 + 1, -2 ** 40]]])[2].tolist() == [2 ** 31 - 1, -2 ** 31]


def test_header_declares_and_lib_binds_the_entry_point():
    hdr = open(HDR).read()
    assert "tsim_encoder_forward_spans(" in hdr
    m = re.search(r"#define\s+TSIM_ENC_ERR_SPAN\s+(\d+)", hdr)
    assert m, "TSIM_ENC_ERR_SPAN is not defined"
    bit = int(m.group(1))
    others = [int(v) for v in re.findall(r"#define\s+TSIM_ENC_ERR_(?!SPAN)[A-Z_]+\s+(\d+)", hdr)]
    assert bit & (bit - 1) == 0 and bit not in others, (bit, others)       # a new bit of the flag word
    assert _lib.ENC_ERR_SPAN == bit
    assert "tsim_encoder_forward_spans" in _lib.DECLARED_SYMBOLS
    from text_similarity_amd.native_encoder import NativeEncoder
    assert bit in NativeEncoder.ERR_BITS and callable(NativeEncoder.forward_spans)
    # the signature bound is the one declared: the arguments of tsim_encoder_forward_ex, then nine span arguments and the stream
    res, args = _lib._SIGS["tsim_encoder_forward_spans"]
    ex = _lib._SIGS["tsim_encoder_forward_ex"][1]
    assert args[:len(ex) - 1] == ex[:-1] and len(args) == len(ex) + 9
    decl = re.search(r"int tsim_encoder_forward_spans\((.*?)\);", hdr, re.S).group(1)
    assert len(decl.split(",")) == len(args)
    if not os.path.exists(_lib.LIB_PATH):
        from text_similarity_amd.build import build
        build(verbose=False)
    L = _lib.lib()
    assert L.tsim_encoder_forward_spans.argtypes is not None
    # refused before any launch: spans without an encoder, a negative span count
    assert L.tsim_encoder_forward_spans(*([None] * 6), 0, 0, 0, None, None, 0, None, None, None, None, None, None, 1, 0,
                                        None, None, 0, None, None) == 1
    assert L.tsim_encoder_forward_spans(*([None] * 6), 0, 0, 0, None, None, 0, None, None, None, None, None, None, -1, 0,
                                        None, None, 0, None, None) == 1


def test_word_encoder_is_exported_and_needs_a_gpu():
    import torch
    from text_similarity_amd.models import WordEncoder
    from text_similarity_amd.models.sentence_encoder import SentenceTransformerWrapper
    assert issubclass(WordEncoder, SentenceTransformerWrapper)
    for name in ("encode_words", "encode_word_pairs", "from_preset", "from_pretrained", "encode_text"):
        assert callable(getattr(WordEncoder, name)), name
    if not torch.cuda.is_available():
        from text_similarity_amd.configurations.config import Configuration, ModelParameters
        params = Configuration(model_parameters=ModelParameters("tiny-bert"), model="tiny-bert", save_path="",
                               device=torch.device("cpu"))
        with pytest.raises(_lib.TsimError):
            WordEncoder.from_preset("tiny-bert", params)


@pytest.mark.parametrize("lower", [True, False])
def test_word_ids_of_added_tokens_in_any_case_equal_the_library(lower):
    """A target word that is an added token written in another letter case: the library matches normalized=True tokens on the
    normalised text, so the native tokenizer must hand such a word to the library and not cut it into word pieces."""
    import tokenizer_cases as tc
    from text_similarity_amd.wordpiece import NativeWordPiece
    if not os.path.exists(_lib.LIB_PATH):
        from text_similarity_amd.build import build
        build(verbose=False)
    vocab, _ = tc.matrix_vocab()
    for variant in tc.VARIANTS:
        tok = tc.make_tokenizer(variant, lower, vocab)
        wp = NativeWordPiece.from_tokenizer(tok)
        assert wp is not None
        added = tc.user_added_ids(tok)
        hits = 0
        for content in tc.every_content():
            for w in tc.case_forms(content) + [content[:2] + "\x01" + content[2:], content.replace(" ", "\t")]:
                want = tok.encode(w, add_special_tokens=False)
                assert word_spans.word_ids(wp, w) == want, (variant, lower, w)
                assert word_spans.word_ids(tok, w) == want
                hits += bool(added & set(want))
        assert hits >= len(tc.CONTENTS[variant]), (variant, hits)     # at least each of its own contents as written
