"""Native ASCII WordPiece tokenizer (csrc/wordpiece.cpp) against its oracle: the `tokenizers` library behind the
HuggingFace BertTokenizer the reference is configured with (sentence_encoder.py:144-153).  Host code only: runs without a GPU.
No published vocabulary ships with the reference or this image, so the vocabularies are generated here (whole words,
'##' continuations, single characters, punctuation): the ALGORITHM is what is compared, id for id."""
import numpy as np
import pytest

from text_similarity_amd import presets
from text_similarity_amd.models.sentence_encoder import _tokenize_library, _tokenize_packed
from text_similarity_amd.wordpiece import NativeWordPiece

transformers = pytest.importorskip("transformers")

import tokenizer_cases as tc                                                       # noqa: E402
from tokenizer_cases import HAND, piece_vocab as _piece_vocab, sentences as _sentences   # noqa: E402


def _tok(vocab, lower=True):
    return transformers.BertTokenizer(vocab=vocab, do_lower_case=lower)


@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("max_len", [256, 16, 3, 2])
def test_native_wordpiece_matches_the_library(lower, max_len):
    vocab, syll = _piece_vocab()
    tok = _tok(vocab, lower)
    wp = NativeWordPiece.from_tokenizer(tok)
    assert wp is not None, "BertTokenizer's backend must be recognised"
    docs = HAND + _sentences(syll, 1500, seed=11 + max_len)
    ref_flat, ref_lens = _tokenize_library(tok, docs, max_len, 64)
    flat, lens = wp.tokenize_packed(docs, max_len, lambda rest: _tokenize_library(tok, rest, max_len, 64))
    assert np.array_equal(lens, ref_lens)
    assert np.array_equal(flat, ref_flat)
    # ... and the native code did the work for the ASCII sentences without added-token text
    asc = [d for d in docs if d.isascii()]
    _, _, handled = wp.encode_ascii(asc, max_len)
    specials = ("[CLS]", "[SEP]", "[MASK]", "[UNK]", "[PAD]")
    assert [bool(h) for h in handled] == [not any(s in d for s in specials) for d in asc]
    assert handled.sum() > 1400


def test_every_sentence_alone_equals_the_batch():
    """No state leaks between sentences or threads: a batch equals its sentences tokenised one by one, on 1 and on 5 threads."""
    vocab, syll = _piece_vocab(seed=3)
    tok = _tok(vocab)
    wp = NativeWordPiece.from_tokenizer(tok)
    docs = [d for d in _sentences(syll, 700, seed=5) if d.isascii()]
    wp.threads = 5
    flat, lens, handled = wp.encode_ascii(docs, 64)
    assert handled.all()
    wp.threads = 1
    flat1, lens1, _ = wp.encode_ascii(docs, 64)
    assert np.array_equal(flat, flat1) and np.array_equal(lens, lens1)
    cu = np.concatenate([[0], np.cumsum(lens)])
    for i in range(0, len(docs), 37):
        one, l1, _ = wp.encode_ascii([docs[i]], 64)
        assert np.array_equal(one, flat[cu[i]:cu[i + 1]]) and l1[0] == lens[i]


def test_tokenize_packed_uses_the_native_path_and_the_bench_vocabulary(monkeypatch):
    """The benchmark's tokenizer (presets.synthetic_vocab: whole-word entries) through the product entry point, native on and
    off: same ids; an unsupported tokenizer keeps the library path."""
    tok = _tok(presets.synthetic_vocab(2000))
    docs = presets.synthetic_sentences(600, seed="wp-test", vocab_size=2000) + ["unknownword w00105", "w00110é"]
    flat, lens = _tokenize_packed(tok, docs, 32, 64)
    assert getattr(tok, "_tsim_native_wordpiece", None), "native tokenizer was not built for a BERT tokenizer"
    monkeypatch.setenv("TSIM_NATIVE_TOKENIZER", "0")
    tok2 = _tok(presets.synthetic_vocab(2000))
    flat2, lens2 = _tokenize_packed(tok2, docs, 32, 64)
    assert getattr(tok2, "_tsim_native_wordpiece", None) is False
    assert np.array_equal(flat, flat2) and np.array_equal(lens, lens2)

    class NotBert:
        is_fast = False
    assert NativeWordPiece.from_tokenizer(NotBert()) is None


def test_capacity_is_checked():
    import ctypes as C
    from text_similarity_amd import _lib
    vocab, _ = _piece_vocab()
    wp = NativeWordPiece.from_tokenizer(_tok(vocab))
    text = b"the and the"
    off = np.array([0, len(text)], dtype=np.int64)
    ids = np.empty(4, dtype=np.int32)
    lens = np.empty(1, dtype=np.int32)
    handled = np.empty(1, dtype=np.uint8)
    rc = _lib.lib().tsim_wordpiece_encode(wp._h, text, off.ctypes.data, 1, 64, 1, ids.ctypes.data, 4, lens.ctypes.data,
                                          handled.ctypes.data)
    assert rc == 3      # TSIM_ENOMEM: out_capacity below bytes + specials


def test_fuzz_ascii_strings_against_the_library():
    """Arbitrary 7-bit strings (every control character, runs of punctuation and blanks, long unbroken words): ids == library."""
    hypothesis = pytest.importorskip("hypothesis")
    from hypothesis import given, settings, strategies as st

    vocab, _ = _piece_vocab(seed=21)
    tok = _tok(vocab)
    wp = NativeWordPiece.from_tokenizer(tok)
    alphabet = st.characters(min_codepoint=0, max_codepoint=127)
    words = st.text(alphabet=st.sampled_from("abnerthstiquxz019 .,'-[]#\t\n\x00\x1f\x7f"), max_size=40)

    @settings(max_examples=150, deadline=None, database=None)
    @given(st.lists(st.one_of(st.text(alphabet=alphabet, max_size=120), words), min_size=1, max_size=12),
           st.sampled_from([4, 9, 64]))
    def run(docs, max_len):
        ref_flat, ref_lens = _tokenize_library(tok, docs, max_len, 64)
        flat, lens = wp.tokenize_packed(docs, max_len, lambda rest: _tokenize_library(tok, rest, max_len, 64))
        assert np.array_equal(lens, ref_lens) and np.array_equal(flat, ref_flat), docs

    run()


# ---- tokenizers with user-added tokens (tokenizer_cases: variants A..H) ----------------------------------------------------
def _native_and_library(tok, wp, docs, max_len):
    ref = _tokenize_library(tok, docs, max_len, 64)
    got = wp.tokenize_packed(docs, max_len, lambda rest: _tokenize_library(tok, rest, max_len, 64))
    return got, ref


def _rows(flat, lens):
    cu = np.concatenate([[0], np.cumsum(lens)])
    return [flat[cu[i]:cu[i + 1]] for i in range(len(lens))]


@pytest.mark.parametrize("lower", [True, False])
@pytest.mark.parametrize("variant", tc.VARIANTS)
def test_added_tokens_match_the_library(variant, lower):
    """Every added content in every letter case and placement (tokenizer_cases.content_texts) plus >= 500 clean sentences:
    ids and lengths equal the library's at max_len 4, 9 and 64.  The native path is still there and still does the clean
    sentences itself, and it hands every sentence in which the library matched an added token to the library."""
    vocab, syll = tc.matrix_vocab()
    tok = tc.make_tokenizer(variant, lower, vocab)
    wp = NativeWordPiece.from_tokenizer(tok)
    assert wp is not None, "a BertTokenizer with added tokens must keep its native path"
    texts = tc.matrix_texts(variant)
    clean = tc.clean_sentences(tok, syll, 500, seed=101)
    assert len(clean) >= 500 and all(s.isascii() for s in texts + clean)
    added_ids = np.fromiter(tc.user_added_ids(tok), dtype=np.int64)
    hit_any = False
    for max_len in tc.MAX_LENS:
        docs = texts + clean
        (flat, lens), (ref_flat, ref_lens) = _native_and_library(tok, wp, docs, max_len)
        bad = [docs[i] for i, (a, b) in enumerate(zip(_rows(flat, lens), _rows(ref_flat, ref_lens))) if not np.array_equal(a, b)]
        assert not bad, (variant, lower, max_len, len(bad), bad[:5])
        assert np.array_equal(lens, ref_lens) and np.array_equal(flat, ref_flat)
        _, _, handled = wp.encode_ascii(docs, max_len)
        lib_hit = np.array([bool(np.isin(r, added_ids).any()) for r in _rows(ref_flat, ref_lens)])
        # the generator's promise, checked against the library: no clean sentence holds an added token
        assert not lib_hit[len(texts):].any()
        assert handled[len(texts):].all(), [s for s, h in zip(clean, handled[len(texts):]) if not h][:5]
        missed = [d for d, h, hit in zip(docs, handled, lib_hit) if hit and h]
        assert not missed, (variant, lower, max_len, missed[:5])
        hit_any = hit_any or bool(lib_hit[:len(texts)].any())
    assert hit_any, "the texts never made the library emit an added token: the case tests nothing"


def test_matrix_texts_reach_the_library_facts():
    """The library facts the matrix rests on (measured with transformers 5 / tokenizers 0.22), so that a library that changes
    them is noticed here and not as a puzzling diff elsewhere."""
    def ids(tok, s):
        return tok(s)["input_ids"]

    a = tc.make_tokenizer("A", True)
    q = len(a) - 1
    assert ids(a, "the QQFOO and")[2] == q and ids(a, "the QQ\x01FOO and")[2] == q
    b = tc.make_tokenizer("B", True)
    assert ids(b, "the qqfoo and")[2] == len(b) - 1
    c = tc.make_tokenizer("C", True)
    y = len(c) - 1
    assert y in ids(c, "new\tyork") and y in ids(c, "new y\x01ork") and y not in ids(c, "NEW  york")
    d = tc.make_tokenizer("D", True)
    z = len(d) - 1
    assert z in ids(d, "ZZtop") and z not in ids(d, "zztop") and z not in ids(d, "ZZ\x01top")


def test_cache_is_rebuilt_when_a_token_is_added():
    """Through the product entry point: tokenise, add a token to the live tokenizer, tokenise again -> the library's ids."""
    vocab, syll = tc.matrix_vocab()
    tok = tc.make_tokenizer(None, True, vocab)
    docs = ["the QQFOO and", "qqfoo", "the Qq\x01Foo and the", "the and"] + tc.content_texts("new york")[:40] \
        + tc.clean_sentences(tok, syll, 100, seed=7)
    before = _tokenize_packed(tok, docs, 16, 64)
    first = tok._tsim_native_wordpiece
    assert first, "the native tokenizer was not built"
    ref0 = _tokenize_library(tok, docs, 16, 64)
    assert np.array_equal(before[0], ref0[0]) and np.array_equal(before[1], ref0[1])
    again = _tokenize_packed(tok, docs, 16, 64)
    assert tok._tsim_native_wordpiece is first, "an unchanged tokenizer must keep its native tokenizer"
    assert np.array_equal(again[0], before[0])
    assert tok.add_tokens(["qqfoo"]) == 1
    after = _tokenize_packed(tok, docs, 16, 64)
    ref1 = _tokenize_library(tok, docs, 16, 64)
    assert not np.array_equal(ref1[0], ref0[0]), "the added token changed nothing: the case tests nothing"
    assert np.array_equal(after[1], ref1[1]) and np.array_equal(after[0], ref1[0])
    assert tok._tsim_native_wordpiece and tok._tsim_native_wordpiece is not first
    # a second kind of change: an additional special token
    tok.add_special_tokens({"additional_special_tokens": ["<ent>"]})
    docs2 = docs + ["the <ent> and", "<ent>", "<ENT> the"]
    after2 = _tokenize_packed(tok, docs2, 16, 64)
    ref2 = _tokenize_library(tok, docs2, 16, 64)
    assert np.array_equal(after2[1], ref2[1]) and np.array_equal(after2[0], ref2[0])


def test_native_path_steps_aside_when_truncation_side_flips():
    vocab, syll = tc.matrix_vocab()
    tok = tc.make_tokenizer("A", True, vocab)
    docs = ["the and " * 10 + "qqfoo", "the QQFOO " + "and " * 12] + tc.clean_sentences(tok, syll, 100, seed=9)
    right = _tokenize_packed(tok, docs, 9, 64)
    assert tok._tsim_native_wordpiece
    tok.truncation_side = "left"
    left = _tokenize_packed(tok, docs, 9, 64)
    assert tok._tsim_native_wordpiece is False, "truncation on the left is the library's"
    enc = tok(text=docs, add_special_tokens=True, padding=False, truncation=True, max_length=9)["input_ids"]
    assert [list(r) for r in _rows(*left)] == [list(r) for r in enc]
    assert not np.array_equal(left[0], right[0])
    tok.truncation_side = "right"
    back = _tokenize_packed(tok, docs, 9, 64)
    assert tok._tsim_native_wordpiece
    assert np.array_equal(back[0], right[0]) and np.array_equal(back[1], right[1])


@pytest.mark.parametrize("preset_truncation", [False, True])
@pytest.mark.parametrize("L", [3, 16, 256])
def test_tokenize_library_equals_the_tokenizer_call(L, preset_truncation):
    """_tokenize_library's backend ``encode_batch`` route against the call it replaces, and the backend's own truncation and
    padding settings as they were before, whether truncation was enabled beforehand or not."""
    vocab, syll = tc.matrix_vocab()
    tok = tc.make_tokenizer("H", True, vocab)
    assert tok.is_fast and hasattr(tok.backend_tokenizer, "encode_batch")
    bt = tok.backend_tokenizer
    if preset_truncation:
        bt.enable_truncation(max_length=7, stride=1, strategy="only_first", direction="left")
        bt.enable_padding(length=11, direction="left", pad_id=0, pad_token="[PAD]")
    else:
        bt.no_truncation()
        bt.no_padding()
    trunc0, pad0 = bt.truncation, bt.padding
    assert (trunc0 is not None) == preset_truncation and (pad0 is not None) == preset_truncation
    docs = HAND + tc.matrix_texts("H")[:200] + _sentences(syll, 300, seed=77)
    flat, lens = _tokenize_library(tok, docs, L, 64)
    assert bt.truncation == trunc0 and bt.padding == pad0
    enc = tok(text=docs, add_special_tokens=True, padding=False, truncation=True, max_length=L)["input_ids"]
    assert lens.tolist() == [len(r) for r in enc]
    assert flat.tolist() == [t for r in enc for t in r]
    assert int(lens.max()) <= L
