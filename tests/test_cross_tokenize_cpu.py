"""Pair tokenisation of the cross-encoder (models/cross_encoder.PairTokenizer) against the library it restates:
``tokenizer(list_a, list_b, truncation=True, max_length=L)`` of a HuggingFace BertTokenizer (the call a
sentence_transformers CrossEncoder makes).  Host code only: runs without a GPU.  The pairs are assembled from each unique
string's single-sentence ids (native WordPiece for ASCII, the library for the rest), so this pins the template, the token
types and the ``longest_first`` truncation rule."""
import numpy as np
import pytest

from text_similarity_amd import presets
from text_similarity_amd.models.cross_encoder import PairTokenizer, longest_first

transformers = pytest.importorskip("transformers")

VOCAB = presets.synthetic_vocab(4000)


def _tok():
    vocab = dict(VOCAB)
    for ch in ("中", "文"):   # non-ASCII pieces in the vocabulary (such strings go through the library fallback)
        vocab[ch] = len(vocab)
    return transformers.BertTokenizer(vocab=vocab)


def _words(n, off):
    return " ".join(f"w{104 + (off * 37 + i * 11) % 3800:05d}" for i in range(n))


def _library(tok, pairs, L):
    enc = tok([a for a, _ in pairs], [b for _, b in pairs], truncation=True, max_length=L)
    return (np.concatenate([np.asarray(x, np.int64) for x in enc["input_ids"]]),
            np.concatenate([np.asarray(x, np.int64) for x in enc["token_type_ids"]]),
            np.asarray([len(x) for x in enc["input_ids"]]))


def _pairs():
    q = [_words(n, o) for o, n in enumerate((1, 3, 7, 12, 40))]
    t = [_words(n, 100 + o) for o, n in enumerate((0, 2, 5, 12, 30, 90))]
    pairs = [[a, b] for a in q for b in t]                               # both long, one long, equal lengths, short
    pairs += [[q[2], t[3]], [q[2], t[3]], [q[0], q[0]]]                    # duplicate queries and identical halves
    pairs += [["", t[2]], [q[1], ""], ["", ""]]                             # empty strings
    pairs += [["é " + _words(4, 7), t[4]], [q[3], "中文 " + _words(9, 8) + " ü"], ["ü", "é"]]   # non-ASCII (library)
    return pairs


@pytest.mark.parametrize("L", [4, 5, 6, 7, 8, 11, 16, 17, 33, 64, 512])
def test_pairs_equal_library(L):
    tok = _tok()
    pt = PairTokenizer(tok, 512)
    pairs = _pairs()
    ids, types, lens = pt(pairs, max_length=L)
    r_ids, r_types, r_lens = _library(tok, pairs, L)
    np.testing.assert_array_equal(lens, r_lens)
    np.testing.assert_array_equal(ids, r_ids)
    np.testing.assert_array_equal(types, r_types)


def test_longest_first_rule_pinned():
    """The rule as the library applies it, over every pair of segment lengths up to 14 and every budget up to 20;
    e.g. 10 + 10 text tokens into a 5-token budget -> (2, 3), into 13 -> (6, 7): the second segment gets the odd token."""
    tok = _tok()
    la, lb, budgets, got_a, got_b = [], [], [], [], []
    for L in range(3, 24):
        pairs, ns = [], []
        for n1 in range(1, 15):
            for n2 in range(1, 15):
                pairs.append([_words(n1, 1), _words(n2, 2)])
                ns.append((n1, n2))
        enc = tok([a for a, _ in pairs], [b for _, b in pairs], truncation=True, max_length=L)
        for (n1, n2), tt in zip(ns, enc["token_type_ids"]):
            tt = np.asarray(tt)
            la.append(n1)
            lb.append(n2)
            budgets.append(L - 3)
            got_a.append(int((tt == 0).sum()) - 2)
            got_b.append(int((tt == 1).sum()) - 1)
    la, lb, budgets = map(np.asarray, (la, lb, budgets))
    for bgt in np.unique(budgets):
        m = budgets == bgt
        ka, kb = longest_first(la[m], lb[m], int(bgt))
        np.testing.assert_array_equal(ka, np.asarray(got_a)[m])
        np.testing.assert_array_equal(kb, np.asarray(got_b)[m])
    assert tuple(int(x) for x in longest_first([10], [10], 5)) == (2, 3)
    assert tuple(int(x) for x in longest_first([10], [10], 13)) == (6, 7)


def test_unique_strings_tokenised_once(monkeypatch):
    from text_similarity_amd.models import cross_encoder as ce
    tok = _tok()
    pt = PairTokenizer(tok, 64)
    seen = []
    real = ce._tokenize_packed

    def spy(tokenizer, docs, max_len, batch):
        seen.append(list(docs))
        return real(tokenizer, docs, max_len, batch)

    monkeypatch.setattr(ce, "_tokenize_packed", spy)
    q = [_words(5, i) for i in range(3)]
    t = [_words(9, 50 + i) for i in range(20)]
    pt([[a, b] for a in q for b in t])
    assert len(seen) == 1 and sorted(seen[0]) == sorted(set(q + t))


def test_non_bert_template_is_refused():
    from tokenizers import processors
    tok = _tok()
    cls, sep = tok.cls_token_id, tok.sep_token_id
    # RoBERTa-style pair template: [CLS] a [SEP] [SEP] b [SEP]
    tok.backend_tokenizer.post_processor = processors.TemplateProcessing(
        single="[CLS] $A [SEP]", pair="[CLS] $A [SEP] [SEP] $B:1 [SEP]:1", special_tokens=[("[CLS]", cls), ("[SEP]", sep)])
    with pytest.raises(ValueError, match="template"):
        PairTokenizer(tok, 128)


def test_max_length_below_four_is_refused():
    with pytest.raises(ValueError):
        PairTokenizer(_tok(), 3)


def _added_tok():
    from tokenizers import AddedToken
    tok = _tok()
    tok.add_tokens(["qqfoo", "QQbar", "new york", AddedToken("ZZtop", normalized=False)])
    return tok


def _added_pairs():
    """Segments that hold the added contents in changed case, glued, cut by a control character, with other white space."""
    import tokenizer_cases as tc
    segs = []
    for c in ("qqfoo", "QQbar", "new york", "ZZtop"):
        for f in tc.case_forms(c):
            segs += [f, _words(3, 5) + " " + f, f + " " + _words(6, 9), _words(2, 1) + " " + f + ", " + f + " " + _words(9, 4),
                     "x" + f + "y " + _words(2, 3), f[:2] + "\x01" + f[2:] + " " + _words(4, 6), f.replace(" ", "\t")]
    plain = [_words(n, 40 + n) for n in (1, 4, 11)]
    pairs = [[a, b] for a in segs[::3] for b in plain] + [[a, b] for a in plain for b in segs[1::3]]
    pairs += [[a, b] for a, b in zip(segs, segs[5:] + segs[:5])]
    return pairs


@pytest.mark.parametrize("L", [9, 64])
def test_pairs_with_added_tokens_equal_library(L):
    """A tokenizer with user-added tokens: the library matches them on the normalised text, so a segment that holds one in
    another letter case must come out with the added id (and ``longest_first`` must count ONE token for it)."""
    tok = _added_tok()
    pt = PairTokenizer(tok, 512)
    assert tok._tsim_native_wordpiece, "the native single-sentence path must stay in use"
    pairs = _added_pairs()
    ids, types, lens = pt(pairs, max_length=L)
    r_ids, r_types, r_lens = _library(tok, pairs, L)
    added = np.fromiter(set(tok.added_tokens_decoder) - {tok.cls_token_id, tok.sep_token_id, tok.unk_token_id}, dtype=np.int64)
    assert np.isin(r_ids, added).sum() > len(pairs) // 2, "the pairs hardly hold an added token: the case tests nothing"
    np.testing.assert_array_equal(lens, r_lens)
    np.testing.assert_array_equal(ids, r_ids)
    np.testing.assert_array_equal(types, r_types)
