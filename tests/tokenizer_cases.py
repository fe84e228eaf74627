"""Tokenizers with user-added tokens and the texts that probe them, shared by the tokenizer tests (test_wordpiece_cpu.py,
test_wordpiece_sanitizer_cpu.py, test_cross_tokenize_cpu.py, test_word_spans_cpu.py, test_tokenizer_boundary_gpu.py).

The `tokenizers` library matches a ``normalized=True`` added token (the default of ``add_tokens``) on the NORMALISED text and
normalises the token's content too; a ``normalized=False`` one (the special tokens) on the raw text.  The variants below cover
both kinds, contents that change under normalisation, a blank or punctuation inside a content, and the ``single_word`` /
``lstrip`` / ``rstrip`` flags; the texts put every content, in every letter case, where a matcher can go wrong.  Everything is
deterministic: no random source besides the seeded generators."""
import random
import string

import pytest

transformers = pytest.importorskip("transformers")

PUNCT = "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~"


def piece_vocab(seed=7, n_words=3000, n_cont=1500):
    rng = random.Random(seed)
    vocab = {"[PAD]": 0}
    for i in range(1, 100):
        vocab[f"[unused{i}]"] = i
    vocab["[UNK]"], vocab["[CLS]"], vocab["[SEP]"], vocab["[MASK]"] = 100, 101, 102, 103

    def add(k):
        if k not in vocab:
            vocab[k] = len(vocab)

    for c in string.ascii_lowercase + string.digits:      # single characters, but not every continuation: some words -> [UNK]
        add(c)
    for c in "aeiourstln0123":
        add("##" + c)
    for c in PUNCT:
        if c not in "^~`":                                   # some punctuation is out of vocabulary
            add(c)
    syll = ["ab", "an", "ing", "er", "th", "on", "re", "st", "en", "qu", "ly", "tion", "un", "pre", "x", "zz", "the", "and"]
    for _ in range(n_words):
        add("".join(rng.choice(syll) for _ in range(rng.randint(1, 4))))
    for _ in range(n_cont):
        add("##" + "".join(rng.choice(syll) for _ in range(rng.randint(1, 3))))
    add("##")                                                # degenerate keys the matcher must not trip over
    add("a" * 101)
    return vocab, syll


def sentences(syll, n, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        words = []
        for _ in range(rng.randint(0, 40)):
            r = rng.random()
            if r < 0.6:
                w = "".join(rng.choice(syll) for _ in range(rng.randint(1, 5)))
            elif r < 0.7:
                w = "".join(rng.choice(string.ascii_letters + string.digits) for _ in range(rng.randint(1, 12)))
            elif r < 0.8:
                w = rng.choice(PUNCT) * rng.randint(1, 3)
            elif r < 0.9:
                w = rng.choice(syll) + rng.choice(PUNCT) + rng.choice(syll)
            else:
                w = rng.choice(syll).upper() + rng.choice(["", "'s", "-", "..."])
            words.append(w)
        sep = rng.choice([" ", "  ", "\t", "\n", " \r\n "])
        out.append(sep.join(words))
    return out


HAND = [
    "", " ", "\t\n", "a", "A", "the", "THE and The", "hello, world!", "x" * 100, "x" * 101, "a" * 101, "ab" * 60,
    "tab\tseparated\nlines\r\nhere", "ctrl\x01chars\x1fin\x7fside", "nul\x00byte", "vertical\x0btab form\x0cfeed",
    "don't stop-me_now (ever) [really] {no}", "a.b.c...d", "##ing ## #", "^caret~tilde`tick", "price: $5.00 + 10% = ?",
    "[CLS] literal special", "ends with [SEP]", "mask [MASK] here", "[unused5] is plain text", "[UNK]", "[ CLS ]",
    "café au lait", "你好 world", "emoji \U0001f600 ok", "naïve", "zero​width",
    " leading and trailing ", "MiXeD CaSe WoRdS", "9 99 999 9999a a9999", "ing", "thethethe", "unprequ" * 20,
]

# ---- the matrix ---------------------------------------------------------------------------------------------------------
VARIANTS = ("A", "B", "C", "D", "E", "F", "G", "H")
# variant -> the contents it adds (what the texts are built around)
CONTENTS = {
    "A": ["qqfoo"],
    "B": ["QQfoo"],                      # the content itself changes under lower-casing
    "C": ["new york"],                   # a blank inside the content
    "D": ["ZZtop"],                      # normalized=False: raw text only
    "E": ["qqfoo", "new york", "zztop"],  # single_word / lstrip / rstrip, one of each
    "F": ["<ent>"],                      # an additional special token
    "G": ["c++", "[x]"],                 # punctuation inside the content
    "H": ["QQfoo", "new york", "ZZtop", "abzz", "c++", "<ent>"],
}
MAX_LENS = (4, 9, 64)


def matrix_vocab(n_words=3000, n_cont=1500):
    """piece_vocab plus the pieces the added contents fall into WITHOUT their added token, so that a native path that misses
    a token returns plausible ids (``qq ##foo``), not [UNK].  With (300, 150) it stays below the 1000 rows of the tiny presets'
    word-embedding table, added tokens included."""
    vocab, syll = piece_vocab(n_words=n_words, n_cont=n_cont)
    for k in ("qq", "##foo", "new", "york", "##top", "ent", "abzz"):
        if k not in vocab:
            vocab[k] = len(vocab)
    return vocab, syll


def make_tokenizer(variant, lower, vocab=None):
    from tokenizers import AddedToken
    tok = transformers.BertTokenizer(vocab=dict(vocab if vocab is not None else matrix_vocab()[0]), do_lower_case=lower)
    if variant == "A":
        tok.add_tokens(["qqfoo"])
    elif variant == "B":
        tok.add_tokens(["QQfoo"])
    elif variant == "C":
        tok.add_tokens(["new york"])
    elif variant == "D":
        tok.add_tokens([AddedToken("ZZtop", normalized=False)])
    elif variant == "E":
        tok.add_tokens([AddedToken("qqfoo", single_word=True), AddedToken("new york", lstrip=True),
                        AddedToken("zztop", rstrip=True)])
    elif variant == "F":
        tok.add_special_tokens({"additional_special_tokens": ["<ent>"]})
    elif variant == "G":
        tok.add_tokens(["c++", "[x]"])
    elif variant == "H":
        tok.add_tokens(["QQfoo", "new york", AddedToken("ZZtop", normalized=False), AddedToken("abzz", single_word=True), "c++"])
        tok.add_special_tokens({"additional_special_tokens": ["<ent>"]})
    elif variant is not None:
        raise ValueError(variant)
    return tok


def case_forms(content):
    """The content as written, in lower, upper and mixed case (every other letter swapped)."""
    mixed = "".join(c.swapcase() if i % 2 == 0 else c for i, c in enumerate(content))
    return list(dict.fromkeys([content, content.lower(), content.upper(), mixed, mixed.swapcase()]))


def content_texts(content):
    """Every case form of ``content``: alone, at the start and the end, glued inside a longer word, next to punctuation, twice,
    cut through by NUL / 0x01 / DEL, with other white space where it has a blank, and straddling the truncation point of
    each of MAX_LENS (``the`` is one token: the content's first piece lands at positions room-2 .. room+1)."""
    out = []
    for f in case_forms(content):
        out += [f, f + " the and", "the and " + f, " " + f + " ", "the " + f + " and"]
        out += ["x" + f + "y", "un" + f, f + "ing", "the pre" + f + "s and", f + f]
        out += ["(" + f + ")", f + ",", "." + f + "!", "the-" + f + "-and", "'" + f + "'s", "#" + f, f + "+"]
        out += [f + " and " + f, f + " " + f, "the " + f + ", " + f.swapcase() + "."]
        half = max(len(f) // 2, 1)
        for ch in ("\x00", "\x01", "\x7f"):
            out += [f[:half] + ch + f[half:], "the " + f[:1] + ch + f[1:] + " and", ch + f + ch, "the" + ch + f]
        if " " in f:
            for ws in ("\t", "\r\n", "  ", "\n", " \t "):
                out += [f.replace(" ", ws), "the " + f.replace(" ", ws) + " and"]
        for max_len in MAX_LENS:
            room = max_len - 2
            for lead in range(max(room - 2, 0), room + 2):
                out.append("the " * lead + f + " and the")
    return out


def matrix_texts(variant):
    out = []
    for c in CONTENTS[variant]:
        out += content_texts(c)
    return list(dict.fromkeys(out))


def every_content():
    return list(dict.fromkeys(c for v in VARIANTS for c in CONTENTS[v]))


def added_contents(tok):
    """Contents of every added token of ``tok`` (special ones included), as written."""
    return [t.content for t in tok.added_tokens_decoder.values()]


def user_added_ids(tok):
    """Ids the library emits only for a MATCHED added token: every added id except [CLS] / [SEP] (the template's) and [UNK]
    (also the model's answer to an unknown word)."""
    return set(tok.added_tokens_decoder) - {tok.cls_token_id, tok.sep_token_id, tok.unk_token_id}


def clean_sentences(tok, syll, n, seed):
    """At least ``n`` generated ASCII sentences that hold no added content of ``tok``, neither in their raw text nor in their
    normalised text, for the content as written, lower-cased, and as the library's normaliser rewrites it."""
    norm = tok.backend_tokenizer.normalizer.normalize_str
    needles = set()
    for c in added_contents(tok):
        needles.update((c, c.lower(), norm(c)))
    needles.discard("")
    out = []
    for s in sentences(syll, 2 * n, seed):
        if not s.isascii():
            continue
        views = (s, s.lower(), norm(s))
        if any(nd in v for nd in needles for v in views):
            continue
        out.append(s)
    assert len(out) >= n, (len(out), n)
    return out
