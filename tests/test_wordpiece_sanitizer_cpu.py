"""The host tokenizer (csrc/wordpiece.cpp) under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program.

wordpiece.cpp walks raw byte ranges with caller-given offsets and capacities.  tests/wordpiece_driver.cpp (its own ``main``)
is compiled together with it by the host ``g++`` with the sanitizers on, fed case files, and must exit 0 without a sanitizer
report and print exactly what the Python binding (the product build of the same source) returns for the same case.  Host
code only: nothing is loaded into the Python process, no GPU is involved, and the test is not marked ``gpu``."""
import os
import shutil
import struct
import subprocess

import pytest

from text_similarity_amd.wordpiece import NativeWordPiece

transformers = pytest.importorskip("transformers")

import tokenizer_cases as tc    # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread"]
# a report of either sanitizer (a leaked handle included) ends the run with a non-zero status
SAN_ENV = {"ASAN_OPTIONS": "abort_on_error=0:detect_leaks=1:exitcode=23", "UBSAN_OPTIONS": "print_stacktrace=1"}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no host g++")
    out = tmp_path_factory.mktemp("wp_driver")
    probe = out / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([gxx, *FLAGS, str(probe), "-o", str(out / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(out / "probe")], capture_output=True).returncode != 0:
        pytest.skip("g++ cannot build or run a program with -fsanitize=address,undefined (sanitizer runtime missing): "
                    + (r.stderr.strip().splitlines() or ["?"])[-1])
    exe = out / "wordpiece_driver"
    r = subprocess.run([gxx, *FLAGS, "-I" + os.path.join(REPO, "include"), os.path.join(REPO, "tests", "wordpiece_driver.cpp"),
                        os.path.join(REPO, "text_similarity_amd", "csrc", "wordpiece.cpp"), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return str(exe)


def _blob(b):
    return struct.pack("<i", len(b)) + b


def _write_case(path, args, docs, max_len, threads, exact):
    parts = [b"WPC1", struct.pack("<6i", int(args["lowercase"]), args["max_chars"], args["unk_id"], max_len, threads, int(exact)),
             _blob(args["continuing_prefix"].encode())]
    for ids in (args["prefix_ids"], args["suffix_ids"]):
        parts.append(struct.pack(f"<i{len(ids)}i", len(ids), *ids))
    for strings in (args["vocab"], args["added"]):
        parts.append(struct.pack("<i", len(strings)))
        parts += [_blob(s.encode("utf-8")) for s in strings]
    parts.append(struct.pack("<q", len(docs)))
    parts += [_blob(d.encode("ascii")) for d in docs]
    with open(path, "wb") as f:
        f.write(b"".join(parts))


def _expected(wp, docs, max_len, threads):
    wp.threads = threads
    flat, lens, handled = wp.encode_ascii(docs, max_len)
    lines, o = ["create 0", "encode 0"], 0
    for i, (n, h) in enumerate(zip(lens, handled)):
        lines.append(f"{i} {int(n)} {int(h)}:" + "".join(f" {int(t)}" for t in flat[o:o + n]))
        o += int(n)
    return "\n".join(lines) + "\n"


def _run(driver, tmp_path, name, tok, docs, max_len, threads, exact=False):
    args = NativeWordPiece.create_args(tok)
    wp = NativeWordPiece.from_tokenizer(tok)
    assert args is not None and wp is not None
    case = tmp_path / f"{name}.case"
    _write_case(case, args, docs, max_len, threads, exact)
    env = {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS")}
    env.update(SAN_ENV)
    r = subprocess.run([driver, str(case)], capture_output=True, text=True, env=env, timeout=300)
    report = [ln for ln in r.stderr.splitlines() if "Sanitizer" in ln or "runtime error" in ln]
    assert r.returncode == 0 and not report and not r.stderr.strip(), (name, r.returncode, r.stderr[-3000:])
    want = _expected(wp, docs, max_len, threads)
    if r.stdout != want:
        got, exp = r.stdout.splitlines(), want.splitlines()
        diff = [(g, e) for g, e in zip(got, exp) if g != e][:3]
        raise AssertionError((name, len(got), len(exp), diff))
    return r.stdout


@pytest.fixture(scope="module")
def tokenizers_h():
    vocab, syll = tc.matrix_vocab()
    return {lower: tc.make_tokenizer("H", lower, vocab) for lower in (True, False)}, syll


@pytest.mark.parametrize("lower", [True, False])
def test_matrix_and_hand_written_texts(driver, tmp_path, tokenizers_h, lower):
    """The hand-written list and the texts of every variant through the tokenizer with the most added tokens (H), at
    max_len 2, 3, 4, 9 and 64, on 1 and on 5 threads (more than 64 sentences: the threads do run)."""
    toks, syll = tokenizers_h
    docs = [d for d in tc.HAND if d.isascii()]
    for v in tc.VARIANTS:
        docs += tc.matrix_texts(v)
    docs = list(dict.fromkeys(docs)) + tc.clean_sentences(toks[lower], syll, 100, seed=3)
    assert len(docs) > 5 * 64
    for max_len in (2, 3, 4, 9, 64):
        for threads in (1, 5):
            out = _run(driver, tmp_path, f"m{max_len}_{threads}", toks[lower], docs, max_len, threads)
            assert out.count("\n") == len(docs) + 2


@pytest.mark.parametrize("variant", ["A", "C", "E", "G", None])
def test_each_kind_of_added_token(driver, tmp_path, variant):
    vocab, _ = tc.matrix_vocab()
    tok = tc.make_tokenizer(variant, True, vocab)
    docs = [d for d in tc.HAND if d.isascii()] + (tc.matrix_texts(variant) if variant else tc.matrix_texts("H")[:300])
    _run(driver, tmp_path, f"v{variant}", tok, docs, 9, 5)


def test_edges_of_the_c_abi(driver, tmp_path, tokenizers_h):
    """Empty sentences, no sentence at all, a sentence of 100 000 bytes (truncated, and with the untruncated max_len the pair
    tokenizer passes), and the least out_capacity the ABI accepts: bytes + n * specials."""
    toks, syll = tokenizers_h
    tok = toks[True]
    _run(driver, tmp_path, "none", tok, [], 64, 1)
    _run(driver, tmp_path, "none_exact", tok, [], 2, 5, exact=True)
    _run(driver, tmp_path, "empty", tok, [""], 64, 1, exact=True)
    _run(driver, tmp_path, "empties", tok, ["", " ", "", "\x00", "\t\r\n", ""] * 30, 3, 5, exact=True)
    long_words = ("the and qqfoo " * 7200)[:100000]
    long_clean = ("the and unprequ " * 6300)[:100000]
    one_word = "x" * 100000
    assert len(long_words) == len(long_clean) == len(one_word) == 100000
    for name, doc in (("words", long_words), ("clean", long_clean), ("word", one_word), ("punct", "." * 100000),
                      ("ctrl", "\x01" * 99999 + "a")):
        for max_len in (2, 3, 4, 64, 1 << 30):
            _run(driver, tmp_path, f"long_{name}_{max_len}", tok, [doc], max_len, 1, exact=True)
    # many sentences at the exact capacity, each max_len of the issue and one that truncates nothing
    docs = [d for d in tc.HAND if d.isascii()] + tc.matrix_texts("H")[:400] + tc.clean_sentences(tok, syll, 100, seed=5)
    for max_len in (2, 3, 4, 1 << 20):
        for threads in (1, 5):
            _run(driver, tmp_path, f"exact_{max_len}_{threads}", tok, docs, max_len, threads, exact=True)


def test_template_without_special_tokens(driver, tmp_path):
    """A tokenizer without special tokens in its template: specials = 0, so the exact capacity is the byte count alone."""
    from tokenizers import processors
    vocab, _ = tc.matrix_vocab()
    tok = tc.make_tokenizer("A", True, vocab)
    tok.backend_tokenizer.post_processor = processors.TemplateProcessing(single="$A", pair="$A $B:1", special_tokens=[])
    args = NativeWordPiece.create_args(tok)
    assert args is not None and args["prefix_ids"] == [] and args["suffix_ids"] == []
    docs = ["the and", "", "a b c d e f", "qqfoo", "x" * 300, "!!!!"]
    for max_len in (2, 3, 4, 64):
        _run(driver, tmp_path, f"nospec_{max_len}", tok, docs, max_len, 1, exact=True)

