"""Word-in-context embeddings on the GPU: span_pool_kernel / tsim_encoder_forward_spans (csrc/span_pool.h) and the Python
surface on top of it (NativeEncoder.forward_spans, models.WordEncoder, encode_text(output_value="token_embeddings")).

Two references, neither computed by the code under test:
  * a host REPLAY of the kernel's fixed arithmetic on the very hidden states the call returned (bf16 -> float32, float32 adds
    in list order starting from 0, one float32 division): the span rows must equal it bit for bit;
  * the float32 CPU oracle (oracle/encoder_ref.encoder_forward): span means of its hidden states, under the bar
    tests/test_encoder_gpu.py:21 applies to last hidden states (HID_TOL, asserted there at :39-40) — a mean of rows that each
    meet a max-abs bar meets it too.
Each preset's forward and oracle are computed once and shared by the tests that read them."""
import functools

import numpy as np
import pytest
import torch

from oracle import encoder_ref
from text_similarity_amd import _lib, ops, presets, word_spans
from text_similarity_amd.native_encoder import NativeEncoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HID_TOL = 8e-2      # tests/test_encoder_gpu.py:21 (max |err| of last hidden states against the fp32 reference)
PRESETS = ["tiny-bert", "tiny-mpnet", "all-MiniLM-L6-v2", "bert-base-uncased"]   # H = 64, 64, 384 (one pass), 768 (two)


def _spans_for(lens):
    """The span cases of one batch of 8 sequences (lengths ``lens``; sequence 1 is the long one, 3 has no span)."""
    L = lens[1]
    long_list = list(range(14, 114)) if L >= 114 else [(7 * i) % L for i in range(100)]    # 100 entries; repeats when L < 100
    return [
        [[3], [0]],                                                  # first sequence: a single token, CLS only
        [list(range(L)), long_list],                                 # every token of the longest sequence; a 100-entry list
        [[1, 4, 9, 2], [5, 5, 5, 2], []],                            # non-contiguous and out of order; repeats; empty
        [],                                                          # a sequence with no span
        [[0]],                                                       # a one-token sequence
        [[i % 16, (3 * i + 1) % 16] for i in range(70)],             # 70 spans on one sequence
        [],
        [[10, 0], list(range(lens[7]))],                             # last sequence of the packed batch
    ]


@functools.lru_cache(maxsize=None)
def _case(preset):
    cfg = presets.PRESETS[preset]
    cap = cfg.max_pos - (cfg.pad_id + 1 if cfg.arch == "mpnet" else 0)
    lens = [9, min(128, cap), 12, 5, 1, 16, 7, 11]        # tiny presets: the long sequence has every position row (64 tokens)
    cu = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=cu[1:])
    ids = presets.randint(f"spans/{preset}/ids", int(cu[-1]), 5, cfg.vocab).astype(np.int32)
    spans = _spans_for(lens)
    sseq, scu, stok = word_spans.span_table(spans)
    enc = NativeEncoder.from_preset(preset, max_tokens=1024, max_seqs=16)
    fd, cd = torch.from_numpy(ids).to(DEV), torch.from_numpy(cu.astype(np.int32)).to(DEV)
    tabs = [torch.from_numpy(a).to(DEV) for a in (sseq, scu, stok)]
    rho = ops.new_rho(DEV)
    r = enc.forward_spans(fd, cd, *tabs, span_unit=True, span_rho=rho, pooled=True, hidden=True)
    enc.check()
    torch.cuda.synchronize()
    # the oracle's hidden states, packed: the long sequence alone, the short ones padded together
    w = presets.synthetic_weights(preset)
    ref_h = np.zeros((int(cu[-1]), cfg.hidden), dtype=np.float32)
    with torch.no_grad():
        for rows in ([1], [b for b in range(len(lens)) if b != 1]):
            pid, mask = encoder_ref.pad_batch(ids, cu, rows, cfg.pad_id)
            h = encoder_ref.encoder_forward(cfg, w, pid, mask).numpy()
            for i, b in enumerate(rows):
                ref_h[cu[b]:cu[b + 1]] = h[i, :lens[b]]
    return dict(cfg=cfg, enc=enc, ids=ids, cu=cu, lens=lens, spans=spans, fd=fd, cd=cd, tabs=tabs, out=r, rho=rho, ref_h=ref_h,
                flat_spans=[(b, sp) for b, ss in enumerate(spans) for sp in ss])


def _span_means(h, cu, flat_spans, H):
    """numpy reference: the mean of the listed rows of ``h`` (float64 accumulate; an empty list gives zeros)."""
    out = np.zeros((len(flat_spans), H), dtype=np.float64)
    for s, (b, sp) in enumerate(flat_spans):
        if sp:
            out[s] = h[cu[b] + np.asarray(sp)].astype(np.float64).mean(0)
    return out


@pytest.mark.parametrize("preset", PRESETS)
def test_span_rows_equal_the_host_replay_bit_for_bit(preset):
    c = _case(preset)
    H, cu = c["cfg"].hidden, c["cu"]
    hidden = c["out"]["hidden"].float().cpu().numpy()           # bf16 -> float32 is exact
    got = c["out"]["spans"].cpu().numpy()
    assert got.shape == (len(c["flat_spans"]), H) and len(c["flat_spans"]) == 80
    ref = np.zeros_like(got)
    for s, (b, sp) in enumerate(c["flat_spans"]):
        acc = np.zeros(H, dtype=np.float32)
        for p in sp:                                            # list order, one float32 add per listed token
            acc = acc + hidden[cu[b] + p]
        assert acc.dtype == np.float32
        ref[s] = acc / np.float32(len(sp)) if sp else acc       # one division; an empty span stays zero
    bad = np.flatnonzero((got.view(np.uint32) != ref.view(np.uint32)).any(1))
    assert bad.size == 0, f"{preset}: spans {bad[:8].tolist()} differ from the replay, max |diff| {np.abs(got - ref).max():.3e}"
    empty = [s for s, (_, sp) in enumerate(c["flat_spans"]) if not sp]
    assert empty and (got[empty] == 0).all()
    # unit rows and rho word: exactly what ops.l2norm_rows makes of the span rows
    unit_ref, rho_ref = ops.l2norm_rows(c["out"]["spans"], return_rho=True)
    assert torch.equal(c["out"]["span_unit"], unit_ref)
    assert (c["out"]["span_unit"][empty] == 0).all()
    assert torch.equal(c["rho"], rho_ref) and float(rho_ref) > 0


@pytest.mark.parametrize("preset", PRESETS)
def test_span_rows_against_the_float32_oracle(preset):
    c = _case(preset)
    got = c["out"]["spans"].cpu().numpy()
    ref = _span_means(c["ref_h"], c["cu"], c["flat_spans"], c["cfg"].hidden)
    hid_err = np.abs(c["out"]["hidden"].float().cpu().numpy() - c["ref_h"]).max()
    err = np.abs(got - ref).max()
    print(f"{preset}: hidden max|err|={hid_err:.4f}  span max|err|={err:.4f}")
    assert hid_err <= HID_TOL, hid_err
    assert err <= HID_TOL, err


@pytest.mark.parametrize("preset", PRESETS)
def test_sentence_outputs_are_unchanged(preset):
    c = _case(preset)
    enc = c["enc"]
    plain = enc.forward_packed(c["fd"], c["cd"], pooled=True, unit=True, hidden=True)
    assert torch.equal(plain["pooled"], c["out"]["pooled"])
    assert torch.equal(plain["hidden"], c["out"]["hidden"])
    # no spans: every output of the call is tsim_encoder_forward_ex's
    z = torch.zeros(0, dtype=torch.int32, device=DEV)
    none = enc.forward_spans(c["fd"], c["cd"], z, torch.zeros(1, dtype=torch.int32, device=DEV), z, span_unit=True, pooled=True,
                             unit=True, hidden=True)
    for k in ("pooled", "unit", "hidden"):
        assert torch.equal(none[k], plain[k]), k
    assert none["spans"].shape == (0, c["cfg"].hidden) and none["span_unit"].shape[0] == 0
    # unit rows alone (the means go through encoder scratch) are the same rows
    only = enc.forward_spans(c["fd"], c["cd"], *c["tabs"], span_out=False, span_unit=True)
    assert set(only) == {"span_unit"} and torch.equal(only["span_unit"], c["out"]["span_unit"])
    enc.check()


def test_out_of_range_entries_are_clamped_and_flagged():
    """A position equal to the sequence length, a negative one, a span_seq equal to B and list offsets beyond the table are
    clamped into range (the row computed is the clamped entry's, bit for bit) and raise TSIM_ENC_ERR_SPAN; a clean call
    afterwards reads 0."""
    c = _case("tiny-bert")
    enc, fd, cd, lens = c["enc"], c["fd"], c["cd"], c["lens"]
    B = len(lens)

    def run(seq, cu_, tok):
        t = [torch.tensor(a, dtype=torch.int32, device=DEV) for a in (seq, cu_, tok)]
        out = enc.forward_spans(fd, cd, *t)["spans"]
        torch.cuda.synchronize()
        return out

    good = run([0, 0, B - 1, 2], [0, 2, 4, 5, 7], [1, lens[0] - 1, 0, 2, 3, 3, 4])
    enc.check()                                                                    # clean: nothing flagged
    for seq, cu_, tok in (([0, 0, B - 1, 2], [0, 2, 4, 5, 7], [1, lens[0], 0, 2, 3, 3, 4]),       # position == len -> len - 1
                          ([0, 0, B - 1, 2], [0, 2, 4, 5, 7], [1, lens[0] - 1, -5, 2, 3, 3, 4]),  # negative -> 0
                          ([0, 0, B, 2], [0, 2, 4, 5, 7], [1, lens[0] - 1, 0, 2, 3, 3, 4]),       # span_seq == B -> B - 1
                          ([0, 0, B - 1, 2], [0, 2, 4, 5, 9], [1, lens[0] - 1, 0, 2, 3, 3, 4])):  # list end beyond the table
        out = run(seq, cu_, tok)
        assert torch.isfinite(out).all()
        assert torch.equal(out, good), (seq, cu_, tok)
        with pytest.raises(IndexError, match="span"):
            enc.check()
        flags = _lib.C.c_int32(-1)
        _lib.check(_lib.lib().tsim_encoder_error_flags(enc._h, _lib.C.byref(flags), torch.cuda.current_stream().cuda_stream))
        assert flags.value == 0                                                    # cleared by the failed check
    # the bit itself
    run([0], [0, 1], [lens[0]])
    flags = _lib.C.c_int32(0)
    _lib.check(_lib.lib().tsim_encoder_error_flags(enc._h, _lib.C.byref(flags), torch.cuda.current_stream().cuda_stream))
    assert flags.value == _lib.ENC_ERR_SPAN
    assert torch.equal(run([0, 0, B - 1, 2], [0, 2, 4, 5, 7], [1, lens[0] - 1, 0, 2, 3, 3, 4]), good)
    enc.check()
    # refused on the host, before any launch
    with pytest.raises(ValueError):
        enc.forward_spans(fd, cd, *c["tabs"], span_out=False, span_unit=False)
    with pytest.raises(ValueError, match="S \\+ 1"):
        enc.forward_spans(fd, cd, c["tabs"][0], c["tabs"][1][:-1], c["tabs"][2])


# ----------------------------------------------------------------------------------------------------------- Python surface
SEQ_MAX = 48          # tiny-bert has 64 position rows
VOCAB = 1000


@functools.lru_cache(maxsize=None)
def _text_case():
    """50 synthetic sentences (one token per word), 0-3 target words each, and the oracle's hidden states of every sentence."""
    preset = "tiny-bert"
    cfg = presets.PRESETS[preset]
    sents = presets.synthetic_sentences(50, seed="spans/text", vocab_size=VOCAB, max_words=60)
    words, expect = [], []
    for i, s in enumerate(sents):
        ws = s.split(" ")[:SEQ_MAX - 2]                  # what survives truncation
        picks = sorted({(5 * i + 3 * j) % len(ws) for j in range(i % 4)})
        words.append([ws[p] for p in picks])
        cursor, pos = 0, []
        for p in picks:                                  # first occurrence behind the previous match; [CLS] is position 0
            at = ws.index(ws[p], cursor)
            pos.append([at + 1])
            cursor = at + 1
        expect.append(pos)
    ids = [[101] + [int(w[1:]) for w in s.split(" ")[:SEQ_MAX - 2]] + [102] for s in sents]
    S = max(len(t) for t in ids)
    pid = np.zeros((len(ids), S), dtype=np.int64)
    mask = np.zeros_like(pid)
    for i, t in enumerate(ids):
        pid[i, :len(t)] = t
        mask[i, :len(t)] = 1
    with torch.no_grad():
        h = encoder_ref.encoder_forward(cfg, presets.synthetic_weights(preset), pid, mask).numpy()
    hidden = [h[i, :len(t)] for i, t in enumerate(ids)]
    return sents, words, expect, hidden


def _word_encoder(max_seqs, max_tokens):
    from transformers import BertTokenizer
    from text_similarity_amd.configurations.config import Configuration, ModelParameters
    from text_similarity_amd.models import WordEncoder
    preset = "tiny-bert"
    tok = BertTokenizer(vocab=presets.synthetic_vocab(VOCAB), do_lower_case=True)
    params = Configuration(model_parameters=ModelParameters(preset, hidden_size=64), model=preset, save_path="", tokenizer=tok,
                           device=torch.device(DEV), batch_size=4, max_tokens_per_batch=max_tokens, max_seqs_per_batch=max_seqs,
                           sequence_max_len=SEQ_MAX)
    return WordEncoder.from_preset(preset, params, parallel_mode=False)


def _expected_rows(hidden, positions):
    rows, owner = [], []
    for i, plist in enumerate(positions):
        for p in plist:
            rows.append(hidden[i][np.asarray(p)].astype(np.float64).mean(0) if len(p) else np.zeros(hidden[i].shape[1]))
            owner.append(i)
    return np.asarray(rows), np.asarray(owner, dtype=np.int64)


def test_word_encoder_encode_words_and_pairs():
    sents, words, expect, hidden = _text_case()
    model = _word_encoder(max_seqs=16, max_tokens=512)       # several forwards: the rows come back in input order
    ref, owner = _expected_rows(hidden, expect)
    emb, span_sentence, sent = model.encode_words(sents, words, return_sentence_embeddings=True)
    assert emb.shape == ref.shape and emb.dtype == torch.float32 and emb.is_cuda
    np.testing.assert_array_equal(span_sentence.cpu().numpy(), owner)
    err = np.abs(emb.cpu().numpy() - ref).max()
    print(f"encode_words: {len(ref)} spans, max|err|={err:.4f}")
    assert err <= HID_TOL, err
    assert model.last_encode_stats["spans"] == len(ref)
    # the sentence embeddings of the same call are encode_text's
    assert torch.equal(sent, model.encode_text(sents))
    # explicit positions bypass the alignment and give the same rows; numpy output
    emb_p, owner_p = model.encode_words(sents, positions=expect, output_np=True)
    np.testing.assert_array_equal(emb_p, emb.cpu().numpy())
    np.testing.assert_array_equal(owner_p, owner)
    # an absent word gives a zero row; a position outside its sentence raises as indexing would
    e0, _ = model.encode_words(["w00200 w00300"], [["w00999", "w00300"]])
    assert (e0[0] == 0).all() and e0[1].abs().sum() > 0
    with pytest.raises(IndexError, match="span"):
        model.encode_words(["w00200 w00300"], positions=[[[4]]])
    with pytest.raises(ValueError):
        model.encode_words(sents, words, positions=expect)
    assert model.encode_words([], [])[0].shape == (0, 64)
    # pairs: row i = words_1[i] in sentences_1[i] / words_2[i] in sentences_2[i]
    first = [s.split(" ")[0] for s in sents]
    a, b = model.encode_word_pairs(sents[:10], sents[10:20], first[:10], first[10:20])
    ref_pairs, _ = _expected_rows(hidden[:20], [[[1]]] * 20)
    assert a.shape == b.shape == (10, 64)
    assert np.abs(torch.cat([a, b]).cpu().numpy() - ref_pairs).max() <= HID_TOL
    same, _ = model.encode_words(sents[:20], [[w] for w in first[:20]])
    assert torch.equal(torch.cat([a, b]), same)


def test_encode_text_token_embeddings_and_default():
    sents, _, _, hidden = _text_case()
    model = _word_encoder(max_seqs=64, max_tokens=4096)      # one forward holds all 50 sentences
    toks = model.encode_text(sents, output_value="token_embeddings")
    assert isinstance(toks, list) and len(toks) == len(sents)
    err = 0.0
    for t, h in zip(toks, hidden):                           # input order, no padding, special tokens included
        assert tuple(t.shape) == h.shape and t.dtype == torch.float32 and t.is_cuda
        err = max(err, float(np.abs(t.cpu().numpy() - h).max()))
    print(f"token_embeddings: max|err|={err:.4f}")
    assert err <= HID_TOL, err
    as_np = model.encode_text(sents[:3], output_np=True, output_value="token_embeddings")
    assert all(isinstance(a, np.ndarray) for a in as_np) and np.array_equal(as_np[1], toks[1].cpu().numpy())
    assert model.encode_text([], output_value="token_embeddings") == []
    with pytest.raises(ValueError):
        model.encode_text(sents, output_value="tokens")
    # the default output: what the call returned before the argument existed — the length-sorted batch through the packed
    # mean-pool forward, un-sorted — bit for bit
    default = model.encode_text(sents)
    assert torch.equal(default, model.encode_text(sents, output_value="sentence_embedding"))
    order = np.argsort([len(s) for s in sents], kind="stable")
    ids = [[101] + [int(w[1:]) for w in sents[i].split(" ")[:SEQ_MAX - 2]] + [102] for i in order]
    cu = np.zeros(len(ids) + 1, dtype=np.int64)
    np.cumsum([len(t) for t in ids], out=cu[1:])
    flat = torch.tensor([t for row in ids for t in row], dtype=torch.int32, device=DEV)
    pooled = model.context_embedder.forward_packed(flat, torch.from_numpy(cu.astype(np.int32)).to(DEV))["pooled"]
    assert torch.equal(default[torch.from_numpy(order).to(DEV)], pooled)
    # and its mean over the tokens is the same sentence embedding up to the order of the float32 adds: a float32 sum of
    # n <= 48 values of |x| <= 4 is within (n - 1) 2^-24 sum|x| <= 5.4e-4 of the exact one whatever the order, its mean within
    # 1.2e-5; two such means differ by at most 2.4e-5
    mean_tok = torch.stack([t.mean(0) for t in toks])
    assert max(float(t.abs().max()) for t in toks) <= 4.0
    assert (mean_tok - default).abs().max() <= 2.4e-5
