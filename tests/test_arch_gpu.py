"""DistilBERT / RoBERTa-family checkpoints and hidden-1024 encoders on the GPU.

* The two new fixtures (HF's own models through the reference's wrapper, tools/make_golden.py g1a) within the tolerances of
  tests/test_encoder_gpu.py, through the preset, an HF-written directory and a sentence-transformers directory.
* The mapping is exact: a RoBERTa encoder equals bit for bit a BERT encoder with the position table shifted by pad_id + 1, a
  DistilBERT encoder a BERT encoder with an all-zero token-type row.
* Hidden 1024 against the float64 probe under the rule of tests/encoder_cases.py (TOL = TOL_FACTOR x the probe's own bf16
  floor, computed at test time), batch-size independence at more projection tiles than CUs, and the classification heads.

Run the file under a time limit of its own, for instance
``timeout -k 10 600 python -m pytest tests/test_arch_gpu.py -q -m gpu -s``."""
from dataclasses import replace

import numpy as np
import pytest
import torch

import arch_cases as ac
import encoder_cases as ec
from conftest import golden
from text_similarity_amd import presets
from text_similarity_amd.native_encoder import NativeEncoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HID_TOL, POOL_TOL, COS_MIN = 8e-2, 5e-2, 0.9995                 # tests/test_encoder_gpu.py
LOGIT_TOL, PEARSON_MIN_TINY = 1.5e-2, 0.995                      # tests/test_cross_encoder_gpu.py


def _cos_rows(a, b):
    return (a * b).sum(1) / np.maximum(np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1), 1e-30)


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrs]


def _params(preset, hidden, **kw):
    from text_similarity_amd.configurations.config import Configuration, ModelParameters
    return Configuration(model_parameters=ModelParameters(preset, hidden_size=hidden), model=preset, save_path="",
                         device=torch.device(DEV), max_tokens_per_batch=1024, max_seqs_per_batch=64, **kw)


def _check_fixture(enc, g):
    ids, mask = _dev(g["input_ids"], g["attention_mask"])
    hidden = enc(input_ids=ids, attention_mask=mask)[0]
    enc.check()
    h, m = hidden.cpu().numpy(), g["attention_mask"].astype(bool)
    err = float(np.abs(h[m] - g["last_hidden_state"][m]).max())
    from text_similarity_amd import ops
    p = ops.mean_pool(hidden, mask).cpu().numpy()
    perr = float(np.abs(p - g["pooled"]).max())
    live = g["attention_mask"].sum(1) > 0
    cos = float(_cos_rows(p[live], g["pooled"][live]).min())
    print(f"hidden max|err|={err:.4f} pooled max|err|={perr:.4f} min cos={cos:.6f}")
    assert err <= HID_TOL and (h[~m] == 0).all()
    assert perr <= POOL_TOL and cos >= COS_MIN and (p[~live] == 0).all()


@pytest.mark.parametrize("preset", ["tiny-distilbert", "tiny-roberta"])
@pytest.mark.parametrize("source", ["preset", "hf_directory"])
def test_fixtures(preset, source, tmp_path):
    g = golden(f"encoder_{preset}.npz")
    if source == "preset":
        enc = NativeEncoder.from_preset(preset, max_tokens=1024, max_seqs=64)
    else:                                          # a directory written by HF's own save_pretrained
        cfg = presets.PRESETS[preset]
        ac.hf_model(cfg, presets.synthetic_weights(preset)).save_pretrained(str(tmp_path))
        enc = NativeEncoder.from_pretrained(str(tmp_path), max_tokens=1024, max_seqs=64)
        assert enc.cfg == cfg and enc.config.model_type == cfg.model_type
    _check_fixture(enc, g)


def test_fixture_through_a_sentence_transformers_directory(tmp_path):
    from text_similarity_amd.dataset.dataset import EmbeddingsFeatures
    from text_similarity_amd.models.sentence_encoder import SentenceTransformerWrapper
    from text_similarity_amd.models.st_format import write_sentence_transformers_modules
    from text_similarity_amd.weights import save_hf_dir
    preset = "tiny-roberta"
    cfg, g = presets.PRESETS[preset], golden(f"encoder_{preset}.npz")
    path = str(tmp_path / "st")
    save_hf_dir(path, cfg, presets.synthetic_weights(preset))
    write_sentence_transformers_modules(path, cfg.hidden, "mean", None, False)
    params = _params(preset, cfg.hidden)
    model = SentenceTransformerWrapper.from_sentence_transformers(path, params, parallel_mode=False)
    assert model.context_embedder.cfg == cfg
    ids, mask = _dev(g["input_ids"], g["attention_mask"])
    p = model.encode(EmbeddingsFeatures(ids, mask)).cpu().numpy()
    assert np.abs(p - g["pooled"]).max() <= POOL_TOL
    # save_pretrained writes the source architecture back; from_pretrained on it gives the same bits
    out = str(tmp_path / "saved")
    model.context_embedder.save_pretrained(out)
    transformers = pytest.importorskip("transformers")
    assert transformers.AutoConfig.from_pretrained(out).model_type == "roberta"
    again = NativeEncoder.from_pretrained(out, max_tokens=1024, max_seqs=64)
    assert torch.equal(again(input_ids=ids, attention_mask=mask)[0], model.context_embedder(input_ids=ids, attention_mask=mask)[0])


def _packed_case(cfg, seed, lens):
    ids = presets.randint(seed, int(sum(lens)), 5, cfg.vocab).astype(np.int32)
    cu = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=cu[1:])
    return ids, cu


@pytest.mark.parametrize("preset", ["tiny-distilbert", "tiny-roberta"])
def test_bit_identical_to_the_bert_encoder_it_maps_to(preset):
    cfg, w = presets.PRESETS[preset], presets.synthetic_weights(preset)
    bcfg, bw = ac.canonical_bert(cfg, w)
    assert bcfg.source_type == "bert" and bcfg.first_pos == 0
    assert bw[ac.POS].shape[0] == cfg.max_pos - cfg.first_pos and (cfg.type_vocab > 0 or not bw[ac.TYPE].any())
    cap = cfg.max_pos - cfg.first_pos
    ids, cu = _packed_case(cfg, preset + "/bits", [17, 1, 0, cap, 33, 2, 31])
    fd, cd = _dev(ids, cu.astype(np.int32))
    a = NativeEncoder(cfg, w, max_tokens=512, max_seqs=16).forward_packed(fd, cd, pooled=True, unit=True, hidden=True)
    b = NativeEncoder(bcfg, bw, max_tokens=512, max_seqs=16).forward_packed(fd, cd, pooled=True, unit=True, hidden=True)
    for k in ("hidden", "pooled", "unit"):
        assert torch.equal(a[k], b[k]), k
    assert torch.isfinite(a["pooled"]).all() and a["pooled"].abs().sum() > 0


def test_roberta_positions():
    preset = "tiny-roberta"
    cfg, w = presets.PRESETS[preset], presets.synthetic_weights(preset)
    enc = NativeEncoder(cfg, w, max_tokens=1024, max_seqs=16)
    lens = [17, 1, 64, 33, 24]
    ids, cu = _packed_case(cfg, "roberta/pos", lens)
    s = len(lens) - 1
    ids[cu[s] + 7] = ids[cu[s] + 15] = cfg.pad_id            # a pad id inside the last sequence: positions skip there
    # padded call == packed call, bit for bit
    B, S = len(lens), max(lens)
    pid = np.full((B, S), cfg.pad_id, np.int64)
    mask = np.zeros((B, S), np.int64)
    for b in range(B):
        pid[b, :lens[b]] = ids[cu[b]:cu[b + 1]]
        mask[b, :lens[b]] = 1
    fd, cd, pd, md = _dev(ids, cu.astype(np.int32), pid, mask)
    packed = enc.forward_packed(fd, cd, pooled=False, hidden=True)["hidden"]
    padded = enc(input_ids=pd, attention_mask=md)[0]
    enc.check()
    assert torch.equal(padded[md.bool()], packed.float())
    # HF's rule: cumsum(ids != pad) * (ids != pad) + pad
    ne = (pid != cfg.pad_id).astype(np.int64)
    want = (np.cumsum(ne, 1) * ne + cfg.pad_id)[mask.astype(bool)]
    pos, cols = enc.positions(fd, cd)
    np.testing.assert_array_equal(pos.cpu().numpy(), want)
    a = int(cu[s])
    assert want[a + 7] == cfg.pad_id and want[a + 8] == cfg.pad_id + 8 and want[a + 23] == cfg.pad_id + 22   # two rows skipped
    np.testing.assert_array_equal(want[:17], cfg.pad_id + 1 + np.arange(17))
    ref = ac.hf_hidden(ac.hf_model(cfg, w), pid, mask)[mask.astype(bool)]
    err = float(np.abs(packed.float().cpu().numpy() - ref).max())
    print(f"tiny-roberta with pad ids inside a sequence vs HF: max|err|={err:.4f}")
    assert err <= HID_TOL
    # a 514-row table holds 512 tokens
    big_cfg = replace(cfg, max_pos=514)
    big = NativeEncoder(big_cfg, presets.synthetic_weights("tiny-roberta-514", big_cfg), max_tokens=513, max_seqs=1)
    long_ids = torch.from_numpy(presets.randint("roberta/long", 513, 5, cfg.vocab).astype(np.int32)).to(DEV)
    with pytest.raises(ValueError, match="position rows"):
        big.forward_packed(long_ids, torch.tensor([0, 513], dtype=torch.int32, device=DEV))
    ok = big.forward_packed(long_ids[:512], torch.tensor([0, 512], dtype=torch.int32, device=DEV))["pooled"]
    big.check()
    assert torch.isfinite(ok).all()
    # no row for a non-zero token type
    with pytest.raises(ValueError, match="token-type"):
        enc(input_ids=pd, attention_mask=md, token_type_ids=torch.ones_like(pd))
    assert torch.equal(enc(input_ids=pd, attention_mask=md, token_type_ids=torch.zeros_like(pd))[0], padded)


# --------------------------------------------------------------------------- hidden 1024
def _compare(label, got, ref, floor, tol):
    e = ec.errors(got, ref)
    print(f"{label}: " + "  ".join(f"{m} measured {e[m]:.4g} floor {floor[m]:.4g} TOL {tol[m]:.4g}" for m in ec.METRICS))
    assert np.isfinite(got).all(), f"{label}: non-finite output"
    for m in ec.METRICS:
        assert e[m] <= tol[m], f"{label}: {m} {e[m]:.4g} > TOL {tol[m]:.4g} (floor {floor[m]:.4g})"


@pytest.mark.parametrize("name", list(ac.CASES_1024))
def test_hidden_1024_after_every_layer(name):
    cfg, wdtype = ac.CASES_1024[name]
    assert (cfg.num_layers, cfg.hidden, cfg.heads, cfg.ffn, cfg.vocab) == (2, 1024, 16, 4096, 2000)
    ids, cu, _ = ac.inputs_1024(name)
    w = ac.weights_1024(name)
    exact, floor, tol = ac.tolerances_1024(name)
    fd, cd = _dev(ids.copy(), cu.astype(np.int32))
    empty = np.diff(cu) == 0
    assert empty.any()
    for l in range(1, cfg.num_layers + 1):
        enc = NativeEncoder(replace(cfg, num_layers=l), w, max_tokens=ids.size, max_seqs=cu.size - 1, weight_dtype=wdtype)
        r = enc.forward_packed(fd, cd, pooled=True, hidden=True)
        torch.cuda.synchronize()
        enc.check()
        h, p = r["hidden"].float().cpu().numpy(), r["pooled"].cpu().numpy()
        assert (p[empty] == 0).all()
        _compare(f"{name} boundary {l}", h, exact[l], floor[l], tol[l])
        if l == cfg.num_layers:
            _compare(f"{name} pooled", p, ec.pooled_rows(exact[l], cu), floor["pooled"], tol["pooled"])
            with pytest.raises(ValueError, match="768"):          # unit rows stay capped at the search width
                enc.forward_packed(fd, cd, pooled=True, unit=True)
        del enc


@pytest.mark.parametrize("wdtype", ["bf16", "mxfp8"])
def test_hidden_1024_large_batch_equals_small_batches_bitwise(wdtype):
    """1 500 sentences (~24 k tokens) in one call: every projection launch has more output tiles than CUs.  Rows are
    independent, so the result equals the same sentences encoded 48 at a time, bit for bit; and a repeated forward gives the
    same bits."""
    cfg, n = ac.CFG_1024, 1500
    w = ac.weights_1024("bert-1024")
    flat, cu = presets.synthetic_token_batch(n, seed="big/1024", vocab_size=ec.LOWVAR_IDS[0], max_len=64)
    cu = cu.astype(np.int64)
    enc = NativeEncoder(cfg, w, max_tokens=int(cu[-1]), max_seqs=n, weight_dtype=wdtype)
    fd, cd = _dev(flat, cu.astype(np.int32))
    first = enc.forward_packed(fd, cd, hidden=True)
    big, big_h = first["pooled"].clone(), first["hidden"].clone()
    torch.cuda.synchronize()
    assert torch.isfinite(big).all() and torch.isfinite(big_h.float()).all()
    for rep in range(5):
        out = enc.forward_packed(fd, cd, hidden=True)
        assert torch.equal(out["hidden"], big_h) and torch.equal(out["pooled"], big), f"forward {rep + 2} differs from the first"
    for s in sorted({0, 480, 1017, n - 48}):
        f = flat[cu[s]:cu[s + 48]]
        c = (cu[s:s + 49] - cu[s]).astype(np.int32)
        small = enc.forward_packed(*_dev(f, c))["pooled"]
        assert torch.equal(small, big[s:s + 48]), f"{wdtype}: rows {s}.. differ between batch sizes"
    enc.check()


# --------------------------------------------------------------------------- classification heads
def _bert_tokenizer(vocab_size):
    transformers = pytest.importorskip("transformers")
    return transformers.BertTokenizer(vocab=presets.synthetic_vocab(vocab_size), do_lower_case=True)


def _roberta_tokenizer(vocab_size, max_len):
    """A word-level fast tokenizer with RoBERTa's special ids and pair template <s> a </s></s> b </s> (no WordPiece)."""
    transformers = pytest.importorskip("transformers")
    from tokenizers import Tokenizer, models, pre_tokenizers, processors
    vocab = {"<s>": 0, "<pad>": 1, "</s>": 2, "<unk>": 3}
    vocab.update({f"<unused{i}>": i for i in range(4, 104)})
    vocab.update({f"w{i:05d}": i for i in range(104, vocab_size)})
    tk = Tokenizer(models.WordLevel(vocab, unk_token="<unk>"))
    tk.pre_tokenizer = pre_tokenizers.Whitespace()
    tk.post_processor = processors.RobertaProcessing(sep=("</s>", 2), cls=("<s>", 0))
    return transformers.PreTrainedTokenizerFast(tokenizer_object=tk, bos_token="<s>", eos_token="</s>", cls_token="<s>",
                                                sep_token="</s>", pad_token="<pad>", unk_token="<unk>", model_max_length=max_len)


def _pairs(n, max_words, seed, vocab_size):
    q = presets.synthetic_sentences(max(n // 8, 1), seed=seed + "/q", vocab_size=vocab_size, max_words=max_words)
    t = presets.synthetic_sentences(n, seed=seed + "/t", vocab_size=vocab_size, max_words=max_words)
    return [[q[i % len(q)], t[i]] for i in range(n)]


def _hf_classifier(cfg, w, preset, num_labels):
    transformers = pytest.importorskip("transformers")
    hc = ac.hf_config(cfg, num_labels=num_labels)
    cls = transformers.DistilBertForSequenceClassification if cfg.model_type == "distilbert" else transformers.RobertaForSequenceClassification
    m = cls(hc)
    head = list(presets.synthetic_head_weights(preset, num_labels, cfg).values())
    if cfg.model_type == "distilbert":
        names, prefix = ("pre_classifier.weight", "pre_classifier.bias", "classifier.weight", "classifier.bias"), "distilbert."
    else:
        names, prefix = ("classifier.dense.weight", "classifier.dense.bias", "classifier.out_proj.weight", "classifier.out_proj.bias"), "roberta."
    sd = {prefix + presets.source_name(cfg.model_type, k): torch.from_numpy(v.copy()) for k, v in w.items()}
    sd.update({k: torch.from_numpy(v.copy()) for k, v in zip(names, head)})
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if "position_ids" not in k and "token_type_ids" not in k], (missing, unexpected)
    return m.eval()


@pytest.mark.parametrize("preset,num_labels", [("tiny-roberta", 1), ("tiny-roberta", 3), ("tiny-distilbert", 1),
                                               ("tiny-distilbert", 3)])
def test_classifier_logits_match_hf(preset, num_labels, tmp_path):
    """HF's classifier on the CPU against CrossEncoder on a directory HF wrote.  The encoder weights are the sharp ones
    (arch_cases.sharp_arch_weights says why: the logits must spread by more than the bf16 error for Pearson to mean anything)."""
    from text_similarity_amd.models.cross_encoder import CrossEncoder, LibraryPairTokenizer, PairTokenizer
    cfg, w = ac.sharp_arch_weights(preset)
    L = cfg.max_pos - cfg.first_pos
    words = ec.LOWVAR_IDS[0]
    tok = _bert_tokenizer(words) if cfg.model_type == "distilbert" else _roberta_tokenizer(words, L)
    model = _hf_classifier(cfg, w, preset, num_labels)
    model.save_pretrained(str(tmp_path))
    tok.save_pretrained(str(tmp_path))
    ce = CrossEncoder(str(tmp_path), max_length=L, tokenizer=tok, max_tokens=16384, max_seqs=512)
    assert ce.num_labels == num_labels and ce.config == cfg
    assert isinstance(ce.pair_tokenizer, PairTokenizer if cfg.model_type == "distilbert" else LibraryPairTokenizer)
    if num_labels == 1:      # max_length is capped at what the position table holds (a 66-row RoBERTa table: 64 tokens) ...
        assert CrossEncoder(str(tmp_path), max_length=cfg.max_pos, tokenizer=tok, max_tokens=256, max_seqs=4).max_length == L
        tok.model_max_length = int(1e30)      # ... also when the tokenizer names no length of its own
        assert CrossEncoder(str(tmp_path), tokenizer=tok, max_tokens=256, max_seqs=4).max_length == L
        with pytest.raises(ValueError, match="max_length"):      # not mistaken for a foreign pair template
            CrossEncoder(str(tmp_path), max_length=3, tokenizer=tok, max_tokens=256, max_seqs=4)
    pairs = _pairs(200, 30, f"arch/logits/{preset}", words)
    pairs[0] = [" ".join([pairs[1][1]] * 10), " ".join([pairs[2][1]] * 12)]           # one pair cut to max_length
    got = ce.predict(pairs, activation_fct=torch.nn.Identity()).reshape(len(pairs), num_labels)
    enc = tok([a for a, _ in pairs], [b for _, b in pairs], truncation=True, max_length=L, padding=True, return_tensors="pt")
    assert int(enc["attention_mask"].sum(1).max()) == L
    with torch.no_grad():
        ref = model(input_ids=enc["input_ids"], attention_mask=enc["attention_mask"]).logits.numpy()
    err = float(np.abs(got - ref).max())
    r = float(np.corrcoef(got.ravel().astype(np.float64), ref.ravel().astype(np.float64))[0, 1])
    print(f"{preset} labels={num_labels}: max|dlogit|={err:.5f} pearson={r:.6f} logit std={ref.std():.4f}")
    assert err <= LOGIT_TOL and r >= PEARSON_MIN_TINY


def head_reference(x, pw, pb, cw, cb, act):
    """(logits, bound) of logits = W_c act(W_p x + b_p) + b_c in float64, with a bound on what the float32 kernel may differ by,
    from its summation orders alone (u = 2^-24): the first layer is one fma chain over k ascending, so each step rounds the
    partial sum S_k once: error <= u sum_k |S_k|, plus u |S + b_p| for the bias add; tanhf is taken at 5 ulp (the OpenCL bound
    that the device library documents) of a value <= 1 and |d act / d pre| <= 1; a logit is 64 lane chains over i = lane,
    lane + 64, .. followed by 6 butterfly stages and the bias add, every add rounding its own result: error <= u (sum of all
    lane partial sums' magnitudes + 6 sum_lanes |lane sum| + |logit|); the first layer's error reaches a logit through |W_c|."""
    u = 2.0 ** -24
    x, pw, pb, cw, cb = (np.asarray(a, np.float64) for a in (x, pw, pb, cw, cb))
    H = x.shape[1]
    pre, pre_err = np.empty((x.shape[0], H)), np.empty((x.shape[0], H))
    for b in range(x.shape[0]):
        S = np.cumsum(pw * x[b][None, :], axis=1)                   # [feature j, k]: partial sums of feature j's chain
        pre[b] = S[:, -1] + pb
        pre_err[b] = u * (np.abs(S).sum(1) + np.abs(pre[b]))
    mid = np.tanh(pre) if act == "tanh" else np.maximum(pre, 0.0)
    mid_err = pre_err + (5 * u * np.abs(mid) if act == "tanh" else 0.0)
    logits = mid @ cw.T + cb
    terms = mid[:, None, :] * cw[None, :, :]                        # [b, label, i]
    lanes = np.cumsum(terms.reshape(x.shape[0], cw.shape[0], H // 64, 64), axis=2)      # chains over i = lane + 64 step
    own = u * (np.abs(lanes).sum((2, 3)) + 6 * np.abs(lanes[:, :, -1, :]).sum(2) + np.abs(logits))
    return logits, mid_err @ np.abs(cw).T + own, pre


@pytest.mark.parametrize("act", ["tanh", "relu"])
def test_hidden_1024_head_equals_a_float64_head_on_its_own_cls_rows(act):
    """The 1 024-thread head instance (and its ReLU form) on the GPU's own first-token rows against numpy float64, within the
    bound of ``head_reference``; the bound stays below 0.01, under the size of a classifier bias, so a dropped bias, the other
    activation or a wrong row would miss it."""
    cfg = ac.CFG_1024
    H, n_labels = cfg.hidden, 3
    enc = NativeEncoder(cfg, ac.weights_1024("bert-1024"), max_tokens=4096, max_seqs=64)
    hw = presets.synthetic_head_weights("head/1024", n_labels, cfg)
    pw, pb, cw, cb = (hw[k] for k in ("pooler.dense.weight", "pooler.dense.bias", "classifier.weight", "classifier.bias"))
    enc.set_cls_head(pw, pb, cw, cb, act=act)
    flat, cu = presets.synthetic_token_batch(19, seed="head/1024", vocab_size=ec.LOWVAR_IDS[0], max_len=40)
    cu = np.concatenate([cu[:7], cu[6:]]).astype(np.int64)            # an empty sequence: reads a zero row
    r = enc.forward_packed(*_dev(flat, cu.astype(np.int32)), pooled=False, hidden=True, logits=True)
    enc.check()
    h = r["hidden"].float().cpu().numpy().astype(np.float64)
    x = np.zeros((len(cu) - 1, H))
    live = np.diff(cu) > 0
    x[live] = h[cu[:-1][live]]
    ref, bound, pre = head_reference(x, pw, pb, cw, cb, act)
    got = r["logits"].cpu().numpy().astype(np.float64)
    other = head_reference(x, pw, pb, cw, cb, "relu" if act == "tanh" else "tanh")[0]
    print(f"hidden-1024 {act} head: max|dlogit|={np.abs(got - ref).max():.3e} bound {bound.min():.3e}..{bound.max():.3e} "
          f"|pre| up to {np.abs(pre).max():.2f}; the other activation is up to {np.abs(other - ref)[live].max():.3f} away")
    assert np.abs(pre).max() > 1.0 and bound.max() < 1e-2 and np.abs(other - ref)[live].max() > 10 * bound.max()
    assert got.shape == (len(cu) - 1, n_labels) and (np.abs(got - ref) <= bound).all()
