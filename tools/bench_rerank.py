#!/usr/bin/env python3
"""Cross-encoder re-ranking benchmark (models/cross_encoder.CrossEncoder): one JSON line per part.

Workload: all-MiniLM-L6-v2 preset, 1 label, max_length 512; 256 synthetic queries x 100 candidate passages each (passages
at a median of ~48 words) = 25 600 pairs, the re-ranking stage of RankingPipeline with top_k = 100.

    python tools/bench_rerank.py --part native [--out DIR]   end-to-end pairs/s of predict (with the tokeniser's share),
                                                             GPU-only pairs/s and tokens/s from device events, MFMA fraction
    python tools/bench_rerank.py --part hf [--out DIR]       HF BertForSequenceClassification on the same GPU and pairs
                                                             (eager fp32 and fp16 autocast) and the Pearson correlation of
                                                             its scores with the native ones (read from DIR)
Run each part as its own process, under its own time limit."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from text_similarity_amd import presets  # noqa: E402

PRESET = "all-MiniLM-L6-v2"
PEAK_BF16_TFLOPS = 2500.0   # MI355X dense bf16 MFMA, as bench.py


def workload(n_q=256, k=100):
    cfg = presets.PRESETS[PRESET]
    queries = presets.synthetic_sentences(n_q, seed="rerank/q", vocab_size=cfg.vocab)
    lens = presets.synthetic_lengths(n_q * k, seed="rerank/p", median=48, max_words=400)
    words = presets.randint("rerank/p/tok", int(lens.sum()), 104, cfg.vocab)
    passages, p = [], 0
    for n in lens:
        passages.append(" ".join(f"w{t:05d}" for t in words[p:p + n]))
        p += n
    return [[queries[i // k], passages[i]] for i in range(n_q * k)]


def tokenizer():
    from transformers import BertTokenizer
    return BertTokenizer(vocab=presets.synthetic_vocab(presets.PRESETS[PRESET].vocab), do_lower_case=True)


def part_native(pairs, out_dir, reps):
    from text_similarity_amd.models import CrossEncoder
    cfg = presets.PRESETS[PRESET]
    ce = CrossEncoder(PRESET, num_labels=1, max_length=512, tokenizer=tokenizer())
    ce.predict(pairs[:2048])                     # warm-up (kernels, tokenizer)
    torch.cuda.synchronize()
    walls, toks = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        ce.predict(pairs)
        walls.append(time.perf_counter() - t0)
        toks.append(ce.last_predict_stats["tokenizer_s"])
    # GPU only: the same packed pairs, device events around the forwards
    ids, types, lens = ce.pair_tokenizer(pairs)
    order = np.argsort(lens, kind="stable")
    cu0 = np.zeros(len(pairs) + 1, np.int64)
    np.cumsum(lens, out=cu0[1:])
    from text_similarity_amd.models.cross_encoder import _spans
    idx = _spans(cu0[:-1][order], lens[order])
    lens_s = lens[order]
    cu = np.zeros(len(pairs) + 1, np.int64)
    np.cumsum(lens_s, out=cu[1:])
    fd, td = torch.from_numpy(ids[idx]).cuda(), torch.from_numpy(types[idx]).cuda()
    cd = torch.from_numpy(cu.astype(np.int32)).cuda()
    ce.logits_packed(fd, td, cd, cu)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ce.logits_packed(fd, td, cd, cu)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    ce.model.check()
    T = int(cu[-1])
    H, F, L = cfg.hidden, cfg.ffn, cfg.num_layers
    sbar = float((lens_s.astype(np.float64) ** 2).sum() / T)
    flops = T * L * (2 * (4 * H * H + 2 * H * F) + 4 * sbar * H)
    wall = float(np.median(walls))
    res = {"part": "native", "preset": PRESET, "pairs": len(pairs), "tokens": T, "mean_pair_tokens": round(T / len(pairs), 1),
           "max_pair_tokens": int(lens.max()), "reps": reps,
           "e2e_pairs_per_s": round(len(pairs) / wall), "e2e_wall_ms_median": round(wall * 1e3, 2),
           "e2e_wall_ms_spread": [round(min(walls) * 1e3, 2), round(max(walls) * 1e3, 2)],
           "tokenizer_share": round(float(np.median(toks)) / wall, 3),
           "gpu_ms": round(ms, 3), "gpu_pairs_per_s": round(len(pairs) / ms * 1e3), "gpu_tokens_per_s": round(T / ms * 1e3),
           "encoder_TFLOPs": round(flops / ms / 1e9, 1), "mfma_fraction": round(flops / ms / 1e9 / PEAK_BF16_TFLOPS, 4)}
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        np.save(os.path.join(out_dir, "rerank_native_logits.npy"), ce.predict(pairs, activation_fct=torch.nn.Identity()))
    print(json.dumps(res), flush=True)


def part_hf(pairs, out_dir, reps, batch=256):
    import transformers
    cfg = presets.PRESETS[PRESET]
    hc = transformers.BertConfig(vocab_size=cfg.vocab, hidden_size=cfg.hidden, num_hidden_layers=cfg.num_layers,
                                 num_attention_heads=cfg.heads, intermediate_size=cfg.ffn, max_position_embeddings=cfg.max_pos,
                                 type_vocab_size=cfg.type_vocab, layer_norm_eps=cfg.ln_eps, hidden_act="gelu", num_labels=1,
                                 attn_implementation="eager")
    m = transformers.BertForSequenceClassification(hc)
    w = presets.synthetic_weights(PRESET)
    w.update(presets.synthetic_head_weights(PRESET, 1))
    m.load_state_dict({("" if k.startswith("classifier.") else "bert.") + k: torch.from_numpy(v) for k, v in w.items()},
                      strict=True)
    m = m.eval().cuda()
    tok = tokenizer()
    t0 = time.perf_counter()
    enc = tok([a for a, _ in pairs], [b for _, b in pairs], truncation=True, max_length=512)
    tok_s = time.perf_counter() - t0
    order = np.argsort([len(x) for x in enc["input_ids"]], kind="stable")
    batches = []
    for s in range(0, len(pairs), batch):
        idx = order[s:s + batch]
        b = tok.pad({"input_ids": [enc["input_ids"][i] for i in idx], "token_type_ids": [enc["token_type_ids"][i] for i in idx]},
                    return_tensors="pt")
        batches.append((idx, {k: v.cuda() for k, v in b.items()}))
    res = {"part": "hf", "preset": PRESET, "pairs": len(pairs), "batch": batch, "tokenizer_s": round(tok_s, 3)}
    for mode in ("fp32", "fp16_autocast"):
        logits = np.empty(len(pairs), np.float32)
        times = []
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16, enabled=mode != "fp32"):
            for r in range(reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs = [(idx, m(**b).logits) for idx, b in batches]
                torch.cuda.synchronize()
                if r:
                    times.append(time.perf_counter() - t0)
            for idx, lg in outs:
                logits[idx] = lg.float()[:, 0].cpu().numpy()
        sec = float(np.median(times))
        res[f"{mode}_gpu_pairs_per_s"] = round(len(pairs) / sec)
        res[f"{mode}_ms"] = round(sec * 1e3, 1)
        nat_path = os.path.join(out_dir or "", "rerank_native_logits.npy")
        if out_dir and os.path.exists(nat_path):
            nat_logit = np.load(nat_path).astype(np.float64)
            res[f"{mode}_pearson_vs_native"] = round(float(np.corrcoef(nat_logit, logits.astype(np.float64))[0, 1]), 6)
            res[f"{mode}_max_abs_dlogit"] = round(float(np.abs(nat_logit - logits).max()), 5)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("native", "hf"), default="native")
    ap.add_argument("--out", default=None, help="directory for the native scores (the hf part correlates against them)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--candidates", type=int, default=100)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_rerank needs an MI355X"
    pairs = workload(a.queries, a.candidates)
    (part_native if a.part == "native" else part_hf)(pairs, a.out, a.reps)


if __name__ == "__main__":
    main()
