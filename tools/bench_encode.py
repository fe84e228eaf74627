#!/usr/bin/env python3
"""Quick encoder timing: python tools/bench_encode.py [preset] [n_sentences] [iters] [bf16|mxfp8] [head]

head: a sentence head run in place of the mean pool, as <pooling>[-dense][-norm] with pooling in mean, cls, max,
meansqrt (e.g. cls-dense-norm: CLS pooling, a seeded Dense hidden -> hidden with tanh, Normalize).
head = spans: times NativeEncoder.forward_spans instead, the mean-pool forward plus two spans of two tokens per sentence
(the WiC shape: a target word of two pieces in each of two places), float32 span rows and unit rows; the result line also
gives the span kernel's algorithmic bytes (listed tokens x H x 2 B read, S x H x 4 B written)."""
import sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from text_similarity_amd import presets
from text_similarity_amd.native_encoder import NativeEncoder

preset = sys.argv[1] if len(sys.argv) > 1 else "all-MiniLM-L6-v2"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 8192
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 5
wdtype = sys.argv[4] if len(sys.argv) > 4 else "bf16"
head_name = sys.argv[5] if len(sys.argv) > 5 else None
cfg = presets.PRESETS[preset]
flat, cu = presets.synthetic_token_batch(n, seed="sent1234", vocab_size=cfg.vocab, max_len=256)
T = int(cu[-1])
enc = NativeEncoder.from_preset(preset, max_tokens=T, max_seqs=n, weight_dtype=wdtype)
fd, cd = torch.from_numpy(flat).cuda(), torch.from_numpy(cu).cuda()
pos, cols = enc.positions(fd, cd)
head = None
span_mode = head_name == "spans"
if span_mode:
    lens = np.diff(cu).astype(np.int64)             # every sentence is CLS w.. SEP: at least 3 tokens
    first = np.stack([np.ones(n, dtype=np.int64), np.minimum(2, lens - 1)], 1)
    last = np.stack([lens - 2, lens - 1], 1)
    span_tok = np.stack([first, last], 1).reshape(-1).astype(np.int32)          # sentence by sentence: [1, 2], [len-2, len-1]
    span_seq = np.repeat(np.arange(n, dtype=np.int32), 2)
    span_cu = (np.arange(2 * n + 1, dtype=np.int64) * 2).astype(np.int32)
    tabs = [torch.from_numpy(a).cuda() for a in (span_seq, span_cu, span_tok)]
    span_bytes = int(span_tok.size * cfg.hidden * 2 + span_seq.size * cfg.hidden * 4)


units = cfg.hidden <= 768   # unit rows stop at the search width: a hidden-1024 preset is timed with its float32 rows alone


def forward():
    if span_mode:
        return enc.forward_spans(fd, cd, *tabs, span_unit=units, pooled=True, unit=units, pos=pos, cols=cols,
                                 max_len=int(np.diff(cu).max()))
    return enc.forward_packed(fd, cd, pos, cols, int(np.diff(cu).max()), pooled=True, unit=units, head=head)


if head_name and not span_mode:
    from text_similarity_amd.native_encoder import SentenceHead
    parts = head_name.split("-")
    mode = {"mean": "mean", "cls": "cls", "max": "max", "meansqrt": "mean_sqrt_len"}[parts[0]]
    unknown = set(parts[1:]) - {"dense", "norm"}
    if unknown:
        raise SystemExit(f"unknown head part(s) {sorted(unknown)}: <pooling>[-dense][-norm]")
    w = b = None
    if "dense" in parts:
        H = cfg.hidden
        w = torch.from_numpy(presets.normal("bench/dense_w", H * H).reshape(H, H) / np.sqrt(H)).float().cuda()
        b = torch.from_numpy(presets.normal("bench/dense_b", H) * 0.02).float().cuda()
    head = SentenceHead(mode, w, b, "tanh" if w is not None else "identity", "norm" in parts)
for _ in range(2):
    forward()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(iters):
    forward()
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / iters
H, F, L = cfg.hidden, cfg.ffn, cfg.num_layers
sbar = float((np.diff(cu).astype(np.float64) ** 2).sum() / T)
flops = T * L * (2 * (4 * H * H + 2 * H * F) + 4 * sbar * H)
print(json.dumps({"preset": preset, "weight_dtype": wdtype, "head": head_name, "sentences": n, "tokens": T, "ms": round(ms, 3),
                  "sentences_per_s": round(n / ms * 1e3), "tokens_per_s": round(T / ms * 1e3),
                  "TFLOPs": round(flops / ms / 1e9, 1),
                  **({"spans": int(span_seq.size), "span_tokens": int(span_tok.size), "span_kernel_bytes": span_bytes}
                     if span_mode else {})}))
