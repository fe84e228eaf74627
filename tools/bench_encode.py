#!/usr/bin/env python3
"""Quick encoder timing: python tools/bench_encode.py [preset] [n_sentences] [iters] [bf16|mxfp8] [head]

head: a sentence head run in place of the mean pool, as <pooling>[-dense][-norm] with pooling in mean, cls, max,
meansqrt (e.g. cls-dense-norm: CLS pooling, a seeded Dense hidden -> hidden with tanh, Normalize)."""
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
if head_name:
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
    enc.forward_packed(fd, cd, pos, cols, int(np.diff(cu).max()), pooled=True, unit=True, head=head)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(iters):
    enc.forward_packed(fd, cd, pos, cols, int(np.diff(cu).max()), pooled=True, unit=True, head=head)
e1.record()
torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / iters
H, F, L = cfg.hidden, cfg.ffn, cfg.num_layers
sbar = float((np.diff(cu).astype(np.float64) ** 2).sum() / T)
flops = T * L * (2 * (4 * H * H + 2 * H * F) + 4 * sbar * H)
print(json.dumps({"preset": preset, "weight_dtype": wdtype, "head": head_name, "sentences": n, "tokens": T, "ms": round(ms, 3),
                  "sentences_per_s": round(n / ms * 1e3), "tokens_per_s": round(T / ms * 1e3),
                  "TFLOPs": round(flops / ms / 1e9, 1)}))
