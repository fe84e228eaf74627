#!/usr/bin/env python3
"""Does the time of the search phase depend on what runs in front of it?  bench.py's step (encode 4 096 sentences, cosine top-10
against 1 M x 384 rows) with the same library in five forms, `phases.search_ms` measured as bench.py measures it (events around
the search call), mean, median and min .. max over the steps:

    encode+search          bench.py's step
    search only            the search calls back to back on embeddings computed beforehand: no encoder phase at all
    encode+pause+search    an idle spin kernel of --pause-us (default 130) between the encoder and the search
    pause+encode+search    the same pause in FRONT of the encoder: the step is as long, the search still follows the encoder directly
    encode+pause4+search   four times the pause between the encoder and the search

    TSIM_LIB=.../libtsim_<tag>.so python3 tools/search_after_encode.py [--steps 20] [--warmup 5] [--pause-us 130]

The search kernels and their inputs are the same in all five; what differs is how much matrix-pipe load and how much idle time
the chip has seen in the milliseconds before."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from text_similarity_amd import ops, presets
from text_similarity_amd.distributed.sharded_search import ShardedCorpusSearch
from text_similarity_amd.native_encoder import NativeEncoder

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--pause-us", type=float, default=130.0)
ap.add_argument("--rows", type=int, default=1_000_000)
ap.add_argument("--rounds", type=int, default=2, help="every form this many times, interleaved")
args = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
cfg = presets.PRESETS["all-MiniLM-L6-v2"]
d, k, Q, nb = cfg.hidden, 10, 4096, 8
g = torch.Generator(device=dev).manual_seed(4321)
corpus_f32 = torch.randn((args.rows, d), generator=g, device=dev)
corpus, rho = ops.l2norm_rows(corpus_f32, return_rho=True)
flat_h, cu_h = presets.synthetic_token_batch(Q * nb, seed="sent1234", vocab_size=cfg.vocab, max_len=256)
batches = []
for b in range(nb):
    t0, t1 = int(cu_h[b * Q]), int(cu_h[b * Q + Q])
    batches.append((torch.from_numpy(flat_h[t0:t1]).to(dev), torch.from_numpy((cu_h[b * Q:b * Q + Q + 1] - cu_h[b * Q]).astype(np.int32)).to(dev)))
enc = NativeEncoder.from_preset("all-MiniLM-L6-v2", max_tokens=max(int(f.numel()) for f, _ in batches), max_seqs=Q, device=dev)
pos = [enc.positions(f, c) for f, c in batches]
max_len = [int((c[1:] - c[:-1]).max().item()) for _, c in batches]
engine = ShardedCorpusSearch(corpus, d, 0, corpus_f32_local=corpus_f32, corpus_rho=rho)
stream = torch.cuda.current_stream(dev)
ev = lambda: torch.cuda.Event(enable_timing=True)


def encode(i):
    f, c = batches[i % nb]
    p, cols = pos[i % nb]
    return enc.forward_packed(f, c, p, cols, max_len[i % nb], pooled=True, unit=False)["pooled"]


embs = [encode(i).clone() for i in range(nb)]
# spin-kernel cycles per microsecond
a, b = ev(), ev()
torch.cuda._sleep(1000)
a.record(stream); torch.cuda._sleep(2_000_000); b.record(stream); torch.cuda.synchronize()
cyc_per_us = 2_000_000 / (a.elapsed_time(b) * 1e3)
pause = int(args.pause_us * cyc_per_us)


def run(mode):
    recs = []
    for i in range(args.warmup + args.steps):
        e0, e1, e2 = ev(), ev(), ev()
        for e in (e0, e1, e2):
            e.record(stream)
        if i == args.warmup:
            torch.cuda.synchronize()
        e0.record(stream)
        if mode == "pause+encode+search":
            torch.cuda._sleep(pause)
        emb = embs[i % nb] if mode == "search only" else encode(i)
        if mode == "encode+pause+search":
            torch.cuda._sleep(pause)
        if mode == "encode+pause4+search":
            torch.cuda._sleep(4 * pause)
        e1.record(stream)
        engine.search(emb, k, counts=[Q])
        e2.record(stream)
        if i >= args.warmup:
            recs.append((e0, e1, e2))
    torch.cuda.synchronize()
    s = [x[1].elapsed_time(x[2]) for x in recs]
    st = [x[0].elapsed_time(x[2]) for x in recs]
    return {"search_ms": round(float(np.mean(s)), 4), "search_med": round(float(np.median(s)), 4), "search_min": round(min(s), 4), "search_max": round(max(s), 4),
            "step_ms": round(float(np.mean(st)), 4)}


out = {"lib": os.path.basename(os.environ.get("TSIM_LIB", "libtsim.so")), "pause_us": args.pause_us, "spin_cycles_per_us": round(cyc_per_us, 1)}
for rnd in range(args.rounds):
    for mode in ("encode+search", "search only", "encode+pause+search", "pause+encode+search", "encode+pause4+search"):
        out[f"{mode} #{rnd + 1}"] = run(mode)
print(json.dumps(out))
