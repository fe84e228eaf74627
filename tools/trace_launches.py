#!/usr/bin/env python3
"""The launches of one encoder forward, to compare two libraries (TSIM_LIB=<path> selects the one that runs).

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 tools/trace_launches.py run CASE
    python3 tools/trace_launches.py list DIR CASE >> launches.txt

run   creates the encoder of CASE and runs ONE forward (pooled rows, unit rows where the width allows, hidden states), one
      process per case.  CASES below: one per family of the encoder's plan and per token-count class of the hidden-384 layer.
list  the dispatches of the newest *kernel_trace.csv under DIR in dispatch order, one line each:
      kernel name | grid | workgroup | LDS bytes.  Two libraries launch the same kernels when their lists are equal (diff).
"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# case -> (name in encoder_cases.CASES / config_cases.CASES, sentences)
CASES = {
    "tiny-bert": ("tiny-bert", 48),
    "bert-384-n48": ("bert-384", 48),                # ln_split
    "bert-384-n2300": ("bert-384", 2300),            # ln_rows_gemm + tail
    "bert-384-n4700": ("bert-384", 4700),            # one whole round: chained launches, + the remainder
    "bert-384-f1024-n2300": ("bert-384-f1024", 2300),   # row-major, K = 1024: gemm_bf16 x 384 tiles behind ln_rows_gemm
    "mpnet-384-n2300": ("mpnet-384", 2300),
    "bert-768": ("bert-768", 48),
    "bert-768-h48-f1984": ("bert-768-h48-f1984", 48),
    "bert-768-mxfp8": ("bert-768-mxfp8", 48),
}


def run(case):
    import torch
    import config_cases
    import encoder_cases
    from text_similarity_amd import presets
    from text_similarity_amd.native_encoder import NativeEncoder
    name, n = CASES[case]
    cfg, wdtype = {**encoder_cases.CASES, **config_cases.CASES}[name]
    flat, cu = presets.synthetic_token_batch(n, seed="trace", vocab_size=encoder_cases.VOCAB, max_len=64)
    enc = NativeEncoder(cfg, presets.synthetic_weights("trace/" + name, cfg), max_tokens=int(cu[-1]), max_seqs=n, weight_dtype=wdtype)
    dev = torch.device("cuda", torch.cuda.current_device())
    r = enc.forward_packed(torch.from_numpy(flat).to(dev), torch.from_numpy(cu).to(dev), pooled=True, unit=cfg.hidden <= 768, hidden=True)
    torch.cuda.synchronize()
    enc.check()
    assert torch.isfinite(r["pooled"]).all()
    print(f"{case}: {n} sentences, {int(cu[-1])} tokens")


def listing(d, case):
    f = max(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True), key=os.path.getmtime)
    rows = [{k.lower(): v for k, v in r.items()} for r in csv.DictReader(open(f, newline=""))]   # (the headers' case varies by version)
    rows.sort(key=lambda r: int(r["dispatch_id"]))
    print(f"# {case}: {len(rows)} dispatches")
    for r in rows:
        grid = "x".join(r[f"grid_size_{a}"] for a in "xyz")
        wg = "x".join(r[f"workgroup_size_{a}"] for a in "xyz")
        print(f"{r['kernel_name']} | {grid} | {wg} | {r['lds_block_size']}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "run" and sys.argv[2] in CASES:
        run(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "list":
        listing(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
