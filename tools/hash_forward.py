#!/usr/bin/env python3
"""sha256 of the hidden rows and pooled rows of the residual-stream cases (tests/residual_cases.py) and of MiniLM at the
benchmark's token count, as JSON on stdout.  Run on the commit whose bits are to be kept and store the output as
tests/golden/residual_stream_parent.json; tests/test_residual_packed_gpu.py recomputes and compares.

    python tools/hash_forward.py > tests/golden/residual_stream_parent.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import residual_cases as rc  # noqa: E402
from text_similarity_amd.native_encoder import NativeEncoder  # noqa: E402

out = {}
flat, cu = rc.sentences()
for L in rc.LAYERS:
    enc = NativeEncoder(rc.config(L), rc.weights(L), max_tokens=rc.MAX_T, max_seqs=rc.N_SENT)
    for T in rc.TOKENS:
        f, c = rc.cut(flat, cu, T)
        out[rc.case_id(L, T)] = rc.digests(*rc.encode(enc, f, c))
    del enc
f, c = rc.minilm_sentences()
enc = NativeEncoder.from_preset("all-MiniLM-L6-v2", max_tokens=rc.MINILM_T, max_seqs=rc.MINILM_SENT)
out[f"all-MiniLM-L6-v2-T{rc.MINILM_T}"] = rc.digests(*rc.encode(enc, f, c))
json.dump(out, sys.stdout, indent=1, sort_keys=True)
print()
