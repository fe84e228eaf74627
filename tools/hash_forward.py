#!/usr/bin/env python3
"""sha256 of the hidden rows and pooled rows of fixed forwards, as JSON on stdout.  Run on the commit whose bits are to be kept
(or on its library: TSIM_LIB=<path>) and store the output under tests/golden/; a test recomputes and compares.

    python tools/hash_forward.py > tests/golden/residual_stream_parent.json
        the residual-stream cases (tests/residual_cases.py) and MiniLM at the benchmark's token count;
        tests/test_residual_packed_gpu.py
    python tools/hash_forward.py x384-rowmajor > tests/golden/x384_rowmajor_parent.json
        the row-major K = 384 projection (residual_cases.X384_*); tests/test_x384_rowmajor_parent_gpu.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import residual_cases as rc  # noqa: E402
from text_similarity_amd.native_encoder import NativeEncoder  # noqa: E402

which = sys.argv[1] if len(sys.argv) > 1 else "residual-stream"
out = {}
flat, cu = rc.sentences()
if which == "residual-stream":
    for L in rc.LAYERS:
        enc = NativeEncoder(rc.config(L), rc.weights(L), max_tokens=rc.MAX_T, max_seqs=rc.N_SENT)
        for T in rc.TOKENS:
            f, c = rc.cut(flat, cu, T)
            out[rc.case_id(L, T)] = rc.digests(*rc.encode(enc, f, c))
        del enc
    f, c = rc.minilm_sentences()
    enc = NativeEncoder.from_preset("all-MiniLM-L6-v2", max_tokens=rc.MINILM_T, max_seqs=rc.MINILM_SENT)
    out[f"all-MiniLM-L6-v2-T{rc.MINILM_T}"] = rc.digests(*rc.encode(enc, f, c))
elif which == "x384-rowmajor":
    enc = rc.x384_encoder()
    for T in rc.X384_TOKENS:
        f, c = rc.cut(flat, cu, T)
        out[rc.x384_case_id(T)] = rc.digests(*rc.encode(enc, f, c))
else:
    raise SystemExit(f"unknown set {which!r}: residual-stream or x384-rowmajor")
json.dump(out, sys.stdout, indent=1, sort_keys=True)
print()
