"""Cases shared by tests/test_residual_packed_gpu.py and tools/hash_forward.py: small hidden-384 BERT encoders (1, 2 and 3
layers: the first layer reads a row-major residual stream, the last one writes one, a one-layer model does both) at token
counts around the 32-row and 256-row block boundaries, the gemm_bf16 fallback form (10 000 tokens: no ln_rows round and more
than 8 192 rows) and ln_rows plus a remainder (32 768 + 33)."""
import hashlib

import numpy as np

from text_similarity_amd import presets
from text_similarity_amd.presets import EncoderConfig

LAYERS = (1, 2, 3)
TOKENS = (1, 31, 32, 33, 255, 256, 257, 10000, 32768 + 33)
MAX_T = 32768 + 33
N_SENT = 2600                       # ~16 tokens per sentence: more than MAX_T tokens
MINILM_T = 65536 + 1650             # the benchmark's shape, on the all-MiniLM-L6-v2 preset
MINILM_SENT = 5000


def config(layers: int) -> EncoderConfig:
    return EncoderConfig("bert", layers, 384, 12, 1536, 1000, 64, 1e-12)


def weights(layers: int):
    return presets.synthetic_weights(f"residual-packed-{layers}", cfg=config(layers))


def cut(flat, cu, T):
    """The first sentences of the list holding exactly T tokens (the last one shortened)."""
    n = int(np.searchsorted(cu, T, side="left"))
    c = cu[:n + 1].astype(np.int64).copy()
    c[n] = T
    assert c[n] > c[n - 1]
    return np.ascontiguousarray(flat[:T]), c


def sentences():
    flat, cu = presets.synthetic_token_batch(N_SENT, seed="residual-packed", vocab_size=1000, max_len=64)
    assert int(cu[-1]) >= MAX_T
    return flat, cu.astype(np.int64)


def minilm_sentences():
    cfg = presets.PRESETS["all-MiniLM-L6-v2"]
    flat, cu = presets.synthetic_token_batch(MINILM_SENT, seed="ln-remainder", vocab_size=cfg.vocab, max_len=64)
    return cut(flat, cu.astype(np.int64), MINILM_T)


def encode(enc, flat, cu):
    """(pooled f32 [B, H], hidden bf16 [T, H]) on the device."""
    import torch
    r = enc.forward_packed(torch.from_numpy(np.ascontiguousarray(flat)).to("cuda:0"),
                           torch.from_numpy(cu.astype(np.int32)).to("cuda:0"), hidden=True)
    torch.cuda.synchronize()
    return r["pooled"], r["hidden"]


def digests(pooled, hidden):
    import torch
    h = hidden.contiguous().view(torch.int16).cpu().numpy().tobytes()
    p = pooled.contiguous().cpu().numpy().tobytes()
    return {"hidden": hashlib.sha256(h).hexdigest(), "pooled": hashlib.sha256(p).hexdigest()}


def case_id(layers: int, T: int) -> str:
    return f"bert384-L{layers}-T{T}"


# The row-major K = 384 projection (gemm_xres2_kernel<EPI, false, false>: an MPNet-style hidden-384 model keeps its residual
# stream row-major): the mpnet-384 case of tests/encoder_cases.py on the sentences above, at the smallest token counts that reach
# every state of the item loop.  Items per workgroup are ceil(T / 256) * N / 96 over min(items, 256) workgroups, N = 1152, 1536:
# 33: one partial block (the row guard of the stores); 257: one item per workgroup (first item and flush only); 10 000: 1-2 and
# 2-3 items (both flush sides, a fragment reload inside a workgroup); 16 417: 3-4 and 4-5 items (the two-item loop body taken
# more than once, odd and even tails).
X384_CASE = "mpnet-384"
X384_TOKENS = (33, 257, 10000, 16417)


def x384_encoder():
    import encoder_cases as ec
    from text_similarity_amd.native_encoder import NativeEncoder
    cfg, wdtype = ec.CASES[X384_CASE]
    return NativeEncoder(cfg, ec.sharp_weights(cfg, X384_CASE), max_tokens=max(X384_TOKENS), max_seqs=N_SENT, weight_dtype=wdtype)


def x384_case_id(T: int) -> str:
    return f"{X384_CASE}-T{T}"
