"""Encoder configurations that tsim_encoder_create accepts and the four shapes of encoder_cases / arch_cases do not reach
(builders only; no GPU).  Used by tests/test_encoder_power_cpu.py (the proof that the bound separates right from wrong) and
tests/test_encoder_config_gpu.py (the kernels against it).  Weights, inputs, probe and tolerance rule are encoder_cases' own,
borrowed through ``registered`` the way arch_cases does.

ROUTE TABLE (DESIGN.md "Encoder routes by configuration" holds the same table).  Read from tsim_encoder_create,
tsim_encoder_forward_ex, gemm_plain, gemm_res_ln, use_packed_layout, gemm_pp / launch_pp.  H = hidden, F = ffn, DH = H / heads,
T = tokens of a call.  "new" cases are this file's, the others encoder_cases' / arch_cases'.

Attention (every H): attention_kernel<DH, REL, PK>, one workgroup = 4 heads, a partial last group when heads % 4 != 0.
    plain  DH 16 tiny-bert, bert-768-h48-f1984 (new) | DH 32 bert-384-f1024, bert-768-h24-f1920, bert-1024-h32-f2816 (new) | DH 64 bert-768
    REL    DH 16 tiny-mpnet | DH 32 mpnet-384 | DH 64 mpnet-768, mpnet-64-h1-f320, mpnet-384-h6-f2048 (new)      (MPNet)
    PK     DH 16 bert-384-h24-f1920 (new) | DH 32 bert-384 | DH 64 bert-384-h6-f768 (new)                        (H 384 packed)
    partial group: bert-64-h2-f64 (2 of 4), mpnet-64-h1-f320 (1 of 4), bert-384-h6-f768 / mpnet-384-h6-f2048 (4 + 2) (new)

H = 64 (bf16 only):
    QKV   gemm_bf16 128x64 tile (N = 192)                      O + LN  gemm_bf16 128x64 RES_LN, K = 64
    FFN1  F % 128 == 0: gemm_bf16 128x128 (tiny-bert)          F % 128 != 0: gemm_bf16 128x64 (bert-64-h2-f64 N = 64, mpnet-64-h1-f320 N = 320)
    FFN2 + LN  gemm_bf16 128x64 RES_LN, K = F (128 tiny-*, 64, 320 new)

H = 384 (bf16 only; MXFP8 refused: 384 % 256 != 0; F = 64 refused: test_refused_configurations):
    packed (BERT family, F % 192 == 0, F <= 1920: use_packed_layout): qkv, h1 and the residual stream block-packed
        QKV / FFN1  gemm_xres2<PK>, or chained behind the previous LayerNorm GEMM (ln_rows_xres2) when F <= 1536 and T has whole
                    rounds of 256 x 256 tokens;  O / FFN2 + LN by T: ln_tail / ln_split (T <= 8192), ln_rows_gemm + tail, + the
                    gemm_bf16 64x384 remainder.  F = 1536: bert-384.  F = 768 (K = 768, other tile counts): bert-384-h6-f768, also at
                    n = 2300 / 4700 sentences (chained).  F = 1920 (chain off): bert-384-h24-f1920, also at n = 4700.
    row-major (MPNet, or F not a multiple of 192, or F > 1920):
        QKV  gemm_xres2 (N = 1152)
        FFN1 F % 192 == 0 and F <= 2048: gemm_xres2 (mpnet-384) | otherwise gemm_bf16 128x128 (bert-384-f1024, mpnet-384-h6-f2048) or,
             when F % 128 != 0, 128x64 (bert-384-f2112).  F % 192 == 0 above 2048 (bert-384-f2112) used to reach gemm_xres2's
             N <= 2048 refusal at the first forward: fixed in gemm_plain, it now takes the plain tiles like any other F
        O / FFN2 + LN  K % 192 == 0: as packed, row-major operands (mpnet-384 K = 1536, bert-384-f2112 K = 2112) | otherwise
             ln_rows_gemm + gemm_bf16 128x384 / 64x384 (bert-384-f1024 K = 1024, also at n = 2300; mpnet-384-h6-f2048 K = 2048)

H = 768 / 1024 (F = 64 refused: FFN2 has no kernel for K = 64; test_refused_configurations):
    bf16, F % 128 == 0: QKV gemm_pp 256-wide tile on packed W (pqkv), O gemm_pp F32 on packed W (po) + res_ln_rows,
        FFN1 gemm_pp GELU on row-major W, 256-wide (F % 256 == 0: bert-768 3072, bert-1024 4096, bert-1024-h32-f2816 11 tiles) or
        128-wide (F = 128 x odd: bert-768-h24-f1920), FFN2 gemm_pp F32 K = F on row-major W + res_ln_rows
    bf16, F = 64 x odd: no packed weights (QKV and O through gemm_pp on row-major W), FFN1 gemm_bf16 128x64, K = H,
        FFN2 gemm_pp F32 with an odd number of k-tiles (bert-768-h48-f1984: 31)
    mxfp8 (F % 256 == 0; any other F refused: test_refused_configurations): quant_mx, gemm_pp_mx BIAS / F32 / GELU_MX, res_ln_rows<QUANT>; F = 3072 / 4096 (encoder_cases, arch_cases),
        F = 2048 (bert-768-h24-f2048-mxfp8: 8 GELU_MX tiles, scale rows of 64 bytes, FFN2 K = 2048)

Departures from the proposed set: bert-768-h24-f1920 runs the 128-wide tile, but not pack_w(.., BN = 128): the encoder packs only
the QKV and O matrices (N = 3H and H, multiples of 256) and FFN1 reads row-major W, so no accepted configuration calls pack_w
with BN = 128.  bert-384-f2112 is added: the route table shows F % 192 == 0, F > 2048 reached gemm_xres2's N <= 2048 refusal at
the first forward.  No case was dropped.

Weight scales: ``encoder_cases._QK_A`` / ``_VO_A`` are keyed by hidden size; ``QK_A`` below holds a case's own scale where the
head_dim moves the median largest probability out of [0.2, 0.9] (figures next to it, float64 probe, layer 1 / layer 2).
"""
import contextlib
import functools

import numpy as np

import encoder_cases as ec
from text_similarity_amd.presets import EncoderConfig

V = ec.VOCAB


def _bert(H, heads, F):
    return EncoderConfig("bert", 2, H, heads, F, V, 260, 1e-12)


def _mpnet(H, heads, F):
    return EncoderConfig("mpnet", 2, H, heads, F, V, 262, 1e-5, type_vocab=0, pad_id=1)


# name -> (configuration, weight_dtype)
CASES = {
    "bert-64-h2-f64": (_bert(64, 2, 64), "bf16"),
    "mpnet-64-h1-f320": (_mpnet(64, 1, 320), "bf16"),
    "bert-384-h6-f768": (_bert(384, 6, 768), "bf16"),
    "bert-384-h24-f1920": (_bert(384, 24, 1920), "bf16"),
    "bert-384-f1024": (_bert(384, 12, 1024), "bf16"),
    "bert-384-f2112": (_bert(384, 12, 2112), "bf16"),
    "mpnet-384-h6-f2048": (_mpnet(384, 6, 2048), "bf16"),
    "bert-768-h24-f1920": (_bert(768, 24, 1920), "bf16"),
    "bert-768-h48-f1984": (_bert(768, 48, 1984), "bf16"),
    "bert-768-h24-f2048-mxfp8": (_bert(768, 24, 2048), "mxfp8"),
    "bert-1024-h32-f2816": (_bert(1024, 32, 2816), "bf16"),
}

# configurations tsim_encoder_create refuses (tests/test_encoder_config_gpu.py::test_refused_configurations):
# (cfg, dtype, pattern of the C error text)
REFUSED = {
    "bert-384-f64": (_bert(384, 12, 64), "bf16", "encoder_create: ffn=64 unsupported at hidden=384 .*at least 128"),
    "bert-768-f64": (_bert(768, 12, 64), "bf16", "encoder_create: ffn=64 unsupported at hidden=768 .*at least 128"),
    "bert-1024-f64": (_bert(1024, 16, 64), "bf16", "encoder_create: ffn=64 unsupported at hidden=1024 .*at least 128"),
    "bert-768-f1920-mxfp8": (_bert(768, 24, 1920), "mxfp8", r"encoder_create: MXFP8 .*multiples of 256 \(got 768, 1920\)"),
}

QK_A_1024, VO_A_1024 = 0.085, 0.10      # arch_cases' hidden-1024 scales (measured there)
# case -> its own Q/K scale.  bert-64-h2-f64: at two heads of 32 dims the hidden-64 scale 0.25 leaves layer 1 at a median
# largest probability of 0.150 (layer 2: 0.344), below the band; 0.32 gives 0.312 / 0.539 (0.38: 0.459 / 0.690).
QK_A = {"bert-64-h2-f64": 0.32}
# case -> factor on the FFN2 columns of the features that ``ffn_tail_dropped`` zeroes.  The MXFP8 case carries
# sharp_weights' FFN2 x 1/4, under which the 64 tail features of 2048 move the output by 1.5 x TOL only; x 4 puts those
# columns back at the bf16 cases' scale (measured ratio in tests/test_encoder_power_cpu.py's docstring).
F2_TAIL = {"bert-768-h24-f2048-mxfp8": 4.0}


@contextlib.contextmanager
def registered():
    """encoder_cases' builders look a case up by name: inside this block they know this file's cases (removed again afterwards,
    so the parametrised tests over ``encoder_cases.CASES`` keep their cases)."""
    ec.CASES.update(CASES)
    had = 1024 in ec._QK_A
    if not had:
        ec._QK_A[1024], ec._VO_A[1024] = QK_A_1024, VO_A_1024
    try:
        yield
    finally:
        for k in CASES:
            ec.CASES.pop(k, None)
        if not had:
            ec._QK_A.pop(1024, None)
            ec._VO_A.pop(1024, None)


@functools.lru_cache(maxsize=None)
def weights(name):
    """``encoder_cases.sharp_weights`` of a case under its own Q/K scale, then its ``F2_TAIL`` factor (a power of two: the
    weights stay bf16-exact).  A new dict; encoder_cases' cached one is left as it is."""
    cfg, _ = CASES[name]
    with registered():
        keep = ec._QK_A[cfg.hidden]
        ec._QK_A[cfg.hidden] = QK_A.get(name, keep)
        try:
            w = dict(ec.sharp_weights(cfg, name))
        finally:
            ec._QK_A[cfg.hidden] = keep
    if name in F2_TAIL:
        tail = cfg.ffn % 128 or 64
        for k in [k for k in w if _is_ffn2_weight(k)]:
            w[k] = w[k].copy()
            w[k][:, cfg.ffn - tail:] *= np.float32(F2_TAIL[name])
    return w


def _is_ffn2_weight(tensor):
    return tensor.startswith("encoder.layer.") and tensor.endswith(".weight") and "LayerNorm" not in tensor and ec._role(tensor) == "f2"


def inputs(name):
    with registered():
        return ec.case_inputs(name)


def probe(name, **kw):
    w = weights(name)
    with registered():
        return ec.probe(name, w, **kw)


@functools.lru_cache(maxsize=None)
def tolerances(name):
    """(exact, floor, tol) by the rule of ``encoder_cases.tolerances``, on this file's weights: floor = the probe's
    bf16-rounded run against its float64 run, tol = TOL_FACTOR x floor, computed here."""
    cfg, _ = CASES[name]
    _, cu, _ = inputs(name)
    exact = probe(name)
    rounded = probe(name, rounding="bf16")
    floor = {b: ec.errors(rounded[b], exact[b]) for b in range(1, cfg.num_layers + 1)}
    floor["pooled"] = ec.errors(ec.pooled_rows(rounded[-1], cu), ec.pooled_rows(exact[-1], cu))
    tol = {b: {m: ec.TOL_FACTOR * v for m, v in f.items()} for b, f in floor.items()}
    return exact, floor, tol
