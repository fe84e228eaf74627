"""Encoder configurations that tsim_encoder_create accepts and the four shapes of encoder_cases / arch_cases do not reach
(builders only; no GPU).  Used by tests/test_encoder_power_cpu.py (the proof that the bound separates right from wrong) and
tests/test_encoder_config_gpu.py (the kernels against it).  Weights, inputs, probe and tolerance rule are encoder_cases' own,
borrowed through ``registered`` the way arch_cases does.

The routes these cases reach (and those of encoder_cases / arch_cases) are DESIGN.md's table "Encoder routes by configuration";
tests/test_encoder_route_cpu.py holds that table as data and checks every case here against the encoder's plan
(tsim_encoder_route_host), so the table is not repeated in this file.

Departures from the proposed set: bert-768-h24-f1920 runs the 128-wide tile, but not pack_w(.., BN = 128): the encoder packs only
the QKV and O matrices (N = 3H and H, multiples of 256) and FFN1 reads row-major W, so no accepted configuration calls pack_w
with BN = 128.  bert-384-f2112 is added: F % 192 == 0 above 2048 used to reach gemm_xres2's N <= 2048 refusal at the first
forward (it takes the 128x64 tile now, like any F that is no multiple of 128).  No case was dropped.

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
