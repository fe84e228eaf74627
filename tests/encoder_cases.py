"""Encoder test cases under which every stage of the forward matters (test data builders and the error metrics; no GPU).

``presets.synthetic_weights`` gives almost-zero attention logits, an almost-uniform softmax and LayerNorm gammas within
10 % of 1: most of the encoder's arithmetic has no visible effect on its output.  ``sharp_weights`` draws weights under
which it does, ``case_inputs`` a packed batch at the lengths and edges where kernels go wrong, and ``tolerances`` derives
the bound a bf16 encoder has to meet from the float64 probe oracle alone (oracle/encoder_probe.py): never from a kernel.
Used by tests/test_encoder_power_cpu.py (the proof that the bound separates right from wrong) and
tests/test_encoder_sharp_gpu.py (the kernels against it)."""
import functools
from dataclasses import replace

import numpy as np

from oracle import encoder_probe, fp8_ref
from text_similarity_amd import presets
from text_similarity_amd.presets import EncoderConfig

VOCAB = 2000
LOWVAR_IDS = tuple(range(1990, 1998))     # vocabulary rows overwritten with c + 2^-10 u (LayerNorm eps check)
LOWVAR_C = 0.5

# name -> (configuration, weight_dtype)
CASES = {
    "tiny-bert": (replace(presets.PRESETS["tiny-bert"], vocab=VOCAB), "bf16"),
    "tiny-mpnet": (replace(presets.PRESETS["tiny-mpnet"], vocab=VOCAB), "bf16"),
    "bert-384": (EncoderConfig("bert", 2, 384, 12, 1536, VOCAB, 260, 1e-12), "bf16"),
    "mpnet-384": (EncoderConfig("mpnet", 2, 384, 12, 1536, VOCAB, 262, 1e-5, type_vocab=0, pad_id=1), "bf16"),
    "bert-768": (EncoderConfig("bert", 2, 768, 12, 3072, VOCAB, 260, 1e-12), "bf16"),
    "mpnet-768": (EncoderConfig("mpnet", 2, 768, 12, 3072, VOCAB, 262, 1e-5, type_vocab=0, pad_id=1), "bf16"),
    "bert-768-mxfp8": (EncoderConfig("bert", 2, 768, 12, 3072, VOCAB, 260, 1e-12), "mxfp8"),
    "mpnet-768-mxfp8": (EncoderConfig("mpnet", 2, 768, 12, 3072, VOCAB, 262, 1e-5, type_vocab=0, pad_id=1), "mxfp8"),
}

# Q/K matrices are U(-a, a) with a chosen per hidden size so that the logits q.k / sqrt(head_dim) have a spread of a few
# units whatever H is (their standard deviation grows like H a^2 / 3 times the mean square of a LayerNorm output).
_QK_A = {64: 0.25, 384: 0.115, 768: 0.085}
_VO_A = {64: 0.19, 384: 0.10, 768: 0.10}


def _lowvar_rows(H):
    u = np.where(np.arange(H) % 2 == 0, 1.0, -1.0)
    return (LOWVAR_C + 2.0 ** -10 * u).astype(np.float32)            # bf16-exact values, row variance 2^-20 = 9.5e-7


def _role(tensor: str) -> str:
    """Which projection of a layer a tensor name belongs to: q, k, v, o, f1 (FFN1) or f2 (FFN2)."""
    part = tensor.split(".")[-2]
    if ".attention." in tensor:
        return {"query": "q", "q": "q", "key": "k", "k": "k", "value": "v", "v": "v"}.get(part, "o")
    return "f1" if ".intermediate." in tensor else "f2"


@functools.lru_cache(maxsize=None)
def sharp_weights(cfg: EncoderConfig, name: str):
    """Deterministic float32 weights from the ``presets`` counter streams (stream "sharp/<name>/<tensor>"), bf16-exact:
    embeddings U(-a0, a0), a0 = 0.02 sqrt(3) (word, position and token-type rows of equal size, so each of them moves the
    embedding LayerNorm input); Q/K matrices U(-a, a) with a = 0.25 / 0.115 / 0.085 at hidden 64 / 384 / 768; V, O and
    FFN2 matrices 2 a0; FFN1 matrix 4 a0; biases of Q, K, V, O and FFN1 U(-10 a0, 10 a0), of FFN2 U(-a0, a0); LayerNorm
    gamma U(0.5, 1.5) with every 17th feature x 3, beta U(-0.2, 0.2); MPNet relative bias U(-3, 3).

    Achieved on the inputs of ``case_inputs`` (float64 probe, layer 1 / layer 2; tests/test_encoder_power_cpu.py prints
    and bounds them): median over (head, query) of the largest probability, sequences of >= 16 tokens, between 0.2 and
    0.9 in every case; FFN1 pre-activations reach |x| >= 3 in every case.

    Eight vocabulary rows (``LOWVAR_IDS``) are set so that the embedding-LayerNorm INPUT of the token LOWVAR_IDS[j] at
    column j is c + 2^-10 u, u = +1, -1, ... (variance 9.5e-7, between the two architectures' eps 1e-12 and 1e-5): the row
    is that target minus the token-type row 0 and the position row of column j, in float32 (these eight rows are not
    bf16-exact; the embedding tables are float32 on the device).

    MXFP8 cases (name ends in "mxfp8"): FFN2 matrix x 1/4 and V, O x 1.4.  Their rounding floor is ~6x the bf16 one (a
    bf16-sized change of an activation flips e4m3 roundings), most of it from the FFN; with a smaller FFN share of the
    residual stream the attention defects stand >= 4 x TOL there too."""
    a0 = np.float32(0.02 * np.sqrt(3.0))
    mx = name.endswith("mxfp8")     # see the docstring: FFN2 x 1/4, V and O x 1.4
    vo = np.float32(_VO_A[cfg.hidden] * (1.4 if mx else 1.0))
    w_scale = {"q": np.float32(_QK_A[cfg.hidden]), "k": np.float32(_QK_A[cfg.hidden]), "v": vo, "o": vo,
               "f1": 4 * a0, "f2": 2 * a0 * np.float32(0.25 if mx else 1.0)}
    b_scale = {"q": np.float32(1.0), "k": np.float32(1.0), "v": 10 * a0, "o": 10 * a0, "f1": 10 * a0, "f2": a0}
    out = {}
    for tensor, shape, kind in presets.weight_names(cfg):
        n = int(np.prod(shape))
        u = presets.uniform01(f"sharp/{name}/{tensor}", n) * np.float32(2.0) - np.float32(1.0)
        if kind == "w":
            x = u * (w_scale[_role(tensor)] if tensor.startswith("encoder.") else a0)
        elif kind == "b":
            x = u * (np.float32(0.2) if "LayerNorm" in tensor else b_scale[_role(tensor)])
        elif kind == "g":
            x = np.float32(1.0) + u * np.float32(0.5)
            x[::17] *= np.float32(3.0)
        else:
            x = u * np.float32(3.0)
        out[tensor] = presets.bf16_round(x.reshape(shape).astype(np.float32))
    word = out["embeddings.word_embeddings.weight"]
    posw = out["embeddings.position_embeddings.weight"]
    target = _lowvar_rows(cfg.hidden)
    for j, tid in enumerate(LOWVAR_IDS):
        if cfg.arch == "bert":
            word[tid] = (target - out["embeddings.token_type_embeddings.weight"][0]) - posw[j]
        else:
            word[tid] = target - posw[cfg.pad_id + 1 + j]
    return out


LENGTHS = (17, 2, 15, 129, 16, 31, 0, 32, 33, 63, 255, 1, 256, 64, 65, 127, 128)


@functools.lru_cache(maxsize=None)
def case_inputs(name: str):
    """Packed (flat ids int32 [T], cu int64 [B+1], notes) of a case.  Sequences, in this order: the lengths ``LENGTHS``
    that the position table allows (an empty sequence among them; the length-1 sequence sits between the two longest),
    a 20-token sequence of one repeated id, for MPNet a 24-token sequence with ``pad_id`` at columns 7 and 15 (positions
    skip there), and the eight ``LOWVAR_IDS`` in order (the LayerNorm-eps tokens).  ``notes`` maps 'lowvar', 'same',
    'pads' to sequence indices."""
    cfg, _ = CASES[name]
    cap = cfg.max_pos - (cfg.pad_id + 1 if cfg.arch == "mpnet" else 0)
    lens = [n for n in LENGTHS if n <= cap]
    notes = {"same": len(lens)}
    lens.append(20)
    if cfg.arch == "mpnet":
        notes["pads"] = len(lens)
        lens.append(24)
    notes["lowvar"] = len(lens)
    lens.append(len(LOWVAR_IDS))
    cu = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(lens, out=cu[1:])
    ids = presets.randint(f"sharp/{name}/ids", int(cu[-1]), 5, LOWVAR_IDS[0]).astype(np.int32)
    s = notes["same"]
    ids[cu[s]:cu[s + 1]] = ids[cu[s]]
    if "pads" in notes:
        s = notes["pads"]
        ids[cu[s] + 7] = ids[cu[s] + 15] = cfg.pad_id
    s = notes["lowvar"]
    ids[cu[s]:cu[s + 1]] = LOWVAR_IDS
    ids.setflags(write=False)
    cu.setflags(write=False)
    return ids, cu, notes


def case_linear(name: str):
    return fp8_ref.mx_linear if CASES[name][1] == "mxfp8" else None


# --------------------------------------------------------------------------- metrics and tolerances
def row_rel(got, ref) -> np.ndarray:
    """Per row: ||got - ref||_2 / ||ref||_2 (float64)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.linalg.norm(got - ref, axis=1) / np.maximum(np.linalg.norm(ref, axis=1), 1e-30)


def errors(got, ref) -> dict:
    """{'row_rel': max over rows of the relative row error, 'max_abs': max |difference|}; empty input gives zeros."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.size == 0:
        return {"row_rel": 0.0, "max_abs": 0.0}
    return {"row_rel": float(row_rel(got, ref).max()), "max_abs": float(np.abs(got - ref).max())}


METRICS = ("row_rel", "max_abs")
TOL_FACTOR = 2.0      # TOL = 2 x floor: room for what the emulation cannot reproduce (MFMA accumulation order in float32,
#                       float32 inside LayerNorm / softmax / GELU, __expf-class intrinsics).  A condition of the design.
POWER_FACTOR = 4.0    # a must-catch defect moves the output by >= 4 x TOL


def probe(name, weights=None, ids=None, cu=None, **kw):
    cfg, _ = CASES[name]
    if ids is None:
        ids, cu, _ = case_inputs(name)
    w = sharp_weights(cfg, name) if weights is None else weights
    return [h.numpy() for h in encoder_probe.probe_forward(cfg, w, ids, cu, linear=case_linear(name), **kw)]


def pooled_rows(hidden, cu) -> np.ndarray:
    return encoder_probe.mean_pool_packed(__import__("torch").from_numpy(np.asarray(hidden, dtype=np.float64)), cu).numpy()


@functools.lru_cache(maxsize=None)
def tolerances(name: str):
    """(exact, floor, tol) of a case on its own inputs.  ``exact``: the float64 probe's hidden states at boundary 0..L.
    ``floor[b][metric]``: error of probe(rounding="bf16") against it at boundary b (b = 1..L; key 'pooled' for the mean-
    pooled rows of the last boundary); ``tol`` = TOL_FACTOR x floor.  Computed here at test time, never typed in."""
    cfg, _ = CASES[name]
    ids, cu, _ = case_inputs(name)
    w = sharp_weights(cfg, name)
    exact = probe(name, w)
    rounded = probe(name, w, rounding="bf16")
    floor = {b: errors(rounded[b], exact[b]) for b in range(1, cfg.num_layers + 1)}
    floor["pooled"] = errors(pooled_rows(rounded[-1], cu), pooled_rows(exact[-1], cu))
    tol = {b: {m: TOL_FACTOR * v for m, v in f.items()} for b, f in floor.items()}
    return exact, floor, tol
