"""sentence-transformers checkpoint directories: the module chain a ``modules.json`` declares on top of the HF encoder
(Transformer -> Pooling -> optional Dense -> optional Normalize), read into a :class:`HeadSpec` and written back.

Host code only (json, numpy, safetensors): the CPU suite parses hand-written directories with it.  What it accepts is what the
native head runs (include/tsim.h tsim_sentence_head); everything else is refused with a ``ValueError`` that names the file
and the field, never loaded into a model that would return different vectors."""
from __future__ import annotations

import json
import os
import warnings
from dataclasses import dataclass
from typing import Optional

import numpy as np

TRANSFORMER = "sentence_transformers.models.Transformer"
POOLING = "sentence_transformers.models.Pooling"
DENSE = "sentence_transformers.models.Dense"
NORMALIZE = "sentence_transformers.models.Normalize"

# Pooling/config.json flag -> pooling mode of the native head (ops.POOL_MODES)
POOL_FLAGS = {"pooling_mode_cls_token": "cls", "pooling_mode_mean_tokens": "mean", "pooling_mode_max_tokens": "max",
              "pooling_mode_mean_sqrt_len_tokens": "mean_sqrt_len"}
UNSUPPORTED_POOL_FLAGS = ("pooling_mode_weightedmean_tokens", "pooling_mode_lasttoken")
# Dense/config.json activation_function -> activation of the native head (ops.ACTIVATIONS)
ACTIVATIONS = {"torch.nn.modules.activation.Tanh": "tanh", "torch.nn.modules.linear.Identity": "identity"}
ACTIVATION_NAMES = {v: k for k, v in ACTIVATIONS.items()}
MAX_DENSE = 1024   # widths of the native Dense kernel: multiples of 8 in [8, 1024]
# config_sentence_transformers.json similarity_fn_name -> score function of the search pipelines ("cosine" | "dot")
ST_CONFIG = "config_sentence_transformers.json"
SIMILARITY_FNS = {"cosine": "cosine", "dot": "dot", "dot_product": "dot"}


@dataclass
class DenseSpec:
    in_features: int
    out_features: int
    activation: str                  # 'identity' | 'tanh'
    weight: np.ndarray               # float32 [out_features, in_features] (nn.Linear layout)
    bias: Optional[np.ndarray]       # float32 [out_features] or None


@dataclass
class HeadSpec:
    transformer_path: str            # directory of the HF encoder, relative to the checkpoint ("" or "0_Transformer")
    hidden: int
    pooling: str                     # 'mean' | 'cls' | 'max' | 'mean_sqrt_len'
    dense: Optional[DenseSpec] = None
    normalize: bool = False
    similarity_fn_name: Optional[str] = None   # 'cosine' | 'dot' | None (the checkpoint does not say)

    @property
    def width(self) -> int:
        return self.dense.out_features if self.dense is not None else self.hidden


def _load_json(path: str, what: str):
    try:
        with open(path) as f:
            return json.load(f)
    except FileNotFoundError:
        raise ValueError(f"{path}: missing ({what})") from None
    except json.JSONDecodeError as e:
        raise ValueError(f"{path}: not valid JSON ({e})") from None


def _load_tensors(d: str) -> dict:
    st = os.path.join(d, "model.safetensors")
    pt = os.path.join(d, "pytorch_model.bin")
    if os.path.exists(st):
        from safetensors.numpy import load_file
        return {k: np.asarray(v, dtype=np.float32) for k, v in load_file(st).items()}
    if os.path.exists(pt):
        import torch
        return {k: v.float().numpy() for k, v in torch.load(pt, map_location="cpu", weights_only=True).items()}
    raise ValueError(f"{d}: no model.safetensors / pytorch_model.bin for the Dense weights")


def _pooling(path: str, hidden: int) -> str:
    f = os.path.join(path, "config.json")
    cfg = _load_json(f, "Pooling config")
    wd = cfg.get("word_embedding_dimension")
    if wd != hidden:
        raise ValueError(f"{f}: word_embedding_dimension={wd} != the transformer's hidden_size {hidden}")
    for k in UNSUPPORTED_POOL_FLAGS:
        if cfg.get(k):
            raise ValueError(f"{f}: {k} is not supported (cls, mean, max, mean_sqrt_len)")
    # sentence-transformers' own default: mean pooling unless the flag says otherwise
    on = [mode for flag, mode in POOL_FLAGS.items() if cfg.get(flag, flag == "pooling_mode_mean_tokens")]
    if len(on) != 1:
        raise ValueError(f"{f}: exactly one of {', '.join(POOL_FLAGS)} must be true (got {on or 'none'}); "
                         "concatenated pooling modes are not supported")
    return on[0]


def _dense(path: str, d_in: int) -> DenseSpec:
    f = os.path.join(path, "config.json")
    cfg = _load_json(f, "Dense config")
    fin, fout = cfg.get("in_features"), cfg.get("out_features")
    if fin != d_in:
        raise ValueError(f"{f}: in_features={fin} != the pooled width {d_in}")
    if not isinstance(fout, int) or not (8 <= fout <= MAX_DENSE and fout % 8 == 0):
        raise ValueError(f"{f}: out_features={fout} is not a multiple of 8 in [8, {MAX_DENSE}]")
    act_name = cfg.get("activation_function", "torch.nn.modules.activation.Tanh")
    if act_name not in ACTIVATIONS:
        raise ValueError(f"{f}: activation_function={act_name!r} is not supported ({', '.join(ACTIVATIONS)})")
    has_bias = bool(cfg.get("bias", True))
    t = _load_tensors(path)
    w = t.get("linear.weight")
    if w is None or w.shape != (fout, fin):
        raise ValueError(f"{path}: linear.weight {None if w is None else w.shape} != ({fout}, {fin})")
    b = t.get("linear.bias") if has_bias else None
    if has_bias and (b is None or b.shape != (fout,)):
        raise ValueError(f"{path}: linear.bias {None if b is None else b.shape} != ({fout},) with bias=true in {f}")
    return DenseSpec(fin, fout, ACTIVATIONS[act_name], np.ascontiguousarray(w), None if b is None else np.ascontiguousarray(b))


def similarity_fn(name, where: str = "similarity_fn_name") -> str:
    """'cosine' -> 'cosine'; 'dot' / 'dot_product' -> 'dot'; anything else warns and keeps 'cosine'."""
    if name in SIMILARITY_FNS:
        return SIMILARITY_FNS[name]
    warnings.warn(f"{where}: similarity function {name!r} is not supported by the search (cosine, dot); ranking by cosine",
                  stacklevel=2)
    return "cosine"


def read_similarity_fn_name(path: str) -> Optional[str]:
    """The score function ``path``/config_sentence_transformers.json declares ('cosine' | 'dot'), or None when the file or the
    key is absent."""
    f = os.path.join(path, ST_CONFIG)
    if not os.path.exists(f):
        return None
    name = _load_json(f, "the sentence-transformers config").get("similarity_fn_name")
    return None if name is None else similarity_fn(name, f"{f}: similarity_fn_name")


def write_similarity_fn_name(path: str, name: str) -> None:
    """Set similarity_fn_name in ``path``/config_sentence_transformers.json, keeping the file's other keys."""
    f = os.path.join(path, ST_CONFIG)
    cfg = _load_json(f, "the sentence-transformers config") if os.path.exists(f) else {}
    cfg["similarity_fn_name"] = similarity_fn(name)
    os.makedirs(path, exist_ok=True)
    with open(f, "w") as fh:
        json.dump(cfg, fh, indent=2)


def read_sentence_transformers_dir(path: str) -> HeadSpec:
    """Parse ``path``/modules.json and the module directories it names.  Accepted chain: Transformer (at "" or
    "0_Transformer"), one Pooling, at most one Dense after it, and an optional Normalize as the last module."""
    mf = os.path.join(path, "modules.json")
    mods = _load_json(mf, "the sentence-transformers module list")
    if not isinstance(mods, list) or not mods:
        raise ValueError(f"{mf}: expected a non-empty list of modules")
    mods = sorted(mods, key=lambda m: int(m.get("idx", 0)))
    spec = None
    hidden = None
    for pos, m in enumerate(mods):
        typ, sub = m.get("type"), m.get("path", "")
        where = f"{mf}: module {m.get('idx', pos)} ({typ})"
        d = os.path.join(path, sub) if sub else path
        if spec is not None and spec.normalize:
            raise ValueError(f"{where}: Normalize must be the last module")
        if typ == TRANSFORMER:
            if pos != 0 or sub not in ("", "0_Transformer"):
                raise ValueError(f"{where}: the Transformer must be the first module, at path \"\" or \"0_Transformer\" "
                                 f"(path={sub!r})")
            hidden = _load_json(os.path.join(d, "config.json"), "the transformer's HF config").get("hidden_size")
            if not isinstance(hidden, int):
                raise ValueError(f"{os.path.join(d, 'config.json')}: hidden_size missing")
            spec = HeadSpec(transformer_path=sub, hidden=hidden, pooling="")
        elif typ == POOLING:
            if spec is None or spec.pooling:
                raise ValueError(f"{where}: Pooling must follow the Transformer, once")
            spec.pooling = _pooling(d, hidden)
        elif typ == DENSE:
            if spec is None or not spec.pooling:
                raise ValueError(f"{where}: a Dense must follow the Pooling (token-level Dense is not supported)")
            if spec.dense is not None:
                raise ValueError(f"{where}: a second Dense is not supported")
            spec.dense = _dense(d, spec.hidden)
        elif typ == NORMALIZE:
            if spec is None or not spec.pooling:
                raise ValueError(f"{where}: Normalize must follow the Pooling")
            spec.normalize = True
        else:
            raise ValueError(f"{where}: unknown module type {typ!r} ({TRANSFORMER}, {POOLING}, {DENSE}, {NORMALIZE})")
    if spec is None or not spec.pooling:
        raise ValueError(f"{mf}: needs a Transformer and a Pooling module")
    spec.similarity_fn_name = read_similarity_fn_name(path)
    return spec


def write_sentence_transformers_modules(path: str, hidden: int, pooling: str, dense: Optional[DenseSpec] = None,
                                        normalize: bool = False) -> None:
    """modules.json, 1_Pooling/config.json, 2_Dense/{config.json, model.safetensors} and the Normalize directory, with the
    Transformer at ``path`` itself (its config.json / model.safetensors are written by the encoder's save_pretrained)."""
    from safetensors.numpy import save_file
    if pooling not in POOL_FLAGS.values():
        raise ValueError(f"unknown pooling mode {pooling!r}")
    mods = [{"idx": 0, "name": "0", "path": "", "type": TRANSFORMER},
            {"idx": 1, "name": "1", "path": "1_Pooling", "type": POOLING}]
    os.makedirs(os.path.join(path, "1_Pooling"), exist_ok=True)
    pcfg = {"word_embedding_dimension": int(hidden)}
    pcfg.update({flag: mode == pooling for flag, mode in POOL_FLAGS.items()})
    pcfg.update({flag: False for flag in UNSUPPORTED_POOL_FLAGS})
    with open(os.path.join(path, "1_Pooling", "config.json"), "w") as f:
        json.dump(pcfg, f, indent=2)
    if dense is not None:
        dd = os.path.join(path, "2_Dense")
        os.makedirs(dd, exist_ok=True)
        with open(os.path.join(dd, "config.json"), "w") as f:
            json.dump({"in_features": int(dense.in_features), "out_features": int(dense.out_features),
                       "bias": dense.bias is not None, "activation_function": ACTIVATION_NAMES[dense.activation]}, f, indent=2)
        t = {"linear.weight": np.ascontiguousarray(dense.weight, dtype=np.float32)}
        if dense.bias is not None:
            t["linear.bias"] = np.ascontiguousarray(dense.bias, dtype=np.float32)
        save_file(t, os.path.join(dd, "model.safetensors"))
        mods.append({"idx": 2, "name": "2", "path": "2_Dense", "type": DENSE})
    if normalize:
        i = len(mods)
        os.makedirs(os.path.join(path, f"{i}_Normalize"), exist_ok=True)
        mods.append({"idx": i, "name": str(i), "path": f"{i}_Normalize", "type": NORMALIZE})
    with open(os.path.join(path, "modules.json"), "w") as f:
        json.dump(mods, f, indent=2)
