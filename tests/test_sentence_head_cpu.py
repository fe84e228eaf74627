"""Sentence-embedding heads on the host: parsing sentence-transformers directories (modules.json, Pooling, Dense, Normalize)
into the head the native forward runs, every refusal, the write/read round trip, and the new ops' refusal of CPU tensors."""
import json
import os

import numpy as np
import pytest
import torch

from text_similarity_amd import _lib, ops
from text_similarity_amd.models.st_format import (DENSE, NORMALIZE, POOLING, TRANSFORMER, DenseSpec,
                                                  read_sentence_transformers_dir, write_sentence_transformers_modules)

H = 64


def _json(path, obj):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        json.dump(obj, f)


def _pool_cfg(mode="mean", wd=H, **extra):
    flags = {"cls": "pooling_mode_cls_token", "mean": "pooling_mode_mean_tokens", "max": "pooling_mode_max_tokens",
             "mean_sqrt_len": "pooling_mode_mean_sqrt_len_tokens"}
    d = {"word_embedding_dimension": wd, **{f: False for f in flags.values()}}
    d[flags[mode]] = True
    d.update(extra)
    return d


def _dense_files(d, fin, fout, act="torch.nn.modules.activation.Tanh", bias=True, fmt="safetensors", seed=0):
    os.makedirs(d, exist_ok=True)
    _json(os.path.join(d, "config.json"), {"in_features": fin, "out_features": fout, "bias": bias, "activation_function": act})
    rng = np.random.default_rng(seed)
    t = {"linear.weight": rng.standard_normal((fout, fin)).astype(np.float32)}
    if bias:
        t["linear.bias"] = rng.standard_normal(fout).astype(np.float32)
    if fmt == "safetensors":
        from safetensors.numpy import save_file
        save_file(t, os.path.join(d, "model.safetensors"))
    else:
        torch.save({k: torch.from_numpy(v) for k, v in t.items()}, os.path.join(d, "pytorch_model.bin"))
    return t


def _st_dir(root, modules, pool=None, transformer_path="", hidden=H):
    """A sentence-transformers directory: modules = list of (type, path)."""
    tdir = os.path.join(root, transformer_path) if transformer_path else str(root)
    _json(os.path.join(tdir, "config.json"), {"model_type": "bert", "hidden_size": hidden})
    mods = []
    for i, (typ, path) in enumerate(modules):
        mods.append({"idx": i, "name": str(i), "path": path, "type": typ})
        if typ == POOLING:
            _json(os.path.join(root, path, "config.json"), pool if pool is not None else _pool_cfg())
        if typ == NORMALIZE:
            os.makedirs(os.path.join(root, path), exist_ok=True)
    _json(os.path.join(root, "modules.json"), mods)
    return str(root)


@pytest.mark.parametrize("mode", ["mean", "cls", "max", "mean_sqrt_len"])
def test_pooling_only(tmp_path, mode):
    d = _st_dir(tmp_path, [(TRANSFORMER, ""), (POOLING, "1_Pooling")], pool=_pool_cfg(mode))
    s = read_sentence_transformers_dir(d)
    assert (s.transformer_path, s.hidden, s.pooling, s.dense, s.normalize, s.width) == ("", H, mode, None, False, H)


def test_default_pooling_flag_is_mean(tmp_path):
    d = _st_dir(tmp_path, [(TRANSFORMER, ""), (POOLING, "1_Pooling")], pool={"word_embedding_dimension": H})
    assert read_sentence_transformers_dir(d).pooling == "mean"


@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
def test_labse_style_cls_dense_tanh_normalize(tmp_path, fmt):
    d = _st_dir(tmp_path, [(TRANSFORMER, "0_Transformer"), (POOLING, "1_Pooling"), (DENSE, "2_Dense"), (NORMALIZE, "3_Normalize")],
                pool=_pool_cfg("cls"), transformer_path="0_Transformer")
    t = _dense_files(os.path.join(d, "2_Dense"), H, 32, fmt=fmt)
    s = read_sentence_transformers_dir(d)
    assert (s.transformer_path, s.pooling, s.normalize, s.width) == ("0_Transformer", "cls", True, 32)
    assert (s.dense.in_features, s.dense.out_features, s.dense.activation) == (H, 32, "tanh")
    assert np.array_equal(s.dense.weight, t["linear.weight"]) and np.array_equal(s.dense.bias, t["linear.bias"])


def test_minilm_style_mean_normalize_and_identity_dense_without_bias(tmp_path):
    d = _st_dir(tmp_path, [(TRANSFORMER, ""), (POOLING, "1_Pooling"), (NORMALIZE, "2_Normalize")])
    s = read_sentence_transformers_dir(d)
    assert (s.pooling, s.dense, s.normalize) == ("mean", None, True)
    d2 = _st_dir(tmp_path / "b", [(TRANSFORMER, ""), (POOLING, "1_Pooling"), (DENSE, "2_Dense")], pool=_pool_cfg("max"))
    _dense_files(os.path.join(d2, "2_Dense"), H, H, act="torch.nn.modules.linear.Identity", bias=False)
    s2 = read_sentence_transformers_dir(d2)
    assert (s2.pooling, s2.dense.activation, s2.dense.bias, s2.normalize) == ("max", "identity", None, False)


def test_write_read_round_trip(tmp_path):
    rng = np.random.default_rng(3)
    dense = DenseSpec(H, 24, "tanh", rng.standard_normal((24, H)).astype(np.float32), rng.standard_normal(24).astype(np.float32))
    _json(os.path.join(tmp_path, "config.json"), {"model_type": "bert", "hidden_size": H})
    write_sentence_transformers_modules(str(tmp_path), H, "mean_sqrt_len", dense, True)
    s = read_sentence_transformers_dir(str(tmp_path))
    assert (s.pooling, s.normalize, s.dense.activation, s.width) == ("mean_sqrt_len", True, "tanh", 24)
    assert np.array_equal(s.dense.weight, dense.weight) and np.array_equal(s.dense.bias, dense.bias)
    assert sorted(os.listdir(tmp_path)) == ["1_Pooling", "2_Dense", "3_Normalize", "config.json", "modules.json"]


def _refuses(d, *needles):
    with pytest.raises(ValueError) as ei:
        read_sentence_transformers_dir(d)
    msg = str(ei.value)
    for n in needles:
        assert n in msg, msg


def test_refuses_two_pooling_flags(tmp_path):
    d = _st_dir(tmp_path, [(TRANSFORMER, ""), (POOLING, "1_Pooling")], pool=_pool_cfg("cls", pooling_mode_mean_tokens=True))
    _refuses(d, os.path.join("1_Pooling", "config.json"), "pooling_mode_cls_token")


@pytest.mark.parametrize("flag", ["pooling_mode_weightedmean_tokens", "pooling_mode_lasttoken"])
def test_refuses_weightedmean_and_lasttoken(tmp_path, flag):
    pool = _pool_cfg("mean", pooling_mode_mean_tokens=False, **{flag: True})
    d = _st_dir(tmp_path, [(TRANSFORMER, ""), (POOLING, "1_Pooling")], pool=pool)
    _refuses(d, os.path.join("1_Pooling", "config.json"), flag)


def test_refuses_word_embedding_dimension_mismatch(tmp_path):
    d = _st_dir(tmp_path, [(TRANSFORMER, ""), (POOLING, "1_Pooling")], pool=_pool_cfg("cls", wd=H * 2))
    _refuses(d, os.path.join("1_Pooling", "config.json"), "word_embedding_dimension")


def test_refuses_unknown_module_type(tmp_path):
    d = _st_dir(tmp_path, [(TRANSFORMER, ""), (POOLING, "1_Pooling"), ("sentence_transformers.models.LayerNorm", "2_LayerNorm")])
    _refuses(d, "modules.json", "sentence_transformers.models.LayerNorm")


def test_refuses_other_activation(tmp_path):
    d = _st_dir(tmp_path, [(TRANSFORMER, ""), (POOLING, "1_Pooling"), (DENSE, "2_Dense")])
    _dense_files(os.path.join(d, "2_Dense"), H, 32, act="torch.nn.modules.activation.ReLU")
    _refuses(d, os.path.join("2_Dense", "config.json"), "activation_function", "ReLU")


def test_refuses_in_features_mismatch(tmp_path):
    d = _st_dir(tmp_path, [(TRANSFORMER, ""), (POOLING, "1_Pooling"), (DENSE, "2_Dense")])
    _dense_files(os.path.join(d, "2_Dense"), H + 8, 32)
    _refuses(d, os.path.join("2_Dense", "config.json"), "in_features")


def test_refuses_normalize_not_last(tmp_path):
    d = _st_dir(tmp_path, [(TRANSFORMER, ""), (POOLING, "1_Pooling"), (NORMALIZE, "2_Normalize"), (DENSE, "3_Dense")])
    _dense_files(os.path.join(d, "3_Dense"), H, 32)
    _refuses(d, "modules.json", "Normalize must be the last module")


def test_refuses_second_dense(tmp_path):
    d = _st_dir(tmp_path, [(TRANSFORMER, ""), (POOLING, "1_Pooling"), (DENSE, "2_Dense"), (DENSE, "3_Dense")])
    _dense_files(os.path.join(d, "2_Dense"), H, H)
    _dense_files(os.path.join(d, "3_Dense"), H, 32)
    _refuses(d, "modules.json", "second Dense")


def test_refuses_dense_width_the_kernel_cannot_run(tmp_path):
    d = _st_dir(tmp_path, [(TRANSFORMER, ""), (POOLING, "1_Pooling"), (DENSE, "2_Dense")])
    _dense_files(os.path.join(d, "2_Dense"), H, 30)
    _refuses(d, os.path.join("2_Dense", "config.json"), "out_features")


def test_head_modules_describe_themselves():
    from text_similarity_amd.modules.modules import BertPoolingStrategy, CLSPoolingStrategy, SentenceEmbeddingHead, st_modules
    bp = BertPoolingStrategy(hidden_size=H)
    assert set(bp.state_dict()) == {"linear.weight", "linear.bias"}     # the reference's module layout
    mode, dense, norm = st_modules(bp)
    assert (mode, dense.activation, dense.out_features, norm) == ("cls", "tanh", H, False)
    assert st_modules(CLSPoolingStrategy()) == ("cls", None, False)
    head = SentenceEmbeddingHead(pooling_mode="max", dense=torch.nn.Linear(H, 16), activation="tanh", normalize=True)
    assert head.output_width(H) == 16 and bp.output_width(H) == H
    with pytest.raises(ValueError):
        SentenceEmbeddingHead(pooling_mode="weightedmean")
    with pytest.raises(ValueError):
        SentenceEmbeddingHead(pooling_mode="cls", activation="relu", dense=torch.nn.Linear(H, H))


def test_new_ops_have_no_cpu_path():
    x = torch.zeros(4, 64)
    for call in (lambda: ops.pool(torch.zeros(1, 2, 8), torch.ones(1, 2), "cls"),
                 lambda: ops.dense_rows(x, torch.zeros(8, 64), None, "tanh", True),
                 lambda: ops.dense_rows(x, None, None, "identity", True)):
        with pytest.raises(_lib.TsimError):
            call()


def test_new_symbols_are_declared():
    for s in ("tsim_pool", "tsim_dense_rows", "tsim_encoder_forward_head"):
        assert s in _lib.DECLARED_SYMBOLS
    import ctypes
    assert ctypes.sizeof(_lib.SentenceHeadC) == 32     # int32, int32, two pointers, int32, int32 (include/tsim.h)
