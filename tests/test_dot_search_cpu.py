"""Inner-product search on the host: similarity_fn_name in sentence-transformers directories, the C ABI of the dot path (symbols,
argument checks, the scale rule), and a CPU replay of the guard's domain conversion on adversarial data."""
import json
import math
import os
import warnings

import numpy as np
import pytest

from oracle import search_ref
from text_similarity_amd import _lib
from text_similarity_amd.models.st_format import (NORMALIZE, POOLING, TRANSFORMER, read_sentence_transformers_dir,
                                                  read_similarity_fn_name, similarity_fn, write_similarity_fn_name)

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tsim.h")
NEW = ("tsim_max_norm_rows", "tsim_dot_scaled_rows", "tsim_dot_scale", "tsim_dot_topk_ex")


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtsim.so is not built")
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------- similarity_fn_name
def _st_dir(root, st_config=None):
    os.makedirs(os.path.join(root, "1_Pooling"), exist_ok=True)
    with open(os.path.join(root, "config.json"), "w") as f:
        json.dump({"model_type": "bert", "hidden_size": 64}, f)
    with open(os.path.join(root, "1_Pooling", "config.json"), "w") as f:
        json.dump({"word_embedding_dimension": 64, "pooling_mode_cls_token": True, "pooling_mode_mean_tokens": False}, f)
    with open(os.path.join(root, "modules.json"), "w") as f:
        json.dump([{"idx": 0, "name": "0", "path": "", "type": TRANSFORMER},
                   {"idx": 1, "name": "1", "path": "1_Pooling", "type": POOLING}], f)
    if st_config is not None:
        with open(os.path.join(root, "config_sentence_transformers.json"), "w") as f:
            json.dump(st_config, f)
    return str(root)


@pytest.mark.parametrize("name,expect", [("cosine", "cosine"), ("dot", "dot"), ("dot_product", "dot")])
def test_similarity_fn_name_read(tmp_path, name, expect):
    path = _st_dir(tmp_path, {"__version__": {"sentence_transformers": "3.0.1"}, "similarity_fn_name": name})
    assert read_similarity_fn_name(path) == expect
    assert read_sentence_transformers_dir(path).similarity_fn_name == expect


def test_similarity_fn_name_absent(tmp_path):
    assert read_similarity_fn_name(_st_dir(tmp_path / "a")) is None
    assert read_sentence_transformers_dir(str(tmp_path / "a")).similarity_fn_name is None
    assert read_similarity_fn_name(_st_dir(tmp_path / "b", {"prompts": {}})) is None


@pytest.mark.parametrize("name", ["euclidean", "manhattan", "bogus"])
def test_similarity_fn_name_unknown_warns_and_keeps_cosine(tmp_path, name):
    path = _st_dir(tmp_path, {"similarity_fn_name": name})
    with pytest.warns(UserWarning, match=name):
        assert read_similarity_fn_name(path) == "cosine"


def test_similarity_fn_name_write_round_trip(tmp_path):
    path = _st_dir(tmp_path, {"__version__": {"sentence_transformers": "3.0.1"}, "prompts": {"query": "q: "}})
    write_similarity_fn_name(path, "dot_product")
    with open(os.path.join(path, "config_sentence_transformers.json")) as f:
        cfg = json.load(f)
    assert cfg["similarity_fn_name"] == "dot" and cfg["prompts"] == {"query": "q: "}    # other keys kept
    assert read_sentence_transformers_dir(path).similarity_fn_name == "dot"
    write_similarity_fn_name(path, "cosine")
    assert read_similarity_fn_name(path) == "cosine"
    fresh = str(tmp_path / "fresh")
    write_similarity_fn_name(fresh, "dot")
    assert read_similarity_fn_name(fresh) == "dot"
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert similarity_fn("dot") == "dot"


def test_pipeline_score_function_resolution():
    from types import SimpleNamespace
    from text_similarity_amd.pipeline.search_pipeline import resolve_score_function
    assert resolve_score_function(None, None) == "cosine"
    assert resolve_score_function(None, SimpleNamespace(similarity_fn_name="dot")) == "dot"
    assert resolve_score_function(None, SimpleNamespace(similarity_fn_name=None)) == "cosine"
    assert resolve_score_function("cosine", SimpleNamespace(similarity_fn_name="dot")) == "cosine"
    assert resolve_score_function("dot_product", None) == "dot"
    with pytest.raises(ValueError):
        resolve_score_function("l2", None)


# ---------------------------------------------------------------------------------------------------------- C ABI
def test_header_symbols_exported_and_bound():
    hdr = open(HDR).read()
    for name in NEW:
        assert f"{name}(" in hdr, name
        assert name in _lib.DECLARED_SYMBOLS, name
    L = _lib_or_skip()
    assert L.tsim_version() == 104
    for name in NEW:
        assert getattr(L, name).argtypes is not None, name


def test_dot_scale_rule():
    L = _lib_or_skip()
    assert L.tsim_dot_scale(0.0) == 1.0
    assert L.tsim_dot_scale(1.0) == 1.0
    assert L.tsim_dot_scale(1.0000001) == 2.0
    assert L.tsim_dot_scale(1000.0) == 1024.0
    assert L.tsim_dot_scale(1024.0) == 1024.0
    assert L.tsim_dot_scale(1e-42) == 2.0 ** -139          # subnormal word
    assert math.isinf(L.tsim_dot_scale(float("inf"))) and math.isinf(L.tsim_dot_scale(float("nan")))
    for v in np.float32([3e-20, 0.7, 5.5, 1.7e38]):
        s = L.tsim_dot_scale(float(v))
        assert s >= v and s / 2 < v and math.frexp(s)[0] == 0.5


def test_dot_topk_refuses_missing_float32_rows_or_rho():
    """Argument checks run before any launch: fake (never dereferenced) 16-byte aligned device pointers are enough."""
    L = _lib_or_skip()
    p = 1 << 20
    ws = L.tsim_cosine_topk_workspace_bytes(4, 100, 10)
    base = dict(eq=p, eq_f32=p, ldq=384, Q=4, ec=p, ec_f32=p, ldc=384, maxnorm=p, rho=p)

    def call(**kw):
        a = {**base, **kw}
        return L.tsim_dot_topk_ex(a["eq"], a["eq_f32"], a["ldq"], a["Q"], a["ec"], a["ec_f32"], a["ldc"], a["maxnorm"],
                                  a["rho"], 100, 384, 384, 10, p, p, None, 0, p, ws, None)

    for kw in ({"eq_f32": None}, {"ec_f32": None}, {"eq_f32": None, "ec_f32": None}, {"rho": None}, {"maxnorm": None}):
        assert call(**kw) == 1, kw                       # TSIM_EINVAL
        assert b"dot_topk" in L.tsim_last_error()
    assert L.tsim_dot_scaled_rows(p, 0, 4, 384, 384, None, p, 384, None, None) == 1
    assert L.tsim_max_norm_rows(p, 0, 4, 384, 384, None, None) == 1
    assert L.tsim_dot_scaled_rows(p, 0, 4, 384, 384, p, p, 300, None, None) == 1   # ld_out < d


# ---------------------------------------------------------------------------------------------------------- guard replay
def _scaled_rows(c):
    """half(c / S) with S the smallest power of two >= the largest row norm, and the flush-safe residual maximum."""
    S = 2.0 ** math.ceil(math.log2(float(np.sqrt(search_ref._lane_sum(c, c)).max())))
    v = c.astype(np.float64) / S
    h = v.astype(np.float16).astype(np.float64)
    e = np.where(np.abs(h) < 2.0 ** -14, np.maximum(np.abs(h - v), np.abs(v)), h - v)
    return h, S, float(np.sqrt((e ** 2).sum(1)).max())


def _flush(h):
    return np.where(np.abs(h) < 2.0 ** -14, 0.0, h)


def test_guard_conversion_covers_every_exact_score():
    """MFMA-model scores of the scaled rows (mfma_model_scores' 'f32seq' accumulation, on kept and on flushed subnormals):
    for every (query, row) |m - float32(q.c) / (nq S)| <= eps, and the two decisions the kernels take from it hold — no row
    above the first pass's cut reaches (cut + eps) nq S, and every row whose exact score reaches the k-th has m > tau."""
    rng = np.random.default_rng(11)
    d = 128
    c = rng.standard_normal((600, d)).astype(np.float32) / np.sqrt(d)
    c *= (10.0 ** rng.uniform(-3, 3, (600, 1))).astype(np.float32)   # norms over six decades: most rows subnormal halves
    c[5] *= 1e4 / np.linalg.norm(c[5])                              # one huge row
    base = rng.standard_normal(d).astype(np.float32)
    c[200:260] = base + 1e-6 * rng.standard_normal((60, d)).astype(np.float32)   # near-ties
    c[300:310] = 0.0
    q = np.concatenate([base[None], rng.standard_normal((6, d)), np.zeros((1, d))]).astype(np.float32)
    h, S, rho_c = _scaled_rows(c)
    uq = search_ref.unit_rows(q).astype(np.float64)
    rho_q = np.sqrt(((np.where(np.abs(uq) < 2.0 ** -14, np.maximum(np.abs(uq - search_ref.l2_normalize_f64(q)),
                                                                      np.abs(search_ref.l2_normalize_f64(q))),
                               uq - search_ref.l2_normalize_f64(q))) ** 2).sum(1))
    nq = np.maximum(np.sqrt(search_ref._lane_sum(q, q)), np.float64(np.float32(1e-8)))
    exact = search_ref._lane_sum(q[:, None, :], c[None, :, :]).astype(np.float32)
    k = 10
    for hh in (h, _flush(h)):
        for uu in (uq, _flush(uq)):
            m = np.zeros((q.shape[0], c.shape[0]), dtype=np.float32)
            for j in range(d):        # float32 accumulation element by element (mfma_model_scores 'f32seq')
                m = (m + (uu[:, j:j + 1] * hh[None, :, j]).astype(np.float32)).astype(np.float32)
            for qi in range(q.shape[0]):
                eps = float(search_ref.guard_eps(rho_q[qi], rho_c, d))
                nqs = float(nq[qi]) * S
                conv = exact[qi].astype(np.float64) / nqs
                assert np.abs(m[qi].astype(np.float64) - conv).max() <= eps
                sk = float(np.sort(exact[qi])[::-1][k - 1])
                order = np.lexsort((np.arange(c.shape[0]), -m[qi].astype(np.float64)))
                cut = float(m[qi][order[16 - 1]])
                bound = (cut + eps) * nqs
                bound += abs(bound) * 1e-15
                assert (exact[qi][order[16:]] <= bound).all()            # dot_bound_up covers every row outside
                lo = sk / nqs - eps - (abs(sk / nqs) + eps) * 1e-15
                tau = np.nextafter(np.float32(lo), np.float32(-np.inf))
                assert (m[qi][exact[qi] >= sk] > tau).all()              # guard_tau_dot collects every row that can reach sk
    assert np.isclose(S, 2.0 ** 14) and rho_c > 0
