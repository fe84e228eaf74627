"""GPU parity of the exact inner-product search (ops.dot_topk, include/tsim.h tsim_dot_topk_ex) and of the layers built on it:
GpuFlatIndex(space='ip'), SentenceMiningPipeline / SemanticSearchPipeline(score_function='dot').
Bar: indices identical and float32 scores == float32(q.c) summed in the canonical lane order (oracle/search_ref._lane_sum), top-k
by (score desc, index asc) — the test-local oracle below."""
import types

import numpy as np
import pytest
import torch

from oracle.search_ref import _lane_sum, cosine_topk_f32, topk_rows
from text_similarity_amd import ops, presets
from text_similarity_amd.index import GpuFlatIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------------- test-local oracle
def dot_scores(q, c, qblock=16, nblock=4096):
    """[Q, N] float32(q.c): float64 sum in the canonical lane order, one rounding."""
    q = np.asarray(q, dtype=np.float32)
    c = np.asarray(c, dtype=np.float32)
    out = np.empty((q.shape[0], c.shape[0]), dtype=np.float32)
    for a in range(0, q.shape[0], qblock):
        for b in range(0, c.shape[0], nblock):
            out[a:a + qblock, b:b + nblock] = _lane_sum(q[a:a + qblock, None, :], c[None, b:b + nblock, :]).astype(np.float32)
    return out


def dot_topk_ref(q, c, k, idx_offset=0):
    s, i = topk_rows(dot_scores(q, c), k)
    return s, i + idx_offset


# ---------------------------------------------------------------------------------------------------------- helpers
def _search(q, c, k, idx_offset=0):
    qf = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(DEV)
    cf = torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).to(DEV)
    d = q.shape[1]
    cn, rho, scale = ops.dot_scaled_rows(cf)
    s, i, st = ops.dot_topk(ops.l2norm_rows(qf), cn, d, k, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale,
                            idx_offset=idx_offset, return_status=True)
    torch.cuda.synchronize()
    return s.cpu().numpy(), i.cpu().numpy(), st.cpu().numpy()


def _check_exact(q, c, k, idx_offset=0):
    s, i, st = _search(q, c, k, idx_offset)
    kk = min(k, c.shape[0])
    rs, ri = dot_topk_ref(q, c, k, idx_offset)
    np.testing.assert_array_equal(i[:, :kk], ri)
    np.testing.assert_array_equal(s[:, :kk], rs)
    if kk < k:
        assert (i[:, kk:] == -1).all() and np.isneginf(s[:, kk:]).all()
    return s, i, st


def _gauss(rng, n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


def _spread(rng, n, d, lo=-3.0, hi=3.0):
    """rows with random directions and norms spread log-uniformly over 10^lo .. 10^hi"""
    x = rng.standard_normal((n, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return (x * 10.0 ** rng.uniform(lo, hi, (n, 1))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- 1. random rows
@pytest.mark.parametrize("d", [128, 300, 384, 768])
@pytest.mark.parametrize("k", [1, 10, 28, 29, 64])
def test_random_rows_exact(d, k):
    rng = np.random.default_rng(1000 * d + k)
    c = _gauss(rng, 3000, d) * rng.uniform(0.5, 2.0, (3000, 1)).astype(np.float32)
    q = _gauss(rng, 24, d)
    _check_exact(q, c, k, idx_offset=7)


def test_large_corpus_two_phase_exact():
    """N >= 4 x 131 072 with more than 768 queries takes the two-phase main pass."""
    rng = np.random.default_rng(5)
    d = 384
    c = _gauss(rng, 530_000, d)
    q = _gauss(rng, 1024, d)
    s, i, st = _search(q, c, 10)
    sel = [0, 1, 511, 1023]                                   # (the CPU oracle is the slow part)
    rs, ri = topk_rows(dot_scores(q[sel], c, qblock=4, nblock=16384), 10)
    np.testing.assert_array_equal(i[sel], ri)
    np.testing.assert_array_equal(s[sel], rs)


# ---------------------------------------------------------------------------------------------------------- 2. spread norms
def test_spread_norms_exact_and_not_cosine():
    rng = np.random.default_rng(2)
    d = 384
    c = _spread(rng, 4000, d)
    q = _spread(rng, 64, d, -1.0, 1.0)
    s, i, st = _check_exact(q, c, 10)
    _, ci = cosine_topk_f32(q, c, 10)
    assert (ci != i).any(axis=1).mean() > 0.5, "on this corpus the dot-product ranking must differ from cosine's"
    print(f"spread norms: status counts {np.bincount(st, minlength=3).tolist()}")


# ---------------------------------------------------------------------------------------------------------- 3. subnormal halves
def test_huge_row_subnormal_halves_and_near_ties():
    """One row of norm 1e6 sets S = 2^20: the other rows (norm ~1) become half subnormals, mostly flushed-size, and the guard's
    residual counts them both ways.  Near-ties (a cluster of rows 1e-7 apart) sit around rank k.  A small corpus resolves its
    flagged queries by widening; a large one overflows the collection and falls back to brute force."""
    rng = np.random.default_rng(3)
    d = 384
    statuses = []
    for n in (900, 3000):
        c = _gauss(rng, n, d) / np.sqrt(d)
        c[0] = _gauss(rng, 1, d)[0] / np.sqrt(d) * 1e6
        base = _gauss(rng, 1, d)[0] / np.sqrt(d)
        c[100:140] = base + 1e-7 * _gauss(rng, 40, d)
        q = np.concatenate([base[None] + 1e-3 * _gauss(rng, 12, d), _gauss(rng, 12, d)]).astype(np.float32)
        cf = torch.from_numpy(c).to(DEV)
        cn, rho, scale = ops.dot_scaled_rows(cf)
        assert ops.dot_scale(scale) == 2.0 ** 20
        halves = cn[1:, :d].float().abs()
        assert bool((halves < 2.0 ** -14).all()) and bool((halves > 0).any())   # every other row is subnormal (or zero)
        _, _, st = _check_exact(q, c, 10)
        statuses.append(st)
    allst = np.concatenate(statuses)
    print(f"huge row: status counts {[np.bincount(s, minlength=3).tolist() for s in statuses]}")
    assert (allst == 1).any() and (allst == 2).any()


# ---------------------------------------------------------------------------------------------------------- 4. brute force
def test_many_near_ties_duplicates_zero_rows_zero_query():
    rng = np.random.default_rng(4)
    d = 256
    base = _gauss(rng, 1, d)[0]
    c = _gauss(rng, 4000, d)
    c[500:2000] = base + 1e-6 * _gauss(rng, 1500, d)        # 1 500 near-ties: more than the 1 024 a widening slot holds
    c[2100:2110] = c[7]                                       # exact duplicates
    c[2200:2300] = 0.0                                        # zero rows
    q = np.concatenate([base[None], base[None] * 3.0, c[7][None], np.zeros((1, d)), _gauss(rng, 8, d)]).astype(np.float32)
    for k in (10, 40):
        s, i, st = _check_exact(q, c, k)
        assert st[0] == 2 and st[1] == 2
        np.testing.assert_array_equal(i[3], np.arange(k))     # zero query: the first k rows, score 0
        assert (s[3] == 0).all()


# ---------------------------------------------------------------------------------------------------------- 5. shard boundaries
def test_chunked_mining_pipeline_equals_single_shot():
    from text_similarity_amd.pipeline.search_pipeline import SentenceMiningPipeline
    rng = np.random.default_rng(6)
    d = 384
    # norms grow chunk by chunk: every chunk of 1 000 rows gets its own S
    c = np.concatenate([_gauss(rng, 1000, d) * (4.0 ** j) for j in range(5)]).astype(np.float32)
    c[::7] *= 1e-3
    q = _gauss(rng, 40, d)
    params = types.SimpleNamespace(device=torch.device(DEV))
    ct, qt = torch.from_numpy(c).to(DEV), torch.from_numpy(q).to(DEV)
    scales = [ops.dot_scale(ops.max_norm_rows(ct[j * 1000:(j + 1) * 1000])) for j in range(5)]
    assert len(set(scales)) == 5
    one = SentenceMiningPipeline(len(c), params, None, corpus=ct, score_function="dot")
    s1, i1 = one.search_tensors(qt, ct, 10)
    rs, ri = dot_topk_ref(q, c, 10)
    np.testing.assert_array_equal(i1.cpu().numpy(), ri)
    np.testing.assert_array_equal(s1.cpu().numpy(), rs)
    for chunk in (1000, 777):
        pipe = SentenceMiningPipeline(chunk, params, None, corpus=ct, score_function="dot")
        assert pipe.score_function == "dot"
        s2, i2 = pipe.search_tensors(qt, ct, 10)
        assert torch.equal(i2, i1) and torch.equal(s2, s1)
    cos = SentenceMiningPipeline(1000, params, None, corpus=ct)
    assert cos.score_function == "cosine"
    assert not torch.equal(cos.search_tensors(qt, ct, 10)[1], i1)


# ---------------------------------------------------------------------------------------------------------- 6. index
def test_flat_index_ip(tmp_path):
    rng = np.random.default_rng(7)
    d = 384
    a = _gauss(rng, 500, d)
    b = _gauss(rng, 300, d) * 50.0                            # a larger norm: S grows, the stored rows are re-derived
    q = _gauss(rng, 16, d)
    idx = GpuFlatIndex(space="ip", dim=d, device=DEV)
    idx.init_index(max_elements=100)
    idx.add_items(a, np.arange(500) + 10_000)
    s0 = ops.dot_scale(idx._maxnorm)
    lab, dist = idx.knn_query(q, k=10)
    rs, ri = dot_topk_ref(q, a, 10)
    np.testing.assert_array_equal(lab, ri + 10_000)
    np.testing.assert_array_equal(dist, (1.0 - torch.from_numpy(rs)).numpy())
    idx.add_items(b, np.arange(300) + 20_000)
    assert ops.dot_scale(idx._maxnorm) > s0
    rows, labels = np.concatenate([a, b]), np.concatenate([np.arange(500) + 10_000, np.arange(300) + 20_000])
    lab, dist = idx.knn_query(q, k=12)
    rs, ri = dot_topk_ref(q, rows, 12)
    np.testing.assert_array_equal(lab, labels[ri])
    np.testing.assert_array_equal(dist, (1.0 - torch.from_numpy(rs)).numpy())
    # delete the best hit of every query
    for lb in set(lab[:, 0].tolist()):
        idx.mark_deleted(int(lb))
    live = ~np.isin(labels, lab[:, 0])
    lab2, _ = idx.knn_query(q, k=12)
    rs2, ri2 = dot_topk_ref(q, rows[live], 12)
    np.testing.assert_array_equal(lab2, labels[live][ri2])
    # save / load
    path = str(tmp_path / "ip.bin")
    idx.save_index(path)
    idx2 = GpuFlatIndex(space="ip", device=DEV)
    idx2.load_index(path)
    lab3, dist3 = idx2.knn_query(q, k=12)
    np.testing.assert_array_equal(lab3, lab2)
    np.testing.assert_array_equal(dist3, (1.0 - torch.from_numpy(rs2)).numpy())
    with pytest.raises(ValueError):
        GpuFlatIndex(space="cosine", device=DEV).load_index(path)
    cpath = str(tmp_path / "cos.bin")
    cidx = GpuFlatIndex(space="cosine", dim=d, device=DEV)
    cidx.add_items(a)
    cidx.save_index(cpath)
    with pytest.raises(ValueError):
        GpuFlatIndex(space="ip", device=DEV).load_index(cpath)
    with pytest.raises(ValueError):
        GpuFlatIndex(space="l2", dim=d, device=DEV)
    bad = a[:4].copy()
    bad[2, 5] = np.nan
    with pytest.raises(ValueError):
        idx2.add_items(bad)


# ---------------------------------------------------------------------------------------------------------- 7. pipeline + model
def test_semantic_search_pipeline_dot_model(tmp_path):
    from transformers import BertTokenizer
    from text_similarity_amd.configurations.config import ModelParameters, SearchConfiguration
    from text_similarity_amd.models.sentence_encoder import SentenceTransformerWrapper
    from text_similarity_amd.pipeline.search_pipeline import SemanticSearchPipeline
    preset = "all-MiniLM-L6-v2"
    tok = BertTokenizer(vocab=presets.synthetic_vocab(30522), do_lower_case=True)
    params = SearchConfiguration(model_parameters=ModelParameters(preset, hidden_size=384), model=preset, save_path="",
                                 tokenizer=tok, device=torch.device(DEV), max_tokens_per_batch=8192, max_seqs_per_batch=512)
    model = SentenceTransformerWrapper.from_preset(preset, params, parallel_mode=False, similarity_fn_name="dot")
    assert model.similarity_fn_name == "dot"
    sents = presets.synthetic_sentences(240, seed="dot/s", vocab_size=30522)
    corpus, queries = list(sents[:200]), list(sents[200:])
    pipe = SemanticSearchPipeline(str(tmp_path / "index"), params, model, corpus=corpus)
    assert pipe.score_function == "dot" and pipe.index.space == "ip"
    res = pipe(queries, 5)
    ce = model.encode_text(corpus).float().cpu().numpy()
    qe = model.encode_text(queries).float().cpu().numpy()
    rs, ri = dot_topk_ref(qe, ce, 5)
    np.testing.assert_array_equal(pipe.last_labels.cpu().numpy(), ri)
    np.testing.assert_array_equal(pipe.last_scores.cpu().numpy(), rs)
    assert all(res[q] == [corpus[j] for j in ri[q]] for q in range(len(queries)))
    # the model's score function survives save_pretrained
    from text_similarity_amd.models.st_format import read_similarity_fn_name
    out = str(tmp_path / "saved")
    model.save_pretrained(out)
    assert read_similarity_fn_name(out) == "dot"
