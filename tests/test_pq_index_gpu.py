"""GpuPQIndex and SemanticSearchPipeline(index_type="pq") on the GPU: the index is ops.pq_encode_rows + ops.pq_adc_topk with
labels, storage and a file around them, so its results are compared for equality with those ops (themselves pinned against the
numpy restatement in tests/test_pq_gpu.py); training is checked by what Lloyd's iterations guarantee, not by a measured bar."""
import os

import numpy as np
import pytest
import torch

import pq_cases as pc
from text_similarity_amd import ops, presets
from text_similarity_amd.pq_index import GpuPQIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, M = 24, 6


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _same(a, b):
    return np.array_equal(a.cpu().numpy().view(np.uint32), b.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("space", ("ip", "l2", "cosine"))
def test_search_is_the_ops_on_the_same_tensors(space):
    rng = np.random.default_rng(1)
    cb = pc.random_codebooks(rng, D, M)
    x, q = _dev(rng.standard_normal((700, D)).astype(np.float32)), _dev(rng.standard_normal((9, D)).astype(np.float32))
    labels = rng.permutation(10_000)[:700].astype(np.int64) + (1 << 33)
    index = GpuPQIndex(space, D, M, device=DEV)
    assert not index.is_trained
    with pytest.raises(RuntimeError):
        index.add_items(x[:3])
    with pytest.raises(RuntimeError):
        index.search(q, 3)
    index.train(codebooks=cb)
    assert index.is_trained and index.get_current_count() == 0
    s0, l0 = index.search(q, 3)                                                    # an empty index pads
    assert (l0 == -1).all() and torch.isinf(s0).all()
    index.add_items(x[:300], labels[:300])
    index.add_items(x[300:], labels[300:])
    assert index.get_current_count() == 700
    xs, qs = (GpuPQIndex.normalise(x), GpuPQIndex.normalise(q)) if space == "cosine" else (x, q)
    codes = ops.pq_encode_rows(xs, _dev(cb))
    want_s, want_i = ops.pq_adc_topk(qs, _dev(cb), codes, 20, "l2" if space == "l2" else "ip")
    got_s, got_l = index.search(q, 20)
    assert _same(got_s, want_s) and np.array_equal(got_l.cpu().numpy(), labels[want_i.cpu().numpy()])
    one = GpuPQIndex(space, D, M, device=DEV)                                      # one batch: the same rows
    one.train(codebooks=cb)
    one.add_items(x, labels)
    s1, l1 = one.search(q, 20)
    assert _same(s1, got_s) and torch.equal(l1, got_l)
    lab, val = index.knn_query(q.cpu().numpy(), 20)
    assert np.array_equal(lab, got_l.cpu().numpy()) and np.array_equal(val, got_s.cpu().numpy())
    with pytest.raises(ValueError):
        GpuPQIndex("hamming", D, M)
    with pytest.raises(ValueError):
        GpuPQIndex("ip", 25, 6)
    with pytest.raises(ValueError):
        index.train(codebooks=np.full((M, 256, D // M), np.nan, np.float32))


def test_lossless_corpus_reconstructs_and_finds_itself():
    rng = np.random.default_rng(2)
    cb = pc.random_codebooks(rng, D, M)
    x, codes = pc.lossless(rng, 600, cb)
    assert len({r.tobytes() for r in x}) == 600
    labels = np.arange(600, dtype=np.int64) * 3 + 1
    index = GpuPQIndex("l2", D, M, device=DEV)
    index.train(codebooks=cb)
    index.add_items(x, labels)
    assert np.array_equal(index.reconstruct(labels[::-1]).cpu().numpy().view(np.uint32), x[::-1].view(np.uint32))
    dist, lab = index.search(x, 1)
    assert np.array_equal(lab.cpu().numpy()[:, 0], labels) and (dist == 0).all()
    with pytest.raises(RuntimeError):
        index.reconstruct([2])
    by_codes = GpuPQIndex("l2", D, M, device=DEV)                                  # codes can be added as they are
    by_codes.train(codebooks=cb)
    by_codes.add_items(codes, labels)
    d2, l2 = by_codes.search(x[:50], 4)
    d1, l1 = index.search(x[:50], 4)
    assert _same(d1, d2) and torch.equal(l1, l2)


def _clustered(rng, n, d, m):
    """rows drawn around 256 well separated centres per sub-space"""
    dsub = d // m
    centres = rng.standard_normal((m, 256, dsub)).astype(np.float32) * 10
    pick = rng.integers(0, 256, size=(n, m))
    x = np.concatenate([centres[s][pick[:, s]] for s in range(m)], axis=1)
    return (x + rng.standard_normal((n, d)) * 0.3).astype(np.float32)


def _mse(index, x):
    codes = ops.pq_encode_rows(_dev(x), index.codebooks)
    return float(((ops.pq_decode_rows(codes, index.codebooks) - _dev(x)).double() ** 2).sum(1).mean())


def test_training_is_seeded_and_lowers_the_reconstruction_error():
    rng = np.random.default_rng(3)
    d, m = 8, 2
    x = _clustered(rng, 6000, d, m)
    a, b = GpuPQIndex("l2", d, m, device=DEV, seed=5), GpuPQIndex("l2", d, m, device=DEV, seed=5)
    a.train(x, niter=4)
    b.train(x, niter=4)
    assert a.is_trained and _same(a.codebooks, b.codebooks) and tuple(a.codebooks.shape) == (m, 256, d // m)
    # Lloyd's descent from given initial codebooks: 256 sample rows per sub-space
    c0 = np.stack([x[:256, s * (d // m):(s + 1) * (d // m)] for s in range(m)])
    start = GpuPQIndex("l2", d, m, device=DEV)
    start.train(codebooks=c0)
    trained = GpuPQIndex("l2", d, m, device=DEV)
    trained.train(x, niter=10, init_codebooks=c0)
    e0, e1 = _mse(start, x), _mse(trained, x)
    assert e1 < e0, (e0, e1)
    # a sample smaller than the data is drawn with the seed; fewer than 256 rows: the missing centroids copy centroid 0
    s1, s2 = GpuPQIndex("l2", d, m, device=DEV, seed=9), GpuPQIndex("l2", d, m, device=DEV, seed=9)
    s1.train(x, niter=2, max_points_per_centroid=4)
    s2.train(x, niter=2, max_points_per_centroid=4)
    assert _same(s1.codebooks, s2.codebooks)
    few = GpuPQIndex("l2", d, m, device=DEV)
    few.train(x[:40], niter=3)
    cb = few.codebooks.cpu().numpy()
    assert (cb[:, 40:] == cb[:, :1]).all() and np.isfinite(cb).all()
    few.add_items(x[:200])
    assert int(few._codes[:200, :m].max()) < 40


@pytest.mark.parametrize("dsub", (1, 2))
def test_training_on_the_narrowest_sub_spaces(dsub):
    """dim == M and dim == 2 M: the k-means behind train() assigns through the dense cosine kernel on rows one and two wide"""
    rng = np.random.default_rng(10 + dsub)
    m = 2
    d = m * dsub
    x = _clustered(rng, 4000, d, m)
    c0 = np.stack([x[:256, s * dsub:(s + 1) * dsub] for s in range(m)])
    start = GpuPQIndex("l2", d, m, device=DEV)
    start.train(codebooks=c0)
    a, b = GpuPQIndex("l2", d, m, device=DEV), GpuPQIndex("l2", d, m, device=DEV)
    a.train(x, niter=6, init_codebooks=c0)
    b.train(x, niter=6, init_codebooks=c0)
    assert _same(a.codebooks, b.codebooks) and bool(torch.isfinite(a.codebooks).all())
    e0, e1 = _mse(start, x), _mse(a, x)
    assert e1 < e0, (e0, e1)
    seeded = GpuPQIndex("l2", d, m, device=DEV, seed=3)      # k-means++ seeding as well
    seeded.train(x, niter=3)
    assert bool(torch.isfinite(seeded.codebooks).all()) and _mse(seeded, x) < float((x.astype(np.float64) ** 2).sum(1).mean())


@pytest.mark.parametrize("space", ("ip", "cosine"))
def test_save_and_load(space, tmp_path):
    rng = np.random.default_rng(4)
    cb = pc.random_codebooks(rng, D, M)
    x, q = rng.standard_normal((500, D)).astype(np.float32), rng.standard_normal((7, D)).astype(np.float32)
    labels = rng.permutation(5000)[:500].astype(np.int64)
    index = GpuPQIndex(space, D, M, device=DEV)
    index.train(codebooks=cb)
    index.add_items(x, labels)
    path = str(tmp_path / "pq.npz")
    index.save_index(path)
    z = np.load(path, allow_pickle=False)
    assert z["pq_codes"].shape == (500, M) and z["pq_codes"].dtype == np.uint8 and int(z["M"]) == M and str(z["space"]) == space
    again = GpuPQIndex(space, D, M, device=DEV)
    again.load_index(path)
    assert again.is_trained and again.get_current_count() == 500
    s0, l0 = index.search(_dev(q), 10)
    s1, l1 = again.search(_dev(q), 10)
    assert _same(s0, s1) and torch.equal(l0, l1)
    again.add_items(x[:5], np.arange(9000, 9005))
    assert again.get_current_count() == 505
    with pytest.raises(ValueError):
        GpuPQIndex("l2", D, M, device=DEV).load_index(path)
    with pytest.raises(ValueError):
        GpuPQIndex(space, D, 3, device=DEV).load_index(path)


def test_semantic_search_pipeline_with_a_pq_index(tmp_path):
    transformers = pytest.importorskip("transformers")
    from text_similarity_amd.configurations.config import ModelParameters, SearchConfiguration
    from text_similarity_amd.models.sentence_encoder import SentenceTransformerWrapper
    from text_similarity_amd.pipeline.search_pipeline import SemanticSearchPipeline
    preset = "tiny-bert"
    cfg = presets.PRESETS[preset]
    tok = transformers.BertTokenizer(vocab=presets.synthetic_vocab(cfg.vocab), do_lower_case=True)
    params = SearchConfiguration(model_parameters=ModelParameters(preset, hidden_size=cfg.hidden), model=preset, save_path="",
                                 tokenizer=tok, device=torch.device(DEV), max_tokens_per_batch=1024, max_seqs_per_batch=64,
                                 sequence_max_len=48)
    model = SentenceTransformerWrapper.from_preset(preset, params, parallel_mode=False)
    sents = list(presets.synthetic_sentences(60, seed="pq/s", vocab_size=cfg.vocab))
    pq = SemanticSearchPipeline(str(tmp_path / "pq"), params, model, corpus=sents, index_type="pq", pq_m=8)
    assert isinstance(pq.index, GpuPQIndex) and pq.index.M == 8 and pq.num_indexed() == 60
    res = pq(sents[:6], 5)
    assert sorted(res) == list(range(6)) and all(len(v) == 5 and set(v) <= set(sents) for v in res.values())
    labels, scores = pq.last_labels.clone(), pq.last_scores.clone()
    assert os.path.exists(os.path.join(str(tmp_path / "pq"), "pq_index.bin"))
    again = SemanticSearchPipeline(str(tmp_path / "pq"), params, model, corpus=sents, index_type="pq", pq_m=8)
    assert again(sents[:6], 5) == res
    assert torch.equal(again.last_labels, labels) and _same(again.last_scores, scores)
    assert _same(again.index.codebooks, pq.index.codebooks)
    with pytest.raises(NotImplementedError, match="flat"):       # deletion is out of scope: refused by name, nothing removed
        pq.remove_from_index([0])
    assert pq.num_indexed() == 60
    with pytest.raises(ValueError, match="'pq'"):
        SemanticSearchPipeline(str(tmp_path / "x"), params, model, corpus=sents, index_type="hnsw")
