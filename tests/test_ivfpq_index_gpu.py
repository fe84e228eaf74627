"""GpuIVFPQIndex and SemanticSearchPipeline(index_type="ivfpq") on the GPU: the index is a coarse quantiser, ops.pq_encode_rows on
residuals and ops.ivfpq_search with labels, storage and a file around them.  Its results are compared for equality with
GpuPQIndex (no residuals, every list probed) and with the numpy restatement in tests/ivfpq_cases.py."""
import os

import numpy as np
import pytest
import torch

import ivfpq_cases as ic
import pq_cases as pc
from text_similarity_amd import ops, presets
from text_similarity_amd.ivfpq_index import GpuIVFPQIndex
from text_similarity_amd.pq_index import GpuPQIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, M, NLIST = 24, 6, 5


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return np.array_equal(_np(a).view(np.uint32), _np(b).view(np.uint32))


def _data(seed, n=700, nq=9, d=D, nlist=NLIST, m=M):
    rng = np.random.default_rng(seed)
    cent = (2 * rng.standard_normal((nlist, d))).astype(np.float32)
    x = (cent[rng.integers(0, nlist, size=n)] + rng.standard_normal((n, d))).astype(np.float32)
    q = (cent[rng.integers(0, nlist, size=nq)] + rng.standard_normal((nq, d))).astype(np.float32)
    return rng, cent, pc.random_codebooks(rng, d, m), x, q


@pytest.mark.parametrize("space", ("ip", "l2", "cosine"))
def test_without_residuals_and_every_list_probed_it_is_the_pq_index(space):
    rng, cent, cb, x, q = _data(1)
    labels = rng.permutation(10_000)[:700].astype(np.int64) + (1 << 33)
    index = GpuIVFPQIndex(space, D, NLIST, NLIST, M, by_residual=False, device=DEV)
    assert not index.is_trained
    with pytest.raises(RuntimeError):
        index.add_items(x[:3])
    with pytest.raises(RuntimeError):
        index.search(q, 3)
    index.train(centroids=cent, codebooks=cb)
    assert index.is_trained and index.get_current_count() == 0
    s0, l0 = index.search(q, 3)                                                   # an empty index pads
    assert (l0 == -1).all() and torch.isinf(s0).all()
    index.add_items(x[:300], labels[:300])
    index.add_items(x[300:], labels[300:])
    flat = GpuPQIndex(space, D, M, device=DEV)
    flat.train(codebooks=cb)
    flat.add_items(x, labels)
    for k in (1, 20, 1024):
        got_s, got_l = index.search(q, k)
        want_s, want_l = flat.search(q, k)
        assert _same(got_s, want_s) and torch.equal(got_l, want_l), k
    lab, val = index.knn_query(q, 20)
    got_s, got_l = index.search(q, 20)
    assert np.array_equal(lab, _np(got_l)) and np.array_equal(val, _np(got_s))
    with pytest.raises(ValueError):
        GpuIVFPQIndex("hamming", D, NLIST, 1, M)
    with pytest.raises(ValueError):
        GpuIVFPQIndex("ip", 25, NLIST, 1, 6)
    with pytest.raises(ValueError):
        GpuIVFPQIndex("ip", D, NLIST, NLIST + 1, M)
    for call in (lambda: index.search(q, 3, filter=[1, 2]), lambda: index.range_search(q, 0.5), lambda: index.radius_query(q, 0.5)):
        with pytest.raises(NotImplementedError, match="GpuFlatIndex"):
            call()


@pytest.mark.parametrize("space", ("ip", "l2", "cosine"))
def test_with_residuals_it_is_the_restatement(space):
    rng, cent, cb, x, q = _data(2)
    index = GpuIVFPQIndex(space, D, NLIST, NLIST, M, device=DEV)
    index.train(centroids=cent, codebooks=cb)
    index.add_items(x)
    xs, qs = (_np(GpuPQIndex.normalise(_dev(x))), _np(GpuPQIndex.normalise(_dev(q)))) if space == "cosine" else (x, q)
    adc = "l2" if space == "l2" else "ip"
    lists = _np(index._list[:700])                                                # the coarse assignment is the exact search's
    codes = ic.encode_ref(xs, cent, lists, cb)
    assert np.array_equal(_np(index._codes[:700]), codes)
    probes = _np(index._coarse(_dev(qs), NLIST))
    assert (np.sort(probes, axis=1) == np.arange(NLIST)).all()
    for k in (10, 1024):
        s, l = index.search(q, k)
        ws, wi = ic.search_ref(qs, cent, cb, codes, lists, probes, k, adc)
        assert np.array_equal(_np(s).view(np.uint32), ws.view(np.uint32)) and np.array_equal(_np(l), wi), k
    index.set_nprobe(1)                                                           # one list: every label lies in the nearest one
    s, l = index.search(q, 10)
    ws, wi = ic.search_ref(qs, cent, cb, codes, lists, probes[:, :1], 10, adc)
    assert np.array_equal(_np(s).view(np.uint32), ws.view(np.uint32)) and np.array_equal(_np(l), wi)
    found = _np(l) >= 0                                                           # (a short list pads)
    assert found[:, 0].all() and (lists[_np(l).clip(min=0)] == probes[:, :1])[found].all()
    with pytest.raises(ValueError):
        index.set_nprobe(0)
    rec = index.reconstruct([5, 0, 699])                                          # centroid + decoded residual
    want = _dev(cent)[_dev(lists[[5, 0, 699]])] + ops.pq_decode_rows(_dev(codes[[5, 0, 699]]), _dev(cb))
    assert _same(rec, want)
    with pytest.raises(RuntimeError):
        index.reconstruct([700])


def test_deletion():
    rng, cent, cb, x, q = _data(3)
    labels = np.arange(700, dtype=np.int64) * 3
    index = GpuIVFPQIndex("l2", D, NLIST, 3, M, device=DEV)
    index.train(centroids=cent, codebooks=cb)
    index.add_items(x, labels)
    s, l = index.search(q, 5)
    gone = [int(v) for v in _np(l[:, 0])]
    for g in set(gone):
        index.mark_deleted(g)
    assert index.num_live() == 700 - len(set(gone)) and index.get_current_count() == 700
    with pytest.raises(RuntimeError):
        index.mark_deleted(gone[0])                                               # already gone
    with pytest.raises(RuntimeError):
        index.mark_deleted(7)                                                     # never there
    s1, l1 = index.search(q, 5)
    assert not np.isin(_np(l1), gone).any() and index.get_current_count() == index.num_live()
    keep = ~np.isin(labels, gone)
    fresh = GpuIVFPQIndex("l2", D, NLIST, 3, M, device=DEV)
    fresh.train(centroids=cent, codebooks=cb)
    fresh.add_items(x[keep], labels[keep])
    s2, l2 = fresh.search(q, 5)
    assert _same(s1, s2) and torch.equal(l1, l2)


def test_seeded_training_is_reproducible():
    rng, cent, cb, x, q = _data(4, n=1500)
    a, b = (GpuIVFPQIndex("l2", D, NLIST, 2, M, device=DEV, seed=5) for _ in range(2))
    for index in (a, b):
        index.train(x, niter=5)
        index.add_items(x)
    assert a.is_trained and a.centroids.shape == (NLIST, D) and a.codebooks.shape == (M, 256, D // M)
    assert _same(a.centroids, b.centroids) and _same(a.codebooks, b.codebooks)
    assert torch.equal(a._codes[:1500], b._codes[:1500]) and torch.equal(a._list[:1500], b._list[:1500])
    sa, la = a.search(q, 10)
    sb, lb = b.search(q, 10)
    assert _same(sa, sb) and torch.equal(la, lb) and (la >= 0).all()
    # the codebooks were trained on residuals: they sit around zero, not around the centroids
    assert float(a.codebooks.abs().mean()) < float(a.centroids.abs().mean())
    given = GpuIVFPQIndex("l2", D, NLIST, 2, M, device=DEV, seed=5)              # given centroids are installed as they are
    given.train(x, niter=5, centroids=cent)
    assert _same(given.centroids, _dev(cent)) and given.codebooks is not None
    with pytest.raises(ValueError):
        GpuIVFPQIndex("l2", D, NLIST, 2, M, device=DEV).train()


@pytest.mark.parametrize("space", ("ip", "cosine"))
def test_save_and_load(space, tmp_path):
    rng, cent, cb, x, q = _data(5, n=500)
    labels = rng.permutation(5000)[:500].astype(np.int64)
    index = GpuIVFPQIndex(space, D, NLIST, 2, M, device=DEV)
    index.train(centroids=cent, codebooks=cb)
    index.add_items(x, labels)
    index.mark_deleted(int(labels[7]))
    path = str(tmp_path / "ivfpq.npz")
    index.save_index(path)
    z = np.load(path, allow_pickle=False)
    assert z["ivfpq_codes"].shape == (499, M) and z["ivfpq_codes"].dtype == np.uint8 and str(z["kind"]) == "ivfpq"
    assert int(z["M"]) == M and str(z["space"]) == space and int(z["nlist"]) == NLIST and int(z["nprobe"]) == 2
    again = GpuIVFPQIndex(space, D, NLIST, 1, M, device=DEV)
    again.load_index(path)
    assert again.is_trained and again.get_current_count() == 499 and again.nprobe == 2
    s0, l0 = index.search(_dev(q), 10)
    s1, l1 = again.search(_dev(q), 10)
    assert _same(s0, s1) and torch.equal(l0, l1)
    again.add_items(x[:5], np.arange(9000, 9005))
    assert again.get_current_count() == 504
    with pytest.raises(ValueError):
        GpuIVFPQIndex("l2", D, NLIST, 1, M, device=DEV).load_index(path)          # another space
    with pytest.raises(ValueError):
        GpuIVFPQIndex(space, D, NLIST, 1, 3, device=DEV).load_index(path)         # another M
    flat = GpuPQIndex(space, D, M, device=DEV)                                    # another kind, both ways
    flat.train(codebooks=cb)
    flat.add_items(x, labels)
    pq_path = str(tmp_path / "pq.npz")
    flat.save_index(pq_path)
    with pytest.raises(ValueError):
        GpuIVFPQIndex(space, D, NLIST, 1, M, device=DEV).load_index(pq_path)
    with pytest.raises(ValueError):                                               # residual codes are not row codes
        GpuPQIndex(space, D, M, device=DEV).load_index(path)


def test_width_1024():
    d, m, nlist = 1024, 64, 4
    rng, cent, cb, x, q = _data(6, n=600, nq=5, d=d, nlist=nlist, m=m)
    for space in ("ip", "l2"):
        index = GpuIVFPQIndex(space, d, nlist, nlist, m, device=DEV)
        index.train(centroids=cent, codebooks=cb)
        index.add_items(x)
        lists = _np(index._list[:600])
        codes = ic.encode_ref(x, cent, lists, cb)
        assert np.array_equal(_np(index._codes[:600]), codes)
        probes = _np(index._coarse(_dev(q), nlist))
        s, l = index.search(q, 20)
        ws, wi = ic.search_ref(q, cent, cb, codes, lists, probes, 20, space)
        assert np.array_equal(_np(s).view(np.uint32), ws.view(np.uint32)) and np.array_equal(_np(l), wi)
        if space == "l2":                                                        # rows sit nearest their own centroid
            assert (lists == np.argmin(((x[:, None, :].astype(np.float64) - cent[None]) ** 2).sum(-1), axis=1)).all()


def test_training_on_rows_wider_than_the_float_searches():
    """train(data) above width 768: the centres from the k-means as it stands, rows assigned by the torch product"""
    d, m, nlist = 832, 13, 4
    rng, cent, _, x, q = _data(7, n=600, nq=5, d=d, nlist=nlist, m=m)
    a, b = (GpuIVFPQIndex("l2", d, nlist, nlist, m, device=DEV, seed=3) for _ in range(2))
    for index in (a, b):
        index.train(x, niter=3)
        index.add_items(x)
    assert a.centroids.shape == (nlist, d) and _same(a.centroids, b.centroids) and _same(a.codebooks, b.codebooks)
    assert torch.equal(a._codes[:600], b._codes[:600])
    c, cb, lists = _np(a.centroids), _np(a.codebooks), _np(a._list[:600])
    assert (lists == np.argmin(((x[:, None, :].astype(np.float64) - c[None]) ** 2).sum(-1), axis=1)).all()
    codes = ic.encode_ref(x, c, lists, cb)
    assert np.array_equal(_np(a._codes[:600]), codes)
    probes = _np(a._coarse(_dev(q), nlist))
    assert (probes[:, 0] == np.argmin(((q[:, None, :].astype(np.float64) - c[None]) ** 2).sum(-1), axis=1)).all()
    s, l = a.search(q, 20)
    ws, wi = ic.search_ref(q, c, cb, codes, lists, probes, 20, "l2")
    assert np.array_equal(_np(s).view(np.uint32), ws.view(np.uint32)) and np.array_equal(_np(l), wi)
    with pytest.raises(ValueError):
        GpuIVFPQIndex("l2", d, 700, 1, m, device=DEV).train(x)                    # fewer rows than lists


def test_semantic_search_pipeline_with_an_ivfpq_index(tmp_path):
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
    sents = list(presets.synthetic_sentences(60, seed="ivfpq/s", vocab_size=cfg.vocab))
    kw = dict(corpus=sents, index_type="ivfpq", nlist=4, nprobe=4, pq_m=8)
    pipe = SemanticSearchPipeline(str(tmp_path / "ix"), params, model, **kw)
    assert isinstance(pipe.index, GpuIVFPQIndex) and pipe.index.M == 8 and pipe.index.nlist == 4 and pipe.num_indexed() == 60
    res = pipe(sents[:6], 5)
    assert sorted(res) == list(range(6)) and all(len(v) == 5 and set(v) <= set(sents) for v in res.values())
    labels, scores = pipe.last_labels.clone(), pipe.last_scores.clone()
    assert os.path.exists(os.path.join(str(tmp_path / "ix"), "ivfpq_index.bin"))
    again = SemanticSearchPipeline(str(tmp_path / "ix"), params, model, **kw)
    assert again(sents[:6], 5) == res
    assert torch.equal(again.last_labels, labels) and _same(again.last_scores, scores)
    assert _same(again.index.codebooks, pipe.index.codebooks) and _same(again.index.centroids, pipe.index.centroids)
    first = [int(v) for v in set(_np(labels[:, 0]).tolist())]
    pipe.remove_from_index(first + [10_000])                                      # (an unknown id is skipped)
    assert pipe.num_indexed() == 60 - len(first)
    pipe(sents[:6], 5)
    assert not np.isin(_np(pipe.last_labels), first).any()
    pipe.add_to_index(["one more sentence"])
    assert pipe.num_indexed() == 61 - len(first)
    with pytest.raises(NotImplementedError):
        pipe(sents[:2], 3, filter=[1, 2, 3])
    with pytest.raises(ValueError, match="'ivfpq'"):
        SemanticSearchPipeline(str(tmp_path / "x"), params, model, corpus=sents, index_type="hnsw")
