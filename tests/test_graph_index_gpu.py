"""GpuGraphIndex on the GPU: the built graph equals the restatement of tests/graph_cases.py id for id, a search equals the
restated beam search on the index's own graph and entry points bit for bit, and with a beam that holds every row the index is
the exact search over the rows its entry points reach — which, for the seeded corpora here, is all of them (asserted: a test
that passed on an almost-empty graph would show nothing).

The corpora are standard-normal rows at (N, d, M, ef_construction, numpy seed) = (300, 32, 8, 32, 0), (600, 32, 4, 16, 0) and
(300, 32, 4, 16, 1) — (R, K0) = (16, 32), (8, 16), (8, 16).  The seeds were chosen with the restatement: with them every row is
reachable in all three spaces (seed 0 leaves one of the 300 rows of the third corpus unreachable under 'euclidean').  The
restated graph of each is built once per space and shared."""
import functools
import os

import numpy as np
import pytest
import torch

from graph_cases import build_graph_ref, degree_params, graph_search_ref, knn_graph_ref, reachable
from list_cases import list_topk_ref, same_bits
from text_similarity_amd import presets
from text_similarity_amd.graph_index import GpuGraphIndex
from text_similarity_amd.index import GpuFlatIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPACES = ("cosine", "ip", "euclidean")
REF_SPACE = {"cosine": "cosine", "ip": "dot", "euclidean": "l2"}
CORPORA = ((300, 32, 8, 32, 0), (600, 32, 4, 16, 0), (300, 32, 4, 16, 1))


@functools.lru_cache(maxsize=None)
def _rows(N, d, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((7, d)).astype(np.float32)
    return c, q


@functools.lru_cache(maxsize=None)
def _ref_graph(space, N, d, M, efc, seed):
    R, K0 = degree_params(M, efc)
    return build_graph_ref(REF_SPACE[space], _rows(N, d, seed)[0], K0, R)


def _index(space, N, d, M, efc, rows_seed, **kw):
    ix = GpuGraphIndex(space, d, device=DEV, **kw)
    ix.init_index(N, ef_construction=efc, M=M)
    ix.add_items(_rows(N, d, rows_seed)[0])
    return ix


def _same(a, b):
    return torch.equal(a[0], b[0]) and same_bits(a[1].cpu().numpy(), b[1].cpu().numpy())


def _assert_search_is_ref(ix, space, q, k, what):
    """ix.search against the restated beam search on the index's own graph, entry points and tombstones."""
    lab, sc = ix.search(q, k)      # (first: a stale graph is rebuilt here)
    n = ix.get_current_count()
    ef, iters = ix.search_params(k)
    dead = ix._dead[:n].cpu().numpy()
    ids = np.where(dead, -1, np.arange(n)).astype(np.int32)
    s, i, _ = graph_search_ref(REF_SPACE[space], q, ix._f32[:n].cpu().numpy(), ix.graph.cpu().numpy(), ix.entries.cpu().numpy(), ef,
                               ix.width, iters, k, row_ids=ids if dead.any() else None)
    labels = ix._labels[:n].cpu().numpy()
    assert (lab.cpu().numpy() == np.where(i >= 0, labels[np.maximum(i, 0)], -1)).all(), what
    assert same_bits(sc.cpu().numpy(), s), what
    return lab.cpu().numpy(), i


@pytest.mark.parametrize("corpus", CORPORA, ids=lambda c: "N%d-d%d-M%d-efc%d-seed%d" % c)
@pytest.mark.parametrize("space", SPACES)
def test_built_graph_search_and_exactness(space, corpus):
    N, d, M, efc, seed = corpus
    c, q = _rows(N, d, seed)
    R, K0 = degree_params(M, efc)
    ix = _index(space, N, d, M, efc, seed)
    assert (ix.R, ix.K0) == (R, K0)
    # the stages of the build, then the whole
    G0 = ix.knn_graph().cpu().numpy()
    assert (G0 == knn_graph_ref(REF_SPACE[space], c, K0)).all()
    ix.build()
    ref = _ref_graph(space, *corpus)
    g = ix.graph.cpu().numpy()
    assert g.shape == (N, R) and g.dtype == np.int32 and (g == ref).all()
    assert (ref >= 0).mean() > 0.9 and (ref != np.arange(N)[:, None]).all()           # a full graph without self edges
    e = ix.entries.cpu().numpy()
    assert e.shape == (64,) and len(set(e.tolist())) == 64 and (np.diff(e) > 0).all() and e.min() >= 0 and e.max() < N
    again = _index(space, N, d, M, efc, seed)
    again.build()
    assert torch.equal(again.entries, ix.entries) and torch.equal(again.graph, ix.graph)      # seeded
    other = _index(space, N, d, M, efc, seed, seed=1)
    other.build()
    assert not torch.equal(other.entries, ix.entries) and torch.equal(other.graph, ix.graph)  # the seed draws the entry points only
    # a search with the index's defaults is the restated beam search
    ix.set_ef(24)
    _assert_search_is_ref(ix, space, q, 10, (space, corpus, "ef=24"))
    # a beam that holds every row: the exact search over what the entry points reach — all N rows
    assert len(reachable(g, e, N)) == N
    wide = _index(space, N, d, M, efc, seed, ef=1024, max_iters=1 << 20)
    lab, sc = wide.search(q, 20)
    rs, ri, _ = list_topk_ref(REF_SPACE[space], q, c, np.arange(N), 20)
    assert (lab.cpu().numpy() == ri).all() and same_bits(sc.cpu().numpy(), rs)
    flat = GpuFlatIndex(space, d, device=DEV)
    flat.add_items(c)
    assert _same(wide.search(q, 20), flat.search(q, 20))


def test_recall_grows_with_ef_and_labels_are_mapped():
    N, d, M, efc, seed = CORPORA[1]
    c, q = _rows(N, d, seed)
    ix = GpuGraphIndex("cosine", d, device=DEV, n_entries=4)
    ix.init_index(N, ef_construction=efc, M=M)
    ix.add_items(c, ids=np.arange(N) * 5 + 2)
    _, ri, _ = list_topk_ref("cosine", q, c, np.arange(N), 10)
    recall = []
    for ef in (10, 40, 160):
        ix.set_ef(ef)
        lab, _ = _assert_search_is_ref(ix, "cosine", q, 10, ef)
        assert (lab[lab >= 0] % 5 == 2).all()
        recall.append(np.mean([len(set(lab[j].tolist()) & set((ri[j] * 5 + 2).tolist())) / 10 for j in range(q.shape[0])]))
    assert recall[0] <= recall[1] <= recall[2] and recall[2] >= 0.9, recall
    lab2, d2 = ix.knn_query(q, 3)
    assert lab2.shape == (7, 3) and (np.diff(d2, axis=1) >= 0).all()


@pytest.mark.parametrize("space", SPACES)
def test_deletion_add_after_build_and_rebuild(space):
    N, d, M, efc, seed = CORPORA[2]
    c, q = _rows(N, d, seed)
    ix = _index(space, N, d, M, efc, seed, ef=48)
    lab0, _ = ix.search(q, 10)
    graph0 = ix.graph.clone()
    # tombstones: the graph stays, the rows route the search and are not returned
    gone = sorted(set(lab0[:, 0].tolist()) | {int(lab0[0, 1])})
    for label in gone:
        ix.mark_deleted(label)
    with pytest.raises(RuntimeError):
        ix.mark_deleted(gone[0])
    assert ix.num_live() == N - len(gone) and ix.get_current_count() == N and torch.equal(ix.graph, graph0)
    lab1, _ = _assert_search_is_ref(ix, space, q, 10, (space, "deleted"))
    assert not np.isin(lab1, gone).any() and (lab1 >= 0).all()
    # add after build: the graph is stale, the next search rebuilds it over the live rows and the new ones
    rng = np.random.default_rng(9)
    extra = rng.standard_normal((40, d)).astype(np.float32)
    extra[0] = q[0]                                        # the best row of query 0 in every space but 'ip' ... and usually there
    ix.add_items(extra, ids=np.arange(10_000, 10_040))
    assert ix.graph is None and ix.get_current_count() == N + 40
    lab2, _ = _assert_search_is_ref(ix, space, q, 10, (space, "rebuilt"))
    n = N - len(gone) + 40
    assert ix.get_current_count() == n == ix.num_live() and ix.graph.shape == (n, ix.R)
    live = np.concatenate([np.delete(c, gone, axis=0), extra])
    assert (ix.graph.cpu().numpy() == build_graph_ref(REF_SPACE[space], live, ix.K0, ix.R)).all()
    assert not np.isin(lab2, gone).any()
    if space != "ip":
        assert lab2[0, 0] == 10_000
    # everything deleted: padding
    small = GpuGraphIndex(space, d, device=DEV)
    small.add_items(c[:3])
    for label in range(3):
        small.mark_deleted(label)
    lab, s = small.search(q, 2)
    assert (lab == -1).all() and torch.isinf(s).all()


@pytest.mark.parametrize("space", SPACES)
def test_save_and_load(space, tmp_path):
    N, d, M, efc, seed = CORPORA[2]
    q = _rows(N, d, seed)[1]
    ix = _index(space, N, d, M, efc, seed, ef=40, width=3, n_entries=16, seed=5)
    ix.search(q, 1)
    ix.mark_deleted(17)
    path = str(tmp_path / "graph.bin")
    ix.save_index(path)
    back = GpuGraphIndex(space, 0, device=DEV)
    back.load_index(path)
    assert (back.R, back.K0, back.dim, back.ef, back.width, back.n_entries, back.seed) == (ix.R, ix.K0, d, 40, 3, 16, 5)
    assert back.num_live() == N - 1 and back.get_current_count() == N
    assert torch.equal(back.graph, ix.graph) and torch.equal(back.entries, ix.entries) and back.entries.numel() == 16
    assert _same(back.search(q, 20), ix.search(q, 20))
    assert 17 not in back.search(q, 20)[0].cpu().numpy()
    other = "ip" if space != "ip" else "cosine"
    with pytest.raises(ValueError):
        GpuGraphIndex(other, d, device=DEV).load_index(path)
    flat_path = str(tmp_path / "flat.bin")
    flat = GpuFlatIndex(space, d, device=DEV)
    flat.add_items(_rows(N, d, seed)[0])
    flat.save_index(flat_path)
    with pytest.raises(ValueError, match="flat"):
        GpuGraphIndex(space, d, device=DEV).load_index(flat_path)
    z = np.load(path, allow_pickle=False)
    assert str(z["kind"]) == "graph" and {"rows_f32", "labels", "dead", "graph", "entries", "space", "R", "K0", "ef"} <= set(z.files)
    # an unbuilt index builds itself on save
    fresh = _index(space, N, d, M, efc, seed)
    fresh.save_index(str(tmp_path))
    assert fresh.graph is not None and os.path.exists(str(tmp_path / "index.bin"))


def test_what_the_index_does_not_do_names_the_flat_index():
    N, d, M, efc, seed = CORPORA[2]
    ix = _index("cosine", N, d, M, efc, seed)
    q = _rows(N, d, seed)[1]
    for call in (lambda: ix.search(q, 5, filter=[1, 2]), lambda: ix.knn_query(q, 5, filter=lambda x: True),
                 lambda: ix.range_search(q, 0.5), lambda: ix.range_query(q, 0.5), lambda: ix.radius_search(q, 1.0),
                 lambda: ix.radius_query(q, 1.0)):
        with pytest.raises(NotImplementedError, match="GpuFlatIndex"):
            call()
    for bad in (dict(space="l2"), dict(space="euclidean", dim=768), dict(width=5), dict(n_entries=257), dict(ef=1025)):
        with pytest.raises(ValueError):
            GpuGraphIndex(**{"space": "cosine", "dim": 64, "device": DEV, **bad})
    empty = GpuGraphIndex("cosine", d, device=DEV)
    lab, s = empty.search(q, 3)
    assert (lab == -1).all() and torch.isinf(s).all()
    # hnswlib's parameters: M and ef_construction set the degree and the build width, k above ef widens the beam
    big = GpuGraphIndex("cosine", d, device=DEV)
    big.init_index(10, ef_construction=400, M=64)
    assert (big.R, big.K0) == (64, 128)
    ix.set_ef(5)
    assert ix.search_params(12)[0] == 12 and ix.search(q, 12)[0].shape == (7, 12)


def test_semantic_search_pipeline_with_a_graph_index(tmp_path):
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
    params.M, params.ef_construction, params.ef = 4, 16, 64
    model = SentenceTransformerWrapper.from_preset(preset, params, parallel_mode=False)
    sents = list(presets.synthetic_sentences(60, seed="graph/s", vocab_size=cfg.vocab))
    flat = SemanticSearchPipeline(str(tmp_path / "flat"), params, model, corpus=sents)
    gr = SemanticSearchPipeline(str(tmp_path / "graph"), params, model, corpus=sents, index_type="graph")
    assert isinstance(gr.index, GpuGraphIndex) and gr.num_indexed() == 60
    assert (gr.index.R, gr.index.K0, gr.index.ef) == (8, 16, 64)          # the parameters reached the index
    assert gr(sents[:6], 5) == flat(sents[:6], 5)                         # a beam of 64 over 60 rows: exact
    assert os.path.exists(os.path.join(str(tmp_path / "graph"), "index.bin"))
    again = SemanticSearchPipeline(str(tmp_path / "graph"), params, model, corpus=sents, index_type="graph")
    assert again.index.ef == 64 and again(sents[:6], 5) == flat(sents[:6], 5)
    gr.remove_from_index([3])
    assert all(sents[3] not in r for r in gr(sents[:6], 5).values())
