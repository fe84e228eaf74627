"""GpuGraphIndex(incremental=True) on the GPU: the graph after ``add_items`` equals tests/graph_insert_cases.insert_ref id for id
— B in {1, 40, 300} new rows with insert_batch = 64: one, one and five sub-batches, new rows choosing each other — in both entry
modes and all three spaces at N = 600, d = 24; the search after it is the restated beam search on the index's own graph;
deleted rows never appear in a new row's edges; ``build(insert_from=m)`` is build-then-add; files round-trip and an old file
loads as non-incremental; the pipeline's ``add_to_index`` keeps the graph; and without ``incremental`` everything is as before.

(M, width, n_entries) = (4, 2, 8): R = 8, K0 = 16, so the candidate search runs ceil(48 / 4) + 8 = 20 iterations.  The restated
base graph of the 600 rows is built once per space and shared."""
import functools
import os

import numpy as np
import pytest
import torch

import graph_insert_cases as gic
from graph_cases import build_graph_ref, graph_search_ref
from graph_seed_cases import graph_search_seeded_ref
from list_cases import same_bits
from text_similarity_amd import ops, presets
from text_similarity_amd.graph_index import GpuGraphIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPACES = ("cosine", "ip", "euclidean")
REF_SPACE = {"cosine": "cosine", "ip": "dot", "euclidean": "l2"}
N, D, M, WIDTH, BATCH = 600, 24, 4, 2, 64
R, K0 = 8, 16
MODES = {"shared": dict(entry="shared", n_entries=8), "coarse": dict(entry="coarse", nlist=16, nprobe=2, seeds_per_list=2)}


@functools.lru_cache(maxsize=None)
def _rows():
    rng = np.random.default_rng(77)
    c = rng.standard_normal((N, D)).astype(np.float32)
    extra = rng.standard_normal((300, D)).astype(np.float32)
    extra[5] = extra[4]                                    # duplicates inside a sub-batch, and of an old row
    extra[70] = c[10]
    q = rng.standard_normal((6, D)).astype(np.float32)
    return c, extra, q


@functools.lru_cache(maxsize=None)
def _base_graph(space):
    return build_graph_ref(REF_SPACE[space], _rows()[0], K0, R)


def _index(space, mode, rows=None, **kw):
    ix = GpuGraphIndex(space, D, M=M, width=WIDTH, device=DEV, **{"incremental": True, "insert_batch": BATCH, **MODES[mode], **kw})
    ix.add_items(_rows()[0] if rows is None else rows)
    return ix


def _how(ix):
    """The entry mode of the index as insert_ref takes it."""
    if ix.entry == "shared":
        return dict(entries=ix.entries.cpu().numpy())
    T = ix.centroids.shape[0]
    return dict(seeded=dict(centroids=ix.centroids.cpu().numpy(), n_probe=min(ix.nprobe, T), seeds=ix.seeds.cpu().numpy()))


def _assert_search_is_ref(ix, space, q, k, what):
    """ix.search against the restated beam search on the index's own graph, entry points and tombstones (the helper of
    tests/test_graph_index_gpu.py and tests/test_graph_seed_index_gpu.py, for either entry mode)."""
    lab, sc = ix.search(q, k)
    n = ix.get_current_count()
    ef, iters = ix.search_params(k)
    dead = ix._dead[:n].cpu().numpy()
    ids = np.where(dead, -1, np.arange(n)).astype(np.int32) if dead.any() else None
    rows, graph = ix._f32[:n].cpu().numpy(), ix.graph.cpu().numpy()
    if ix.entry == "shared":
        s, i, _ = graph_search_ref(REF_SPACE[space], q, rows, graph, ix.entries.cpu().numpy(), ef, ix.width, iters, k, row_ids=ids)
    else:
        s, i, _, _ = graph_search_seeded_ref(REF_SPACE[space], q, rows, graph, ef, ix.width, iters, k, row_ids=ids, **_how(ix)["seeded"])
    labels = ix._labels[:n].cpu().numpy()
    assert (lab.cpu().numpy() == np.where(i >= 0, labels[np.maximum(i, 0)], -1)).all(), what
    assert same_bits(sc.cpu().numpy(), s), what


@pytest.mark.parametrize("B", [1, 40, 300])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("space", SPACES)
def test_add_items_inserts_and_the_graph_is_the_restatement(space, mode, B):
    c, extra, q = _rows()
    ix = _index(space, mode)
    ix.build()
    base = ix.graph.cpu().numpy()
    assert (base == _base_graph(space)).all()
    entries, centroids, seeds = ix.entries.clone(), ix.centroids, ix.seeds
    ix.add_items(extra[:B], ids=np.arange(10_000, 10_000 + B))
    assert ix.graph is not None and ix.graph.shape == (N + B, R) and ix.graph.dtype == torch.int32 and ix.get_current_count() == N + B
    assert torch.equal(ix.entries, entries) and ix.centroids is centroids and ix.seeds is seeds      # nothing else moved
    ef, iters = ix.insert_params()
    assert (ef, iters) == (K0, 20)
    want = gic.insert_ref(REF_SPACE[space], c, base, extra[:B], K0, R, BATCH, WIDTH, iters, **_how(ix))
    got = ix.graph.cpu().numpy()
    assert (got == want).all(), (space, mode, B, np.argwhere(got != want)[:5].tolist())
    assert (got[N:, 0] >= 0).all()                                         # every new row has an edge ...
    if B == 300:
        assert (got[N:] >= N).any() and (got[:N] >= N).any()               # ... new rows choose each other, old rows take new ones
        assert not (got[:N, :R // 2] != base[:, :R // 2]).any()            # the front half of an old row never moves
    _assert_search_is_ref(ix, space, q, 10, (space, mode, B))


@pytest.mark.parametrize("mode", list(MODES))
def test_deleted_rows_route_the_insertion_and_are_never_linked(mode):
    space = "cosine"
    c, extra, q = _rows()
    ix = _index(space, mode)
    ix.build()
    base = ix.graph.cpu().numpy()
    near = ix.search(extra[:40], 3)[0].cpu().numpy()
    gone = sorted(set(near.reshape(-1).tolist()))[:25]                     # the rows the new ones would have chosen first
    for label in gone:
        ix.mark_deleted(label)
    ix.add_items(extra[:40])
    got = ix.graph.cpu().numpy()
    assert not np.isin(got[N:], gone).any()
    dead = np.zeros((N,), dtype=bool)
    dead[gone] = True
    want = gic.insert_ref(REF_SPACE[space], c, base, extra[:40], K0, R, BATCH, WIDTH, ix.insert_params()[1], dead=dead, **_how(ix))
    assert (got == want).all()
    assert ix.num_live() == N + 40 - len(gone) and ix.get_current_count() == N + 40      # nothing was compacted
    _assert_search_is_ref(ix, space, q, 10, (mode, "deleted"))
    ix.build()                                                             # an explicit build still rebuilds and compacts
    assert ix.get_current_count() == N + 40 - len(gone) and ix.graph.shape[0] == N + 40 - len(gone)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("space", SPACES)
def test_build_by_insertion_is_build_then_add(space, mode):
    c, extra, q = _rows()
    m = 400
    a = _index(space, mode, rows=c[:m])
    a.build()
    a.add_items(np.concatenate([c[m:], extra[:30]]))
    b = _index(space, mode, rows=np.concatenate([c, extra[:30]]), incremental=False)
    b.build(insert_from=m)
    assert torch.equal(a.graph, b.graph) and torch.equal(a.entries, b.entries) and a.graph.shape == (N + 30, R)
    if mode == "coarse":
        assert torch.equal(a.centroids, b.centroids) and torch.equal(a.seeds, b.seeds)
    # ... which is NOT the exact build, and a plain build() afterwards is
    b.build()
    assert not torch.equal(a.graph, b.graph)
    assert (b.graph.cpu().numpy() == build_graph_ref(REF_SPACE[space], np.concatenate([c, extra[:30]]), K0, R)).all()


def test_without_incremental_add_items_marks_the_graph_stale():
    c, extra, q = _rows()
    ix = _index("cosine", "shared", incremental=False)
    ix.build()
    ix.add_items(extra[:5])
    assert ix.graph is None
    fresh = _index("cosine", "shared")                     # incremental, but no graph yet: as today
    fresh.add_items(extra[:5])
    assert fresh.graph is None
    lab, _ = fresh.search(q, 3)
    assert fresh.graph.shape == (N + 5, R) and (lab >= 0).all()
    with pytest.raises(ValueError):
        GpuGraphIndex("cosine", D, device=DEV, insert_batch=0)


def test_files_round_trip_and_an_old_file_loads_as_non_incremental(tmp_path):
    c, extra, q = _rows()
    ix = _index("euclidean", "coarse")
    ix.add_items(extra[:70])                               # (no graph yet: stored)
    ix.build(insert_from=N)
    path = str(tmp_path / "graph.bin")
    ix.save_index(path)
    back = GpuGraphIndex("euclidean", 0, device=DEV)
    assert not back.incremental
    back.load_index(path)
    assert back.incremental and back.insert_batch == BATCH and torch.equal(back.graph, ix.graph)
    ix.add_items(extra[70:110])
    back.add_items(extra[70:110])
    assert back.graph is not None and torch.equal(back.graph, ix.graph)    # the loaded index inserts as the saved one does
    z = dict(np.load(path, allow_pickle=False))
    del z["incremental"], z["insert_batch"]
    old = str(tmp_path / "old.bin")
    with open(old, "wb") as f:
        np.savez(f, **z)
    legacy = GpuGraphIndex("euclidean", 0, device=DEV, incremental=True, insert_batch=7)
    legacy.load_index(old)
    assert not legacy.incremental and legacy.insert_batch == 1024
    legacy.add_items(extra[70:75])
    assert legacy.graph is None


def test_ops_graph_insert_is_one_step_and_refuses_what_it_cannot_do():
    c, extra, q = _rows()
    ix = _index("ip", "shared")
    ix.build()
    rows = torch.from_numpy(np.concatenate([c, extra[:64]])).to(DEV)
    graph = torch.cat([ix.graph, torch.full((64, R), -7, dtype=torch.int32, device=DEV)])
    new, st_prune, targets, st_link = ops.graph_insert("dot", rows, graph, N, K0, entries=ix.entries, width=WIDTH, max_iters=20)
    want = gic.insert_ref("dot", c, ix.graph.cpu().numpy(), extra[:64], K0, R, 64, WIDTH, 20, entries=ix.entries.cpu().numpy())
    assert (graph.cpu().numpy() == want).all() and new.data_ptr() == graph[N:].data_ptr()
    assert not st_prune.any() and not st_link.any() and st_prune.shape == (64,) and st_link.shape == targets.shape
    assert (np.diff(targets.cpu().numpy()) > 0).all()
    for bad in (dict(entries=None), dict(seeded=dict(probes=None))):
        with pytest.raises(ValueError):
            ops.graph_insert("dot", rows, graph, N, K0, width=WIDTH, **{"entries": ix.entries, **bad})
    with pytest.raises(ValueError):
        ops.graph_insert("dot", rows, graph, N + 64, K0, entries=ix.entries)       # no new rows
    with pytest.raises(ValueError):
        ops.graph_insert("dot", rows, graph, N, R - 1, entries=ix.entries)         # K0 < R


def test_the_pipeline_inserts_with_graph_incremental(tmp_path):
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
    sents = list(presets.synthetic_sentences(70, seed="graph/insert", vocab_size=cfg.vocab))
    gr = SemanticSearchPipeline(str(tmp_path / "graph"), params, model, corpus=sents[:60], index_type="graph", graph_incremental=True)
    assert isinstance(gr.index, GpuGraphIndex) and gr.index.incremental and gr.index.graph is not None
    gr.add_to_index(sents[60:])
    assert gr.index.graph is not None and gr.index.graph.shape[0] == 70 and gr.num_indexed() == 70
    assert (gr.index.graph[60:, 0] >= 0).all().item()      # every new row has an edge
    found = gr(sents[60:], 3)
    assert len(found) == 10 and all(len(r) == 3 for r in found.values())
    plain = SemanticSearchPipeline(str(tmp_path / "plain"), params, model, corpus=sents[:60], index_type="graph")
    plain.add_to_index(sents[60:])
    assert plain.index.graph is None
    again = SemanticSearchPipeline(str(tmp_path / "graph"), params, model, corpus=sents[:60], index_type="graph")
    assert not again.index.incremental                     # (the pipeline's word, not the file's)
    with pytest.raises(ValueError):
        SemanticSearchPipeline(str(tmp_path / "flat"), params, model, corpus=sents[:60], graph_incremental=True)
