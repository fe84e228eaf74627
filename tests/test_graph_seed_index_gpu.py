"""GpuGraphIndex(entry='coarse') on the GPU: the seed table against the list oracle, the search against the restatement of
tests/graph_seed_cases.py fed the index's own graph, centroids and seeds — bit for bit — and, on a corpus whose kNN graph is a
set of islands, the recall that per-query entry points restore and shared entry points do not have."""
import functools

import numpy as np
import pytest
import torch

from graph_cases import graph_search_ref
from graph_seed_cases import graph_search_seeded_ref, island_corpus, recall, seed_table_ref
from list_cases import same_bits
from text_similarity_amd import presets
from text_similarity_amd.graph_index import GpuGraphIndex
from text_similarity_amd.index import GpuFlatIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SPACES = ("cosine", "ip", "euclidean")
REF_SPACE = {"cosine": "cosine", "ip": "dot", "euclidean": "l2"}
ISLAND = dict(M=4, ef=16, width=2, max_iters=32)      # R = 8, K0 = 16: the CPU check of tests/test_graph_seed_cpu.py


@functools.lru_cache(maxsize=None)
def _island():
    return island_corpus()      # rows [2048, 32], centres [64, 32], queries [48, 32]


def _coarse_index(space, rows, **kw):
    ix = GpuGraphIndex(space, rows.shape[1], device=DEV, entry="coarse", **kw)
    ix.add_items(rows)
    return ix


def _assert_search_is_ref(ix, space, q, k, what, route=None):
    """ix.search against the restatement on the index's own graph, centroids, seeds and tombstones; returns the row numbers."""
    ix.coarse = route or "auto"
    lab, sc = ix.search(q, k)      # (first: a stale graph is rebuilt here)
    ix.coarse = "auto"
    n = ix.get_current_count()
    ef, iters = ix.search_params(k)
    dead = ix._dead[:n].cpu().numpy()
    ids = np.where(dead, -1, np.arange(n)).astype(np.int32)
    T = ix.centroids.shape[0]
    s, i, _, _ = graph_search_seeded_ref(REF_SPACE[space], q, ix._f32[:n].cpu().numpy(), ix.graph.cpu().numpy(), ef, ix.width, iters, k,
                                         centroids=ix.centroids.cpu().numpy(), n_probe=min(ix.nprobe, T), seeds=ix.seeds.cpu().numpy(),
                                         row_ids=ids if dead.any() else None)
    labels = ix._labels[:n].cpu().numpy()
    assert (lab.cpu().numpy() == np.where(i >= 0, labels[np.maximum(i, 0)], -1)).all(), what
    assert same_bits(sc.cpu().numpy(), s), what
    return i


@pytest.mark.parametrize("space", SPACES)
def test_island_corpus(space):
    rows, cent, qs = _island()
    k = 5
    ix = _coarse_index(space, rows, nprobe=2, seeds_per_list=2, **ISLAND)
    ix.build(centroids=cent)
    assert ix.graph.shape == (2048, 8) and ix.seeds.shape == (64, 2) and ix.seeds.dtype == torch.int32
    assert (ix.seeds.cpu().numpy() == seed_table_ref(REF_SPACE[space], cent, rows, 2)).all()
    assert ix.search_params(k) == (16, 32)
    i_kernel = _assert_search_is_ref(ix, space, qs, k, (space, "kernel"), route="kernel")
    i_flat = _assert_search_is_ref(ix, space, qs, k, (space, "flat"), route="flat")      # the two routes of the probes
    assert (i_kernel == i_flat).all()
    flat = GpuFlatIndex(space=space, dim=32, device=DEV)
    flat.add_items(rows)
    truth = flat.search(qs, k)[0].cpu().numpy()
    r_coarse = recall(ix.search(qs, k)[0].cpu().numpy(), truth)
    shared = GpuGraphIndex(space, 32, device=DEV, entry="shared", n_entries=8, **ISLAND)
    shared.add_items(rows)
    r_shared = recall(shared.search(qs, k)[0].cpu().numpy(), truth)
    assert torch.equal(shared.graph, ix.graph)
    print(f"{space}: recall@5 coarse {r_coarse:.3f}, shared {r_shared:.3f}")
    assert r_coarse >= 0.9
    assert r_shared <= 0.25


TRAINED_NPROBE = 2      # the island case's; k-means centres need not sit one an island, so this is where to raise it


@pytest.mark.parametrize("space", SPACES)
def test_device_trained_centres(space):
    """nlist = 64 centres from the device k-means: the search is the restatement's on them, and they still route the queries
    into their islands — recall@5 over the 48 queries >= 0.8, the floor of the issue."""
    rows, _, qs = _island()
    ix = _coarse_index(space, rows, nlist=64, nprobe=TRAINED_NPROBE, seeds_per_list=2, **ISLAND)
    _assert_search_is_ref(ix, space, qs[:16], 5, space)
    flat = GpuFlatIndex(space=space, dim=32, device=DEV)
    flat.add_items(rows)
    r = recall(ix.search(qs, 5)[0].cpu().numpy(), flat.search(qs, 5)[0].cpu().numpy())
    print(f"{space}: trained centres, nprobe {TRAINED_NPROBE}: recall@5 {r:.3f}")
    assert r >= 0.8
    assert ix.centroids.shape == (64, 32) and ix.seeds.shape == (64, 2)
    assert (ix.seeds.cpu().numpy() == seed_table_ref(REF_SPACE[space], ix.centroids.cpu().numpy(), rows, 2)).all()
    # the quantiser is GpuIVFIndex's, bit for bit
    from text_similarity_amd.ivf_index import GpuIVFIndex
    ivf = GpuIVFIndex(space=space, dim=32, nlist=64, device=DEV)
    ivf.add_items(rows)
    ivf.train()
    assert torch.equal(ivf.centroids, ix.centroids)


def test_nlist_default_and_clamp():
    rng = np.random.default_rng(2)
    rows = rng.standard_normal((150, 16)).astype(np.float32)
    ix = _coarse_index("cosine", rows, M=4, nprobe=64, seeds_per_list=4)
    ix.build()
    assert ix.centroids.shape[0] == 12 and ix.search_params(5)[1] >= 1      # int(sqrt(150)); nprobe is clamped to the lists
    _assert_search_is_ref(ix, "cosine", rows[:3] + 0.5, 5, "nprobe > nlist")
    ix = _coarse_index("cosine", rows[:40], M=4, nlist=50, nprobe=2, seeds_per_list=8)
    ix.build()
    assert ix.centroids.shape[0] == 40 and ix.seeds.shape == (40, 8)
    _assert_search_is_ref(ix, "cosine", rows[:3] + 0.5, 3, "nlist > n")


@pytest.mark.parametrize("space", SPACES)
def test_shared_entry_is_unchanged_by_the_new_arguments(space):
    rng = np.random.default_rng(3)
    rows, q = rng.standard_normal((300, 32)).astype(np.float32), rng.standard_normal((7, 32)).astype(np.float32)
    ix = GpuGraphIndex(space, 32, M=4, device=DEV)
    ix.add_items(rows)
    lab, sc = ix.search(q, 10)
    assert ix.entry == "shared" and ix.centroids is None and ix.seeds is None
    ef, iters = ix.search_params(10)
    s, i, _ = graph_search_ref(REF_SPACE[space], q, rows, ix.graph.cpu().numpy(), ix.entries.cpu().numpy(), ef, ix.width, iters, 10)
    assert (lab.cpu().numpy() == i).all() and same_bits(sc.cpu().numpy(), s)
    other = GpuGraphIndex(space, 32, M=4, device=DEV, entry="shared", nlist=7, nprobe=3, seeds_per_list=5)
    other.add_items(rows)
    lab2, sc2 = other.search(q, 10)
    assert torch.equal(lab, lab2) and same_bits(sc.cpu().numpy(), sc2.cpu().numpy()) and torch.equal(ix.graph, other.graph)


@pytest.mark.parametrize("space", SPACES)
def test_deletion_add_and_rebuild(space):
    rows, cent, qs = _island()
    ix = _coarse_index(space, rows[:1024], nlist=32, nprobe=2, seeds_per_list=2, **ISLAND)
    ix.build()
    seeds0 = ix.seeds.clone()
    # a deleted seed still routes: the tables stay, the row is never returned
    gone = sorted({int(ix.seeds[p, 0]) for p in range(4)})
    for r in gone:
        ix.mark_deleted(r)
    i = _assert_search_is_ref(ix, space, qs[:12], 5, (space, "deleted"))
    assert torch.equal(ix.seeds, seeds0) and not np.isin(i, gone).any()
    # adding rows makes graph, centroids and seeds stale together; the next search rebuilds them over the compacted rows
    ix.add_items(rows[1024:1200], ids=np.arange(5000, 5176))
    assert ix.graph is None
    _assert_search_is_ref(ix, space, qs[:12], 5, (space, "added"))
    n = ix.get_current_count()
    assert n == 1200 - len(gone) and ix.seeds.shape == (32, 2) and int(ix.seeds.max()) < n
    assert (ix.seeds.cpu().numpy() == seed_table_ref(REF_SPACE[space], ix.centroids.cpu().numpy(), ix._f32[:n].cpu().numpy(), 2)).all()
    # given centroids survive a rebuild
    ix.build(centroids=cent)
    ix.add_items(rows[1200:1210], ids=np.arange(6000, 6010))
    _assert_search_is_ref(ix, space, qs[:12], 5, (space, "given centroids, rebuilt"))
    assert torch.equal(ix.centroids.cpu(), torch.from_numpy(cent))


@pytest.mark.parametrize("space", SPACES)
def test_save_and_load(space, tmp_path):
    rows, cent, qs = _island()
    shared = GpuGraphIndex(space, 32, device=DEV, **ISLAND)
    shared.add_items(rows[:600])
    shared.save_index(str(tmp_path / "shared.bin"))
    z = np.load(str(tmp_path / "shared.bin"))
    assert sorted(z.files) == sorted(["rows_f32", "labels", "dead", "graph", "entries", "dim", "space", "R", "K0", "ef", "width",
                                      "n_entries", "seed", "kind"])      # exactly the arrays of a file written before entry= existed
    ix = GpuGraphIndex(space, 32, device=DEV, entry="coarse")
    ix.load_index(str(tmp_path / "shared.bin"))
    assert ix.entry == "shared" and ix.centroids is None
    want, got = shared.search(qs, 5), ix.search(qs, 5)
    assert torch.equal(want[0], got[0]) and same_bits(want[1].cpu().numpy(), got[1].cpu().numpy())

    co = _coarse_index(space, rows[:600], nlist=16, nprobe=3, seeds_per_list=2, **ISLAND)
    co.mark_deleted(7)
    want = co.search(qs, 5)
    co.save_index(str(tmp_path / "coarse.bin"))
    z = np.load(str(tmp_path / "coarse.bin"))
    assert {"centroids", "seeds", "entry", "nprobe", "seeds_per_list"} <= set(z.files) and str(z["entry"]) == "coarse"
    back = GpuGraphIndex(space, 32, device=DEV)
    back.load_index(str(tmp_path / "coarse.bin"))
    assert (back.entry, back.nprobe, back.seeds_per_list, back.nlist) == ("coarse", 3, 2, 16)
    assert torch.equal(back.centroids, co.centroids) and torch.equal(back.seeds, co.seeds) and torch.equal(back.graph, co.graph)
    got = back.search(qs, 5)
    assert torch.equal(want[0], got[0]) and same_bits(want[1].cpu().numpy(), got[1].cpu().numpy())
    _assert_search_is_ref(back, space, qs[:8], 5, (space, "loaded"))
    # a file with the five fields the format promises and no more
    kept = {name: z[name] for name in z.files if name not in ("nlist", "given_centroids")}
    with open(str(tmp_path / "five.bin"), "wb") as f:
        np.savez(f, **kept)
    five = GpuGraphIndex(space, 32, device=DEV)
    five.load_index(str(tmp_path / "five.bin"))
    assert (five.entry, five.nprobe, five.seeds_per_list, five.nlist) == ("coarse", 3, 2, 0) and torch.equal(five.seeds, co.seeds)
    got = five.search(qs, 5)
    assert torch.equal(want[0], got[0]) and same_bits(want[1].cpu().numpy(), got[1].cpu().numpy())
    # an empty coarse index stays coarse through its file
    empty = GpuGraphIndex(space, 32, device=DEV, entry="coarse", nlist=16, nprobe=3, seeds_per_list=2, **ISLAND)
    empty.save_index(str(tmp_path / "empty.bin"))
    back = GpuGraphIndex(space, 32, device=DEV)
    back.load_index(str(tmp_path / "empty.bin"))
    assert (back.entry, back.nprobe, back.seeds_per_list, back.nlist, back.get_current_count()) == ("coarse", 3, 2, 16, 0)
    assert back.centroids is None and (back.search(qs[:2], 5)[0] == -1).all()
    back.add_items(rows[:600])
    back.mark_deleted(7)
    got = back.search(qs, 5)
    assert torch.equal(back.centroids, co.centroids) and torch.equal(want[0], got[0]) and same_bits(want[1].cpu().numpy(), got[1].cpu().numpy())


def test_entry_point_budget():
    for nprobe, S in ((257, 1), (1, 257), (129, 2), (0, 4), (4, 0), (-1, 4)):
        with pytest.raises(ValueError):
            GpuGraphIndex("cosine", 8, device=DEV, entry="coarse", nprobe=nprobe, seeds_per_list=S)
    ix = GpuGraphIndex("cosine", 8, device=DEV, entry="coarse", nprobe=64, seeds_per_list=4)
    with pytest.raises(ValueError, match="257|outside"):
        ix.set_nprobe(65)
    ix.set_nprobe(1)
    assert ix.nprobe == 1
    with pytest.raises(ValueError):
        GpuGraphIndex("cosine", 8, device=DEV, entry="per-query")
    with pytest.raises(ValueError, match="coarse"):
        GpuGraphIndex("cosine", 8, device=DEV).build(centroids=np.zeros((2, 8), np.float32))
    # the budget is the coarse mode's: shared entry points ignore both numbers
    shared = GpuGraphIndex("cosine", 8, device=DEV, entry="shared", nprobe=100, seeds_per_list=300)
    shared.set_nprobe(1000)
    assert shared.entry == "shared"


def test_semantic_search_pipeline_with_coarse_entries(tmp_path):
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
    params.M, params.ef_construction, params.ef = 4, 16, 16
    model = SentenceTransformerWrapper.from_preset(preset, params, parallel_mode=False)
    sents = list(presets.synthetic_sentences(60, seed="graph/s", vocab_size=cfg.vocab))
    gr = SemanticSearchPipeline(str(tmp_path / "graph"), params, model, corpus=sents, index_type="graph", graph_entry="coarse",
                                nlist=6, nprobe=2)
    ix = gr.index
    assert isinstance(ix, GpuGraphIndex) and (ix.entry, ix.nlist, ix.nprobe) == ("coarse", 6, 2) and ix.centroids.shape[0] == 6
    out = gr(sents[:6], 5)
    emb = gr.encode_corpus(sents[:6])
    i = _assert_search_is_ref(ix, gr.index.space, emb.float().cpu().numpy(), 5, "pipeline")
    assert out == {q: [sents[j] for j in row if j >= 0] for q, row in enumerate(i.tolist())}
    again = SemanticSearchPipeline(str(tmp_path / "graph"), params, model, corpus=sents, index_type="graph", graph_entry="coarse",
                                   nlist=6, nprobe=2)
    assert again.index.entry == "coarse" and torch.equal(again.index.seeds, ix.seeds) and again(sents[:6], 5) == out
    with pytest.raises(ValueError, match="graph"):
        SemanticSearchPipeline(str(tmp_path / "flat"), params, model, corpus=sents, graph_entry="coarse")
    default = SemanticSearchPipeline(str(tmp_path / "shared"), params, model, corpus=sents, index_type="graph", nprobe=100)
    assert default.index.entry == "shared" and default.index.centroids is None
