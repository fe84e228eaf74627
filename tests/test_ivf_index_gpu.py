"""GpuIVFIndex on the GPU: at nprobe == nlist it returns what GpuFlatIndex returns on the same rows, bit for bit; at a partial
nprobe what the oracle of tests/ivf_cases.py returns for the list numbers and probes recomputed on the host from the index's
centroids.  N = 3 000 rows of a seeded mixture, nlist = 16, the centroids given (one case is trained, with a seed)."""
import functools
import os

import numpy as np
import pytest
import torch

from ivf_cases import ivf_ref
from list_cases import pair_scores, same_bits
from text_similarity_amd import presets
from text_similarity_amd.index import GpuFlatIndex
from text_similarity_amd.ivf_index import GpuIVFIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, NLIST, NQ = 3000, 16, 8
SPACES = ("cosine", "ip", "euclidean")
REF_SPACE = {"cosine": "cosine", "ip": "dot", "euclidean": "l2"}


@functools.lru_cache(maxsize=None)
def _data(d, seed=0):
    """(centres [NLIST, d], rows [N, d], queries [NQ, d]): a mixture around the centres, the queries drawn from it too."""
    rng = np.random.default_rng(1000 * seed + d)
    cent = rng.standard_normal((NLIST, d)).astype(np.float32)
    rows = (cent[rng.integers(0, NLIST, size=N)] + 0.35 * rng.standard_normal((N, d))).astype(np.float32)
    q = (cent[rng.integers(0, NLIST, size=NQ)] + 0.35 * rng.standard_normal((NQ, d))).astype(np.float32)
    return cent, rows, q


def _coarse_ref(space, x, cent, k):
    """The k nearest centres of each row of x, best first, ties to the lower list — and the assertion that the data has no
    tie among the first k + 1 (so that the prediction does not rest on the tie rule)."""
    n, m = x.shape[0], cent.shape[0]
    sc = pair_scores(REF_SPACE[space], x, cent, np.repeat(np.arange(n), m), np.tile(np.arange(m), n)).reshape(n, m)
    key = sc.astype(np.float64) if space == "euclidean" else -sc.astype(np.float64)
    order = np.argsort(key, axis=1, kind="stable")
    best = np.take_along_axis(key, order, axis=1)[:, :min(k + 1, m)]
    assert (np.diff(best, axis=1) > 0).all(), "the data has a coarse tie"
    return order[:, :k]


def _ivf(space, d, nprobe, labels=None, train_first=True):
    cent, rows, _ = _data(d)
    ix = GpuIVFIndex(space, d, NLIST, nprobe=nprobe, device=DEV)
    if train_first:
        ix.train(centroids=cent)
    ix.add_items(rows, labels)
    if not train_first:
        ix.train(centroids=cent)
    return ix


def _flat(space, d, labels=None):
    fl = GpuFlatIndex(space, d, device=DEV)
    fl.add_items(_data(d)[1], labels)
    return fl


def _same(a, b):
    return bool(torch.equal(a[0], b[0])) and same_bits(a[1].cpu().numpy(), b[1].cpu().numpy())


@pytest.mark.parametrize("d", [64, 384])
@pytest.mark.parametrize("space", SPACES)
def test_full_probing_equals_the_flat_index(space, d):
    q = _data(d)[2]
    ix, fl = _ivf(space, d, NLIST), _flat(space, d)
    for k in (1, 10, 100):
        assert _same(ix.search(q, k), fl.search(q, k)), (space, d, k)
    few_i = GpuIVFIndex(space, d, NLIST, nprobe=NLIST, device=DEV)
    few_i.train(centroids=_data(d)[0])
    few_f = GpuFlatIndex(space, d, device=DEV)
    for ix2 in (few_i, few_f):
        ix2.add_items(_data(d)[1][:7], np.arange(7) + 50)
    got, ref = few_i.search(q, 12), few_f.search(q, 12)                     # k > N: padding
    assert _same(got, ref) and (got[0][:, 7:] == -1).all() and torch.isinf(got[1][:, 7:]).all()
    labels, dist = ix.knn_query(q, 5)
    fl_labels, fl_dist = fl.knn_query(q, 5)
    assert (labels == fl_labels).all() and same_bits(dist, fl_dist)


@pytest.mark.parametrize("d", [64, 384])
@pytest.mark.parametrize("space", SPACES)
def test_partial_probing_equals_the_oracle(space, d):
    cent, rows, q = _data(d)
    ln = _coarse_ref(space, rows, cent, 1)[:, 0]
    for nprobe in (1, 3):
        ix = _ivf(space, d, nprobe, train_first=nprobe == 1)        # (trained before / after the rows came: the same lists)
        assert (ix._list[:N].cpu().numpy() == ln).all()
        probes = _coarse_ref(space, q, cent, nprobe)
        for k in (10, 100):
            rs, ri, _ = ivf_ref(REF_SPACE[space], q, rows, ln, probes, k, nlist=NLIST)
            lab, s = ix.search(q, k)
            assert (lab.cpu().numpy() == ri).all() and same_bits(s.cpu().numpy(), rs), (space, d, nprobe, k)
    ix.set_nprobe(NLIST)
    assert _same(ix.search(q, 10), _flat(space, d).search(q, 10))
    for bad in (0, NLIST + 1):
        with pytest.raises(ValueError):
            ix.set_nprobe(bad)
    ix.set_ef(50)                                                   # accepted, ignored


@pytest.mark.parametrize("space", SPACES)
def test_deletion(space):
    d = 64
    q = _data(d)[2]
    ix, fl = _ivf(space, d, NLIST), _flat(space, d)
    for lab in range(0, N, 3):
        ix.mark_deleted(lab)
        fl.mark_deleted(lab)
    assert ix.num_live() == fl.num_live() == N - len(range(0, N, 3)) and ix.get_current_count() == N
    got = ix.search(q, 50)
    assert _same(got, fl.search(q, 50))
    assert (got[0] % 3 != 0).all()
    ix.set_nprobe(2)
    lab = ix.search(q, 50)[0]
    assert ((lab % 3 != 0) | (lab < 0)).all()
    with pytest.raises(RuntimeError):
        ix.mark_deleted(0)


@pytest.mark.parametrize("space", SPACES)
def test_add_after_train_with_large_labels(space):
    d = 64
    cent, rows, q = _data(d)
    labels = (np.random.default_rng(2).permutation(N).astype(np.int64) << 20) + (1 << 33)
    ix = GpuIVFIndex(space, d, NLIST, nprobe=NLIST, device=DEV)
    ix.init_index(max_elements=100)
    ix.train(centroids=cent)
    fl = GpuFlatIndex(space, d, device=DEV)
    for a in range(0, N, 1100):                                     # three batches, growing past the reserved capacity
        ix.add_items(rows[a:a + 1100], labels[a:a + 1100])
        fl.add_items(rows[a:a + 1100], labels[a:a + 1100])
        assert _same(ix.search(q, 10), fl.search(q, 10))
    got = ix.search(q, 10)[0]
    assert (got > (1 << 32)).all() and np.isin(got.cpu().numpy(), labels).all()
    ix.set_nprobe(3)
    ln = _coarse_ref(space, rows, cent, 1)[:, 0]
    rs, ri, _ = ivf_ref(REF_SPACE[space], q, rows, ln, _coarse_ref(space, q, cent, 3), 10, nlist=NLIST)
    lab, s = ix.search(q, 10)
    assert (lab.cpu().numpy() == labels[ri]).all() and same_bits(s.cpu().numpy(), rs)


def test_training_is_seeded_and_an_untrained_index_trains_itself():
    d = 64
    _, rows, q = _data(d)
    a = GpuIVFIndex("cosine", d, NLIST, nprobe=2, device=DEV, seed=5)
    a.add_items(rows)
    a.train(niter=10, max_points_per_list=64)                       # a seeded sample of 64 * 16 rows
    b = GpuIVFIndex("cosine", d, NLIST, nprobe=2, device=DEV, seed=5)
    b.train(rows, niter=10, max_points_per_list=64)
    b.add_items(rows)
    assert a.centroids.shape == (NLIST, d) and torch.equal(a.centroids, b.centroids)
    assert _same(a.search(q, 10), b.search(q, 10))
    # hnswlib's call sequence: no train call at all
    c = GpuIVFIndex("cosine", d, NLIST, nprobe=NLIST, device=DEV, seed=5)
    c.init_index(max_elements=N)
    c.add_items(rows)
    assert not c.is_trained
    labels, dist = c.knn_query(q, k=10)
    assert c.is_trained and c.centroids.shape == (NLIST, d)
    fl_labels, fl_dist = _flat("cosine", d).knn_query(q, k=10)
    assert (labels == fl_labels).all() and same_bits(dist, fl_dist)
    with pytest.raises(ValueError):
        GpuIVFIndex("cosine", d, NLIST, device=DEV).train(rows[:NLIST - 1])


def test_recall_grows_with_nprobe():
    d = 64
    _, rows, _ = _data(d)
    q = _data(d, seed=1)[1][:64]                                    # queries from ANOTHER mixture: they fall between the lists
    ix = GpuIVFIndex("euclidean", d, NLIST, device=DEV, seed=3)
    ix.add_items(rows)
    ix.train(niter=10)
    truth = _flat("euclidean", d).search(q, 10)[0].cpu().numpy()
    recall = []
    for nprobe in (1, 4, 16):
        ix.set_nprobe(nprobe)
        got = ix.search(q, 10)[0].cpu().numpy()
        recall.append(np.mean([len(set(got[j]) & set(truth[j])) / 10.0 for j in range(q.shape[0])]))
    assert recall[0] <= recall[1] <= recall[2] == 1.0, recall


@pytest.mark.parametrize("space", SPACES)
def test_save_and_load(space, tmp_path):
    d = 64
    q = _data(d)[2]
    ix = _ivf(space, d, 3)
    ix.mark_deleted(17)
    path = str(tmp_path / "ivf.bin")
    ix.save_index(path)
    back = GpuIVFIndex(space, 0, 1, device=DEV)
    back.load_index(path)
    assert (back.nlist, back.nprobe, back.dim, back.num_live()) == (NLIST, 3, d, N - 1)
    assert torch.equal(back.centroids, ix.centroids) and torch.equal(back._list[:N - 1], ix._list[:N - 1])
    assert _same(back.search(q, 20), ix.search(q, 20))
    other = "ip" if space != "ip" else "cosine"
    with pytest.raises(ValueError):
        GpuIVFIndex(other, d, NLIST, device=DEV).load_index(path)
    flat_path = str(tmp_path / "flat.bin")
    _flat(space, d).save_index(flat_path)
    with pytest.raises(ValueError):
        GpuIVFIndex(space, d, NLIST, device=DEV).load_index(flat_path)
    z = np.load(path, allow_pickle=False)
    assert str(z["kind"]) == "ivf" and {"rows_f32", "labels", "lists", "centroids", "space", "nlist", "nprobe"} <= set(z.files)


def test_what_the_index_does_not_do_names_the_flat_index():
    ix = _ivf("cosine", 64, 2)
    q = _data(64)[2]
    for call in (lambda: ix.search(q, 5, filter=[1, 2]), lambda: ix.knn_query(q, 5, filter=lambda x: True),
                 lambda: ix.range_search(q, 0.5), lambda: ix.range_query(q, 0.5), lambda: ix.radius_search(q, 1.0),
                 lambda: ix.radius_query(q, 1.0)):
        with pytest.raises(NotImplementedError, match="GpuFlatIndex"):
            call()
    with pytest.raises(ValueError):
        GpuIVFIndex("l2", 64, 4, device=DEV)
    with pytest.raises(ValueError):
        GpuIVFIndex("euclidean", 768, 4, device=DEV)
    empty = GpuIVFIndex("cosine", 64, 4, device=DEV)
    lab, s = empty.search(q, 3)
    assert (lab == -1).all() and torch.isinf(s).all()


def test_semantic_search_pipeline_with_an_ivf_index(tmp_path):
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
    sents = list(presets.synthetic_sentences(60, seed="ivf/s", vocab_size=cfg.vocab))
    flat = SemanticSearchPipeline(str(tmp_path / "flat"), params, model, corpus=sents)
    ivf = SemanticSearchPipeline(str(tmp_path / "ivf"), params, model, corpus=sents, index_type="ivf", nlist=8, nprobe=8)
    assert isinstance(ivf.index, GpuIVFIndex) and isinstance(flat.index, GpuFlatIndex) and ivf.num_indexed() == 60
    assert ivf(sents[:6], 5) == flat(sents[:6], 5)
    assert os.path.exists(os.path.join(str(tmp_path / "ivf"), "index.bin"))
    again = SemanticSearchPipeline(str(tmp_path / "ivf"), params, model, corpus=sents, index_type="ivf", nlist=8, nprobe=8)
    assert again(sents[:6], 5) == flat(sents[:6], 5)
    with pytest.raises(ValueError):
        SemanticSearchPipeline(str(tmp_path / "x"), params, model, corpus=sents, index_type="hnsw")
