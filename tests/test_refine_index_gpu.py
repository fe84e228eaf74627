"""The refine stage of GpuPQIndex and GpuIVFPQIndex on the GPU: the row store, search(..., rescore_multiplier=), files and the
pipeline.  Results are compared for equality — scores as bits — with the numpy restatement of tests/refine_cases.py, with
GpuFlatIndex / GpuIVFIndex over the stored rows once every row is a candidate, and with the ADC search where none is asked for."""
import os

import numpy as np
import pytest
import torch

import ivfpq_cases as ic
import pq_cases as pc
import refine_cases as rc
from text_similarity_amd import ops, presets
from text_similarity_amd.index import GpuFlatIndex
from text_similarity_amd.ivf_index import GpuIVFIndex
from text_similarity_amd.ivfpq_index import GpuIVFPQIndex
from text_similarity_amd.pq_index import GpuPQIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, M, NLIST, N = rc.D, rc.M, rc.NLIST, rc.N_ROWS
SPACES = ("ip", "l2", "cosine")
STORES = ("float32", "float16")
FLAT_SPACE = {"ip": "ip", "l2": "euclidean", "cosine": "cosine"}
NP_DTYPE = {"float32": np.float32, "float16": np.float16}


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _np(t):
    return t.cpu().numpy()


def _bits(a):
    a = np.ascontiguousarray(_np(a) if isinstance(a, torch.Tensor) else a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint16) if a.dtype == np.float16 else a


def _eq(got, want, what):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=str(what))


def _prepared(space, x):
    return _np(GpuPQIndex.normalise(_dev(x))) if space == "cosine" else x


def _labels(rng, n=N):
    return rng.permutation(10_000)[:n].astype(np.int64) + (1 << 33)


def _pq(space, refine, x, labels, cb):
    index = GpuPQIndex(space, x.shape[1], cb.shape[0], device=DEV, refine=refine)
    index.train(codebooks=cb)
    index.add_items(x[:300], labels[:300])
    index.add_items(_dev(x[300:]), labels[300:])
    return index


def _ivfpq(space, refine, x, labels, cent, cb, nprobe=NLIST, by_residual=True):
    index = GpuIVFPQIndex(space, x.shape[1], cent.shape[0], nprobe, cb.shape[0], by_residual=by_residual, device=DEV, refine=refine)
    index.train(centroids=cent, codebooks=cb)
    index.add_items(x[:300], labels[:300])
    index.add_items(_dev(x[300:]), labels[300:])
    return index


def _flat(space, rows, labels, q, k):
    flat = GpuFlatIndex(FLAT_SPACE[space], rows.shape[1], device=DEV)
    flat.init_index(rows.shape[0])
    flat.add_items(rows, labels)
    lab, s = flat.search(q, k)
    return s, lab


@pytest.mark.parametrize("refine", STORES)
@pytest.mark.parametrize("space", SPACES)
def test_pq_index(space, refine):
    cent, cb, x, q = rc.small_data()
    labels = _labels(np.random.default_rng(1))
    index = _pq(space, refine, x, labels, cb)
    store = rc.store_rows(x, refine)
    assert index.refine == refine and index._store.rows.dtype == getattr(torch, refine) and index._store.rows.shape[0] >= N
    _eq(index._store.rows[:N], store, "the store holds the rows as given, in arrival order")
    xs, qs = _prepared(space, x), _prepared(space, q)
    codes = pc.encode_ref(xs, cb)
    _eq(index._codes[:N], codes, "codes")
    for k in (1, 10, 64):
        for mult in (1, 3, 16):
            s, l = index.search(q, k, rescore_multiplier=mult)
            ws, wi, _ = rc.pq_refined_ref(space, q, qs, cb, codes, store, k, mult)
            _eq(s, ws, (k, mult, "scores"))
            _eq(l, np.where(wi >= 0, labels[wi.clip(min=0)], -1), (k, mult, "labels"))
    lab, val = index.knn_query(q, 10, rescore_multiplier=3)
    s, l = index.search(_dev(q), 10, 3)
    _eq(lab, l, "knn_query labels"), _eq(val, s, "knn_query values")
    # every row a candidate: the flat index of the matching space over the stored rows
    for k in (10, 64):
        s, l = index.search(q, k, rescore_multiplier=-(-N // k))
        fs, fl = _flat(space, store.astype(np.float32), labels, q, k)
        _eq(s, fs, (k, "flat scores")), _eq(l, fl, (k, "flat labels"))
    assert int(l.min()) > 1 << 33


@pytest.mark.parametrize("by_residual", (True, False))
@pytest.mark.parametrize("refine", STORES)
@pytest.mark.parametrize("space", SPACES)
def test_ivfpq_index(space, refine, by_residual):
    cent, cb, x, q = rc.small_data()
    if refine == "float16":            # (rows that ARE halves: GpuIVFIndex below then assigns the same rows to the same lists)
        x = rc.to_f16(x).astype(np.float32)
    labels = _labels(np.random.default_rng(2))
    index = _ivfpq(space, refine, x, labels, cent, cb, by_residual=by_residual)
    store = rc.store_rows(x, refine)
    _eq(index._store.rows[:N], store, "store")
    xs, qs = _prepared(space, x), _prepared(space, q)
    lists = _np(index._list[:N])
    codes = ic.encode_ref(xs, cent, lists, cb, by_residual=by_residual)
    _eq(index._codes[:N], codes, "codes")
    all_probes = _np(index._coarse(_dev(qs), NLIST))
    for nprobe in (1, 2, NLIST):
        index.set_nprobe(nprobe)
        probes = all_probes[:, :nprobe]
        for k, mult in ((10, 1), (10, 3), (64, 16), (1, 3)):
            s, l = index.search(q, k, rescore_multiplier=mult)
            ws, wi, _ = rc.ivfpq_refined_ref(space, q, qs, cent, cb, codes, lists, probes, store, k, mult, by_residual=by_residual)
            _eq(s, ws, (nprobe, k, mult, "scores"))
            _eq(l, np.where(wi >= 0, labels[wi.clip(min=0)], -1), (nprobe, k, mult, "labels"))
        if space != "cosine":          # every row of the probed lists a candidate: the float IVF index on the same centroids
            ivf = GpuIVFIndex(FLAT_SPACE[space], D, NLIST, nprobe, device=DEV)
            ivf.train(centroids=cent)
            ivf.add_items(store.astype(np.float32), labels)
            il, is_ = ivf.search(q, 10)
            s, l = index.search(q, 10, rescore_multiplier=70)
            _eq(s, is_, (nprobe, "ivf scores")), _eq(l, il, (nprobe, "ivf labels"))
    s, l = index.search(q, 10, rescore_multiplier=70)                               # nprobe = NLIST, 700 candidates
    fs, fl = _flat(space, store.astype(np.float32), labels, q, 10)
    _eq(s, fs, "flat scores"), _eq(l, fl, "flat labels")
    lab, val = index.knn_query(q, 10, rescore_multiplier=3)
    s, l = index.search(q, 10, rescore_multiplier=3)
    _eq(lab, l, "knn_query labels"), _eq(val, s, "knn_query values")


@pytest.mark.parametrize("kind", ("pq", "ivfpq"))
@pytest.mark.parametrize("space", SPACES)
def test_recall_rises_with_the_multiplier(space, kind):
    """The GPU twin of theorem 3 of tests/test_refine_cpu.py, on the data checked there."""
    cent, cb, x, q = rc.small_data()
    labels = np.arange(N, dtype=np.int64)
    index = _pq(space, "float32", x, labels, cb) if kind == "pq" else _ivfpq(space, "float32", x, labels, cent, cb)
    _, exact = _flat(space, x, labels, q, rc.K)
    exact = _np(exact)
    _, adc = index.search(q, rc.K)
    got = [rc.recall(_np(index.search(q, rc.K, rescore_multiplier=m)[1]), exact) for m in (1, 2, 4, 8, 16, 32, 64, 128)]
    print(f"{kind} {space}: recall@10 {got}")
    assert got[0] == rc.recall(_np(adc), exact) and got[0] < 1.0
    assert all(a <= b for a, b in zip(got, got[1:])) and got[-1] == 1.0          # (10 x 128 >= 700: every row a candidate)


def test_one_real_shape():
    d, m, n = 384, 48, 1500
    rng = np.random.default_rng(8)
    cb = pc.random_codebooks(rng, d, m, scale=0.05)
    x = (rng.standard_normal((n, d)) * 3).astype(np.float32)
    q = rng.standard_normal((7, d)).astype(np.float32)
    labels = np.arange(n, dtype=np.int64)[::-1].copy()
    index = _pq("cosine", "float16", x, labels, cb)
    xs, qs = _prepared("cosine", x), _prepared("cosine", q)
    codes = pc.encode_ref(xs, cb)
    _eq(index._codes[:n, :m], codes[:, :m], "codes")
    store = rc.to_f16(x)
    _eq(index._store.rows[:n], store, "store")
    for k, mult in ((10, 4), (10, 100)):
        s, l = index.search(q, k, rescore_multiplier=mult)
        ws, wi, _ = rc.pq_refined_ref("cosine", q, qs, cb, codes, store, k, mult)
        _eq(s, ws, (k, mult)), _eq(l, labels[wi], (k, mult))


def test_deletion_compacts_the_store_with_the_codes():
    cent, cb, x, q = rc.small_data(seed=3)
    labels = np.arange(N, dtype=np.int64) * 3
    for refine in STORES:
        index = _ivfpq("l2", refine, x, labels, cent, cb, nprobe=3)
        s, l = index.search(q, 5, rescore_multiplier=4)
        gone = sorted(set(int(v) for v in _np(l[:, :2]).ravel()))
        for g in gone:
            index.mark_deleted(g)
        s1, l1 = index.search(q, 5, rescore_multiplier=4)
        assert not np.isin(_np(l1), gone).any() and index.get_current_count() == N - len(gone)
        keep = ~np.isin(labels, gone)
        probes = _np(index._coarse(_dev(q), 3))

        def check(got, rows, labs, what):      # the restatement on the rows the index should hold now, in their order
            n = rows.shape[0]
            _eq(index._store.rows[:n], rc.store_rows(rows, refine), what + ": store")
            lists = _np(index._list[:n])
            codes = ic.encode_ref(rows, cent, lists, cb)
            _eq(index._codes[:n], codes, what + ": codes")
            ws, wi, _ = rc.ivfpq_refined_ref("l2", q, q, cent, cb, codes, lists, probes, rc.store_rows(rows, refine), 5, 4)
            _eq(got[0], ws, what), _eq(got[1], labs[wi], what)

        check((s1, l1), x[keep], labels[keep], "after deletion")
        index.add_items(x[~keep], labels[~keep] + 1)                               # add after delete
        assert index.get_current_count() == N
        check(index.search(q, 5, rescore_multiplier=4), np.concatenate([x[keep], x[~keep]]),
              np.concatenate([labels[keep], labels[~keep] + 1]), "after adding them again")


@pytest.mark.parametrize("space", SPACES)
def test_rescore_multiplier_handling(space):
    cent, cb, x, q = rc.small_data()
    labels = np.arange(N, dtype=np.int64)
    plain = (_pq(space, None, x, labels, cb), _ivfpq(space, None, x, labels, cent, cb, nprobe=2))
    for refine in STORES:
        for bare, index in zip(plain, (_pq(space, refine, x, labels, cb), _ivfpq(space, refine, x, labels, cent, cb, nprobe=2))):
            for k in (10, 1024):
                s0, l0 = bare.search(q, k)
                for got in (index.search(q, k), index.search(q, k, rescore_multiplier=None)):
                    _eq(got[0], s0, "ADC scores with a store"), _eq(got[1], l0, "ADC labels with a store")
            for bad in (0, -1, 1.5):
                with pytest.raises(ValueError):
                    index.search(q, 10, rescore_multiplier=bad)
            s, l = index.search(q[:0], 4, rescore_multiplier=2)                    # Q = 0
            assert s.shape == (0, 4) and l.shape == (0, 4)
    for bare in plain:
        assert bare.refine is None
        with pytest.raises(ValueError, match="refine="):
            bare.search(q, 10, rescore_multiplier=2)
    for make in (lambda: GpuPQIndex(space, D, M, device=DEV, refine="float16"),
                 lambda: GpuIVFPQIndex(space, D, NLIST, 1, M, device=DEV, refine="float16")):
        empty = make()                                                           # an empty index pads
        empty.train(**({"codebooks": cb} if isinstance(empty, GpuPQIndex) else {"centroids": cent, "codebooks": cb}))
        s, l = empty.search(q, 3, rescore_multiplier=2)
        assert (_np(l) == -1).all() and (np.isposinf(_np(s)) if space == "l2" else np.isneginf(_np(s))).all()


def test_construction_and_adding():
    cent, cb, x, q = rc.small_data()
    for cls, args in ((GpuPQIndex, ()), (GpuIVFPQIndex, (NLIST, 1))):
        with pytest.raises(ValueError, match="refine"):
            cls("ip", D, *args, M, device=DEV, refine="int8")
        with pytest.raises(ValueError, match="768"):
            cls("ip", 1024, *args, 64, device=DEV, refine="float32")
        with pytest.raises(ValueError, match="767"):
            cls("l2", 768, *args, 48, device=DEV, refine="float16")
        cls("cosine", 768, *args, 48, device=DEV, refine="float16")
        cls("l2", 1024, *args, 64, device=DEV)                                     # without a store every width still builds
    for refine in STORES:
        pq = _pq("ip", refine, x, np.arange(N), cb)
        with pytest.raises(ValueError, match="codes"):
            pq.add_items(np.zeros((3, M), np.uint8))
        ivf = _ivfpq("ip", refine, x, np.arange(N), cent, cb)
        for index in (pq, ivf):
            bad = x[:5].copy()
            bad[3, 7] = np.inf if refine == "float32" else 1e5
            before = (_np(index._codes[:N]).copy(), _np(index._store.rows[:N]).copy(), _np(index._labels[:N]).copy())
            with pytest.raises(ValueError):
                index.add_items(bad, np.arange(5) + 9000)
            assert index.get_current_count() == N
            for a, b in zip(before, (index._codes[:N], index._store.rows[:N], index._labels[:N])):
                _eq(b, a, "unchanged after a refused add")
            bad[3, 7] = np.nan
            with pytest.raises(ValueError):
                index.add_items(bad)
    plain = _pq("ip", None, x, np.arange(N), cb)
    plain.add_items(np.zeros((3, M), np.uint8))                                     # codes still go into an index without a store
    assert plain.get_current_count() == N + 3


@pytest.mark.parametrize("refine", STORES)
def test_files(refine, tmp_path):
    cent, cb, x, q = rc.small_data(n=500)
    labels = _labels(np.random.default_rng(5), 500)
    store = rc.store_rows(x, refine)
    for kind in ("pq", "ivfpq"):
        make = (lambda r: GpuPQIndex("cosine", D, M, device=DEV, refine=r)) if kind == "pq" else \
               (lambda r: GpuIVFPQIndex("cosine", D, NLIST, 2, M, device=DEV, refine=r))
        index = make(refine)
        index.train(**({"codebooks": cb} if kind == "pq" else {"centroids": cent, "codebooks": cb}))
        index.add_items(x, labels)
        path = str(tmp_path / f"{kind}.npz")
        index.save_index(path)
        z = np.load(path, allow_pickle=False)
        assert str(z["refine"]) == refine and z["refine_rows"].dtype == NP_DTYPE[refine] and z["refine_rows"].shape == (500, D)
        _eq(z["refine_rows"], store, "file rows")
        want = index.search(q, 10, rescore_multiplier=4)
        for built_with in (refine, None, "float32"):                              # the file decides
            again = make(built_with)
            again.load_index(path)
            assert again.refine == refine and again.get_current_count() == 500
            _eq(again._store.rows[:500], store, "loaded rows")
            got = again.search(q, 10, rescore_multiplier=4)
            _eq(got[0], want[0], "scores after load"), _eq(got[1], want[1], "labels after load")
        again.add_items(x[:5], np.arange(5))
        _eq(again._store.rows[500:505], store[:5], "rows added after load")
        bare = make(None)
        bare.train(**({"codebooks": cb} if kind == "pq" else {"centroids": cent, "codebooks": cb}))
        bare.add_items(x, labels)
        bare_path = str(tmp_path / f"{kind}_bare.npz")
        bare.save_index(bare_path)
        assert "refine" not in np.load(bare_path).files and "refine_rows" not in np.load(bare_path).files
        loaded = make(refine)
        loaded.load_index(bare_path)                                               # a file without a store loads as None
        assert loaded.refine is None and loaded._store is None
        with pytest.raises(ValueError, match="refine="):
            loaded.search(q, 10, rescore_multiplier=2)
        fields = dict(z)
        for rows in (fields["refine_rows"][:-1], fields["refine_rows"][:, :-1], fields["refine_rows"].astype(np.float64)):
            cut = str(tmp_path / f"{kind}_cut.npz")
            with open(cut, "wb") as f:
                np.savez(f, **{**fields, "refine_rows": rows})
            with pytest.raises(ValueError, match="malformed"):
                make(refine).load_index(cut)
    with pytest.raises(ValueError):                                                # an IVF-PQ file is still not a PQ file
        GpuPQIndex("cosine", D, M, device=DEV, refine=refine).load_index(str(tmp_path / "ivfpq.npz"))


def test_pipeline(tmp_path):
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
    sents = list(presets.synthetic_sentences(60, seed="refine/s", vocab_size=cfg.vocab))
    kw = dict(corpus=sents, index_type="ivfpq", nlist=4, nprobe=4, pq_m=8, refine="float16", rescore_multiplier=4)
    pipe = SemanticSearchPipeline(str(tmp_path / "ix"), params, model, **kw)
    assert pipe.index.refine == "float16" and pipe.num_indexed() == 60
    res = pipe(sents[:6], 5)
    emb = pipe.encode_corpus(sents[:6])
    s, l = pipe.index.search(emb, 5, rescore_multiplier=4)
    assert torch.equal(pipe.last_labels, l) and torch.equal(pipe.last_scores, s)
    assert res == {j: [sents[i] for i in row] for j, row in enumerate(_np(l).tolist())}
    s60, l60 = pipe.index.search(emb, 5, rescore_multiplier=12)                     # 60 candidates: every row
    _, fl = _flat("cosine", rc.to_f16(_np(pipe.encode_corpus(sents))).astype(np.float32), np.arange(60), emb, 5)
    assert torch.equal(l60, fl)
    again = SemanticSearchPipeline(str(tmp_path / "ix"), params, model, **kw)        # loads the file, store included
    assert again(sents[:6], 5) == res and again.index.refine == "float16"
    pq = SemanticSearchPipeline(str(tmp_path / "pq"), params, model, corpus=sents, index_type="pq", pq_m=8, refine="float32",
                                rescore_multiplier=12)
    pq(sents[:6], 5)
    assert torch.equal(pq.last_labels, _flat("cosine", _np(pq.encode_corpus(sents)), np.arange(60), emb, 5)[1])
    with pytest.raises(ValueError, match="refine"):
        SemanticSearchPipeline(str(tmp_path / "flat"), params, model, corpus=sents, index_type="flat", refine="float16")
    with pytest.raises(ValueError, match="refine"):                                # the file holds a store; this pipeline wants none
        SemanticSearchPipeline(str(tmp_path / "ix"), params, model, corpus=sents, index_type="ivfpq", nlist=4, nprobe=4, pq_m=8)
