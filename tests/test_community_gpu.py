"""ops.community_detection and the two pipelines on top of it, bit for bit against the restatement (tests/community_cases.
detect_ref) fed the scores and the order ops.cosine_range / ops.dot_range report for the same rows."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from community_cases import detect_ref, planted_rows
from conftest import golden
from text_similarity_amd import ops
from text_similarity_amd.pipeline.clustering import ClusteringPipeline
from text_similarity_amd.pipeline.search_pipeline import SentenceMiningPipeline

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAU, MIN_SIZE = 0.75, 10
_cache = {}


def _range(x, space, tau):
    """The range search of the rows against themselves, with the operands community_detection makes."""
    d = x.shape[1]
    if space == "cosine":
        u, rho = ops.l2norm_rows(x, return_rho=True)
        r = ops.cosine_range(u, u, d, tau, eq_f32=x, ec_f32=x, rho_c=rho)
    else:
        sc, rho, scale = ops.dot_scaled_rows(x)
        r = ops.dot_range(ops.l2norm_rows(x), sc, d, tau, eq_f32=x, ec_f32=x, rho_c=rho, scale_c=scale)
    return [t.cpu().numpy() for t in r]


def _planted(d, space):
    """(rows on the device, planted labels, the restatement's result): computed once per (d, space), never modified."""
    if (d, space) not in _cache:
        x, planted = planted_rows(d)
        xt = torch.from_numpy(x).to(DEV)
        _cache[(d, space)] = (xt, planted, detect_ref(*_range(xt, space, TAU), len(x), MIN_SIZE))
    return _cache[(d, space)]


def _equal(got, ref):
    for g, r, name in zip(got[:4], ref[:4], ("lims", "members", "centres", "labels")):
        g = g.cpu().numpy()
        assert g.dtype == np.int64 and np.array_equal(g, r), name


@pytest.mark.parametrize("space", ["cosine", "dot"])
@pytest.mark.parametrize("d", [32, 384])
def test_planted_clusters_equal_the_restatement(d, space):
    x, planted, ref = _planted(d, space)
    got = ops.community_detection(None, x, d, TAU, MIN_SIZE, space=space, return_info=True)
    _equal(got, ref)
    assert np.array_equal(got[4]["scores"].cpu().numpy().view(np.uint32), ref[4].view(np.uint32))
    lims, members = ref[0], ref[1]
    found = set()
    for k in range(len(lims) - 1):                           # every community lies inside one planted cluster
        inside = set(planted[members[lims[k]:lims[k + 1]]].tolist())
        assert len(inside) == 1 and -1 not in inside
        found |= inside
    assert found == set(range(6))                            # all six have at least MIN_SIZE rows: all are found
    assert (np.diff(np.diff(lims)) <= 0).all()               # largest first
    # the operands handed in ready, and the serial form alone, give the same
    if space == "cosine":
        u, rho = ops.l2norm_rows(x, return_rho=True)
        _equal(ops.community_detection(u, x, d, TAU, MIN_SIZE, rho=rho), ref)
    else:
        sc, rho, scale = ops.dot_scaled_rows(x)
        _equal(ops.community_detection(sc, x, d, TAU, MIN_SIZE, space="dot", rho=rho, scale=scale), ref)
    _equal(ops.community_detection(None, x, d, TAU, MIN_SIZE, space=space, max_rounds=0), ref)


def test_threshold_above_every_score_gives_nothing():
    x, _, _ = _planted(32, "cosine")
    lims, members, centres, labels = ops.community_detection(None, x, 32, 1.5, MIN_SIZE)
    assert lims.tolist() == [0] and members.numel() == 0 and centres.numel() == 0 and (labels == -1).all()
    assert labels.shape == (x.shape[0],)


@pytest.mark.parametrize("space", ["cosine", "dot"])
def test_min_size_one_labels_every_row(space):
    x, _, _ = _planted(32, space)
    got = ops.community_detection(None, x, 32, TAU, 1, space=space)
    _equal(got, detect_ref(*_range(x, space, TAU), x.shape[0], 1))
    assert (got[3] >= 0).all() and got[1].numel() == x.shape[0]         # a row alone is a community of one


def test_exact_duplicates_follow_the_tie_order():
    """Copies of rows, also of whole neighbourhoods: equal scores (ordered by index inside a community) and equal sizes
    (ordered by centre index among the candidates)."""
    x, _, _ = _planted(32, "cosine")
    x = x.clone()
    x[300:340] = x[100:140]
    x[7] = x[500]
    x[x.shape[0] - 1] = x[0]
    ref = detect_ref(*_range(x, "cosine", TAU), x.shape[0], MIN_SIZE)
    _equal(ops.community_detection(None, x, 32, TAU, MIN_SIZE), ref)
    _equal(ops.community_detection(None, x, 32, TAU, 3, max_rounds=1), detect_ref(*_range(x, "cosine", TAU), x.shape[0], 3))


def test_query_slice_boundary(monkeypatch):
    x, _, ref = _planted(32, "cosine")
    monkeypatch.setattr(ops, "MAX_RANGE_QUERIES_PER_CALL", 128)        # N ~ 590 rows: five slices, the last one short
    _equal(ops.community_detection(None, x, 32, TAU, MIN_SIZE), ref)


def test_max_members_is_checked_before_allocating(monkeypatch):
    x, _, ref = _planted(32, "cosine")
    lims = _range(x, "cosine", TAU)[0]
    sizes = np.diff(lims)
    need = int(sizes[sizes >= MIN_SIZE].sum())
    _equal(ops.community_detection(None, x, 32, TAU, MIN_SIZE, max_members=need), ref)
    real_empty, made = torch.empty, []

    def spy(*a, **kw):
        made.append(a[0] if a else kw.get("size"))
        return real_empty(*a, **kw)
    monkeypatch.setattr(torch, "empty", spy)
    with pytest.raises(ValueError, match="threshold is too low"):
        ops.community_detection(None, x, 32, TAU, MIN_SIZE, max_members=need - 1)
    assert need > 16 * x.shape[0]
    # nothing of the hits' size was allocated (the largest 1-D tensor is counts [N])
    assert not [m for m in made if isinstance(m, tuple) and len(m) == 1 and isinstance(m[0], int) and m[0] > x.shape[0]]
    monkeypatch.setattr(ops, "MAX_RANGE_QUERIES_PER_CALL", 128)        # the cap holds the RUNNING total over the slices
    with pytest.raises(ValueError, match="threshold is too low"):
        ops.community_detection(None, x, 32, TAU, MIN_SIZE, max_members=need - 1)


def test_pipelines_on_the_same_rows():
    x, planted, ref = _planted(384, "cosine")
    lims, members, centres, labels, scores = ref
    params = SimpleNamespace(device=torch.device(DEV))
    texts = [f"s{i}" for i in range(x.shape[0])]
    model = SimpleNamespace(encode_text=lambda docs, output_np=False: x[[int(t[1:]) for t in docs]])
    groups = SentenceMiningPipeline(64, params, model, corpus=texts).communities(TAU, MIN_SIZE)
    assert [len(g) for g in groups] == np.diff(lims).tolist()
    assert [i for g in groups for i, _, _ in g] == members.tolist() and all(t == f"s{i}" for g in groups for i, t, _ in g)
    assert np.array_equal(np.array([s for g in groups for _, _, s in g], np.float32).view(np.uint32), scores.view(np.uint32))
    assert [g[0][0] for g in groups] == centres.tolist()     # nobody took a centre here: it leads its community
    dot = SentenceMiningPipeline(64, params, model, corpus=texts, score_function="dot").communities(TAU, MIN_SIZE)
    assert [i for g in dot for i, _, _ in g] == _planted(384, "dot")[2][1].tolist()
    pipe = ClusteringPipeline(None, params, None, method="community", threshold=TAU, min_community_size=MIN_SIZE)
    out = pipe(x)
    assert np.array_equal(pipe.labels_.cpu().numpy(), labels) and pipe.n_iter_ >= 1 and pipe.inertia_ is None
    assert torch.equal(pipe.cluster_centers_, x[torch.from_numpy(centres).to(DEV)])
    assert sorted(out) == list(range(len(centres))) and -1 not in out
    assert all(out[k] == sorted(members[lims[k]:lims[k + 1]].tolist()) for k in out)
    assert ClusteringPipeline(3, params, model, method="community", threshold=TAU)(texts)[0][0].startswith("s")
    with pytest.raises(ValueError):
        ClusteringPipeline(3, params, None, method="community")         # no threshold
    with pytest.raises(ValueError):
        ClusteringPipeline(3, params, None, method="dbscan")


@pytest.mark.parametrize("case", ["separated", "overlap", "norms"])
def test_kmeans_is_untouched(case):
    """method='k-means' on tests/golden/kmeans.npz: the bounds of tests/test_adjacent_gpu.py, and no noise label."""
    g = golden("kmeans.npz")
    x, init = g[f"{case}_x"], g[f"{case}_init"]
    pipe = ClusteringPipeline(init.shape[0], SimpleNamespace(device=DEV), None, method="k-means", init=init)
    out = pipe(torch.from_numpy(x).to(DEV))
    assert (pipe.labels_.cpu().numpy() == g[f"{case}_labels"]).mean() >= 0.999
    np.testing.assert_allclose(pipe.cluster_centers_.cpu().numpy(), g[f"{case}_centers"], rtol=0, atol=5e-3)
    assert abs(pipe.inertia_ - float(g[f"{case}_inertia"])) <= 1e-4 * float(g[f"{case}_inertia"])
    assert sum(len(v) for v in out.values()) == x.shape[0] and min(out) >= 0
