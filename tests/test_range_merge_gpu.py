"""ops.range_merge (include/tsim.h tsim_range_merge): per-shard range results with global indices, merged on the device, are bit
for bit the range search over the whole corpus — lims, scores and indices.  One process, one GPU.
N = 12 000, d = 128, Q = 33, shards of 5 000 / 6 999 / 1 rows (and a fourth list of empty segments only), every shard searched with
its own idx_offset and its own rho_c.  The data holds duplicate rows in different shards (equal scores ordered by index ACROSS
lists), a query with hits in one shard only, a query with none anywhere, and a query with tau = -inf whose segments are whole
shards (5 000 + 6 999 + 1 entries: no LDS block holds them)."""
import types

import numpy as np
import pytest
import torch

from text_similarity_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, D, Q = 12_000, 128, 33
BOUNDS = (0, 5000, 11_999, 12_000)
TAU = 0.22           # cosines of Gaussian rows at d = 128 are ~ N(0, 1/128): 0.22 is 2.5 sigma, about 75 of 12 000 rows


def _data():
    rng = np.random.default_rng(77)
    c = rng.standard_normal((N, D)).astype(np.float32)
    q = rng.standard_normal((Q, D)).astype(np.float32)
    c[6000] = c[10]                    # duplicates of row 10 in the second shard ...
    c[11_999] = c[10] * 2.0            # ... and, scaled (cosine cannot tell), as the single row of the third
    c[4000] = c[10]                    # and one in its own shard
    q[0] = c[10]                       # query 0 finds them: equal scores across the lists, ordered by index
    only = rng.standard_normal(D).astype(np.float32)
    c[7000:7030] = only + 0.05 * rng.standard_normal((30, D)).astype(np.float32)
    q[1] = only                        # (with its threshold below) hits in the second shard only
    return q, c


def _tau_vector():
    tau = np.full(Q, TAU, np.float32)
    tau[1] = 0.9                       # the planted cluster only: one shard
    tau[2] = 2.0                       # above every cosine: no hit anywhere
    tau[3] = -np.inf                   # whole shards
    tau[5] = np.nan                    # no hit, by definition
    tau[6:20] = np.linspace(0.15, 0.35, 14, dtype=np.float32)
    return tau


@pytest.fixture(scope="module")
def setup():
    q, c = _data()
    qf = torch.from_numpy(q).to(DEV)
    cf = torch.from_numpy(c).to(DEV)
    qn = ops.l2norm_rows(qf)

    def search(lo, hi, threshold):
        part = cf[lo:hi].contiguous()
        cn, rho = ops.l2norm_rows(part, return_rho=True)
        return ops.cosine_range(qn, cn, D, threshold, eq_f32=qf, ec_f32=part, rho_c=rho, idx_offset=lo)

    return types.SimpleNamespace(qf=qf, cf=cf, qn=qn, search=search)


def _same(got, want):
    for g, w, name in zip(got, want, ("lims", "scores", "idx")):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, w.view(torch.int32) if w.dtype == torch.float32 else w), name


@pytest.mark.parametrize("per_query", [False, True])
@pytest.mark.parametrize("lists", [3, 4])
def test_merged_shards_equal_the_whole_corpus(setup, per_query, lists):
    thr = torch.from_numpy(_tau_vector()).to(DEV) if per_query else TAU
    whole = setup.search(0, N, thr)
    parts = [setup.search(lo, hi, thr) for lo, hi in zip(BOUNDS[:-1], BOUNDS[1:])]
    if lists == 4:                     # a list that contributes empty segments only
        parts.insert(2, (torch.zeros((Q + 1,), dtype=torch.int64, device=DEV), torch.empty((0,), dtype=torch.float32, device=DEV),
                         torch.empty((0,), dtype=torch.int64, device=DEV)))
    got = ops.range_merge(parts)
    torch.cuda.synchronize()
    _same(got, whole)
    _same(ops.range_merge(parts, total=int(whole[0][-1])), whole)          # the total known on the host: no read-back
    # what the data was built to hold
    lims, s, i = (t.cpu().numpy() for t in whole)
    sizes = [np.diff(p[0].cpu().numpy()) for p in parts if p[1].numel()]
    assert i[:4].tolist() == [10, 4000, 6000, 11_999] and len(set(s[:4].view(np.uint32).tolist())) == 1   # ties across lists, by index
    assert all(z[0] >= 1 for z in sizes)
    if per_query:
        assert sizes[0][1] == 0 and sizes[1][1] >= 30 and sizes[2][1] == 0     # one shard only
        assert lims[3] == lims[2]                                              # none anywhere
        assert lims[4] - lims[3] == N and [int(z[3]) for z in sizes] == [5000, 6999, 1]   # whole shards
        np.testing.assert_array_equal(np.sort(i[lims[3]:lims[4]]), np.arange(N))
        assert lims[6] == lims[5]                                              # NaN
    assert lims[-1] > 20 * Q


def test_one_list_is_a_copy_and_empty_input(setup):
    part = setup.search(0, 5000, torch.from_numpy(_tau_vector()).to(DEV))
    got = ops.range_merge([part])
    _same(got, part)
    assert got[1].data_ptr() != part[1].data_ptr()
    # a payload longer than lims[-1] (padded for an exchange): the excess is ignored
    padded = (part[0], torch.cat([part[1], torch.full((7,), 9.0, device=DEV)]), torch.cat([part[2], torch.full((7,), -5, device=DEV)]))
    _same(ops.range_merge([padded]), part)
    # nothing anywhere, and Q = 0: empty results, no launch
    e = (torch.zeros((Q + 1,), dtype=torch.int64, device=DEV), torch.empty((0,), dtype=torch.float32, device=DEV),
         torch.empty((0,), dtype=torch.int64, device=DEV))
    lims, s, i = ops.range_merge([e, e])
    assert lims.tolist() == [0] * (Q + 1) and s.numel() == 0 and i.numel() == 0
    z = (torch.zeros((1,), dtype=torch.int64, device=DEV), e[1], e[2])
    lims, s, i = ops.range_merge([z, z, z])
    assert lims.tolist() == [0] and s.numel() == 0 and i.dtype == torch.int64
    with pytest.raises(ValueError):
        ops.range_merge([])
    with pytest.raises(ValueError):
        ops.range_merge([e] * 65)
    with pytest.raises(ValueError):
        ops.range_merge([e, z])


def test_equal_entries_give_a_permutation():
    """(score, index) equal in two lists — disjoint shards do not produce it — is ordered by list number: every input entry
    appears exactly once."""
    lims = torch.tensor([0, 3, 3, 5], dtype=torch.int64, device=DEV)
    s = torch.tensor([0.9, 0.5, 0.5, 0.7, 0.1], device=DEV)
    i = torch.tensor([4, 2, 8, 1, 1], dtype=torch.int64, device=DEV)
    ml, ms, mi = ops.range_merge([(lims, s, i)] * 3)
    assert ml.tolist() == [0, 9, 9, 15]
    assert ms.tolist() == pytest.approx([0.9] * 3 + [0.5] * 6 + [0.7] * 3 + [0.1] * 3)
    assert mi.tolist() == [4] * 3 + [2] * 3 + [8] * 3 + [1] * 6


@pytest.mark.parametrize("score_function", ["cosine", "dot"])
def test_range_tensors_chunked_with_a_threshold_array(setup, score_function):
    from text_similarity_amd.pipeline.search_pipeline import SentenceMiningPipeline
    params = types.SimpleNamespace(device=torch.device(DEV))
    tau = _tau_vector()
    if score_function == "dot":        # inner products of these rows are ~ |q||c| = 128 times the cosine
        tau = np.where(np.isfinite(tau), tau * 128.0, tau).astype(np.float32)
    thr = torch.from_numpy(tau).to(DEV)
    one = SentenceMiningPipeline(N, params, None, corpus=setup.cf, score_function=score_function).range_tensors(setup.qf, thr)
    assert one[0][-1] > N
    for chunk in (5000, 1100):         # 3 chunks; 11 chunks, the last of 1 000 rows
        got = SentenceMiningPipeline(chunk, params, None, corpus=setup.cf, score_function=score_function).range_tensors(setup.qf, thr)
        _same(got, one)
