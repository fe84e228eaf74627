"""Filtered search on GpuFlatIndex (``filter=`` of search / knn_query) and the pipeline keywords built on it: both regimes of a
shared allow-list ("list": the list kernel; "compact": gather + the ordinary MFMA search) return identical tensors, and both
equal the numpy oracle of tests/list_cases.py on the live allowed rows — scores bit for bit, ties by row of the index.

N = 20 000 rows of width 64; labels are 1000 + 3 * position (never a row number); every 7th of the first 700 rows is deleted
before the first query, so rows move when the index compacts.  The allow-lists of 3, 500 and 10 000 labels are prefixes of one
permutation: each query is scored once per space against the 10 000 and every case ranks a subset of that."""
import functools
import types

import numpy as np
import pytest
import torch

from list_cases import pair_scores, rank_list, same_bits
from text_similarity_amd import ops
from text_similarity_amd.index import GpuFlatIndex

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, D, QMAX = 20000, 64, 130
SPACES = {"cosine": "cosine", "ip": "dot", "euclidean": "l2"}
DEAD = np.arange(0, 700, 7)


def _label(pos):
    return 1000 + 3 * np.asarray(pos, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _data():
    rng = np.random.default_rng(77)
    c = rng.standard_normal((N, D)).astype(np.float32)
    q = rng.standard_normal((QMAX, D)).astype(np.float32)
    # positions (before deletion), some of them deleted rows.  The 3-label list: two live rows and one DELETED row (14);
    # entries 9 .. 14: six live rows made equal — ties inside the 500, across both regimes
    fixed = [15000, 9, 14, 300, 301, 303, 304, 305, 306, 12001, 705, 8000, 8003, 19999, 5000]
    allowed = np.concatenate([fixed, np.setdiff1d(rng.permutation(N), fixed, assume_unique=True)[:10000 - len(fixed)]])
    allowed[15:] = rng.permutation(allowed[15:])
    assert len(set(allowed.tolist())) == 10000 and not np.isin(allowed[9:15], DEAD).any() and np.isin(allowed, DEAD).any()
    c[allowed[10:15]] = c[allowed[9]]
    q[1] = c[allowed[9]]
    return q, c, allowed


@functools.lru_cache(maxsize=None)
def _index(space):
    q, c, _ = _data()
    ix = GpuFlatIndex(space=space, dim=D, device=DEV)
    ix.add_items(c, _label(np.arange(N)))
    for p in DEAD:
        ix.mark_deleted(int(_label(p)))
    return ix


@functools.lru_cache(maxsize=None)
def _scores(space):
    """[QMAX, 10 000] float32: every query against every allowed position (deleted ones included; they are dropped per case)."""
    q, c, allowed = _data()
    return np.stack([pair_scores(SPACES[space], q, c, np.full(allowed.shape, j), allowed) for j in range(QMAX)])


def _oracle(space, Q, sel, k):
    """labels / scores of the live rows among allowed[sel] (sel: indices into the 10 000) for queries 0 .. Q-1.  Ties go to the
    lower ROW of the index: deletion keeps the order of the live rows, so positions rank as rows do."""
    _, _, allowed = _data()
    sel = np.asarray(sel, dtype=np.int64)
    sel = sel[~np.isin(allowed[sel], DEAD)]
    sc = _scores(space)
    S = np.empty((Q, k), dtype=np.float32)
    L = np.empty((Q, k), dtype=np.int64)
    for j in range(Q):
        s, pos = rank_list(SPACES[space], allowed[sel], sc[j, sel], k)
        S[j], L[j] = s, np.where(pos >= 0, _label(pos), -1)
    return L, S


def _check(got, want, what):
    lab, s = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert (lab == want[0]).all(), (what, np.argwhere(lab != want[0])[:5])
    assert same_bits(s, want[1]), what


@pytest.mark.parametrize("Q", [2, 130])
@pytest.mark.parametrize("n_allowed", [3, 500, 10000])
@pytest.mark.parametrize("space", list(SPACES))
def test_both_regimes_equal_each_other_and_the_oracle(space, n_allowed, Q):
    q, c, allowed = _data()
    ix = _index(space)
    k = 10
    labels = np.concatenate([_label(allowed[:n_allowed]), [7, 1001, 10 ** 12]])       # + labels the index never held
    want = _oracle(space, Q, np.arange(n_allowed), k)
    if n_allowed == 3:
        assert (want[0][:, 2:] == -1).all() and (want[0][:, :2] >= 0).all()           # two live matches: padding behind them
        assert not np.isin(want[0], _label(14)).any()                                 # the deleted label never comes back
    qd = torch.from_numpy(q[:Q]).to(DEV)
    a = ix.search(qd, k, filter=labels, filter_plan="list")
    b = ix.search(qd, k, filter=torch.from_numpy(labels).to(DEV), filter_plan="compact")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    _check(a, want, "list")
    _check(b, want, "compact")
    _check(ix.search(qd, k, filter=labels.tolist()), want, "planned")
    if Q == 2 and n_allowed == 500:
        assert (want[0][1, :6] == np.sort(_label(allowed[9:15]))).all()               # query 1: its six copies, by row
        lab, dist = ix.knn_query(q[:Q], k=k, filter=labels)
        assert (lab == want[0]).all()
        ref = want[1] if space == "euclidean" else (1.0 - torch.from_numpy(want[1])).numpy()
        assert same_bits(dist, ref)


@pytest.mark.parametrize("space", list(SPACES))
def test_callable_and_per_query_filters(space):
    q, c, allowed = _data()
    ix = _index(space)
    Q, k = 5, 10
    qd = torch.from_numpy(q[:Q]).to(DEV)
    # hnswlib's form: label -> bool, over the live labels
    sel = np.nonzero(_label(allowed) % 5 == 0)[0]
    allowed_labels = set(_label(allowed).tolist())
    want = _oracle(space, Q, sel, k)
    for plan in ("list", "compact", None):
        _check(ix.search(qd, k, filter=lambda l: l % 5 == 0 and l in allowed_labels, filter_plan=plan), want, ("callable", plan))
    # one allow-list per query: a list of Q arrays, and the (lims, labels) pair; unknown and deleted labels inside, one list
    # empty, one with a repeat
    sels = [np.arange(0, 40), np.arange(3), np.zeros((0,), np.int64), np.arange(100, 1300), np.array([9, 10, 9, 11])]
    lists = [np.concatenate([_label(allowed[s]), [5, 10 ** 12]]) if len(s) else _label(allowed[s]) for s in sels]
    wl = np.empty((Q, k), dtype=np.int64)
    ws = np.empty((Q, k), dtype=np.float32)
    for j, s in enumerate(sels):
        one = _oracle(space, Q, np.unique(s), k)
        wl[j], ws[j] = one[0][j], one[1][j]
    _check(ix.search(qd, k, filter=lists), (wl, ws), "list of arrays")
    lims = np.concatenate([[0], np.cumsum([len(x) for x in lists])])
    _check(ix.search(qd, k, filter=(lims, np.concatenate(lists))), (wl, ws), "(lims, labels)")
    _check(ix.search(qd, k, filter=(torch.from_numpy(lims).to(DEV), torch.from_numpy(np.concatenate(lists)).to(DEV))), (wl, ws),
           "(lims, labels) on the device")
    assert (wl[2] == -1).all()
    # a filter that matches nothing: all padding, as hnswlib returns nothing
    lab, s = ix.search(qd, k, filter=np.array([5, 8]))
    assert (lab == -1).all() and (torch.isposinf(s) if space == "euclidean" else torch.isneginf(s)).all()


@pytest.mark.parametrize("space", list(SPACES))
def test_no_filter_is_the_unfiltered_call(space):
    q, _, _ = _data()
    ix = _index(space)
    qd = torch.from_numpy(q[:7]).to(DEV)
    a = ix.search(qd, 12)
    b = ix.search(qd, 12, filter=None)
    c = ix.search(qd, 12, None, None)
    for x in (b, c):
        assert torch.equal(a[0], x[0]) and torch.equal(a[1].view(torch.int32), x[1].view(torch.int32))
    la, da = ix.knn_query(q[:7], 12)
    lb, db = ix.knn_query(q[:7], k=12, filter=None)
    assert (la == lb).all() and same_bits(da, db)
    # a filter that allows every live label answers like the unfiltered call, in both regimes
    live = np.setdiff1d(np.arange(N), DEAD)
    for plan in ("list", "compact"):
        x = ix.search(qd, 12, filter=_label(live), filter_plan=plan)
        assert torch.equal(a[0], x[0]) and torch.equal(a[1].view(torch.int32), x[1].view(torch.int32)), plan


@pytest.mark.parametrize("score_function", ["cosine", "dot"])
def test_pipeline_keywords(score_function, tmp_path):
    from text_similarity_amd.pipeline.search_pipeline import SemanticSearchPipeline, SentenceMiningPipeline
    q, c, allowed = _data()
    n, Q, k = 3000, 4, 10
    ct, qt = torch.from_numpy(c[:n]).to(DEV), torch.from_numpy(q[:Q]).to(DEV)
    params = types.SimpleNamespace(device=torch.device(DEV), model_parameters=types.SimpleNamespace(hidden_size=D))
    fn = ops.dot_list_topk if score_function == "dot" else ops.cosine_list_topk
    rng = np.random.default_rng(9)
    # SentenceMiningPipeline(candidates=...): the three forms, against the ops call underneath
    pipe = SentenceMiningPipeline(700, params, None, corpus=ct, score_function=score_function)      # (chunking does not apply)
    two_d = torch.from_numpy(np.stack([rng.permutation(n)[:200] for _ in range(Q)])).to(DEV)
    two_d[1, 50:] = -1
    want = fn(qt, ct, two_d, k=k)
    for cand in (two_d, [row[row >= 0].tolist() for row in two_d.cpu()]):
        s, i = pipe.search_tensors(qt, max_num_results=k, candidates=cand)
        assert torch.equal(i, want[1]) and torch.equal(s.view(torch.int32), want[0].view(torch.int32))
    shared = rng.permutation(n)[:300]
    want = fn(qt, ct, torch.from_numpy(shared).to(DEV), k=k)
    for cand in (shared.tolist(), torch.from_numpy(shared)):
        s, i = pipe.search_tensors(qt, max_num_results=k, candidates=cand)
        assert torch.equal(i, want[1]) and torch.equal(s.view(torch.int32), want[0].view(torch.int32))
    res = pipe(qt, k, candidates=shared.tolist())
    assert [[p for p, _ in res[j]] for j in range(Q)] == want[1].cpu().tolist()
    assert torch.equal(pipe.last_indices, want[1])
    plain = pipe(qt, k)                                                        # candidates=None: the ordinary search
    assert torch.equal(pipe.last_indices, pipe.search_tensors(qt, max_num_results=k)[1]) and len(plain) == Q
    # SemanticSearchPipeline(filter=...): passed through to the index (its labels are corpus positions)
    sem = SemanticSearchPipeline(str(tmp_path / "ix"), params, None, corpus=ct, score_function=score_function)
    out = sem(qt, k, filter=shared)
    lab, sc = sem.index.search(qt, k, filter=shared)
    assert torch.equal(sem.last_labels, lab) and torch.equal(sem.last_scores.view(torch.int32), sc.view(torch.int32))
    assert torch.equal(lab, want[1]) and torch.equal(sc.view(torch.int32), want[0].view(torch.int32))
    assert all(torch.equal(torch.stack(out[j]), ct[lab[j]]) for j in range(Q))
    out = sem(qt, k)
    assert torch.equal(sem.last_labels, sem.index.search(qt, k)[0])
