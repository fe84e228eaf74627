"""Cases of tests/test_running_list_gpu.py, shared with tools/hash_running_list.py: every kernel that keeps a running sorted list
in LDS (bf_partial / bf_merge, topk_merge_large, list_partial / list_merge) on inputs from the deterministic generators of
text_similarity_amd.presets, the oracle of each case, and the sha256 of the raw output bytes.

One corpus of 3 200 x 384 float32 rows serves everything: the brute-force shards are its first 600 and 2 500 rows, the lists
draw from all of it."""
import functools
import hashlib

import numpy as np
import torch

from l2_cases import l2_topk_ref
from list_cases import csr, list_topk_ref
from oracle.search_ref import _lane_sum, cosine_topk_f32, merge_topk, topk_rows
from text_similarity_amd import ops, presets

DEV = "cuda:0"
D, NQ, NROWS = 384, 6, 3200
SPACES = ("cosine", "dot", "l2")
# ------------------------------------------------------------------------------------------------------------ brute force
BF_N = (600, 2500)      # 600: k > N pads; 2 500: several chunks and a last block of the list that is not full
BF_Q = 3
BF_K = (1, 40, 64, 65, 1000, 1024)
# ------------------------------------------------------------------------------------------------------------------ merge
MERGE_LISTS, MERGE_Q, MERGE_K_IN = 3, 5, 700
MERGE_K_OUT = (1024, 65)
# ------------------------------------------------------------------------------------------------------------------ lists
LIST_LENS = (0, 1, 1023, 1024, 1025, 2500)     # CSR: lists that begin, end and straddle a slice boundary (1 024 entries)
LIST_K = (10, 1024)
SHARED_LEN, SHARED_K = 3000, 100
LIST_FN = {"cosine": ops.cosine_list_topk, "dot": ops.dot_list_topk, "l2": ops.l2_list_topk}


@functools.lru_cache(maxsize=None)
def rows():
    c = presets.normal("running_list/corpus", NROWS * D).reshape(NROWS, D)
    q = presets.normal("running_list/queries", NQ * D).reshape(NQ, D)
    return q, c


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _host(out):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _permutation(stream, n):
    return np.argsort(presets.uniform01(stream, n), kind="stable").astype(np.int64)


# ------------------------------------------------------------------------------------------------------------ brute force
def bf_id(space, n, k):
    return f"bf-{space}-N{n}-k{k}"


def bf_run(space, n, k):
    """(scores [Q, k], idx [Q, k], status [Q]) of the full search over the first n rows."""
    q, c = rows()
    qf, cf = _dev(q[:BF_Q]), _dev(c[:n])
    if space == "cosine":
        cu, rho = ops.l2norm_rows(cf, return_rho=True)
        out = ops.cosine_topk(ops.l2norm_rows(qf), cu, D, k, eq_f32=qf, ec_f32=cf, rho_c=rho, return_status=True)
    elif space == "dot":
        cn, rho, scale = ops.dot_scaled_rows(cf)
        out = ops.dot_topk(ops.l2norm_rows(qf), cn, D, k, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale, return_status=True)
    else:
        cn, rho, scale = ops.l2_rows(cf)
        out = ops.l2_topk(ops.l2_query_rows(qf, scale), cn, D, k, eq_f32=qf, ec_f32=cf, rho_c=rho, scale_c=scale, return_status=True)
    return _host(out)


@functools.lru_cache(maxsize=None)
def bf_oracle(space, n):
    """The oracle's min(n, 1 024) best per query, ordered: the list of every k is its first k columns."""
    q, c = rows()
    q, c = q[:BF_Q], c[:n]
    if space == "cosine":
        return cosine_topk_f32(q, c, max(BF_K))
    if space == "l2":
        return l2_topk_ref(q, c, max(BF_K))
    return topk_rows(_lane_sum(q[:, None, :], c[None, :, :]).astype(np.float32), max(BF_K))


# ------------------------------------------------------------------------------------------------------------------ merge
def merge_id(k_out):
    return f"merge-k{k_out}"


@functools.lru_cache(maxsize=None)
def merge_inputs():
    """scores, idx [3, 5, 700]: coarse scores (many ties), 50 (score, index) pairs of list 0 planted in list 1, a few skipped
    entries in list 0, list 2 nothing but -1 padding; each list sorted by (score desc, index asc)."""
    n = MERGE_LISTS * MERGE_Q * MERGE_K_IN
    shape = (MERGE_LISTS, MERGE_Q, MERGE_K_IN)
    s = (np.round(presets.normal("running_list/merge_s", n) * 4.0) / 4.0).astype(np.float32).reshape(shape)
    s += np.float32(0.0)      # -0 -> +0: the two compare equal, so which one survives as the duplicate would be anyone's guess
    i = presets.randint("running_list/merge_i", n, 0, 2000).astype(np.int64).reshape(shape)
    s[1, :, :50], i[1, :, :50] = s[0, :, 100:150], i[0, :, 100:150]
    i[0, :, 7::97] = -1
    i[2] = -1
    for l in range(MERGE_LISTS):
        for q in range(MERGE_Q):
            o = np.lexsort((i[l, q], -s[l, q].astype(np.float64)))
            s[l, q], i[l, q] = s[l, q][o], i[l, q][o]
    return s, i


def merge_run(k_out):
    s, i = merge_inputs()
    return _host(ops.topk_merge(_dev(s), _dev(i), k_out))


def merge_oracle(k_out):
    """Entries with index < 0 dropped, equal (score, index) pairs once, then oracle.search_ref.merge_topk; (-inf, -1) padding."""
    s, i = merge_inputs()
    out_s = np.full((MERGE_Q, k_out), -np.inf, dtype=np.float32)
    out_i = np.full((MERGE_Q, k_out), -1, dtype=np.int64)
    for q in range(MERGE_Q):
        pairs = sorted({(float(a), int(b)) for a, b in zip(s[:, q].ravel(), i[:, q].ravel()) if b >= 0})
        v = np.array([p[0] for p in pairs], dtype=np.float32)[None]
        x = np.array([p[1] for p in pairs], dtype=np.int64)[None]
        ms, mi = merge_topk([v], [x], k_out)
        out_s[q, :ms.shape[1]], out_i[q, :mi.shape[1]] = ms[0], mi[0]
    return out_s, out_i


# ------------------------------------------------------------------------------------------------------------------ lists
def list_id(space, k, dtype):
    return f"list-{space}-k{k}-{np.dtype(dtype).name}"


def shared_id(space, dtype):
    return f"shared-{space}-{np.dtype(dtype).name}"


@functools.lru_cache(maxsize=None)
def csr_lists():
    """One list per query, each a prefix of the query's own permutation of the rows; the list of 1 025 holds one padding entry
    and one row beyond the corpus (TSIM_LIST_ST_ROW)."""
    lists = [_permutation(f"running_list/perm{j}", NROWS)[:n].copy() for j, n in enumerate(LIST_LENS)]
    lists[4][500] = -1
    lists[4][777] = NROWS + 5
    return lists


@functools.lru_cache(maxsize=None)
def shared_list():
    return _permutation("running_list/shared", NROWS)[:SHARED_LEN].copy()


def list_run(space, k, dtype):
    q, c = rows()
    cand, lims = csr(csr_lists())
    return _host(LIST_FN[space](_dev(q), _dev(c), _dev(cand.astype(dtype)), _dev(lims), k=k, return_status=True, assume_unique=True))


def shared_run(space, dtype):
    q, c = rows()
    return _host(LIST_FN[space](_dev(q), _dev(c), _dev(shared_list().astype(dtype)), k=SHARED_K, return_status=True,
                                assume_unique=True))


@functools.lru_cache(maxsize=None)
def list_oracle(space, k):
    q, c = rows()
    return list_topk_ref(space, q, c, csr_lists(), k, unique=False)


@functools.lru_cache(maxsize=None)
def shared_oracle(space):
    q, c = rows()
    return list_topk_ref(space, q, c, shared_list(), SHARED_K, unique=False)


def all_runs():
    """(case id, function returning the case's output arrays), every case of the test."""
    for space in SPACES:
        for n in BF_N:
            for k in BF_K:
                yield bf_id(space, n, k), functools.partial(bf_run, space, n, k)
    for k_out in MERGE_K_OUT:
        yield merge_id(k_out), functools.partial(merge_run, k_out)
    for space in SPACES:
        for dtype in (np.int32, np.int64):
            for k in LIST_K:
                yield list_id(space, k, dtype), functools.partial(list_run, space, k, dtype)
            yield shared_id(space, dtype), functools.partial(shared_run, space, dtype)

