"""The numpy restatement of the IVF-PQ ops (include/tsim.h tsim_ivfpq_*, text_similarity_amd/csrc/ivfpq_search.h) and the cases the
IVF-PQ tests share.  Written from the definitions on top of tests/pq_cases.py: float64 and int64, every float64 operation rounded
on its own, loops over dsub, M and (for the centroid products) d only."""
import numpy as np

import pq_cases as pc

INT32_MIN, INT32_MAX = pc.INT32_MIN, pc.INT32_MAX
ST_LIST, ST_OFF = 1, 2


# ------------------------------------------------------------------------------------------------- definitions
def residuals(x, centroids, lists):
    """float32 [n, d]: r_i = float32(x_i - c_l,i), one rounded float32 subtraction"""
    with np.errstate(all="ignore"):
        return np.asarray(x, np.float32) - np.asarray(centroids, np.float32)[np.asarray(lists)]


def encode_ref(x, centroids, lists, codebooks, by_residual=True):
    """uint8 [n, code_bytes(M)]: pq_encode of the residual to the row's list centroid, or of the row itself"""
    return pc.encode_ref(residuals(x, centroids, lists) if by_residual else x, codebooks)


def valid_probes(probes, nlist):
    return (probes >= 0) & (probes < nlist)


def row_dot(q, c):
    """float64 [Q, P]: the ordered sum over i = 0 .. d - 1 of (double)q[a, i] (double)c[a, b, i] for c [Q, P, d]"""
    q, c = np.asarray(q, np.float32).astype(np.float64), np.asarray(c, np.float32).astype(np.float64)
    acc = np.zeros(c.shape[:2], np.float64)
    with np.errstate(all="ignore"):
        for i in range(q.shape[1]):
            p = q[:, i, None] * c[:, :, i]
            acc = acc + p
    return acc


def _exponent(A, clog):
    """(usable, e): A zero, NaN or infinite is not usable"""
    if A == 0 or not np.isfinite(A):
        return False, 0
    return True, 23 - clog - int(np.frexp(A)[1])                  # A < 2^x, x = ilogb(A) + 1


def tables_ip_ref(q, centroids, probes, codebooks):
    """(tables int32 [Q, M, 256], bias int32 [Q, nprobe], exps int32 [Q]); the bias of a padding probe is 0"""
    q = np.asarray(q, np.float32)
    M, _, dsub = codebooks.shape
    Q, nprobe, nlist = q.shape[0], probes.shape[1], centroids.shape[0]
    ok = valid_probes(probes, nlist)
    L = np.zeros((Q, M, 256), np.float64)
    for m in range(M):
        L[:, m] = pc.dot(q[:, m * dsub:(m + 1) * dsub], codebooks[m])
    B = row_dot(q, centroids[np.where(ok, probes, 0)])
    tables, bias, exps = np.zeros((Q, M, 256), np.int32), np.zeros((Q, nprobe), np.int32), np.zeros((Q,), np.int32)
    for i in range(Q):
        with np.errstate(all="ignore"):
            A = np.max(np.concatenate([np.abs(L[i]).ravel(), np.abs(B[i][ok[i]])]))       # NaN propagates
        usable, e = _exponent(A, pc.ceil_log2(M + 1))
        if not usable:
            continue
        tables[i] = np.rint(L[i] * np.ldexp(1.0, e)).astype(np.int32)
        bias[i] = np.where(ok[i], np.rint(B[i] * np.ldexp(1.0, e)), 0).astype(np.int32)
        exps[i] = e
    return tables, bias, exps


def tables_l2_ref(q, centroids, probes, codebooks):
    """(tables int32 [Q, nprobe, M, 256], exps int32 [Q]): one table per pair on the query's common exponent; the tables of
    padding probes are zero here and unspecified in the library"""
    q = np.asarray(q, np.float32)
    M, _, dsub = codebooks.shape
    Q, nprobe, nlist = q.shape[0], probes.shape[1], centroids.shape[0]
    ok = valid_probes(probes, nlist)
    rq = residuals(q[:, None, :], centroids, np.where(ok, probes, 0))               # [Q, nprobe, d]
    L = np.zeros((Q, nprobe, M, 256), np.float64)
    for m in range(M):
        L[:, :, m] = -pc.sqdist(rq[:, :, m * dsub:(m + 1) * dsub].reshape(Q * nprobe, dsub), codebooks[m]).reshape(Q, nprobe, 256)
    tables, exps = np.zeros((Q, nprobe, M, 256), np.int32), np.zeros((Q,), np.int32)
    for i in range(Q):
        if not ok[i].any():
            continue
        with np.errstate(all="ignore"):
            A = np.max(np.abs(L[i][ok[i]]))
        usable, e = _exponent(A, pc.ceil_log2(M))
        if not usable:
            continue
        tables[i][ok[i]] = np.rint(L[i][ok[i]] * np.ldexp(1.0, e)).astype(np.int32)
        exps[i] = e
    return tables, exps


def tables_loop(q, centroids, probes, codebooks, space):
    """the same as literal loops (tiny inputs only): (tables, bias or None, exps)"""
    M, _, dsub = codebooks.shape
    Q, nprobe, nlist, d = len(q), probes.shape[1], len(centroids), M * dsub
    f64 = np.float64
    tables = np.zeros((Q, M, 256) if space == "ip" else (Q, nprobe, M, 256), np.int32)
    bias, exps = np.zeros((Q, nprobe), np.int32), np.zeros((Q,), np.int32)
    for a in range(Q):
        pairs = [j for j in range(nprobe) if 0 <= probes[a, j] < nlist]
        entries = {}
        with np.errstate(all="ignore"):
            if space == "ip":
                for m in range(M):
                    for j in range(256):
                        acc = f64(0)
                        for i in range(dsub):
                            p = f64(q[a][m * dsub + i]) * f64(codebooks[m][j][i])
                            acc = acc + p
                        entries["T", m, j] = acc
                for b in pairs:
                    acc = f64(0)
                    for i in range(d):
                        p = f64(q[a][i]) * f64(centroids[probes[a, b]][i])
                        acc = acc + p
                    entries["B", b] = acc
            else:
                for b in pairs:
                    rq = [np.float32(q[a][i]) - np.float32(centroids[probes[a, b]][i]) for i in range(d)]
                    for m in range(M):
                        for j in range(256):
                            dist = f64(0)
                            for i in range(dsub):
                                t = f64(rq[m * dsub + i]) - f64(codebooks[m][j][i])
                                p = t * t
                                dist = dist + p
                            entries["T", b, m, j] = -dist
        vals = list(entries.values())
        if not vals or any(not np.isfinite(v) for v in vals):
            continue
        A = max(abs(v) for v in vals)
        usable, e = _exponent(A, pc.ceil_log2(M + 1 if space == "ip" else M))
        if not usable:
            continue
        exps[a] = e
        for key, v in entries.items():
            r = np.int32(np.rint(v * np.ldexp(1.0, e)))
            if key[0] == "B":
                bias[a, key[1]] = r
            else:
                tables[(a,) + key[1:]] = r
    return tables, (bias if space == "ip" else None), exps


def score_bound(tables, bias=None):
    """per query: max |bias| + sum_m max_j |T[m][j]| (per-pair tables: the largest over the pairs)"""
    t = np.abs(tables.astype(np.int64)).max(axis=-1).sum(axis=-1)
    if t.ndim == 2:
        t = t.max(axis=1)
    return t if bias is None else t + np.abs(bias.astype(np.int64)).max(axis=1)


def clean_offsets(list_off, N):
    """every word the running maximum of the words up to it, clamped to [0, N]"""
    return np.clip(np.maximum.accumulate(np.asarray(list_off, np.int64)), 0, N)


def scan_ref(tables, bias, codes, list_off, row_ids, probes, k, space, idx_offset=0):
    """(value int32 [Q, k], idx int64 [Q, k], status int32 [Q]).  tables [Q, M, 256] (one a query) or [Q, nprobe, M, 256] (one a
    pair); score = bias[q][j] + sum_m T[m][code[m]] over the rows of the probed lists with row_ids >= 0; ip by (score desc, id
    asc), l2 by (-score asc, id asc) with value = -score; padding as pq_cases.adc_topk_ref"""
    Q, nprobe = probes.shape
    N, nlist = codes.shape[0], len(list_off) - 1
    M = tables.shape[-2]
    off = clean_offsets(list_off, N)
    ov = np.full((Q, k), INT32_MIN if space == "ip" else INT32_MAX, np.int32)
    oi = np.full((Q, k), -1, np.int64)
    status = np.zeros((Q,), np.int32)
    sub = np.arange(M)
    for q in range(Q):
        ss, ii = [np.zeros((0,), np.int64)], [np.zeros((0,), np.int64)]
        for j in range(nprobe):
            l = int(probes[q, j])
            if l < 0:
                continue
            if l >= nlist:
                status[q] |= ST_LIST
                continue
            if off[l] != list_off[l] or off[l + 1] != list_off[l + 1]:
                status[q] |= ST_OFF
            lo, hi = int(off[l]), int(off[l + 1])
            T = (tables[q, j] if tables.ndim == 4 else tables[q]).astype(np.int64)
            s = T[sub[None, :], codes[lo:hi, :M]].sum(axis=1) + (0 if bias is None else int(bias[q, j]))
            ids = row_ids[lo:hi].astype(np.int64)
            ss.append(s[ids >= 0]), ii.append(ids[ids >= 0])
        s, ids = np.concatenate(ss), np.concatenate(ii)
        order = np.lexsort((ids, -s))[:k]
        ov[q, :order.size] = s[order] if space == "ip" else -s[order]
        oi[q, :order.size] = ids[order] + idx_offset
    return ov, oi, status


def pack(lists, nlist):
    """(order int64 [n], list_off int64 [nlist + 1], row_ids int32 [n]): the stable sort of the list numbers"""
    lists = np.asarray(lists, np.int64)
    order = np.argsort(lists, kind="stable")
    list_off = np.zeros((nlist + 1,), np.int64)
    list_off[1:] = np.cumsum(np.bincount(lists, minlength=nlist))
    return order, list_off, order.astype(np.int32)


def search_ref(q, centroids, codebooks, codes, lists, probes, k, space, by_residual=True, row_ids=None):
    """(scores float32 [Q, k], ids int64 [Q, k]) of ops.ivfpq_search: ``codes`` [n, >= M] in ARRIVAL order with list numbers
    ``lists``; ids are arrival rows, or ``row_ids[arrival row]`` (negative: a tombstone)"""
    nlist = centroids.shape[0]
    order, list_off, ids = pack(lists, nlist)
    if row_ids is not None:
        ids = np.asarray(row_ids, np.int32)[order]
    if not by_residual:
        tables, exps = pc.tables_ref(q, codebooks, space)
        bias = None
    elif space == "ip":
        tables, bias, exps = tables_ip_ref(q, centroids, probes, codebooks)
    else:
        (tables, exps), bias = tables_l2_ref(q, centroids, probes, codebooks), None
    v, i, _ = scan_ref(tables, bias, codes[order], list_off, ids, probes, k, space)
    return pc.values_to_float(v, exps, space), i


# ------------------------------------------------------------------------------------------------- cases
def seg_lengths(seg):
    """list lengths around the step (256) and the segment: 0, 1, 255, 256, 257, seg - 1, seg, seg + 1, 2 seg + 1"""
    return [0, 1, 255, 256, 257, seg - 1, seg, seg + 1, 2 * seg + 1]


def lists_of_lengths(rng, lengths):
    """(list_off int64 [nlist + 1], which: the list number holding each length) with the lengths in a shuffled list order"""
    which = rng.permutation(len(lengths))
    lens = np.zeros(len(lengths), np.int64)
    lens[which] = lengths
    list_off = np.zeros(len(lengths) + 1, np.int64)
    list_off[1:] = np.cumsum(lens)
    return list_off, which


def ids_with_tombstones(rng, N, every=7):
    """int32 [N]: a permutation of 0 .. N - 1 with every ``every``-th position a tombstone (-1 - id)"""
    ids = rng.permutation(N).astype(np.int32)
    ids[::every] = -1 - ids[::every]
    return ids


def header_seg():
    """TSIM_IVFPQ_SEG as include/tsim.h defines it: the tests' list lengths follow the header"""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tsim.h")).read()
    return int(re.search(r"#define TSIM_IVFPQ_SEG (\d+)", hdr).group(1))
