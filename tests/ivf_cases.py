"""Test-local oracle of the inverted-list scan (include/tsim.h tsim_ivf_scan_topk) and of GpuIVFIndex, shared by
tests/test_ivf_cpu.py, tests/test_ivf_gpu.py and tests/test_ivf_index_gpu.py.  numpy only.  The scores and the ranking are those
of tests/list_cases.py (imported, not restated): an IVF search IS a list search over the union of the probed lists' rows."""
import numpy as np

from list_cases import list_topk_ref, rank_list

ST_LIST, ST_OFF = 1, 2      # include/tsim.h TSIM_IVF_ST_LIST / TSIM_IVF_ST_OFF
SL_NB = 1024                # csrc/search.hip: one block of the running list


def list_lengths(seg):
    """The list lengths of the length test: around a wave, a block of the running list and one and two segments."""
    return [0, 1, 63, 64, 65, SL_NB - 1, SL_NB, SL_NB + 1, seg - 1, seg, seg + 1, 2 * seg + 1]


def pack_ref(list_numbers, nlist):
    """(order, list_off, row_ids) of text_similarity_amd.ivf_index.pack_lists, restated: the stable sort of the list numbers, the
    exclusive cumulative counts, the arrival row of each position."""
    ln = np.asarray(list_numbers, dtype=np.int64)
    order = np.argsort(ln, kind="stable")
    off = np.zeros((nlist + 1,), dtype=np.int64)
    off[1:] = np.cumsum(np.bincount(ln, minlength=nlist))
    return order, off, order.astype(np.int32)


def clean_offsets(list_off, N):
    """What the kernel reads list_off as: the running maximum, clamped to [0, N]."""
    return np.clip(np.maximum.accumulate(np.asarray(list_off, dtype=np.int64)), 0, N)


def arrival_from_packed(packed_rows, list_off, row_ids):
    """The arrival-order view of a packed layout, for ivf_ref: (rows [M, d], list_numbers [M]) with rows[row_ids[p]] =
    packed_rows[p]; M = max id + 1, an id nobody holds (and a position with a negative id, or outside every list) is in list -1.
    list_off must be clean."""
    row_ids = np.asarray(row_ids, dtype=np.int64)
    M = int(row_ids.max()) + 1 if row_ids.size and row_ids.max() >= 0 else 1
    rows = np.zeros((M, packed_rows.shape[1]), dtype=np.float32)
    ln = np.full((M,), -1, dtype=np.int64)
    for l in range(len(list_off) - 1):
        for p in range(int(list_off[l]), int(list_off[l + 1])):
            if row_ids[p] >= 0:
                rows[row_ids[p]] = packed_rows[p]
                ln[row_ids[p]] = l
    return rows, ln


def probed_rows(list_numbers, probes_row, nlist):
    """(arrival row numbers of the union of the probed lists, status): repeats kept for a list probed twice, negative probes and
    probes >= nlist dropped, the latter setting ST_LIST."""
    st, parts = 0, []
    for l in np.asarray(probes_row, dtype=np.int64).reshape(-1):
        if l >= nlist:
            st |= ST_LIST
        elif l >= 0:
            parts.append(np.flatnonzero(list_numbers == l))
    return (np.concatenate(parts) if parts else np.zeros((0,), np.int64)), st


def ivf_ref(space, q, rows, list_numbers, probes, k, idx_offset=0, nlist=None, scores=None):
    """(scores [Q, k], ids [Q, k], status [Q]): query j against the rows (arrival order; the id is the arrival row number) of the
    lists probes[j].  ``scores``: a precomputed [Q, N] matrix of list_cases.pair_scores to rank from instead of scoring again."""
    list_numbers = np.asarray(list_numbers, dtype=np.int64)
    probes = np.asarray(probes, dtype=np.int64).reshape(q.shape[0], -1)
    nlist = int(list_numbers.max()) + 1 if nlist is None else nlist
    unions, st = [], np.zeros((q.shape[0],), dtype=np.int32)
    for j in range(q.shape[0]):
        u, st[j] = probed_rows(list_numbers, probes[j], nlist)
        unions.append(u)
    if scores is None:
        S, I, _ = list_topk_ref(space, q, rows, unions, k, idx_offset=idx_offset, unique=False)
        return S, I, st
    S = np.empty((q.shape[0], k), dtype=np.float32)
    I = np.empty((q.shape[0], k), dtype=np.int64)
    for j, u in enumerate(unions):
        sc = scores[j, u]
        ok = ~np.isnan(sc)
        S[j], I[j] = rank_list(space, u[ok], sc[ok], k, idx_offset)
    return S, I, st
