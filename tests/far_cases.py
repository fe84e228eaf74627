"""Rows placed FAR APART, and a CPU model of wrong addressing; shared by tests/test_far_cases_cpu.py, tests/test_far_rows_gpu.py
and tests/test_large_corpus_gpu.py.

Every kernel that touches rows computes ``row * ld`` by hand.  A few thousand rows placed a megabyte apart run through the same
address arithmetic as a few billion packed rows, and the result can still be checked bit for bit.  A layout places a dense
[N, w] matrix into one large byte buffer as a strided view: row r starts ``r * stride`` elements after the pointer the kernel is
handed (all offsets below are relative to THAT pointer).  The buffer is filled with 0xFF first, so whatever is read from a
wrong place is a NaN float, a -1 int8 or an all-ones code.

Layout B (byte rows: the sign-bit, int8 and PQ codes): 6 000 rows 786 480 bytes apart, 4.72 GB; row offsets cross 2^31 and
2^32 bytes; row 5 461 starts 16 bytes below 2^32 bytes (5 461 x 786 480 = 2^32 - 16), so every row of 32 bytes or more straddles.
Layout F (float32 rows): 6 000 rows 719 184 elements apart, 17.26 GB; row offsets cross 2^31, 2^32, 2^33 (2^31 elements) and
2^34 bytes (2^32 elements); row 1 493 starts 112 elements below 2^32 bytes (1 493 x 719 184 = 2^30 - 112).
A straddling row tells a 64-bit row base joined with a 32-bit offset inside the row (a lost carry) from correct addressing:
every other defect modelled here also misplaces whole rows.

``misread`` is the CPU model: what a kernel with a named truncation would read from such a buffer.  tests/test_far_cases_cpu.py
shows that the oracles flag each of them, so the GPU tests have teeth without a wrong kernel ever running on a GPU.

The corpora are those of tests/test_search_boundary_gpu.py (Gaussian rows; 1 500 near-ties of query 0) with one change: the rows
beside every boundary of the layout (``Layout.sentinels``) are a query plus noise, so that each of them sits in a top-10 list and
a wrong read of it alone changes a result."""
import functools

import numpy as np

import hamming_cases as hc
import int8_cases as i8
import pq_cases as pc
from l2_cases import l2_dists
from oracle.search_ref import _lane_sum, exact_cosine, topk_rows

N, Q = 6000, 8
DIMS = (256, 300)
KINDS = ("gauss", "near_ties")
MODELS = ("byte_mod_2^32", "elem_mod_2^31", "elem_mod_2^32", "elem_int32_wrap", "byte_int32_wrap", "lost_carry_2^32")
FILL = 0xFF


class Layout:
    def __init__(self, name, itemsize, stride, i0, boundaries, rows=N):
        self.name, self.itemsize, self.stride, self.i0, self.rows = name, itemsize, stride, i0, rows
        self.boundaries = tuple(boundaries)             # byte offsets the row starts cross
        self.row_bytes = stride * itemsize
        self.nbytes = rows * self.row_bytes

    def start(self, r):
        """byte offset of row r from the pointer handed to the kernel"""
        return int(r) * self.row_bytes

    def sentinels(self):
        """the rows beside every boundary (the last row starting at or below it, its neighbours), the first and the last row"""
        s = {0, self.rows - 1}
        for b in self.boundaries:
            rb = b // self.row_bytes
            s.update((rb - 1, rb, rb + 1))
        return sorted(s)


LAYOUT_B = Layout("B", 1, 786480, 5461, (1 << 31, 1 << 32))
LAYOUT_F = Layout("F", 4, 719184, 1493, (1 << 31, 1 << 32, 1 << 33, 1 << 34))
LAYOUTS = {"B": LAYOUT_B, "F": LAYOUT_F}
# Eight float32 QUERY rows in the Layout F buffer, (2^32 - 4) / 7 elements apart: rows 1, 2 and 4 start beyond 2^31, 2^32 and 2^33
# bytes (2^31 elements), and row 7 starts 4 elements below 2^32 elements (2^34 bytes) and straddles them.
QUERY_STRIDE_F = ((1 << 32) - 4) // 7


# ------------------------------------------------------------------------------------------------- the CPU model of wrong addressing
def misread(layout, x, model):
    """What a kernel with the truncation ``model`` reads for the matrix ``x`` [rows, w] placed in ``layout``: for every byte the
    offset the defect computes, then the byte that lies there — another row's, or the fill.  An offset outside the buffer (a
    negative one after an int32 wrap) reads as the fill."""
    x = np.ascontiguousarray(x)
    assert x.dtype.itemsize == layout.itemsize and x.shape[0] == layout.rows
    xb = x.view(np.uint8).reshape(x.shape[0], -1)
    wb, es, sb = xb.shape[1], layout.itemsize, layout.row_bytes
    base = np.arange(x.shape[0], dtype=np.int64)[:, None] * sb
    j = np.arange(wb, dtype=np.int64)[None, :]
    b = base + j
    e, within = b // es, b % es
    if model == "byte_mod_2^32":
        b2 = b % (1 << 32)
    elif model == "elem_mod_2^31":
        b2 = (e % (1 << 31)) * es + within
    elif model == "elem_mod_2^32":
        b2 = (e % (1 << 32)) * es + within
    elif model == "elem_int32_wrap":
        b2 = (((e + (1 << 31)) % (1 << 32)) - (1 << 31)) * es + within
    elif model == "byte_int32_wrap":
        b2 = ((b + (1 << 31)) % (1 << 32)) - (1 << 31)
    elif model == "lost_carry_2^32":      # a 64-bit row base whose low word takes the offset inside the row without the carry
        b2 = (base >> 32 << 32) + (base + j) % (1 << 32)
    else:
        raise ValueError(model)
    r, w = b2 // sb, b2 % sb
    ok = (b2 >= 0) & (r < x.shape[0]) & (w < wb)
    out = np.full_like(xb, FILL)
    out[ok] = xb[r[ok], w[ok]]
    return out.view(x.dtype).reshape(x.shape)


def rows_misread(x, read):
    """the rows of ``x`` that ``read`` = misread(layout, x, model) holds wrongly"""
    a = np.ascontiguousarray(x).view(np.uint8).reshape(x.shape[0], -1)
    return np.flatnonzero((np.ascontiguousarray(read).view(np.uint8).reshape(a.shape) != a).any(1))


# ------------------------------------------------------------------------------------------------- corpora
@functools.lru_cache(maxsize=None)
def rows(layout, kind, d):
    """(queries [Q, d], corpus [N, d]) float32: the recipe of tests/test_search_boundary_gpu.py, then sentinel t of the layout
    becomes query 1 + t % 7 plus noise of a quarter of its size."""
    rng = np.random.default_rng(1729)
    c = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    if kind == "near_ties":
        base = rng.standard_normal(d).astype(np.float32)
        c[500:2000] = base + 1e-6 * rng.standard_normal((1500, d)).astype(np.float32)
        q[0] = base
    prng = np.random.default_rng(4242)
    for t, r in enumerate(LAYOUTS[layout].sentinels()):
        c[r] = q[1 + t % (Q - 1)] + np.float32(0.25) * prng.standard_normal(d).astype(np.float32)
    q.setflags(write=False), c.setflags(write=False)
    return q, c


def dot_scores(q, c):
    return np.concatenate([_lane_sum(q[a:a + 2, None, :], c[None, :, :]).astype(np.float32) for a in range(0, q.shape[0], 2)])


def scores(space, q, c):
    """[Q, N] float32 scores of the three exact spaces, NaN where a row holds one (l2: squared distances)"""
    with np.errstate(all="ignore"):
        return exact_cosine(q, c) if space == "cosine" else dot_scores(q, c) if space == "dot" else l2_dists(q, c)


def topk(space, s, k):
    """(scores [Q, k], idx [Q, k]) of a score matrix by (score desc, index asc) — l2: (distance asc, index asc); NaN scores lose"""
    s = np.where(np.isnan(s), np.float32(np.inf if space == "l2" else -np.inf), s)
    if space == "l2":
        _, i = topk_rows(-s, k)
        return np.take_along_axis(s, i, 1), i
    return topk_rows(s, k)


@functools.lru_cache(maxsize=None)
def exact(layout, kind, d, space):
    return scores(space, *rows(layout, kind, d))


@functools.lru_cache(maxsize=None)
def oracle_topk(layout, kind, d, space, k=100):
    """the oracle's k = 100 lists: its k lists are their first k columns"""
    return topk(space, exact(layout, kind, d, space), k)


def range_ref(space, s, taus):
    """per query the rows with score >= float32(tau) ordered by (score desc, index asc); l2: distance <= tau, (distance asc,
    index asc).  ``taus``: one threshold or one per query."""
    taus = np.broadcast_to(np.asarray(taus, dtype=np.float32), (s.shape[0],))
    out = []
    for row, tau in zip(s, taus):
        hit = np.nonzero(row <= tau if space == "l2" else row >= tau)[0]
        key = row[hit].astype(np.float64)
        out.append(hit[np.lexsort((hit, key if space == "l2" else -key))])
    return out


# ------------------------------------------------------------------------------------------------- code rows (Layout B)
def pq_shape(d):
    """(M, dsub) with a code row of 32 bytes, so that it straddles: 256 = 32 x 8, 300 = 30 x 10"""
    return {256: (32, 8), 300: (30, 10)}[d]


@functools.lru_cache(maxsize=None)
def codes(kind, d, family):
    """The code rows of rows("B", kind, d) by the restatements: 'hamming' -> (q_codes, c_codes) uint8; 'int8' -> (q_codes,
    c_codes, ranges); 'pq' -> (codebooks float32 [M, 256, dsub], c_codes uint8 [N, 32])."""
    q, c = rows("B", kind, d)
    if family == "hamming":
        return hc.pack_ref(q), hc.pack_ref(c)
    if family == "int8":
        ranges = i8.ranges_of(c)
        return i8.quantize_ref(q, ranges), i8.quantize_ref(c, ranges), ranges
    M, dsub = pq_shape(d)
    cb = pc.random_codebooks(np.random.default_rng(77 + d), d, M)
    return cb, pc.encode_ref(c, cb)


def code_topk(kind, d, family, c_codes, k):
    """the first-stage oracle of a code family on the code rows ``c_codes`` (the true ones, or what a defect reads)"""
    if family == "hamming":
        return hc.hamming_topk_ref(codes(kind, d, family)[0], c_codes, d, k)
    if family == "int8":
        return i8.ip_topk_ref(codes(kind, d, family)[0], c_codes, d, k)
    cb = codes(kind, d, family)[0]
    tables, _ = pc.tables_ref(rows("B", kind, d)[0], cb, "ip")
    return pc.adc_topk_ref(tables, c_codes, k, "ip")


# ------------------------------------------------------------------------------------------------- placing rows on the device
class FarBuffer:
    """One device byte buffer of a layout, filled with 0xFF, holding one placed matrix at a time."""

    def __init__(self, layout, device):
        import torch
        self.layout, self.device = layout, device
        self.buf = torch.empty(layout.nbytes, dtype=torch.uint8, device=device)
        self.buf.fill_(FILL)
        self._last = None

    def place(self, x, stride=None):
        """``x`` [n, w] (numpy, the layout's item size) as a view of the buffer with row stride ``stride`` elements (default: the
        layout's); whatever was placed before is wiped back to the fill first.  The first, the last and the straddling row are
        read back through plain 1-D slices of the buffer."""
        import torch
        x = np.array(x, order="C")                      # (a copy: the cached corpora are read-only)
        es = self.layout.itemsize
        stride = self.layout.stride if stride is None else stride
        n, w = x.shape
        assert x.dtype.itemsize == es and stride >= w and ((n - 1) * stride + w) * es <= self.layout.nbytes
        if self._last is not None:
            torch.as_strided(self.buf, *self._last).fill_(FILL)
        self._last = ((n, w * es), (stride * es, 1))
        src = torch.from_numpy(x).to(self.device)
        view = torch.as_strided(self.buf.view(src.dtype), (n, w), (stride, 1))
        view.copy_(src)
        for r in {0, n - 1, min(self.layout.i0, n - 1), 2 % n}:
            a = r * stride * es
            assert torch.equal(self.buf[a:a + w * es], src[r].view(torch.uint8)), f"row {r} is not where the layout puts it"
        assert view.data_ptr() == self.buf.data_ptr() and not (n > 1 and view.is_contiguous())
        return view


# ------------------------------------------------------------------------------------------------- the large flat corpus
LARGE_N, LARGE_D, LARGE_BLOCK, LARGE_PLANTS = 2_900_000, 768, 4096, 128
LARGE_HALF_ROW = (1 << 32) // (2 * LARGE_D)        # 2 796 202: the first half row that ends beyond 2^32 bytes (2^31 elements)
LARGE_F32_ROW = (1 << 32) // (4 * LARGE_D)         # 1 398 101: the same for the float32 rows
LARGE_MARGIN = 0.2                                 # cosine; asserted by tests/test_far_cases_cpu.py


@functools.lru_cache(maxsize=None)
def large_inputs():
    """(queries [8, 768], block [4096, 768], positions int64 [128], planted [128, 768]) float32.  The corpus is the block tiled to
    2 900 000 rows with the planted rows written over it.  The queries share a direction g (q = g + 0.3 noise); planted row p is
    a_p g + sqrt(1 - a_p^2) noise with a_p from 0.55 to 0.98, so every planted row scores between 0.5 and 0.95 or so against EVERY
    query, far above the block's rows (about 0.15 at most).  Positions: the first rows; around the half rows' 2^32-byte boundary;
    around the float32 rows' one; the last two rows; the rest spread over the corpus."""
    rng = np.random.default_rng(2900)
    g = rng.standard_normal(LARGE_D)
    q = (g + 0.3 * rng.standard_normal((Q, LARGE_D))).astype(np.float32)
    block = rng.standard_normal((LARGE_BLOCK, LARGE_D)).astype(np.float32)
    a = np.linspace(0.55, 0.98, LARGE_PLANTS)[rng.permutation(LARGE_PLANTS)][:, None]
    planted = (a * g + np.sqrt(1 - a * a) * rng.standard_normal((LARGE_PLANTS, LARGE_D))).astype(np.float32)
    fixed = ([0, 1, 2, 31, 32] + [LARGE_HALF_ROW + o for o in (-33, -2, -1, 0, 1, 2, 32)]
             + [LARGE_F32_ROW + o for o in (-2, -1, 0, 1, 2)] + [LARGE_N - 2, LARGE_N - 1])
    rest = np.linspace(5000, LARGE_N - 5000, LARGE_PLANTS - len(fixed)).astype(np.int64) + 7
    pos = np.array(sorted(fixed + rest.tolist()), dtype=np.int64)
    assert np.unique(pos).size == LARGE_PLANTS and pos[-1] == LARGE_N - 1
    for x in (q, block, pos, planted):
        x.setflags(write=False)
    return q, block, pos, planted


def large_row(i):
    """rows ``i`` (an index array) of the large corpus, from its parts"""
    q, block, pos, planted = large_inputs()
    i = np.asarray(i, dtype=np.int64)
    out = block[i % LARGE_BLOCK].copy()
    at = np.searchsorted(pos, i)
    hit = (at < pos.size) & (pos[np.minimum(at, pos.size - 1)] == i)
    out[hit] = planted[at[hit]]
    return out
