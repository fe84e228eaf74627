"""Device ops: thin wrappers that pass raw device pointers of torch tensors to libtsim.so.

torch is used for allocation, stream identity and host<->device copies only.  Every function requires
CUDA (ROCm) tensors and raises otherwise: there is no CPU path in the product."""
from __future__ import annotations

import functools
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib


def _need_gpu(*ts):
    dev = None
    for t in ts:
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.TsimError("text_similarity_amd ops run on MI355X only: expected a CUDA/ROCm tensor, "
                                 f"got {type(t).__name__} on {getattr(t, 'device', None)}")
        if dev is not None and t.device != dev:
            raise ValueError(f"operands on different devices: {dev} and {t.device}")
        dev = t.device


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


UNIT_DTYPE = torch.float16      # storage type of the unit rows the MFMA search kernel streams (csrc/common.h unit_t)

_workspaces = {}


def _workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    """Scratch for one search call, keyed by (device, current stream): calls on different streams never share it, and
    calls on one stream are ordered by the stream."""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), torch.cuda.current_stream(dev).cuda_stream)
    w = _workspaces.get(key)
    if w is None or w.numel() < nbytes:
        w = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=dev)
        _workspaces[key] = w
    return w


def pad_dim(d: int) -> int:
    p = _lib.lib().tsim_pad_dim(int(d))
    if p == 0:
        raise ValueError(f"embedding width {d} > 768 is not supported by the search kernels")
    return p


def new_rho(device) -> torch.Tensor:
    """A zeroed device float for the rounding-residual maximum of a set of unit rows (see :func:`l2norm_rows`)."""
    return torch.zeros((1,), dtype=torch.float32, device=device)


def l2norm_rows(x: torch.Tensor, eps: float = 1e-8, rho: Optional[torch.Tensor] = None, return_rho: bool = False):
    """[rows, d] float32/bf16 -> unit rows in float16 (IEEE half), zero-padded to [rows, pad_dim(d)] (A7 operand prep).

    ``rho`` (a device float32 tensor of one element, e.g. from :func:`new_rho`) is atomically raised to the largest
    rounding residual ||half(u_r) - u_r||_2 of the rows written; several calls may accumulate into one word (a corpus built
    chunk by chunk).  ``return_rho=True`` allocates a fresh word and returns ``(unit_rows, rho)``.  Passing that word to
    :func:`cosine_topk` as ``rho_c`` gives the search's exactness guard its measured (tightest) error bound."""
    _need_gpu(x)
    if x.dim() != 2:
        raise ValueError("l2norm_rows expects a 2-D tensor")
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    x = x.contiguous()
    rows, d = x.shape
    ld = pad_dim(d)
    out = torch.empty((rows, ld), dtype=UNIT_DTYPE, device=x.device)
    dt = _lib.TSIM_F32 if x.dtype == torch.float32 else _lib.TSIM_BF16
    if rho is None and return_rho:
        rho = new_rho(x.device)
    if rho is not None:
        _check_rho(rho, x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().tsim_l2norm_rows(x.data_ptr(), dt, rows, d, _row_stride(x), out.data_ptr(), ld, eps,
                                               rho.data_ptr() if rho is not None else 0, _stream(x)), "l2norm_rows")
    return (out, rho) if return_rho else out


def _row_stride(t: torch.Tensor) -> int:
    """Elements between consecutive rows of a 2-D tensor with unit inner stride.  A tensor of one row may carry any stride(0)
    (a [1, d] view made with ``x[None]`` in numpy has 0, and ``contiguous()`` keeps it); the kernels check ld >= d."""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _check_rho(rho, dev):
    if not isinstance(rho, torch.Tensor) or rho.dtype != torch.float32 or rho.numel() != 1 or rho.device != dev:
        raise ValueError(f"rho must be a float32 tensor of one element on {dev}")


MAX_QUERIES_PER_CALL = 16384    # workspace grows by ~16 KB + 512 k bytes per query: larger query sets are searched in slices
MAX_K = 1024                    # include/tsim.h TSIM_TOPK_MAX_K; k > 64 runs tsim_cosine_topk_large / tsim_dot_topk_large
_LIST_MAX_K = 64                # largest k of tsim_cosine_topk_ex / tsim_dot_topk_ex
MAX_LARGE_WORKSPACE = 1 << 30   # k > 64: queries per call are halved until one call's workspace fits


def cosine_topk(eq_unit: torch.Tensor, ec_unit: torch.Tensor, d: int, k: int, idx_offset: int = 0,
                eq_f32: Optional[torch.Tensor] = None, ec_f32: Optional[torch.Tensor] = None,
                return_status: bool = False, rho_c: Optional[torch.Tensor] = None,
                out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """Top-k of every query row against every corpus row: scores [Q,k] f32, idx [Q,k] i64, ordered by (score desc,
    index asc).  ``eq_unit`` / ``ec_unit`` are the unit float16 rows from :func:`l2norm_rows` (what the MFMA kernel streams).
    With ``eq_f32`` / ``ec_f32`` (the float32 embeddings the unit rows were made from) the returned scores are the
    reference's ``F.cosine_similarity`` of the float32 rows (/root/reference/src/pipeline/search_pipeline.py:76-78) and the
    order is exact for them; without, the inner product of the unit rows as stored.  ``rho_c``: the residual maximum of
    ``ec_unit`` from :func:`l2norm_rows` (tightens the guard's proven error bound; without it the a-priori bound of a
    correctly rounded unit row is used — results are exact either way, more queries take the widening pass).
    ``return_status`` adds an int32 [Q] tensor: 0 = first pass, 1 = widened, 2 = brute force (include/tsim.h).
    1 <= k <= 1024 (MAX_K), d <= 768.  Query sets above MAX_QUERIES_PER_CALL rows are searched in slices (queries are
    independent); for k > 64 also so that one call's workspace stays within MAX_LARGE_WORKSPACE bytes.
    ``out`` = (scores, idx): preallocated contiguous [Q,k] float32 / int64 tensors to write into (e.g. two views of one
    exchange buffer, :func:`packed_result_buffer`)."""
    return _topk("cosine_topk", eq_unit, ec_unit, d, k, idx_offset, eq_f32, ec_f32, return_status, rho_c, None, out)


def _topk(what, eq_unit, ec_unit, d, k, idx_offset, eq_f32, ec_f32, return_status, rho_c, scale_c, out, l2=False):
    """cosine_topk (scale_c is None), dot_topk (scale_c = the corpus rows' max-norm word) and l2_topk (the same word; the half
    rows are one element wider than the float32 rows)."""
    _need_gpu(eq_unit, ec_unit)
    if eq_unit.dtype != UNIT_DTYPE or ec_unit.dtype != UNIT_DTYPE:
        raise ValueError(f"{what} expects float16 rows from " + ("l2_query_rows / l2_rows" if l2 else "l2norm_rows" +
                         (" / dot_scaled_rows" if scale_c is not None else "")))
    ld = pad_dim(d + 1 if l2 else d)
    if eq_unit.shape[1] != ld or ec_unit.shape[1] != ld or not eq_unit.is_contiguous() or not ec_unit.is_contiguous():
        raise ValueError(f"{what}: rows must be contiguous with stride pad_dim({d + 1 if l2 else d})={ld}")
    if (eq_f32 is None) != (ec_f32 is None):
        raise ValueError(f"{what}: pass both float32 matrices or neither")
    Q, N = eq_unit.shape[0], ec_unit.shape[0]
    dev = eq_unit.device
    if ec_unit.device != dev:
        raise ValueError(f"{what}: operands on different devices ({dev} vs {ec_unit.device})")
    qf = cf = 0
    ldq = ldc = 0
    if eq_f32 is not None:
        _need_gpu(eq_f32, ec_f32)
        for t, rows, name in ((eq_f32, Q, "eq_f32"), (ec_f32, N, "ec_f32")):
            if t.dtype != torch.float32 or t.dim() != 2 or t.shape != (rows, d) or t.stride(1) != 1 or t.device != dev:
                raise ValueError(f"{what}: {name} must be float32 [{rows}, {d}] with unit inner stride on {dev}")
        qf, cf, ldq, ldc = eq_f32.data_ptr(), ec_f32.data_ptr(), _row_stride(eq_f32), _row_stride(ec_f32)
    if rho_c is not None:
        _check_rho(rho_c, dev)
    if scale_c is not None:
        _check_rho(scale_c, dev)
    if out is not None:
        scores, idx = out
        _need_gpu(scores, idx)
        if (scores.shape != (Q, k) or idx.shape != (Q, k) or scores.dtype != torch.float32 or idx.dtype != torch.int64
                or not scores.is_contiguous() or not idx.is_contiguous() or scores.device != dev or idx.device != dev):
            raise ValueError(f"{what}: out must be contiguous float32 / int64 [{Q}, {k}] tensors on {dev}")
    else:
        scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
        idx = torch.empty((Q, k), dtype=torch.int64, device=dev)
    status = torch.zeros((Q,), dtype=torch.int32, device=dev) if return_status else None
    if Q == 0:
        return (scores, idx, status) if return_status else (scores, idx)
    L = _lib.lib()
    with torch.cuda.device(dev):
        step = min(Q, MAX_QUERIES_PER_CALL)
        large = k > _LIST_MAX_K
        wsb = L.tsim_topk_large_workspace_bytes if large else L.tsim_cosine_topk_workspace_bytes
        nbytes = wsb(step, N, k)
        if nbytes == 0:
            raise ValueError(f"{what}: unsupported shape Q={Q} N={N} k={k} (1 <= k <= {MAX_K})")
        while large and step > 1 and nbytes > MAX_LARGE_WORKSPACE:
            step = (step + 1) // 2
            nbytes = wsb(step, N, k)
        ws = _workspace(dev, nbytes)
        for q0 in range(0, Q, step):
            nq = min(step, Q - q0)
            qargs = (eq_unit.data_ptr() + q0 * ld * 2, qf + q0 * ldq * 4 if qf else 0, ldq, nq, ec_unit.data_ptr(), cf, ldc)
            rest = (N, d, ld, k, scores.data_ptr() + q0 * k * 4, idx.data_ptr() + q0 * k * 8,
                    status.data_ptr() + q0 * 4 if return_status else 0, idx_offset, ws.data_ptr(), ws.numel(), _stream(eq_unit))
            rho_p = rho_c.data_ptr() if rho_c is not None else 0
            if scale_c is None:
                rc = (L.tsim_cosine_topk_large if large else L.tsim_cosine_topk_ex)(*qargs, rho_p, *rest)
            elif l2:
                rc = (L.tsim_l2_topk_large if large else L.tsim_l2_topk_ex)(*qargs, scale_c.data_ptr(), rho_p, *rest)
            else:
                rc = (L.tsim_dot_topk_large if large else L.tsim_dot_topk_ex)(*qargs, scale_c.data_ptr(), rho_p, *rest)
            _lib.check(rc, what)
    return (scores, idx, status) if return_status else (scores, idx)


def max_norm_rows(x: torch.Tensor, maxnorm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Raise the max-norm word ``maxnorm`` (device float32 [1], zeroed by the caller; a fresh one when None) to an upper bound
    of the L2 norms of the rows of ``x`` [rows, d] (float32/bf16) and return it.  A row with a non-finite element makes it
    +inf.  The inner-product search scales its corpus rows by :func:`dot_scale` of this word."""
    _need_gpu(x)
    x = _rows_operand(x, "max_norm_rows")
    if maxnorm is None:
        maxnorm = new_rho(x.device)
    _check_rho(maxnorm, x.device)
    dt = _lib.TSIM_F32 if x.dtype == torch.float32 else _lib.TSIM_BF16
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().tsim_max_norm_rows(x.data_ptr(), dt, x.shape[0], x.shape[1], _row_stride(x), maxnorm.data_ptr(),
                                                 _stream(x)), "max_norm_rows")
    return maxnorm


def dot_scale(maxnorm) -> float:
    """S, the power of two the inner-product search divides corpus rows by, for a max-norm word (a float, or the device word,
    which is read back): the smallest 2^e >= the word; 1.0 for 0 (an all-zero corpus); inf for a non-finite word."""
    if isinstance(maxnorm, torch.Tensor):
        maxnorm = float(maxnorm.item())
    return float(_lib.lib().tsim_dot_scale(float(maxnorm)))


def dot_scaled_rows(x: torch.Tensor, maxnorm: Optional[torch.Tensor] = None, rho: Optional[torch.Tensor] = None):
    """Corpus operand of :func:`dot_topk`: [rows, d] float32/bf16 -> ``(rows, rho, scale)``.  ``rows`` = half(x / S) zero-padded
    to [rows, pad_dim(d)], S = :func:`dot_scale` of the max-norm word ``scale`` (device float32 [1]); ``rho`` (device float32
    [1]) raised to the rows' largest residual ||rows_r - x_r / S||_2, counting subnormal halves as kept and as flushed.
    ``maxnorm`` None: a fresh word from :func:`max_norm_rows` of ``x``; given: a word that already covers ``x`` (e.g. a whole
    index's), used as it is.  ``rho`` None: a fresh word; given: accumulated into.  No host synchronisation."""
    _need_gpu(x)
    x = _rows_operand(x, "dot_scaled_rows")
    rows, d = x.shape
    ld = pad_dim(d)
    if maxnorm is None:
        maxnorm = max_norm_rows(x)
    _check_rho(maxnorm, x.device)
    if rho is None:
        rho = new_rho(x.device)
    _check_rho(rho, x.device)
    out = torch.empty((rows, ld), dtype=UNIT_DTYPE, device=x.device)
    dt = _lib.TSIM_F32 if x.dtype == torch.float32 else _lib.TSIM_BF16
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().tsim_dot_scaled_rows(x.data_ptr(), dt, rows, d, _row_stride(x), maxnorm.data_ptr(), out.data_ptr(), ld,
                                                   rho.data_ptr(), _stream(x)), "dot_scaled_rows")
    return out, rho, maxnorm


def _rows_operand(x: torch.Tensor, what: str) -> torch.Tensor:
    if x.dim() != 2:
        raise ValueError(f"{what} expects a 2-D tensor")
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    return x.contiguous()


def dot_topk(eq_unit: torch.Tensor, ec_scaled: torch.Tensor, d: int, k: int, eq_f32: torch.Tensor, ec_f32: torch.Tensor,
             rho_c: torch.Tensor, scale_c: torch.Tensor, idx_offset: int = 0, return_status: bool = False,
             out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """Exact top-k by inner product (dot-product sentence-transformers models; hnswlib space='ip'): scores [Q,k] = float32(q.c)
    of the float32 rows (float64 sum in the canonical lane order, one rounding), idx [Q,k] i64, ordered by (score desc, index
    asc).  ``eq_unit``: the queries' unit rows (:func:`l2norm_rows`); ``(ec_scaled, rho_c, scale_c)``: :func:`dot_scaled_rows`
    of ``ec_f32``.  All four float32/word arguments are required (include/tsim.h tsim_dot_topk_ex); the rest as
    :func:`cosine_topk`.  A zero query returns the first k rows with score 0."""
    if eq_f32 is None or ec_f32 is None or rho_c is None or scale_c is None:
        raise ValueError("dot_topk needs eq_f32, ec_f32 and the corpus rows' rho_c and scale_c (dot_scaled_rows)")
    return _topk("dot_topk", eq_unit, ec_scaled, d, k, idx_offset, eq_f32, ec_f32, return_status, rho_c, scale_c, out)


# ------------------------------------------------------------------------------------------------- exact Euclidean search
L2_MAX_DIM = 767                # the half operands are one element wider than the rows: pad_dim(d + 1) <= 768


def _l2_dim(d: int, what: str) -> int:
    if d > L2_MAX_DIM:
        raise ValueError(f"{what}: embedding width {d} > {L2_MAX_DIM} is not supported (the half rows are d + 1 wide)")
    return pad_dim(d + 1)


def l2_rows(x: torch.Tensor, maxnorm: Optional[torch.Tensor] = None, rho: Optional[torch.Tensor] = None):
    """Corpus operand of :func:`l2_topk`: [rows, d] float32/bf16 -> ``(rows, rho, maxnorm)``.  ``rows`` = half((x, -|x|^2 / (2A))
    / 2A) zero-padded to [rows, pad_dim(d + 1)], A = :func:`dot_scale` of the max-norm word ``maxnorm``; ``rho`` raised to the
    rows' largest flush-safe residual.  ``maxnorm`` / ``rho`` None or given: as in :func:`dot_scaled_rows`.  d <= 767."""
    _need_gpu(x)
    x = _rows_operand(x, "l2_rows")
    rows, d = x.shape
    ld = _l2_dim(d, "l2_rows")
    if maxnorm is None:
        maxnorm = max_norm_rows(x)
    _check_rho(maxnorm, x.device)
    if rho is None:
        rho = new_rho(x.device)
    _check_rho(rho, x.device)
    out = torch.empty((rows, ld), dtype=UNIT_DTYPE, device=x.device)
    dt = _lib.TSIM_F32 if x.dtype == torch.float32 else _lib.TSIM_BF16
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().tsim_l2_rows(x.data_ptr(), dt, rows, d, _row_stride(x), maxnorm.data_ptr(), out.data_ptr(), ld,
                                           rho.data_ptr(), _stream(x)), "l2_rows")
    return out, rho, maxnorm


def l2_query_rows(x: torch.Tensor, maxnorm: torch.Tensor) -> torch.Tensor:
    """Query operand of :func:`l2_topk`: [rows, d] float32/bf16 -> half((x, A) / sqrt(|x|^2 + A^2)) zero-padded to
    [rows, pad_dim(d + 1)], A = :func:`dot_scale` of the CORPUS' max-norm word ``maxnorm`` (the one :func:`l2_rows` used)."""
    _need_gpu(x)
    x = _rows_operand(x, "l2_query_rows")
    rows, d = x.shape
    ld = _l2_dim(d, "l2_query_rows")
    _check_rho(maxnorm, x.device)
    out = torch.empty((rows, ld), dtype=UNIT_DTYPE, device=x.device)
    dt = _lib.TSIM_F32 if x.dtype == torch.float32 else _lib.TSIM_BF16
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().tsim_l2_query_rows(x.data_ptr(), dt, rows, d, _row_stride(x), maxnorm.data_ptr(), out.data_ptr(), ld,
                                                 _stream(x)), "l2_query_rows")
    return out


def l2_topk(eq_aug: torch.Tensor, ec_aug: torch.Tensor, d: int, k: int, eq_f32: torch.Tensor, ec_f32: torch.Tensor,
            rho_c: torch.Tensor, scale_c: torch.Tensor, idx_offset: int = 0, return_status: bool = False,
            out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """Exact top-k by Euclidean distance (the 'l2' space of hnswlib and faiss): scores [Q,k] = float32 SQUARED distances of the
    float32 rows (canonical float64 evaluation, include/tsim.h tsim_l2_topk_ex), ascending, ties to the lower index; idx [Q,k]
    i64; padding +inf / -1.  ``eq_aug``: :func:`l2_query_rows` of ``eq_f32`` under ``scale_c``; ``(ec_aug, rho_c, scale_c)``:
    :func:`l2_rows` of ``ec_f32``.  All are required; the rest as :func:`cosine_topk`.  d <= 767."""
    if eq_f32 is None or ec_f32 is None or rho_c is None or scale_c is None:
        raise ValueError("l2_topk needs eq_f32, ec_f32 and the corpus rows' rho_c and scale_c (l2_rows)")
    _l2_dim(d, "l2_topk")
    return _topk("l2_topk", eq_aug, ec_aug, d, k, idx_offset, eq_f32, ec_f32, return_status, rho_c, scale_c, out, l2=True)


# ------------------------------------------------------------------------------------------------- exact search within lists
LIST_SLICE = 1024               # include/tsim.h TSIM_LIST_SLICE
LIST_ST_ROW, LIST_ST_LIMS = _lib.LIST_ST_ROW, _lib.LIST_ST_LIMS
LIST_MAX_WORKSPACE = 256 << 20  # csrc/search.hip BF_BUDGET


def _list_operands(what, cand, lims, Q, N, dev, assume_unique):
    """(cand 1-D int32/int64 contiguous, lims int64 [Q+1] or None, extra status int32 [Q] or None) on the device.  A 2-D ``cand``
    gets its implicit lims; unless ``assume_unique``, negatives and repeats inside a list are removed (torch plumbing: one sort
    of the keys query * (N + 1) + min(row, N), so every entry >= N survives as ONE entry N and still raises its status bit) and
    the lims are rebuilt from the per-query counts — the bit of a bad lims pair is computed here then, from the same rule as the
    kernel's (running maximum, clamped)."""
    _need_gpu(cand)
    if cand.device != dev:
        raise ValueError(f"{what}: cand on {cand.device}, rows on {dev}")
    if cand.dtype not in (torch.int32, torch.int64):
        if cand.dtype.is_floating_point or cand.dtype == torch.bool:
            raise ValueError(f"{what}: cand must hold integers, not {cand.dtype}")
        cand = cand.long()
    if cand.dim() == 2:
        if lims is not None:
            raise ValueError(f"{what}: a 2-D cand [Q, m] carries its own lists; pass lims with a 1-D cand")
        if cand.shape[0] != Q:
            raise ValueError(f"{what}: cand has {cand.shape[0]} rows for {Q} queries")
        m = cand.shape[1]
        lims = torch.arange(Q + 1, dtype=torch.int64, device=dev) * m
        cand = cand.reshape(-1)
    elif cand.dim() != 1:
        raise ValueError(f"{what}: cand must be 1-D (with lims: CSR; without: one shared list) or 2-D [Q, m]")
    elif lims is not None:
        lims = torch.as_tensor(lims).to(dev, dtype=torch.int64).contiguous()
        if lims.shape != (Q + 1,):
            raise ValueError(f"{what}: lims must be int64 [{Q + 1}], got {tuple(lims.shape)}")
    cand = cand.contiguous()
    if assume_unique:
        return cand, lims, None
    T = cand.numel()
    if lims is None:
        c = cand[cand >= 0]
        return torch.unique(c.clamp(max=N)), None, None
    clean = torch.cummax(lims, 0).values.clamp(0, T)
    bad = ((clean[:-1] != lims[:-1]) | (clean[1:] != lims[1:])).to(torch.int32) * LIST_ST_LIMS
    pos = torch.arange(T, dtype=torch.int64, device=dev)
    qid = torch.searchsorted(clean[1:].contiguous(), pos, right=True)          # the query owning position p (Q: none)
    keep = (cand >= 0) & (qid < Q) & (pos >= clean[:-1][qid.clamp(max=Q - 1)])
    key = torch.unique(qid[keep] * (N + 1) + cand[keep].long().clamp(max=N))
    counts = torch.bincount(torch.div(key, N + 1, rounding_mode="floor"), minlength=Q)
    new_lims = torch.zeros((Q + 1,), dtype=torch.int64, device=dev)
    new_lims[1:] = torch.cumsum(counts, 0)
    return (key % (N + 1)).contiguous(), new_lims, bad


def _list_topk(what, fn_name, eq_f32, ec_f32, cand, lims, k, idx_offset, return_status, assume_unique, f16_space=None):
    """``f16_space``: the corpus (still called ``ec_f32`` here) holds float16 rows and ``fn_name`` takes the space first."""
    _need_gpu(eq_f32, ec_f32)
    dev = eq_f32.device
    for t, name, dt in ((eq_f32, "eq_f32", torch.float32),
                        (ec_f32, "ec_f32" if f16_space is None else "ec_f16", torch.float32 if f16_space is None else torch.float16)):
        if t.dtype != dt or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"{what}: {name} must be {str(dt)[6:]} [rows, d] with unit inner stride")
    Q, d = eq_f32.shape
    N = ec_f32.shape[0]
    if ec_f32.shape[1] != d:
        raise ValueError(f"{what}: query rows are {d} wide, corpus rows {ec_f32.shape[1]}")
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{what}: k={k} outside 1..{MAX_K}")
    if not isinstance(cand, torch.Tensor):
        raise _lib.TsimError(f"{what}: cand must be a CUDA/ROCm tensor, got {type(cand).__name__}")
    cand, lims, extra = _list_operands(what, cand, lims, Q, N, dev, assume_unique)
    scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
    idx = torch.empty((Q, k), dtype=torch.int64, device=dev)
    status = torch.zeros((Q,), dtype=torch.int32, device=dev) if return_status else None
    if Q == 0:
        return (scores, idx, status) if return_status else (scores, idx)
    if N == 0:
        raise ValueError(f"{what}: empty corpus")
    L = _lib.lib()
    T = cand.numel()
    dt = _lib.TSIM_I32 if cand.dtype == torch.int32 else _lib.TSIM_I64
    ldq, ldc = _row_stride(eq_f32), _row_stride(ec_f32)
    with torch.cuda.device(dev):
        # queries per call: the workspace stays within what the full search of the same queries asks for (or within the budget
        # of its brute-force lists, which the list kernels' own chunk lists are sized by)
        step = min(Q, MAX_QUERIES_PER_CALL)
        nbytes = L.tsim_list_topk_workspace_bytes(step, T, k)
        while step > 1 and nbytes > max(L.tsim_topk_large_workspace_bytes(step, N, k), LIST_MAX_WORKSPACE):
            step = (step + 1) // 2
            nbytes = L.tsim_list_topk_workspace_bytes(step, T, k)
        ws = _workspace(dev, nbytes)
        fn = getattr(L, fn_name)
        if f16_space is not None:
            fn = functools.partial(fn, f16_space)
        for q0 in range(0, Q, step):
            nq = min(step, Q - q0)
            rc = fn(eq_f32.data_ptr() + q0 * ldq * 4, ldq, nq, ec_f32.data_ptr(), ldc, N, d, cand.data_ptr() if T else 0, dt, T,
                    lims.data_ptr() + q0 * 8 if lims is not None else 0, int(lims is None), k, scores.data_ptr() + q0 * k * 4,
                    idx.data_ptr() + q0 * k * 8, idx_offset, status.data_ptr() + q0 * 4 if return_status else 0, ws.data_ptr(),
                    ws.numel(), _stream(eq_f32))
            _lib.check(rc, what)
    if return_status and extra is not None:
        status |= extra
    return (scores, idx, status) if return_status else (scores, idx)


def cosine_list_topk(eq_f32: torch.Tensor, ec_f32: torch.Tensor, cand: torch.Tensor, lims: Optional[torch.Tensor] = None,
                     k: int = 10, idx_offset: int = 0, return_status: bool = False, assume_unique: bool = False):
    """Exact top-k of every query WITHIN ITS OWN LIST of corpus rows: scores [Q,k] f32 and idx [Q,k] i64 ordered by (score desc,
    row asc), padded with -inf / -1 where a list has fewer than k usable rows.  Float32 rows only (``eq_f32`` [Q,d], ``ec_f32``
    [N,d]; strided row views are fine): nothing is selected by MFMA, every listed row is scored with the exact cosine of
    :func:`cosine_topk`'s float32 mode — a list that holds every row returns the same bits.
    ``cand``: 1-D with ``lims=None`` — ONE list shared by all queries; 1-D with ``lims`` int64 [Q+1] — CSR, query q owns
    ``cand[lims[q]:lims[q+1]]``; 2-D [Q, m] — fixed-width lists (the ``idx`` of an earlier search can be passed as it is).
    int32 or int64.  Negative entries are padding.  Entries >= N are skipped and set status bit ``LIST_ST_ROW``; a lims pair
    that is decreasing or outside [0, len(cand)] is clamped (include/tsim.h) and sets ``LIST_ST_LIMS``; ``return_status`` adds
    the int32 [Q] status.  Rows repeated inside a list are removed first (a device sort; the lists come out sorted by row)
    unless ``assume_unique=True``, which passes the lists to the kernel untouched — a row listed twice is then returned twice,
    adjacent.  CPU tensors raise ``TsimError``."""
    return _list_topk("cosine_list_topk", "tsim_cosine_list_topk", eq_f32, ec_f32, cand, lims, k, idx_offset, return_status,
                      assume_unique)


def dot_list_topk(eq_f32: torch.Tensor, ec_f32: torch.Tensor, cand: torch.Tensor, lims: Optional[torch.Tensor] = None,
                  k: int = 10, idx_offset: int = 0, return_status: bool = False, assume_unique: bool = False):
    """:func:`cosine_list_topk` by inner product: scores = float32(q.c) as :func:`dot_topk` returns them."""
    return _list_topk("dot_list_topk", "tsim_dot_list_topk", eq_f32, ec_f32, cand, lims, k, idx_offset, return_status,
                      assume_unique)


def l2_list_topk(eq_f32: torch.Tensor, ec_f32: torch.Tensor, cand: torch.Tensor, lims: Optional[torch.Tensor] = None,
                 k: int = 10, idx_offset: int = 0, return_status: bool = False, assume_unique: bool = False):
    """:func:`cosine_list_topk` by Euclidean distance: SQUARED distances as :func:`l2_topk` returns them, ascending, ties to the
    lower row, padded with +inf / -1.  d <= 767, as there."""
    if eq_f32.dim() == 2:
        _l2_dim(eq_f32.shape[1], "l2_list_topk")
    return _list_topk("l2_list_topk", "tsim_l2_list_topk", eq_f32, ec_f32, cand, lims, k, idx_offset, return_status,
                      assume_unique)


def f16_rows(x: torch.Tensor) -> torch.Tensor:
    """[rows, d] float rows -> ``torch.float16`` [rows, d] on the device, each element rounded to nearest, ties to even: the bits of
    numpy's ``astype(np.float16)`` (subnormals included).  The row store of a refine stage (:func:`f16_list_topk`).  A row
    that is not finite after the rounding — an element beyond +-65 504 (it would become inf), inf or NaN — raises
    ``ValueError``.  The conversion is torch's; it runs once per added row, never in a search."""
    _need_gpu(x)
    if x.dim() != 2:
        raise ValueError("f16_rows expects a 2-D tensor")
    if not x.dtype.is_floating_point:
        raise ValueError(f"f16_rows: rows must be floating point, not {x.dtype}")
    out = x.to(torch.float16).contiguous()
    if out.numel() and not bool(torch.isfinite(out).all()):
        bad = int((~torch.isfinite(out)).any(dim=1).nonzero()[0])
        raise ValueError(f"f16_rows: row {bad} is not finite in float16 (|x| > 65504, inf or NaN)")
    return out


F16_LIST_SPACES = {"cosine": _lib.SPACE_COSINE, "dot": _lib.SPACE_DOT, "l2": _lib.SPACE_L2}


def f16_list_topk(space: str, eq_f32: torch.Tensor, ec_f16: torch.Tensor, cand: torch.Tensor, lims: Optional[torch.Tensor] = None,
                  k: int = 10, idx_offset: int = 0, return_status: bool = False, assume_unique: bool = False):
    """:func:`cosine_list_topk` / :func:`dot_list_topk` / :func:`l2_list_topk` (``space`` "cosine" / "dot" / "l2") over a corpus of
    FLOAT16 rows (``ec_f16`` [N, d] ``torch.float16``, unit inner stride, any row stride; :func:`f16_rows` makes them): the
    second stage of a refine search whose row store keeps half the bytes.  The float32 query is scored against the rows
    widened to float32 — exactly, subnormals kept — so the result holds the bits the float32 op gives on ``ec_f16.float()``.
    Lists, padding, status and errors are those of the float32 ops."""
    if space not in F16_LIST_SPACES:
        raise ValueError(f"f16_list_topk: space must be one of {sorted(F16_LIST_SPACES)}, not {space!r}")
    if space == "l2" and isinstance(eq_f32, torch.Tensor) and eq_f32.dim() == 2:
        _l2_dim(eq_f32.shape[1], "f16_list_topk")
    return _list_topk("f16_list_topk", "tsim_list_topk_f16", eq_f32, ec_f16, cand, lims, k, idx_offset, return_status, assume_unique,
                      f16_space=F16_LIST_SPACES[space])


# ------------------------------------------------------------------------------------------------- inverted lists
IVF_SEG = _lib.IVF_SEG          # include/tsim.h TSIM_IVF_SEG: rows of one segment of an inverted list
IVF_ST_LIST, IVF_ST_OFF = _lib.IVF_ST_LIST, _lib.IVF_ST_OFF
IVF_SPACES = {"cosine": _lib.SPACE_COSINE, "dot": _lib.SPACE_DOT, "l2": _lib.SPACE_L2}
IVF_MAX_WORKSPACE = 64 << 20    # csrc/ivf_search.h IVF_BUDGET (a call of one query may exceed it: one slot per probe)


def ivf_scan_topk(space: str, eq_f32: torch.Tensor, rows_f32: torch.Tensor, list_off: torch.Tensor, row_ids: torch.Tensor,
                  probes: torch.Tensor, k: int, idx_offset: int = 0, return_status: bool = False,
                  max_list_len: Optional[int] = None):
    """Exact top-k of every query among the rows of the inverted lists it probes (include/tsim.h tsim_ivf_scan_topk): scores
    [Q,k] f32 and ids [Q,k] i64 ordered by (score desc, id asc) — ``space`` 'cosine' | 'dot' | 'l2' (squared distances, ascending) —
    with the bits of :func:`cosine_list_topk` / :func:`dot_list_topk` / :func:`l2_list_topk`.  ``rows_f32`` [N,d] float32 holds
    the rows in LIST order (strided row views are fine), ``list_off`` int64 [nlist+1] the lists' bounds, ``row_ids`` int32 [N] the
    id reported for each position (negative: a tombstone, skipped), ``probes`` int64 [Q,nprobe] the list numbers per query (the
    ``idx`` of a search against the centroids as it stands; negative: padding).  A probe >= nlist sets status bit
    ``IVF_ST_LIST``, a list whose offsets are decreasing or outside [0, N] is clamped and sets ``IVF_ST_OFF``; ``return_status``
    adds the int32 [Q] status.  ``max_list_len``: the longest list's length, known to the caller on the host — a sizing hint
    for the grid, never read back from the device; the result does not depend on it (default: N / nlist, the mean).  Query sets are
    searched in slices that keep one call's workspace within IVF_MAX_WORKSPACE."""
    what = "ivf_scan_topk"
    if space not in IVF_SPACES:
        raise ValueError(f"{what}: space {space!r}: one of {tuple(IVF_SPACES)}")
    _need_gpu(eq_f32, rows_f32, list_off, row_ids, probes)
    dev = eq_f32.device
    for t, name in ((eq_f32, "eq_f32"), (rows_f32, "rows_f32")):
        if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"{what}: {name} must be float32 [rows, d] with unit inner stride")
    Q, d = eq_f32.shape
    N = rows_f32.shape[0]
    if rows_f32.shape[1] != d:
        raise ValueError(f"{what}: query rows are {d} wide, stored rows {rows_f32.shape[1]}")
    if space == "l2":
        _l2_dim(d, what)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{what}: k={k} outside 1..{MAX_K}")
    if list_off.dtype != torch.int64 or list_off.dim() != 1 or list_off.numel() < 2 or not list_off.is_contiguous():
        raise ValueError(f"{what}: list_off must be a contiguous int64 [nlist + 1] tensor")
    nlist = list_off.numel() - 1
    if row_ids.dtype != torch.int32 or row_ids.shape != (N,) or not row_ids.is_contiguous():
        raise ValueError(f"{what}: row_ids must be a contiguous int32 [{N}] tensor")
    if probes.dtype != torch.int64 or probes.dim() != 2 or probes.shape[0] != Q or probes.shape[1] < 1 or not probes.is_contiguous():
        raise ValueError(f"{what}: probes must be a contiguous int64 [{Q}, nprobe >= 1] tensor")
    nprobe = probes.shape[1]
    hint = max(1, N // nlist) if max_list_len is None else int(max_list_len)
    if hint < 0:
        raise ValueError(f"{what}: max_list_len={hint} < 0")
    scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
    idx = torch.empty((Q, k), dtype=torch.int64, device=dev)
    status = torch.zeros((Q,), dtype=torch.int32, device=dev) if return_status else None
    if Q == 0:
        return (scores, idx, status) if return_status else (scores, idx)
    if N == 0:
        raise ValueError(f"{what}: no rows")
    L = _lib.lib()
    ldq, ldr = _row_stride(eq_f32), _row_stride(rows_f32)
    with torch.cuda.device(dev):
        step = min(Q, MAX_QUERIES_PER_CALL)
        nbytes = L.tsim_ivf_scan_workspace_bytes(step, nprobe, hint, k)
        while step > 1 and nbytes > IVF_MAX_WORKSPACE + 1024:      # (+ the flag word and the alignment of the two halves)
            step = (step + 1) // 2
            nbytes = L.tsim_ivf_scan_workspace_bytes(step, nprobe, hint, k)
        ws = _workspace(dev, nbytes)
        for q0 in range(0, Q, step):
            nq = min(step, Q - q0)
            rc = L.tsim_ivf_scan_topk(IVF_SPACES[space], eq_f32.data_ptr() + q0 * ldq * 4, ldq, nq, rows_f32.data_ptr(), ldr, N, d,
                                      list_off.data_ptr(), nlist, row_ids.data_ptr(), probes.data_ptr() + q0 * nprobe * 8, nprobe, hint,
                                      k, scores.data_ptr() + q0 * k * 4, idx.data_ptr() + q0 * k * 8, idx_offset,
                                      status.data_ptr() + q0 * 4 if return_status else 0, ws.data_ptr(), ws.numel(), _stream(eq_f32))
            _lib.check(rc, what)
    return (scores, idx, status) if return_status else (scores, idx)


# ------------------------------------------------------------------------------------------------- graph index
GRAPH_ST_ROW, GRAPH_ST_ITERS = _lib.GRAPH_ST_ROW, _lib.GRAPH_ST_ITERS
GRAPH_MAX_DEGREE, GRAPH_MAX_ENTRIES, GRAPH_MAX_WIDTH, GRAPH_MAX_EF = 64, 256, 4, 1024     # include/tsim.h TSIM_GRAPH_MAX_*
GRAPH_PRUNE_MAX_K0 = 128                                                                  # TSIM_GRAPH_PRUNE_MAX_K0
GRAPH_MAX_COARSE_LISTS = _lib.GRAPH_MAX_COARSE_LISTS                                      # TSIM_GRAPH_MAX_COARSE_LISTS
GRAPH_LDS_LIMIT = _lib.GRAPH_STATIC_LDS_BYTES + _lib.GRAPH_MAX_TABLE_BYTES                # what one workgroup may take


def graph_search_lds_bytes(n_entries: int, R: int, width: int, max_iters: int) -> int:
    """LDS of one workgroup of :func:`graph_search` (include/tsim.h tsim_graph_search_lds_bytes): pure host, 0 for arguments
    out of range; a call is accepted iff this is <= GRAPH_LDS_LIMIT."""
    return int(_lib.lib().tsim_graph_search_lds_bytes(int(n_entries), int(R), int(width), int(max_iters)))


def graph_max_iters(n_entries: int, R: int, width: int) -> int:
    """The largest max_iters whose visited table fits the LDS limit: a query visits at most n_entries + max_iters width R
    rows and the table holds GRAPH_MAX_TABLE_BYTES / 8 of them."""
    return max(0, (_lib.GRAPH_MAX_TABLE_BYTES // 8 - int(n_entries)) // (int(width) * int(R)))


def graph_search(space: str, eq_f32: torch.Tensor, rows_f32: torch.Tensor, graph: torch.Tensor, entries: torch.Tensor, k: int,
                 ef: int, width: int = 4, max_iters: Optional[int] = None, row_ids: Optional[torch.Tensor] = None,
                 idx_offset: int = 0, return_status: bool = False):
    """Beam search of every query over a proximity graph (include/tsim.h tsim_graph_search states the algorithm): scores [Q,k]
    f32 and ids [Q,k] i64 ordered by (score desc, row asc) — ``space`` 'cosine' | 'dot' | 'l2' (squared distances, ascending) — with
    the bits of :func:`cosine_list_topk` / :func:`dot_list_topk` / :func:`l2_list_topk`, so a result is a subset of the exact
    search's.  ``graph`` int32 [N,R] (R <= 64; negative: padding), ``entries`` int32 [E] (E <= 256) the rows every query starts
    from, ``row_ids`` int32 [N] the id reported for each row (negative: a tombstone — traversed, never returned; None: row +
    ``idx_offset``).  ``ef`` (k <= ef <= 1024) is the beam, ``width`` (1..4) the beam entries expanded per iteration,
    ``max_iters`` the cap on iterations (default: the largest the LDS limit allows, :func:`graph_max_iters`).  An id >= N met by
    a query sets status bit ``GRAPH_ST_ROW``, a search cut by ``max_iters`` ``GRAPH_ST_ITERS``; ``return_status`` adds the int32
    [Q] status."""
    what = "graph_search"
    if space not in IVF_SPACES:
        raise ValueError(f"{what}: space {space!r}: one of {tuple(IVF_SPACES)}")
    _need_gpu(eq_f32, rows_f32, graph, entries)
    dev = eq_f32.device
    for t, name in ((eq_f32, "eq_f32"), (rows_f32, "rows_f32")):
        if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"{what}: {name} must be float32 [rows, d] with unit inner stride")
    Q, d = eq_f32.shape
    N = rows_f32.shape[0]
    if rows_f32.shape[1] != d:
        raise ValueError(f"{what}: query rows are {d} wide, stored rows {rows_f32.shape[1]}")
    if space == "l2":
        _l2_dim(d, what)
    if graph.dtype != torch.int32 or graph.dim() != 2 or graph.shape[0] != N or not graph.is_contiguous():
        raise ValueError(f"{what}: graph must be a contiguous int32 [{N}, R] tensor")
    if entries.dtype != torch.int32 or entries.dim() != 1 or not entries.is_contiguous():
        raise ValueError(f"{what}: entries must be a contiguous int32 [E] tensor")
    if row_ids is not None:
        _need_gpu(row_ids)
        if row_ids.dtype != torch.int32 or row_ids.shape != (N,) or not row_ids.is_contiguous():
            raise ValueError(f"{what}: row_ids must be a contiguous int32 [{N}] tensor")
    k, ef, width, R, E = int(k), int(ef), int(width), int(graph.shape[1]), int(entries.numel())
    if max_iters is None:
        max_iters = max(1, graph_max_iters(E, max(R, 1), min(max(width, 1), GRAPH_MAX_WIDTH)))
    scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
    idx = torch.empty((Q, k), dtype=torch.int64, device=dev)
    status = torch.zeros((Q,), dtype=torch.int32, device=dev) if return_status else None
    if Q == 0:
        return (scores, idx, status) if return_status else (scores, idx)
    if N == 0:
        raise ValueError(f"{what}: no rows")
    L = _lib.lib()
    with torch.cuda.device(dev):
        rc = L.tsim_graph_search(IVF_SPACES[space], eq_f32.data_ptr(), _row_stride(eq_f32), Q, rows_f32.data_ptr(), _row_stride(rows_f32),
                                 N, d, graph.data_ptr(), R, entries.data_ptr(), E, row_ids.data_ptr() if row_ids is not None else 0,
                                 ef, width, int(max_iters), k, scores.data_ptr(), idx.data_ptr(), idx_offset,
                                 status.data_ptr() if return_status else 0, _stream(eq_f32))
        _lib.check(rc, what)
    return (scores, idx, status) if return_status else (scores, idx)


def graph_search_seeded(space: str, eq_f32: torch.Tensor, rows_f32: torch.Tensor, graph: torch.Tensor, k: int, ef: int, *,
                        probes: Optional[torch.Tensor] = None, centroids: Optional[torch.Tensor] = None,
                        n_probe: Optional[int] = None, seeds: Optional[torch.Tensor] = None, width: int = 4,
                        max_iters: Optional[int] = None, row_ids: Optional[torch.Tensor] = None, idx_offset: int = 0,
                        return_status: bool = False, return_probes: bool = False):
    """:func:`graph_search` with entry points per QUERY, in two levels (include/tsim.h tsim_graph_search_seeded): query q starts
    from ``seeds[probes[q][p]][s]`` for all p, s.  ``seeds`` int32 [T,S] contiguous: the rows a search entering through list l
    starts from; None: a probe IS a row (S = 1, T = N) and ``probes`` is the plain [Q,E] table of entry points.  Exactly one of
    ``probes`` int32 [Q,P] (unit inner stride; rows may be strided) and ``centroids`` float32 [T,d] (T <= GRAPH_MAX_COARSE_LISTS)
    with ``n_probe`` = P: with centroids the kernel finds the probes itself, the P centroids of best score to the query ordered by
    (score desc, list asc), NaN dropped, -1 padded — the ids of the list search of the query against the centroids.  1 <= P S <=
    256.  A negative probe or seed is padding; a probe >= T or a seed >= N is never dereferenced and sets ``GRAPH_ST_ROW``.
    ``max_iters`` defaults to ``graph_max_iters(P S, R, width)``.  ``return_probes`` adds the int32 [Q,P] probes used.  Everything
    else is :func:`graph_search`'s."""
    what = "graph_search_seeded"
    if space not in IVF_SPACES:
        raise ValueError(f"{what}: space {space!r}: one of {tuple(IVF_SPACES)}")
    if (probes is None) == (centroids is None):
        raise ValueError(f"{what}: exactly one of probes and centroids must be given")
    _need_gpu(eq_f32, rows_f32, graph)
    dev = eq_f32.device
    for t, name in ((eq_f32, "eq_f32"), (rows_f32, "rows_f32")) + (((centroids, "centroids"),) if centroids is not None else ()):
        if t.dtype != torch.float32 or t.dim() != 2 or t.stride(1) != 1:
            raise ValueError(f"{what}: {name} must be float32 [rows, d] with unit inner stride")
    Q, d = eq_f32.shape
    N = rows_f32.shape[0]
    if rows_f32.shape[1] != d:
        raise ValueError(f"{what}: query rows are {d} wide, stored rows {rows_f32.shape[1]}")
    if space == "l2":
        _l2_dim(d, what)
    if graph.dtype != torch.int32 or graph.dim() != 2 or graph.shape[0] != N or not graph.is_contiguous():
        raise ValueError(f"{what}: graph must be a contiguous int32 [{N}, R] tensor")
    T, S = N, 1
    if seeds is not None:
        _need_gpu(seeds)
        if seeds.dtype != torch.int32 or seeds.dim() != 2 or not seeds.is_contiguous():
            raise ValueError(f"{what}: seeds must be a contiguous int32 [T, S] tensor")
        T, S = int(seeds.shape[0]), int(seeds.shape[1])
    if probes is not None:
        _need_gpu(probes)
        if probes.dtype != torch.int32 or probes.dim() != 2 or probes.shape[0] != Q or probes.stride(1) != 1:
            raise ValueError(f"{what}: probes must be int32 [{Q}, P] with unit inner stride")
        if n_probe is not None and int(n_probe) != probes.shape[1]:
            raise ValueError(f"{what}: n_probe={n_probe}, probes hold {probes.shape[1]} a query")
        P = int(probes.shape[1])
    else:
        _need_gpu(centroids)
        if n_probe is None:
            raise ValueError(f"{what}: centroids need n_probe")
        if centroids.shape != (T, d):
            raise ValueError(f"{what}: centroids must have shape ({T}, {d}), got {tuple(centroids.shape)}")
        P = int(n_probe)
    if row_ids is not None:
        _need_gpu(row_ids)
        if row_ids.dtype != torch.int32 or row_ids.shape != (N,) or not row_ids.is_contiguous():
            raise ValueError(f"{what}: row_ids must be a contiguous int32 [{N}] tensor")
    k, ef, width, R = int(k), int(ef), int(width), int(graph.shape[1])
    if max_iters is None:
        max_iters = max(1, graph_max_iters(P * S, max(R, 1), min(max(width, 1), GRAPH_MAX_WIDTH)))
    scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
    idx = torch.empty((Q, k), dtype=torch.int64, device=dev)
    status = torch.zeros((Q,), dtype=torch.int32, device=dev) if return_status else None
    used = torch.full((Q, max(P, 0)), -1, dtype=torch.int32, device=dev) if return_probes else None
    out = (scores, idx) + ((status,) if return_status else ()) + ((used,) if return_probes else ())
    if Q == 0:
        return out
    if N == 0:
        raise ValueError(f"{what}: no rows")
    L = _lib.lib()
    with torch.cuda.device(dev):
        rc = L.tsim_graph_search_seeded(IVF_SPACES[space], eq_f32.data_ptr(), _row_stride(eq_f32), Q, rows_f32.data_ptr(),
                                        _row_stride(rows_f32), N, d, graph.data_ptr(), R, seeds.data_ptr() if seeds is not None else 0, T,
                                        S, probes.data_ptr() if probes is not None else 0,
                                        _row_stride(probes) if probes is not None else 0, P,
                                        centroids.data_ptr() if centroids is not None else 0,
                                        _row_stride(centroids) if centroids is not None else 0,
                                        row_ids.data_ptr() if row_ids is not None else 0, ef, width, int(max_iters), k, scores.data_ptr(),
                                        idx.data_ptr(), idx_offset, status.data_ptr() if return_status else 0,
                                        used.data_ptr() if return_probes else 0, _stream(eq_f32))
        _lib.check(rc, what)
    return out


def graph_prune(knn: torch.Tensor, R: int, return_detours: bool = False):
    """The forward lists [N,R] int32 of an exact kNN graph ``knn`` int32 [N,K0] (K0 <= 128, best first): the R entries of each
    row with the fewest two-hop detours through better-ranked neighbours, ties by rank (include/tsim.h tsim_graph_prune; CAGRA's
    rank-based pruning).  ``return_detours`` adds the counts [N,K0] int32."""
    what = "graph_prune"
    _need_gpu(knn)
    if knn.dtype != torch.int32 or knn.dim() != 2 or not knn.is_contiguous():
        raise ValueError(f"{what}: knn must be a contiguous int32 [N, K0] tensor")
    N, K0 = knn.shape
    fwd = torch.empty((N, int(R)), dtype=torch.int32, device=knn.device)
    det = torch.empty((N, K0), dtype=torch.int32, device=knn.device) if return_detours else None
    if N:
        with torch.cuda.device(knn.device):
            rc = _lib.lib().tsim_graph_prune(knn.data_ptr(), N, K0, int(R), fwd.data_ptr(), det.data_ptr() if return_detours else 0,
                                             _stream(knn))
            _lib.check(rc, what)
    return (fwd, det) if return_detours else fwd


def graph_merge_reverse(fwd: torch.Tensor) -> torch.Tensor:
    """The final graph rows [N,R] int32 of forward lists ``fwd`` [N,R]: row j is the first R distinct ids of fwd[j][:R/2] ++
    Rev[j][:R/2] ++ fwd[j][R/2:], -1 padded, where Rev[j] lists the sources i of the edges i -> j ordered by (the position of j in
    fwd[i], i).  Integers only (torch stable sorts on the tensor's device), so it is exact by construction."""
    N, R = fwd.shape
    h = R // 2
    dev = fwd.device
    F = fwd.to(torch.int64)
    dst = F.t().reshape(-1)                                     # edges in (position, source) order
    src = torch.arange(N, device=dev).repeat(R)
    ok = dst >= 0
    dst, src = dst[ok], src[ok]
    dst, o = torch.sort(dst, stable=True)
    src = src[o]
    start = torch.searchsorted(dst, torch.arange(N, device=dev))
    rank = torch.arange(dst.numel(), device=dev) - start[dst]
    rev = torch.full((N, max(h, 1)), -1, dtype=torch.int64, device=dev)
    keep = rank < h
    rev[dst[keep], rank[keep]] = src[keep]
    cat = torch.cat([F[:, :h], rev[:, :h], F[:, h:]], dim=1)
    sv, o = torch.sort(cat, dim=1, stable=True)
    dup_sorted = torch.zeros_like(sv, dtype=torch.bool)
    dup_sorted[:, 1:] = sv[:, 1:] == sv[:, :-1]
    dup = torch.zeros_like(dup_sorted).scatter_(1, o, dup_sorted)
    good = (cat >= 0) & ~dup
    place = torch.cumsum(good, dim=1) - 1
    sel = good & (place < R)
    out = torch.full((N, R), -1, dtype=torch.int64, device=dev)
    rows = torch.arange(N, device=dev)[:, None].expand_as(cat)
    out[rows[sel], place[sel]] = cat[sel]
    return out.to(torch.int32)


# ------------------------------------------------------------------------------------------------- graph index: insertion
GRAPH_INSERT_ST_ROW = _lib.GRAPH_INSERT_ST_ROW                  # include/tsim_graph_insert.h
GRAPH_LINK_POOL = _lib.GRAPH_LINK_POOL
GRAPH_LINK_ST_CUT, GRAPH_LINK_ST_ROW, GRAPH_LINK_ST_LIMS = _lib.GRAPH_LINK_ST_CUT, _lib.GRAPH_LINK_ST_ROW, _lib.GRAPH_LINK_ST_LIMS


def graph_insert_prune(cand: torch.Tensor, graph: torch.Tensor, R: Optional[int] = None, return_detours: bool = False):
    """The forward rows [B,R] int32 of B new rows n .. n + B - 1 from their candidates ``cand`` int32 [B,K0] (best first, -1 padded)
    over the graph ``graph`` int32 [n,R] of the rows before them (include/tsim_graph_insert.h tsim_graph_insert_prune):
    :func:`graph_prune`'s detour rule with the neighbour lists that exist at insertion time — ``graph[c]`` for an old candidate,
    the first R candidates of a batch row.  Returns (forward, status [B] int32) — ``GRAPH_INSERT_ST_ROW`` where a row held an id
    >= n + B — with the counts [B,K0] int32 in between when ``return_detours``.  ``R`` defaults to the graph's degree (and must be
    it)."""
    what = "graph_insert_prune"
    _need_gpu(cand, graph)
    if cand.dtype != torch.int32 or cand.dim() != 2 or not cand.is_contiguous():
        raise ValueError(f"{what}: cand must be a contiguous int32 [B, K0] tensor")
    if graph.dtype != torch.int32 or graph.dim() != 2 or not graph.is_contiguous():
        raise ValueError(f"{what}: graph must be a contiguous int32 [n, R] tensor")
    B, K0 = cand.shape
    n = int(graph.shape[0])
    if R is not None and int(R) != graph.shape[1]:
        raise ValueError(f"{what}: R={R}, the graph's rows hold {graph.shape[1]}")
    R = int(graph.shape[1])
    fwd = torch.empty((B, R), dtype=torch.int32, device=cand.device)
    det = torch.empty((B, K0), dtype=torch.int32, device=cand.device) if return_detours else None
    status = torch.zeros((B,), dtype=torch.int32, device=cand.device)
    if B:
        if n == 0:
            raise ValueError(f"{what}: no graph rows")
        with torch.cuda.device(cand.device):
            rc = _lib.lib().tsim_graph_insert_prune(cand.data_ptr(), B, K0, graph.data_ptr(), n, R, fwd.data_ptr(),
                                                    det.data_ptr() if return_detours else 0, status.data_ptr(), _stream(cand))
            _lib.check(rc, what)
    return (fwd, det, status) if return_detours else (fwd, status)


def graph_link_reverse(space: str, rows_f32: torch.Tensor, graph: torch.Tensor, targets: torch.Tensor, in_lims: torch.Tensor,
                       in_ids: torch.Tensor) -> torch.Tensor:
    """Link incoming rows into the graph rows of ``targets``, IN PLACE (include/tsim_graph_insert.h tsim_graph_link_reverse):
    target t keeps the first R/2 of its valid entries; its other entries and its incoming rows ``in_ids[in_lims[j] :
    in_lims[j + 1]]`` (int32 / int64 [T+1], CSR in the targets' order) — without ids already kept and without repeats, the first
    ``GRAPH_LINK_POOL`` of them — compete for the other R - R/2 places by their exact score against row t, the order and bits of
    the list searches.  ``targets`` int32 [T]: distinct rows.  ``graph`` int32 [N,R] contiguous, updated; ``rows_f32`` [N,d].
    Returns the status [T] int32: ``GRAPH_LINK_ST_CUT`` / ``_ROW`` / ``_LIMS``."""
    what = "graph_link_reverse"
    if space not in IVF_SPACES:
        raise ValueError(f"{what}: space {space!r}: one of {tuple(IVF_SPACES)}")
    _need_gpu(rows_f32, graph, targets, in_lims, in_ids)
    if rows_f32.dtype != torch.float32 or rows_f32.dim() != 2 or rows_f32.stride(1) != 1:
        raise ValueError(f"{what}: rows_f32 must be float32 [rows, d] with unit inner stride")
    N, d = rows_f32.shape
    if space == "l2":
        _l2_dim(d, what)
    if graph.dtype != torch.int32 or graph.dim() != 2 or graph.shape[0] != N or not graph.is_contiguous():
        raise ValueError(f"{what}: graph must be a contiguous int32 [{N}, R] tensor")
    if targets.dtype != torch.int32 or targets.dim() != 1 or not targets.is_contiguous():
        raise ValueError(f"{what}: targets must be a contiguous int32 [T] tensor")
    T = int(targets.numel())
    if in_lims.dtype != torch.int64 or in_lims.shape != (T + 1,) or not in_lims.is_contiguous():
        raise ValueError(f"{what}: in_lims must be a contiguous int64 [{T + 1}] tensor")
    if in_ids.dtype != torch.int32 or in_ids.dim() != 1 or not in_ids.is_contiguous():
        raise ValueError(f"{what}: in_ids must be a contiguous int32 [in_lims[T]] tensor")
    status = torch.zeros((T,), dtype=torch.int32, device=graph.device)
    if T:
        if in_ids.numel() == 0:      # (nothing comes in, but a row may still be re-ranked: the kernel wants a pointer)
            in_ids = torch.zeros((1,), dtype=torch.int32, device=graph.device)
        with torch.cuda.device(graph.device):
            rc = _lib.lib().tsim_graph_link_reverse(IVF_SPACES[space], rows_f32.data_ptr(), _row_stride(rows_f32), N, d, graph.data_ptr(),
                                                    int(graph.shape[1]), targets.data_ptr(), T, in_lims.data_ptr(), in_ids.data_ptr(),
                                                    status.data_ptr(), _stream(graph))
            _lib.check(rc, what)
    return status


_LIST_TOPK = {"cosine": "cosine_list_topk", "dot": "dot_list_topk", "l2": "l2_list_topk"}


def graph_insert_candidates(space: str, rows_f32: torch.Tensor, n: int, old_scores: torch.Tensor, old_idx: torch.Tensor, K0: int):
    """Step 1 of :func:`graph_insert` behind the beam search: ``old_scores`` / ``old_idx`` [b,K0] are what the search of the new
    rows ``rows_f32[n:]`` over the graph returned (rows, -1 padded).  Each new row's exact best ``min(K0 + 1, b)`` among the b new
    rows come from the space's list search (ids n + j), the row itself dropped by the build's rule — itself, or the last entry when
    duplicates pushed it out — and the candidates int32 [b,K0] are the first K0 of both by (score desc, id asc), 'l2' (dist^2 asc,
    id asc), -1 padded.  Both searches return the same exact float32 scores, so the merge compares like with like."""
    dev = rows_f32.device
    new = rows_f32[n:]
    b = new.shape[0]
    kn = min(int(K0) + 1, b)
    s, i = globals()[_LIST_TOPK[space]](new, new, torch.arange(b, dtype=torch.int32, device=dev), None, kn, idx_offset=n,
                                        assume_unique=True)
    own = i == (n + torch.arange(b, device=dev))[:, None]
    drop = torch.where(own.any(1), own.to(torch.int8).argmax(1), torch.full((b,), kn - 1, device=dev))
    keep = torch.arange(kn, device=dev)[None, :] != drop[:, None]
    s, i = s[keep].view(b, kn - 1), i[keep].view(b, kn - 1)
    ids = torch.cat([old_idx, i], dim=1)
    sc = torch.cat([old_scores, s], dim=1)
    # three stable sorts, the last key first: id, then score, then padding behind everything real
    o = torch.sort(ids, dim=1, stable=True)[1]
    ids, sc = ids.gather(1, o), sc.gather(1, o)
    o = torch.sort(sc, dim=1, stable=True, descending=space != "l2")[1]
    ids, sc = ids.gather(1, o), sc.gather(1, o)
    o = torch.sort((ids < 0).to(torch.int8), dim=1, stable=True)[1]
    ids = ids.gather(1, o)[:, :int(K0)]
    if ids.shape[1] < int(K0):
        ids = torch.cat([ids, torch.full((b, int(K0) - ids.shape[1]), -1, dtype=ids.dtype, device=dev)], dim=1)
    return ids.to(torch.int32).contiguous()


def graph_insert_incoming(forward: torch.Tensor, n: int):
    """(targets int32 [T], in_lims int64 [T+1], in_ids int32) of the forward rows ``forward`` [b,R] of the new rows n .. n + b - 1:
    the sorted distinct rows some new row chose, and for each the new rows that chose it ordered by (the position of the target in
    the chooser's forward row, chooser) — :func:`graph_merge_reverse`'s order.  Integers only (a stable sort on the device)."""
    b, R = forward.shape
    dev = forward.device
    dst = forward.t().reshape(-1)                                 # edges in (position, chooser) order
    src = (int(n) + torch.arange(b, dtype=torch.int32, device=dev)).repeat(R)
    ok = dst >= 0
    dst, src = dst[ok], src[ok]
    dst, o = torch.sort(dst, stable=True)
    targets, counts = torch.unique_consecutive(dst, return_counts=True)
    lims = torch.zeros((targets.numel() + 1,), dtype=torch.int64, device=dev)
    lims[1:] = torch.cumsum(counts, 0)
    return targets.to(torch.int32).contiguous(), lims, src[o].contiguous()


def graph_insert(space: str, rows_f32: torch.Tensor, graph: torch.Tensor, n: int, K0: int, *, entries: Optional[torch.Tensor] = None,
                 seeded: Optional[dict] = None, width: int = 4, max_iters: Optional[int] = None,
                 row_ids: Optional[torch.Tensor] = None, ef: Optional[int] = None):
    """One insertion step (include/tsim_graph_insert.h): link the b new rows ``rows_f32[n:]`` into the graph over ``rows_f32[:n]``.
    ``graph`` int32 [n + b, R] contiguous holds that graph in its first n rows and is UPDATED IN PLACE: rows n .. n + b - 1 are
    written, the rows some new row chose re-ranked.
      1. candidates: :func:`graph_search` from ``entries``, or :func:`graph_search_seeded` with the keyword arguments ``seeded``
         (probes / centroids / n_probe / seeds), of the new rows over ``graph[:n]`` with ``k = K0`` and a beam of ``ef`` (default
         K0), ``width``, ``max_iters``, ``row_ids`` (int32 [n]: tombstones route and are not returned, so no new row links to
         one; the ids must be the rows), merged with the exact search among the new rows (:func:`graph_insert_candidates`);
      2. forward rows: :func:`graph_insert_prune`;
      3. reverse edges: :func:`graph_link_reverse` over the targets of :func:`graph_insert_incoming`.
    Returns (the new graph rows ``graph[n:]``, prune status [b], targets int32 [T], link status [T]).  Nothing is read back from
    the device except the sizes of the edge lists."""
    what = "graph_insert"
    if space not in IVF_SPACES:
        raise ValueError(f"{what}: space {space!r}: one of {tuple(IVF_SPACES)}")
    if (entries is None) == (seeded is None):
        raise ValueError(f"{what}: exactly one of entries and seeded must be given")
    _need_gpu(rows_f32, graph)
    n, K0 = int(n), int(K0)
    total = rows_f32.shape[0]
    if graph.dtype != torch.int32 or graph.dim() != 2 or graph.shape[0] != total or not graph.is_contiguous():
        raise ValueError(f"{what}: graph must be a contiguous int32 [{total}, R] tensor")
    if not 1 <= n < total:
        raise ValueError(f"{what}: n={n} outside 1..{total - 1}: the step needs a graph and new rows")
    R = int(graph.shape[1])
    if not R <= K0 <= GRAPH_PRUNE_MAX_K0:
        raise ValueError(f"{what}: K0={K0} outside R={R}..{GRAPH_PRUNE_MAX_K0}")
    ef = K0 if ef is None else int(ef)
    new, old, g_old = rows_f32[n:], rows_f32[:n], graph[:n]
    if entries is not None:
        s, i = graph_search(space, new, old, g_old, entries, K0, ef, width=width, max_iters=max_iters, row_ids=row_ids)
    else:
        s, i = graph_search_seeded(space, new, old, g_old, K0, ef, width=width, max_iters=max_iters, row_ids=row_ids, **seeded)
    cand = graph_insert_candidates(space, rows_f32, n, s, i, K0)
    fwd, st_prune = graph_insert_prune(cand, g_old)
    graph[n:] = fwd
    targets, lims, ids = graph_insert_incoming(fwd, n)
    st_link = graph_link_reverse(space, rows_f32, graph, targets, lims, ids)
    return graph[n:], st_prune, targets, st_link


# ------------------------------------------------------------------------------------------------- code searches: the shared frame
MAX_CODE_DIM = 1024             # include/tsim.h: 1 <= d <= 1024 for the sign-bit and the int8 codes


def _check_code_rows(what, name, t, d, dev, dtype, width_fn, made_by):
    """the row stride of a code matrix ``t``: ``dtype`` [rows, >= width_fn(d)], rows read with 16-byte loads"""
    cb = width_fn(d)
    if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or t.dim() != 2 or t.shape[1] < cb
            or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) % 16) or t.data_ptr() % 16):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            _need_gpu(t)
        kind = str(dtype).replace("torch.", "")
        raise ValueError(f"{what}: {name} must be {kind} [rows, >= {width_fn.__name__}({d})={cb}] on the device with unit inner stride, "
                         f"rows a multiple of 16 bytes apart and 16-byte aligned ({made_by})")
    if dev is not None and t.device != dev:
        raise ValueError(f"{what}: operands on different devices ({dev} vs {t.device})")
    return t.stride(0) if t.shape[0] > 1 else (t.shape[1] // 16) * 16


def _code_topk(what, rows, ws_fn_name, fn_name, q_codes, c_codes, d, k, idx_offset, out):
    """the first stage over code rows (``rows``: the code type's arguments of _check_code_rows): (value int32 [Q,k], idx int64
    [Q,k])"""
    _need_gpu(q_codes, c_codes)
    dev = q_codes.device
    ldq = _check_code_rows(what, "q_codes", q_codes, d, None, **rows)
    ldc = _check_code_rows(what, "c_codes", c_codes, d, dev, **rows)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{what}: k={k} outside 1..{MAX_K}")
    Q, N = q_codes.shape[0], c_codes.shape[0]
    if out is not None:
        val, idx = out
        _need_gpu(val, idx)
        if (val.shape != (Q, k) or idx.shape != (Q, k) or val.dtype != torch.int32 or idx.dtype != torch.int64
                or not val.is_contiguous() or not idx.is_contiguous() or val.device != dev or idx.device != dev):
            raise ValueError(f"{what}: out must be contiguous int32 / int64 [{Q}, {k}] tensors on {dev}")
    else:
        val = torch.empty((Q, k), dtype=torch.int32, device=dev)
        idx = torch.empty((Q, k), dtype=torch.int64, device=dev)
    if Q == 0:
        return val, idx
    L = _lib.lib()
    fn = getattr(L, fn_name)
    with torch.cuda.device(dev):
        step = min(Q, MAX_QUERIES_PER_CALL)
        nbytes = getattr(L, ws_fn_name)(step, N, k)
        if nbytes == 0:
            raise ValueError(f"{what}: unsupported shape Q={Q} N={N} k={k}")
        ws = _workspace(dev, nbytes)
        for q0 in range(0, Q, step):
            nq = min(step, Q - q0)
            rc = fn(q_codes.data_ptr() + q0 * ldq, ldq, nq, c_codes.data_ptr() if N else 0, ldc, N, int(d), k,
                    val.data_ptr() + q0 * k * 4, idx.data_ptr() + q0 * k * 8, idx_offset, ws.data_ptr(), ws.numel(), _stream(q_codes))
            _lib.check(rc, what)
    return val, idx


def _code_rescore(what, rows, fn_name, eq_f32, c_codes, d, cand, k, idx_offset, return_status):
    """the second stage: the float32 queries against the code rows of every query's candidates"""
    _need_gpu(eq_f32, c_codes, cand)
    dev = eq_f32.device
    if eq_f32.dtype != torch.float32 or eq_f32.dim() != 2 or eq_f32.shape[1] != d or eq_f32.stride(1) != 1:
        raise ValueError(f"{what}: eq_f32 must be float32 [Q, {d}] with unit inner stride")
    ldc = _check_code_rows(what, "c_codes", c_codes, d, dev, **rows)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{what}: k={k} outside 1..{MAX_K}")
    Q, N = eq_f32.shape[0], c_codes.shape[0]
    if cand.dim() != 2 or cand.shape[0] != Q or cand.dtype.is_floating_point or cand.dtype == torch.bool:
        raise ValueError(f"{what}: cand must hold integers [{Q}, m]")
    cand = cand.to(torch.int64).contiguous()
    m = cand.shape[1]
    scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
    idx = torch.empty((Q, k), dtype=torch.int64, device=dev)
    status = torch.zeros((Q,), dtype=torch.int32, device=dev) if return_status else None
    if Q:
        with torch.cuda.device(dev):
            rc = getattr(_lib.lib(), fn_name)(eq_f32.data_ptr(), _row_stride(eq_f32), Q, c_codes.data_ptr() if N else 0, ldc, N, int(d),
                                              cand.data_ptr() if m else 0, m, k, scores.data_ptr(), idx.data_ptr(), idx_offset,
                                              status.data_ptr() if return_status else 0, _stream(eq_f32))
            _lib.check(rc, what)
    return (scores, idx, status) if return_status else (scores, idx)


# ------------------------------------------------------------------------------------------------- binary embeddings


def code_bytes(d: int) -> int:
    """Bytes between the rows of a [rows, code_bytes(d)] uint8 code matrix: ceil(d / 8) rounded up to a multiple of 16."""
    b = _lib.lib().tsim_code_bytes(int(d))
    if b == 0:
        raise ValueError(f"binary codes take 1 <= d <= {MAX_CODE_DIM}, got d={d}")
    return b


def pack_sign_rows(x: torch.Tensor) -> torch.Tensor:
    """[rows, d] float32/bf16 -> uint8 [rows, code_bytes(d)]: the ``np.packbits(x > 0, axis=1)`` bytes of every row (element 8j
    is bit 7 of byte j; sentence-transformers' ``precision="ubinary"``), zero from byte ceil(d / 8) on.  The bit is ``x > 0``:
    0.0, -0.0, NaN, -inf and negative subnormals give 0.  Strided row views are read in place."""
    _need_gpu(x)
    if x.dim() != 2:
        raise ValueError("pack_sign_rows expects a 2-D tensor")
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    rows, d = x.shape
    cb = code_bytes(d)
    out = torch.empty((rows, cb), dtype=torch.uint8, device=x.device)
    dt = _lib.TSIM_F32 if x.dtype == torch.float32 else _lib.TSIM_BF16
    if rows:
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().tsim_pack_sign_rows(x.data_ptr(), dt, rows, d, _row_stride(x), out.data_ptr(), cb, _stream(x)),
                       "pack_sign_rows")
    return out


def codes_from_packbits(a, d: int, device=None) -> torch.Tensor:
    """A ``[rows, ceil(d / 8)]`` uint8 array or tensor (``np.packbits(x > 0, axis=1)``, ``encode_text(precision="ubinary")``,
    sentence-transformers' ubinary embeddings) -> the padded device layout uint8 [rows, code_bytes(d)].  A numpy array goes to
    ``device`` (default: the current one); the unused bits of the last byte are cleared."""
    cb = code_bytes(d)
    nb = (int(d) + 7) // 8
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a)).to(device if device is not None else torch.device("cuda"))
    _need_gpu(a)
    if a.dtype != torch.uint8 or a.dim() != 2 or a.shape[1] != nb:
        raise ValueError(f"codes_from_packbits: expected uint8 [rows, {nb}] for d={d}, got {a.dtype} {tuple(a.shape)}")
    out = torch.zeros((a.shape[0], cb), dtype=torch.uint8, device=a.device)
    out[:, :nb] = a
    if d % 8:
        out[:, nb - 1] &= (0xFF00 >> (d % 8)) & 0xFF
    return out


_BINARY_ROWS = dict(dtype=torch.uint8, width_fn=code_bytes, made_by="pack_sign_rows / codes_from_packbits")


def hamming_topk(q_codes: torch.Tensor, c_codes: torch.Tensor, d: int, k: int, idx_offset: int = 0,
                 out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """Exact Hamming top-k over the first ``d`` bits of the code rows: dist [Q,k] int32, idx [Q,k] int64, ordered by
    (distance asc, row asc); fewer than k rows are padded with (2**31 - 1, -1), as faiss' ``IndexBinaryFlat`` pads.
    ``q_codes`` / ``c_codes``: uint8 from :func:`pack_sign_rows` or :func:`codes_from_packbits` (row views with a stride that is
    a multiple of 16 bytes are read in place; bits at positions >= d are ignored).  1 <= k <= 1024, 1 <= d <= 1024.  Query sets
    above MAX_QUERIES_PER_CALL rows are searched in slices.  ``out`` = (dist, idx): preallocated contiguous tensors."""
    return _code_topk("hamming_topk", _BINARY_ROWS, "tsim_hamming_topk_workspace_bytes", "tsim_hamming_topk", q_codes, c_codes, d, k,
                      idx_offset, out)


def sign_rescore_topk(eq_f32: torch.Tensor, c_codes: torch.Tensor, d: int, cand: torch.Tensor, k: int, idx_offset: int = 0,
                      return_status: bool = False):
    """The second stage of a binary search: every query's candidates ``cand`` [Q, m] (row numbers; the ``idx`` of
    :func:`hamming_topk` as it stands) scored with the FLOAT32 query against the +-1 expansion of the code rows, scores [Q,k] f32
    and idx [Q,k] i64 ordered by (score desc, row asc), padded with (-inf, -1).  score = float32(sum_j q_j (2 bit_j - 1)) summed
    in float64 in the library's canonical order — for d <= 768 the bits of :func:`dot_list_topk` on the unpacked matrix.
    Negative entries are skipped; entries >= N are skipped and set ``LIST_ST_ROW`` in the status (``return_status``); a row
    listed twice is returned twice."""
    return _code_rescore("sign_rescore_topk", _BINARY_ROWS, "tsim_sign_rescore_topk", eq_f32, c_codes, d, cand, k, idx_offset,
                         return_status)


# ------------------------------------------------------------------------------------------------- int8 embeddings
def int8_bytes(d: int) -> int:
    """Bytes between the rows of a [rows, int8_bytes(d)] int8 code matrix: d rounded up to a multiple of 16."""
    b = _lib.lib().tsim_int8_bytes(int(d))
    if b == 0:
        raise ValueError(f"int8 codes take 1 <= d <= {MAX_CODE_DIM}, got d={d}")
    return b


_INT8_ROWS = dict(dtype=torch.int8, width_fn=int8_bytes, made_by="quantize_int8_rows / int8_codes_from_numpy")


def int8_ranges(x: torch.Tensor) -> torch.Tensor:
    """The calibration ranges of sentence-transformers' ``quantize_embeddings(precision="int8")``: float32 [2, d], row 0 the
    per-column minimum of ``x`` [rows, d], row 1 the maximum.  Once per corpus; not on the search path."""
    _need_gpu(x)
    if x.dim() != 2 or x.shape[0] == 0 or not x.dtype.is_floating_point:
        raise ValueError("int8_ranges expects a non-empty 2-D float tensor")
    x = x.float()
    return torch.stack([torch.amin(x, dim=0), torch.amax(x, dim=0)]).contiguous()


def _check_ranges(what, ranges, d, dev):
    if not isinstance(ranges, torch.Tensor):
        ranges = torch.as_tensor(np.asarray(ranges, dtype=np.float32), device=dev)
    _need_gpu(ranges)
    if ranges.dim() != 2 or tuple(ranges.shape) != (2, d) or not ranges.dtype.is_floating_point:
        raise ValueError(f"{what}: ranges must be float [2, {d}] (per-column minimum and maximum), got {ranges.dtype} {tuple(ranges.shape)}")
    if ranges.device != dev:
        raise ValueError(f"{what}: operands on different devices ({dev} vs {ranges.device})")
    return ranges.to(torch.float32).contiguous()


def quantize_int8_rows(x: torch.Tensor, ranges, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[rows, d] float32 -> int8 [rows, int8_bytes(d)]: sentence-transformers' ``quantize_embeddings(x, "int8", ranges=ranges)``
    in float32 — ``((x - ranges[0]) / ((ranges[1] - ranges[0]) / 255) - 128).astype(np.int8)`` — zero from column d on.  Where
    numpy's cast is undefined the value saturates to [-128, 127] (+-inf included) and NaN gives 0.  Strided row views are read
    in place.  ``out``: an int8 [rows, >= int8_bytes(d)] tensor (or row view, stride a multiple of 16) whose first int8_bytes(d)
    columns are written."""
    what = "quantize_int8_rows"
    _need_gpu(x)
    if x.dim() != 2:
        raise ValueError(f"{what} expects a 2-D tensor")
    if not x.dtype.is_floating_point:
        raise ValueError(f"{what} expects float rows, got {x.dtype}")
    if x.dtype != torch.float32:
        x = x.float()
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    rows, d = x.shape
    cb = int8_bytes(d)
    ranges = _check_ranges(what, ranges, d, x.device)
    if out is None:
        out = torch.empty((rows, cb), dtype=torch.int8, device=x.device)
        ld = cb
    else:
        ld = _check_code_rows(what, "out", out, d, x.device, **_INT8_ROWS)
        if out.shape[0] != rows:
            raise ValueError(f"{what}: out has {out.shape[0]} rows, x {rows}")
    if rows:
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().tsim_quantize_int8_rows(x.data_ptr(), rows, d, _row_stride(x), ranges.data_ptr(), out.data_ptr(), ld,
                                                          _stream(x)), what)
    return out


def int8_codes_from_numpy(a, d: int, device=None) -> torch.Tensor:
    """A ``[rows, d]`` int8 array or tensor (sentence-transformers' int8 embeddings, ``encode_text(precision="int8")``) -> the
    padded device layout int8 [rows, int8_bytes(d)], zero from column d on.  A numpy array goes to ``device`` (default: the
    current one)."""
    cb = int8_bytes(d)
    if isinstance(a, np.ndarray):
        if a.dtype != np.int8:
            raise ValueError(f"int8_codes_from_numpy: expected int8 [rows, {d}], got {a.dtype} {a.shape}")
        a = torch.from_numpy(np.ascontiguousarray(a)).to(device if device is not None else torch.device("cuda"))
    _need_gpu(a)
    if a.dtype != torch.int8 or a.dim() != 2 or a.shape[1] != int(d):
        raise ValueError(f"int8_codes_from_numpy: expected int8 [rows, {d}], got {a.dtype} {tuple(a.shape)}")
    out = torch.zeros((a.shape[0], cb), dtype=torch.int8, device=a.device)
    out[:, :int(d)] = a
    return out


def int8_ip_topk(q_codes: torch.Tensor, c_codes: torch.Tensor, d: int, k: int, idx_offset: int = 0,
                 out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """Exact inner-product top-k over the first ``d`` values of int8 code rows: score [Q,k] int32 = sum_j q_j c_j, idx [Q,k]
    int64, ordered by (score desc, row asc); fewer than k rows are padded with (-2**31, -1).  ``q_codes`` / ``c_codes``: int8
    from :func:`quantize_int8_rows` or :func:`int8_codes_from_numpy` (row views with a stride that is a multiple of 16 bytes are
    read in place; bytes at positions >= d are ignored).  1 <= k <= 1024, 1 <= d <= 1024.  Query sets above
    MAX_QUERIES_PER_CALL rows are searched in slices.  ``out`` = (score, idx): preallocated contiguous tensors."""
    return _code_topk("int8_ip_topk", _INT8_ROWS, "tsim_int8_ip_topk_workspace_bytes", "tsim_int8_ip_topk", q_codes, c_codes, d, k,
                      idx_offset, out)


def int8_rescore_topk(eq_f32: torch.Tensor, c_codes: torch.Tensor, d: int, cand: torch.Tensor, k: int, idx_offset: int = 0,
                      return_status: bool = False):
    """The second stage of an int8 search: every query's candidates ``cand`` [Q, m] (row numbers; the ``idx`` of
    :func:`int8_ip_topk` as it stands) scored with the FLOAT32 query against the int8 code rows, scores [Q,k] f32 and idx [Q,k]
    i64 ordered by (score desc, row asc), padded with (-inf, -1).  score = float32(sum_j q_j c_j) summed in float64 in the
    library's canonical order — for d <= 768 the bits of :func:`dot_list_topk` on ``c_codes.float()``.  Negative entries are
    skipped; entries >= N are skipped and set ``LIST_ST_ROW`` in the status (``return_status``); a row listed twice is returned
    twice."""
    return _code_rescore("int8_rescore_topk", _INT8_ROWS, "tsim_int8_rescore_topk", eq_f32, c_codes, d, cand, k, idx_offset,
                         return_status)


# ------------------------------------------------------------------------------------------------- product quantisation
PQ_MAX_M = 64                   # include/tsim.h: 1 <= M <= 64 sub-quantisers of 256 centroids, d % M == 0, d / M <= 64
PQ_MAX_DSUB = 64
PQ_SPACES = {"ip": _lib.SPACE_DOT, "l2": _lib.SPACE_L2}
PQ_TABLE_BUDGET = 64 << 20      # int32 tables of one call (M KiB a query): larger query sets are searched in slices
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def pq_code_bytes(M: int) -> int:
    """Bytes between the rows of a [rows, pq_code_bytes(M)] uint8 PQ code matrix: M rounded up to a multiple of 16."""
    b = _lib.lib().tsim_pq_code_bytes(int(M))
    if b == 0:
        raise ValueError(f"PQ codes take 1 <= M <= {PQ_MAX_M}, got M={M}")
    return b


_PQ_ROWS = dict(dtype=torch.uint8, width_fn=pq_code_bytes, made_by="pq_encode_rows / pq_codes_from_numpy")


def _check_codebooks(what, codebooks, dev, d=None, trusted=False):
    """float32 [M, 256, dsub] contiguous and finite on ``dev`` -> (codebooks, d, M).  ``trusted``: the caller (GpuPQIndex) has
    checked these codebooks for finiteness where they entered, so the search path does not read the device back."""
    if not isinstance(codebooks, torch.Tensor):
        codebooks = torch.as_tensor(np.asarray(codebooks, dtype=np.float32))
    if codebooks.dim() != 3 or codebooks.shape[1] != 256 or not codebooks.dtype.is_floating_point:
        raise ValueError(f"{what}: codebooks must be float [M, 256, dsub], got {codebooks.dtype} {tuple(codebooks.shape)}")
    M, dsub = codebooks.shape[0], codebooks.shape[2]
    if not (1 <= M <= PQ_MAX_M and 1 <= dsub <= PQ_MAX_DSUB and M * dsub <= MAX_CODE_DIM):
        raise ValueError(f"{what}: codebooks [M={M}, 256, dsub={dsub}] need 1 <= M <= {PQ_MAX_M}, dsub <= {PQ_MAX_DSUB} and "
                         f"M dsub <= {MAX_CODE_DIM}")
    if d is not None and M * dsub != d:
        raise ValueError(f"{what}: rows of width {d} against codebooks for width {M * dsub}")
    if not codebooks.is_cuda:
        _need_gpu(codebooks)
    if dev is not None and codebooks.device != dev:
        raise ValueError(f"{what}: operands on different devices ({dev} vs {codebooks.device})")
    codebooks = codebooks.to(torch.float32).contiguous()
    if not trusted and not bool(torch.isfinite(codebooks).all()):
        raise ValueError(f"{what}: codebooks must be finite")
    return codebooks, M * dsub, M


def _pq_space(what, space):
    if space not in PQ_SPACES:
        raise ValueError(f"{what}: space must be 'ip' or 'l2', got {space!r}")
    return PQ_SPACES[space]


def pq_encode_rows(x: torch.Tensor, codebooks, out: Optional[torch.Tensor] = None, _trusted: bool = False) -> torch.Tensor:
    """[rows, d] float32/bf16 -> uint8 [rows, pq_code_bytes(M)]: byte m of a row is the number of the centroid of
    ``codebooks`` [M, 256, d / M] nearest to the row's sub-vector m, zero from byte M on.  The squared distance is summed in
    float64 in element order without FMA; ties go to the lower centroid number and a sub-vector holding a NaN or an infinity
    gets code 0.  Strided row views are read in place.  ``out``: a uint8 [rows, >= pq_code_bytes(M)] tensor (or row view, stride
    a multiple of 16) whose first pq_code_bytes(M) columns are written."""
    what = "pq_encode_rows"
    _need_gpu(x)
    if x.dim() != 2:
        raise ValueError(f"{what} expects a 2-D tensor")
    if not x.dtype.is_floating_point:
        raise ValueError(f"{what} expects float rows, got {x.dtype}")
    if x.dtype not in (torch.float32, torch.bfloat16):
        x = x.float()
    if x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.contiguous()
    rows, d = x.shape
    codebooks, _, M = _check_codebooks(what, codebooks, x.device, d, _trusted)
    cb = pq_code_bytes(M)
    if out is None:
        out = torch.empty((rows, cb), dtype=torch.uint8, device=x.device)
        ld = cb
    else:
        ld = _check_code_rows(what, "out", out, M, x.device, **_PQ_ROWS)
        if out.shape[0] != rows:
            raise ValueError(f"{what}: out has {out.shape[0]} rows, x {rows}")
    dt = _lib.TSIM_F32 if x.dtype == torch.float32 else _lib.TSIM_BF16
    if rows:
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().tsim_pq_encode_rows(x.data_ptr(), dt, rows, d, _row_stride(x), codebooks.data_ptr(), M, out.data_ptr(),
                                                      ld, _stream(x)), what)
    return out


def pq_codes_from_numpy(a, M: int, device=None) -> torch.Tensor:
    """A ``[rows, M]`` uint8 array or tensor of centroid numbers (faiss' ``ProductQuantizer.compute_codes`` with nbits = 8) -> the
    padded device layout uint8 [rows, pq_code_bytes(M)], zero from column M on.  A numpy array goes to ``device`` (default: the
    current one)."""
    cb = pq_code_bytes(M)
    if isinstance(a, np.ndarray):
        if a.dtype != np.uint8:
            raise ValueError(f"pq_codes_from_numpy: expected uint8 [rows, {M}], got {a.dtype} {a.shape}")
        a = torch.from_numpy(np.ascontiguousarray(a)).to(device if device is not None else torch.device("cuda"))
    _need_gpu(a)
    if a.dtype != torch.uint8 or a.dim() != 2 or a.shape[1] != int(M):
        raise ValueError(f"pq_codes_from_numpy: expected uint8 [rows, {M}], got {a.dtype} {tuple(a.shape)}")
    out = torch.zeros((a.shape[0], cb), dtype=torch.uint8, device=a.device)
    out[:, :int(M)] = a
    return out


def pq_decode_rows(codes: torch.Tensor, codebooks) -> torch.Tensor:
    """uint8 [rows, >= M] codes -> float32 [rows, d]: every sub-vector replaced by its centroid (a gather, no kernel of ours)."""
    _need_gpu(codes)
    codebooks, d, M = _check_codebooks("pq_decode_rows", codebooks, codes.device)
    if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[1] < M:
        raise ValueError(f"pq_decode_rows: codes must be uint8 [rows, >= {M}], got {codes.dtype} {tuple(codes.shape)}")
    sub = torch.arange(M, device=codes.device)
    return codebooks[sub, codes[:, :M].long()].reshape(codes.shape[0], d)


def _pq_queries(what, eq_f32, d):
    _need_gpu(eq_f32)
    if eq_f32.dtype != torch.float32 or eq_f32.dim() != 2 or eq_f32.shape[1] != d or eq_f32.stride(1) != 1:
        raise ValueError(f"{what}: eq_f32 must be float32 [Q, {d}] with unit inner stride")
    if eq_f32.shape[0] > 1 and eq_f32.stride(0) < d:
        eq_f32 = eq_f32.contiguous()
    return eq_f32


def pq_tables(eq_f32: torch.Tensor, codebooks, space: str, _trusted: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """The integer lookup tables of every query: (tables int32 [Q, M, 256], exps int32 [Q]).  L[m][j] in float64 is the inner
    product of the query's sub-vector m with centroid j (``space="ip"``) or minus their squared distance (``"l2"``);
    tables = rint(L 2^e) with e = 23 - ceil(log2 M) - (ilogb(max |L|) + 1) per query, so that every sum of M entries is an exact
    int32 below 2^24.  A query whose table holds a NaN or an infinity, or nothing but zeros, gets a zero table and e = 0."""
    what = "pq_tables"
    sp = _pq_space(what, space)
    _need_gpu(eq_f32)
    codebooks, d, M = _check_codebooks(what, codebooks, eq_f32.device, None, _trusted)
    eq_f32 = _pq_queries(what, eq_f32, d)
    Q = eq_f32.shape[0]
    tables = torch.empty((Q, M, 256), dtype=torch.int32, device=eq_f32.device)
    exps = torch.empty((Q,), dtype=torch.int32, device=eq_f32.device)
    if Q:
        with torch.cuda.device(eq_f32.device):
            _lib.check(_lib.lib().tsim_pq_tables(sp, eq_f32.data_ptr(), _row_stride(eq_f32), Q, codebooks.data_ptr(), d, M,
                                                 tables.data_ptr(), exps.data_ptr(), _stream(eq_f32)), what)
    return tables, exps


def pq_adc_topk_tables(tables: torch.Tensor, codes: torch.Tensor, k: int, space: str = "ip", idx_offset: int = 0):
    """The scan on its own: ``tables`` int32 [Q, M, 256] contiguous (from :func:`pq_tables`, or any whose per-query
    sum_m max_j |T[m][j]| stays within 2^24) against ``codes`` -> (value int32 [Q, k], idx int64 [Q, k]).  value = sum_m
    tables[q][m][codes[r][m]]: "ip" ordered by (value desc, row asc), padded with (-2**31, -1); "l2" (tables <= 0) returns
    -sum ordered by (value asc, row asc), padded with (2**31 - 1, -1)."""
    what = "pq_adc_topk"
    sp = _pq_space(what, space)
    _need_gpu(tables, codes)
    if tables.dtype != torch.int32 or tables.dim() != 3 or tables.shape[2] != 256 or not tables.is_contiguous():
        raise ValueError(f"{what}: tables must be contiguous int32 [Q, M, 256]")
    Q, M = tables.shape[0], tables.shape[1]
    ldc = _check_code_rows(what, "codes", codes, M, tables.device, **_PQ_ROWS)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{what}: k={k} outside 1..{MAX_K}")
    N = codes.shape[0]
    val = torch.empty((Q, k), dtype=torch.int32, device=tables.device)
    idx = torch.empty((Q, k), dtype=torch.int64, device=tables.device)
    if Q == 0:
        return val, idx
    L = _lib.lib()
    with torch.cuda.device(tables.device):
        step = min(Q, MAX_QUERIES_PER_CALL)
        nbytes = L.tsim_pq_adc_topk_workspace_bytes(step, N, M, k)
        if nbytes == 0:
            raise ValueError(f"{what}: unsupported shape Q={Q} N={N} M={M} k={k}")
        ws = _workspace(tables.device, nbytes)
        for q0 in range(0, Q, step):
            nq = min(step, Q - q0)
            rc = L.tsim_pq_adc_topk(sp, tables.data_ptr() + q0 * M * 1024, nq, codes.data_ptr() if N else 0, ldc, N, M, k,
                                    val.data_ptr() + q0 * k * 4, idx.data_ptr() + q0 * k * 8, idx_offset, ws.data_ptr(), ws.numel(),
                                    _stream(tables))
            _lib.check(rc, what)
    return val, idx


def pq_values_to_float(val: torch.Tensor, exps: torch.Tensor, space: str) -> torch.Tensor:
    """int32 values of :func:`pq_adc_topk_tables` and the queries' exponents -> float32(float64(v) 2^-e); padding becomes -inf
    ("ip") or +inf ("l2")."""
    pad, inf = (INT32_MIN, float("-inf")) if space == "ip" else (INT32_MAX, float("inf"))
    scale = ((1023 - exps.to(torch.int64)) << 52).view(torch.float64)     # 2^-e exactly: it need not be a float32
    f = (val.to(torch.float64) * scale[:, None]).to(torch.float32)
    return torch.where(val == pad, torch.full_like(f, inf), f)


def pq_adc_topk(eq_f32: torch.Tensor, codebooks, codes: torch.Tensor, k: int, space: str = "ip", idx_offset: int = 0,
                raw: bool = False, _trusted: bool = False):
    """Exact ADC top-k of float queries against PQ codes: (scores float32 [Q, k], idx int64 [Q, k]).  The score of a row is the
    sum of the M integer table entries its code bytes select (:func:`pq_tables`), turned back into float32(float64(v) 2^-e):
    the inner product of the query with the row's reconstruction ("ip", ordered by (score desc, row asc), padded with
    (-inf, -1)) or their squared distance ("l2", ordered by (distance asc, row asc), padded with (+inf, -1)), each within
    2^-18 or so of the table's largest entry.  The order is exact for the integer scores.  ``raw=True`` returns
    (value int32 [Q, k], idx, exps int32 [Q]) instead.  ``codes``: uint8 from :func:`pq_encode_rows` or
    :func:`pq_codes_from_numpy` (row views with a stride that is a multiple of 16 bytes are read in place; bytes at positions
    >= M are ignored).  Tables are built for PQ_TABLE_BUDGET bytes of queries at a time.

    To refine, keep the float rows and re-score the returned ``idx`` with ``ops.dot_list_topk`` / ``ops.l2_list_topk`` /
    ``ops.cosine_list_topk(eq_f32, ec_f32, cand)``: they take a first stage's candidates as they stand."""
    what = "pq_adc_topk"
    _pq_space(what, space)
    _need_gpu(eq_f32, codes)
    codebooks, d, M = _check_codebooks(what, codebooks, eq_f32.device, None, _trusted)
    eq_f32 = _pq_queries(what, eq_f32, d)
    Q = eq_f32.shape[0]
    step = max(1, min(MAX_QUERIES_PER_CALL, PQ_TABLE_BUDGET // (M * 1024)))
    vals, idxs, exps = [], [], []
    for q0 in range(0, max(Q, 1), step):
        tables, e = pq_tables(eq_f32[q0:q0 + step], codebooks, space, _trusted=True)
        v, i = pq_adc_topk_tables(tables, codes, k, space, idx_offset)
        vals.append(v), idxs.append(i), exps.append(e)
    val, idx, exp = (torch.cat(t) if len(t) > 1 else t[0] for t in (vals, idxs, exps))
    if raw:
        return val, idx, exp
    return pq_values_to_float(val, exp, space), idx


# ------------------------------------------------------------------------------------------------- IVF-PQ
IVFPQ_SEG = _lib.IVFPQ_SEG      # include/tsim.h TSIM_IVFPQ_SEG: rows of one segment of a PQ-coded inverted list
IVFPQ_TABLE_BUDGET = 256 << 20  # int32 tables of one ivfpq_search slice (l2 with residuals: nprobe M KiB a query)


def _ivfpq_lists(what, list_off, row_ids, probes, Q, N):
    if list_off.dtype != torch.int64 or list_off.dim() != 1 or list_off.numel() < 2 or not list_off.is_contiguous():
        raise ValueError(f"{what}: list_off must be a contiguous int64 [nlist + 1] tensor")
    if row_ids.dtype != torch.int32 or row_ids.shape != (N,) or not row_ids.is_contiguous():
        raise ValueError(f"{what}: row_ids must be a contiguous int32 [{N}] tensor")
    _ivfpq_probes(what, probes, Q)
    return list_off.numel() - 1


def _ivfpq_probes(what, probes, Q):
    if probes.dtype != torch.int64 or probes.dim() != 2 or probes.shape[0] != Q or probes.shape[1] < 1 or not probes.is_contiguous():
        raise ValueError(f"{what}: probes must be a contiguous int64 [{Q}, nprobe >= 1] tensor")


def ivfpq_tables(eq_f32: torch.Tensor, centroids: torch.Tensor, probes: torch.Tensor, codebooks, space: str, _trusted: bool = False):
    """The integer tables of residual PQ codes (include/tsim.h tsim_ivfpq_tables): ``(tables, bias, exps)``.  "ip": tables int32
    [Q, M, 256] as :func:`pq_tables` and bias int32 [Q, nprobe], the query's inner product with each probed centroid, on one
    exponent e = 23 - ceil(log2(M + 1)) - (ilogb(A) + 1), A the largest of the table entries and the valid probes' products.
    "l2": tables [Q, nprobe, M, 256], one per (query, probe) pair, of minus the squared distances of the residual query
    float32(q - c) to the codebook entries, on ONE exponent per query (A over all its valid pairs); bias is None.  ``probes``
    int64 [Q, nprobe], entries < 0 or >= nlist are padding (their tables are not written).  A query with a NaN or an infinity
    among its entries, or with nothing but zeros, gets zero tables, zero biases and e = 0."""
    what = "ivfpq_tables"
    sp = _pq_space(what, space)
    _need_gpu(eq_f32, centroids, probes)
    dev = eq_f32.device
    codebooks, d, M = _check_codebooks(what, codebooks, dev, None, _trusted)
    eq_f32 = _pq_queries(what, eq_f32, d)
    if centroids.dtype != torch.float32 or centroids.dim() != 2 or centroids.shape[1] != d or centroids.shape[0] < 1 \
            or centroids.stride(1) != 1 or (centroids.shape[0] > 1 and centroids.stride(0) < d):
        raise ValueError(f"{what}: centroids must be float32 [nlist >= 1, {d}] with unit inner stride")
    Q, nlist = eq_f32.shape[0], centroids.shape[0]
    _ivfpq_probes(what, probes, Q)
    nprobe = probes.shape[1]
    l2 = space == "l2"
    tables = torch.empty((Q, nprobe, M, 256) if l2 else (Q, M, 256), dtype=torch.int32, device=dev)
    bias = None if l2 else torch.empty((Q, nprobe), dtype=torch.int32, device=dev)
    exps = torch.empty((Q,), dtype=torch.int32, device=dev)
    if Q:
        L = _lib.lib()
        with torch.cuda.device(dev):
            nbytes = L.tsim_ivfpq_tables_workspace_bytes(Q, nprobe)
            if nbytes == 0:
                raise ValueError(f"{what}: unsupported shape Q={Q} nprobe={nprobe}")
            ws = _workspace(dev, nbytes) if l2 else None
            _lib.check(L.tsim_ivfpq_tables(sp, eq_f32.data_ptr(), _row_stride(eq_f32), Q, centroids.data_ptr(), _row_stride(centroids),
                                           nlist, probes.data_ptr(), nprobe, codebooks.data_ptr(), d, M, tables.data_ptr(),
                                           0 if l2 else bias.data_ptr(), exps.data_ptr(), ws.data_ptr() if l2 else 0,
                                           ws.numel() if l2 else 0, _stream(eq_f32)), what)
    return tables, bias, exps


def ivfpq_scan_topk(space: str, tables: torch.Tensor, bias: Optional[torch.Tensor], codes: torch.Tensor, list_off: torch.Tensor,
                    row_ids: torch.Tensor, probes: torch.Tensor, k: int, idx_offset: int = 0, return_status: bool = False,
                    max_list_len: Optional[int] = None):
    """Exact ADC top-k over the PQ-coded inverted lists each query probes (include/tsim.h tsim_ivfpq_scan_topk): (value int32
    [Q, k], idx int64 [Q, k]).  ``tables`` int32 contiguous, [Q, M, 256] (one a query) or [Q, nprobe, M, 256] (one a pair);
    ``bias`` int32 [Q, nprobe] or None; ``codes`` uint8 code rows in LIST order; ``list_off``, ``row_ids``, ``probes``, the status
    bits and the hint ``max_list_len`` as in :func:`ivf_scan_topk`.  value = bias + sum_m table[m][code[m]]: "ip" by (value
    desc, id asc), padded (-2**31, -1); "l2" returns -value by (value asc, id asc), padded (2**31 - 1, -1).  |bias| +
    sum_m max_j |T| must stay below 2**24."""
    what = "ivfpq_scan_topk"
    sp = _pq_space(what, space)
    _need_gpu(tables, codes, list_off, row_ids, probes)
    dev = tables.device
    if tables.dtype != torch.int32 or tables.dim() not in (3, 4) or tables.shape[-1] != 256 or not tables.is_contiguous():
        raise ValueError(f"{what}: tables must be contiguous int32 [Q, M, 256] or [Q, nprobe, M, 256]")
    per_pair = tables.dim() == 4
    Q, M = tables.shape[0], tables.shape[-2]
    N = codes.shape[0]
    ldc = _check_code_rows(what, "codes", codes, M, dev, **_PQ_ROWS)
    nlist = _ivfpq_lists(what, list_off, row_ids, probes, Q, N)
    nprobe = probes.shape[1]
    if per_pair and tables.shape[1] != nprobe:
        raise ValueError(f"{what}: tables hold {tables.shape[1]} pairs a query, probes {nprobe}")
    if bias is not None:
        _need_gpu(bias)
        if bias.dtype != torch.int32 or bias.shape != (Q, nprobe) or not bias.is_contiguous():
            raise ValueError(f"{what}: bias must be a contiguous int32 [{Q}, {nprobe}] tensor")
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"{what}: k={k} outside 1..{MAX_K}")
    hint = max(1, N // nlist) if max_list_len is None else int(max_list_len)
    if hint < 0:
        raise ValueError(f"{what}: max_list_len={hint} < 0")
    val = torch.empty((Q, k), dtype=torch.int32, device=dev)
    idx = torch.empty((Q, k), dtype=torch.int64, device=dev)
    status = torch.zeros((Q,), dtype=torch.int32, device=dev) if return_status else None
    if Q == 0:
        return (val, idx, status) if return_status else (val, idx)
    if N == 0:
        raise ValueError(f"{what}: no rows")
    L = _lib.lib()
    tstride = (nprobe if per_pair else 1) * M * 1024
    with torch.cuda.device(dev):
        step = min(Q, MAX_QUERIES_PER_CALL)
        nbytes = L.tsim_ivfpq_scan_workspace_bytes(step, nprobe, hint, k)
        while step > 1 and nbytes > IVF_MAX_WORKSPACE + 1024:      # (+ the flag word and the alignment of the two halves)
            step = (step + 1) // 2
            nbytes = L.tsim_ivfpq_scan_workspace_bytes(step, nprobe, hint, k)
        ws = _workspace(dev, nbytes)
        for q0 in range(0, Q, step):
            nq = min(step, Q - q0)
            rc = L.tsim_ivfpq_scan_topk(sp, tables.data_ptr() + q0 * tstride, int(per_pair),
                                        bias.data_ptr() + q0 * nprobe * 4 if bias is not None else 0, nq, codes.data_ptr(), ldc, N, M,
                                        list_off.data_ptr(), nlist, row_ids.data_ptr(), probes.data_ptr() + q0 * nprobe * 8, nprobe,
                                        hint, k, val.data_ptr() + q0 * k * 4, idx.data_ptr() + q0 * k * 8, idx_offset,
                                        status.data_ptr() + q0 * 4 if return_status else 0, ws.data_ptr(), ws.numel(), _stream(tables))
            _lib.check(rc, what)
    return (val, idx, status) if return_status else (val, idx)


def ivfpq_search(eq_f32: torch.Tensor, centroids: torch.Tensor, codebooks, codes: torch.Tensor, list_off: torch.Tensor,
                 row_ids: torch.Tensor, probes: torch.Tensor, k: int, space: str = "ip", by_residual: bool = True,
                 idx_offset: int = 0, max_list_len: Optional[int] = None, raw: bool = False, _trusted: bool = False,
                 table_budget: int = IVFPQ_TABLE_BUDGET):
    """IVF-PQ search of float queries: (scores float32 [Q, k], ids int64 [Q, k]) over the lists ``probes`` names, exact for the
    integer scores of :func:`ivfpq_tables` (``by_residual``) or :func:`pq_tables` (codes of the rows themselves) under (score desc,
    id asc) — "l2": (distance asc, id asc) — and turned into floats by :func:`pq_values_to_float`.  ``raw=True`` returns (value
    int32, ids, exps int32 [Q]).  The queries are searched in slices whose tables stay within ``table_budget`` bytes (l2 with
    residuals: nprobe M KiB a query); the exponent is per query, so the result does not depend on the slicing."""
    what = "ivfpq_search"
    _pq_space(what, space)
    _need_gpu(eq_f32, codes)
    codebooks, d, M = _check_codebooks(what, codebooks, eq_f32.device, None, _trusted)
    eq_f32 = _pq_queries(what, eq_f32, d)
    Q = eq_f32.shape[0]
    _ivfpq_probes(what, probes, Q)
    per_query = M * 1024 * (probes.shape[1] if by_residual and space == "l2" else 1)
    step = max(1, min(MAX_QUERIES_PER_CALL, int(table_budget) // per_query))
    vals, idxs, exps = [], [], []
    for q0 in range(0, max(Q, 1), step):
        qs, pr = eq_f32[q0:q0 + step], probes[q0:q0 + step]
        if by_residual:
            tables, bias, e = ivfpq_tables(qs, centroids, pr, codebooks, space, _trusted=True)
        else:
            (tables, e), bias = pq_tables(qs, codebooks, space, _trusted=True), None
        v, i = ivfpq_scan_topk(space, tables, bias, codes, list_off, row_ids, pr, k, idx_offset, max_list_len=max_list_len)
        vals.append(v), idxs.append(i), exps.append(e)
    val, idx, exp = (torch.cat(t) if len(t) > 1 else t[0] for t in (vals, idxs, exps))
    if raw:
        return val, idx, exp
    return pq_values_to_float(val, exp, space), idx


# ------------------------------------------------------------------------------------------------- exact range search
RANGE_SLOT_CAP = _lib.RANGE_SLOT_CAP    # include/tsim.h TSIM_RANGE_SLOT_CAP: rows one query may collect before the exact pass takes over
RANGE_MERGE_MAX_LISTS = _lib.RANGE_MERGE_MAX_LISTS    # include/tsim.h TSIM_RANGE_MERGE_MAX_LISTS: results one range_merge call joins
MAX_RANGE_QUERIES_PER_CALL = 4096       # the workspace holds RANGE_SLOT_CAP entries of 8 bytes per query: 64 MiB per call


def _f32_below(f):
    """csrc/search.hip float_below: the next float32 towards -inf of a finite f, stepping from +-0 to the smallest normal."""
    f = np.float32(f)
    if f == 0:
        return np.float32(-1.17549435e-38)
    b = f.view(np.int32)
    return (b - np.int32(1) if f > 0 else b + np.int32(1)).view(np.float32)


def range_collect_threshold(threshold, rho_q, rho_c, ld: int, nqs: Optional[float] = None):
    """Host mirror of the range search's threshold set-up kernel (csrc/range_search.h range_setup_kernel) for ONE query:
    ``(thr, eps)`` with ``eps`` = the float32 bound on |MFMA score - exact score| (csrc/common.h guard_eps) from the query's and
    the corpus' residuals, and ``thr`` the collect threshold in the MFMA domain: every row whose MFMA score is strictly above it is
    collected.  Cosine (``nqs`` None): a float32 strictly below ``threshold - eps``.  Inner product: ``nqs`` = max(|q|, 1e-8) * S
    in float64, ``thr`` strictly below ``threshold / nqs - eps``.  ``thr`` is None when no finite threshold is safe (the kernel
    then hands the query to the exact pass).  This is the executable statement of the guard: a row with exact score >=
    threshold has an MFMA score >= threshold - eps > thr."""
    f32 = np.float32
    tau = f32(threshold)
    rq, rc = float(f32(rho_q)), float(f32(rho_c))
    acc = ld * 1.1920928955078125e-7 * (1.0 + rq) * (1.0 + rc)
    eps = f32((rq + rc + rq * rc + acc + 2.384185791015625e-7) * (1.0 + 1e-6))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        if not (eps < f32(3.0e38)) or not (tau > f32(-3.0e38)):
            return None, eps
        if nqs is None:
            thr = _f32_below(f32(float(tau) - float(eps)))
            if float(thr) + float(eps) >= float(tau):
                thr = _f32_below(thr)
        else:
            nqs = float(nqs)
            if not (0.0 < nqs < float("inf")):
                return None, eps
            t = float(tau) / nqs
            lo = t - float(eps) - (abs(t) + float(eps)) * 1e-15
            if not (lo > -3.0e38):
                return None, eps
            thr = _f32_below(f32(lo))
    return (thr if thr > f32(-3.4e38) else None), eps


def _threshold_array(what, threshold, Q: int, dev):
    """None for one threshold per call (a number or a 0-dim tensor / array); else the per-query thresholds as contiguous float32 [Q] on ``dev``.  Another dtype or device is converted; another length is
    a ValueError."""
    if isinstance(threshold, (np.ndarray, list, tuple)):
        threshold = torch.as_tensor(np.asarray(threshold))
    if not isinstance(threshold, torch.Tensor) or threshold.dim() == 0:
        return None
    if threshold.dim() != 1 or threshold.shape[0] != Q:
        raise ValueError(f"{what}: a per-query threshold must have shape [{Q}] (one per query), got {tuple(threshold.shape)}")
    if threshold.is_complex() or threshold.dtype == torch.bool:
        raise ValueError(f"{what}: a per-query threshold must be real-valued, got {threshold.dtype}")
    return threshold.detach().to(device=dev, dtype=torch.float32).contiguous()


def _range(what, space, eq_unit, ec_half, d, threshold, eq_f32, ec_f32, rho_c, scale_c, idx_offset, return_status,
           centre_min: Optional[int] = None, max_members: Optional[int] = None):
    """cosine_range (scale_c is None), dot_range and l2_range (space SPACE_L2: the half rows are one element wider than the
    float32 rows, the threshold is the squared radius and the scores that come back are squared distances).
    ``centre_min`` (community_detection): only the queries with at least that many hits are materialised — the others get a
    zero-length segment in the fill's lims, which the fill never overruns (csrc/range_search.h: range_fill_kernel copies
    min(hits, segment) entries of a status-1 query, range_bf_kernel tests every position against the segment and
    range_bf_sort_kernel leaves segments of fewer than two entries alone, the status-2 path) — and the running total is held
    against ``max_members`` BEFORE the slice's output is allocated."""
    _need_gpu(eq_unit, ec_half, eq_f32, ec_f32)
    l2 = space == _lib.SPACE_L2
    if eq_unit.dtype != UNIT_DTYPE or ec_half.dtype != UNIT_DTYPE:
        raise ValueError(f"{what} expects float16 rows from " + ("l2_query_rows / l2_rows" if l2 else "l2norm_rows" +
                         (" / dot_scaled_rows" if scale_c is not None else "")))
    dw = d + 1 if l2 else d
    ld = pad_dim(dw)
    if eq_unit.shape[1] != ld or ec_half.shape[1] != ld or not eq_unit.is_contiguous() or not ec_half.is_contiguous():
        raise ValueError(f"{what}: rows must be contiguous with stride pad_dim({dw})={ld}")
    Q, N = eq_unit.shape[0], ec_half.shape[0]
    dev = eq_unit.device
    tau_q = _threshold_array(what, threshold, Q, dev)
    if tau_q is None:
        tau = float(threshold)
        if tau != tau:
            raise ValueError(f"{what}: the {'radius' if l2 else 'threshold'} is NaN")
    for t, rows, name in ((eq_f32, Q, "eq_f32"), (ec_f32, N, "ec_f32")):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape != (rows, d) or t.stride(1) != 1 or t.device != dev:
            raise ValueError(f"{what}: {name} must be float32 [{rows}, {d}] with unit inner stride on {dev}")
    if rho_c is not None:
        _check_rho(rho_c, dev)
    if scale_c is not None:
        _check_rho(scale_c, dev)
    lims = torch.zeros((Q + 1,), dtype=torch.int64, device=dev)
    status = torch.zeros((Q,), dtype=torch.int32, device=dev)
    parts_s, parts_i = [], []
    if Q > 0 and N > 0:
        L = _lib.lib()
        with torch.cuda.device(dev):
            step = min(Q, MAX_RANGE_QUERIES_PER_CALL)
            ws = _workspace(dev, L.tsim_range_workspace_bytes(step, N))
            counts = torch.empty((Q,), dtype=torch.int64, device=dev)
            st = _stream(eq_unit)
            rho_p = rho_c.data_ptr() if rho_c is not None else 0
            total = 0
            for q0 in range(0, Q, step):
                nq = min(step, Q - q0)
                ldq, ldc = _row_stride(eq_f32), _row_stride(ec_f32)
                qf = eq_f32.data_ptr() + q0 * ldq * 4
                head = (eq_unit.data_ptr() + q0 * ld * 2, qf, ldq, nq, ec_half.data_ptr(), ec_f32.data_ptr(), ldc)
                # (a threshold array is sliced with the queries; the _tau entries are the scalar ones reading tau_q[q])
                tau_arg = tau if tau_q is None else tau_q.data_ptr() + q0 * 4
                tail = (N, d, ld, tau_arg, counts.data_ptr() + q0 * 8, status.data_ptr() + q0 * 4, ws.data_ptr(), ws.numel(), st)
                if scale_c is None:
                    rc = (L.tsim_cosine_range_scan if tau_q is None else L.tsim_cosine_range_scan_tau)(*head, rho_p, *tail)
                elif l2:
                    rc = (L.tsim_l2_range_scan if tau_q is None else L.tsim_l2_range_scan_tau)(*head, scale_c.data_ptr(), rho_p, *tail)
                else:
                    rc = (L.tsim_dot_range_scan if tau_q is None else L.tsim_dot_range_scan_tau)(*head, scale_c.data_ptr(), rho_p, *tail)
                _lib.check(rc, what)
                sl = torch.zeros((nq + 1,), dtype=torch.int64, device=dev)
                if centre_min is None:
                    torch.cumsum(counts[q0:q0 + nq], 0, out=sl[1:])
                else:
                    cnt = counts[q0:q0 + nq]
                    torch.cumsum(torch.where(cnt >= centre_min, cnt, torch.zeros_like(cnt)), 0, out=sl[1:])
                t_slice = int(sl[-1].item())       # the one host read: the fill's output is allocated from it
                if max_members is not None and total + t_slice > max_members:
                    raise ValueError(f"{what}: the candidate communities hold more than max_members={max_members} rows: the "
                                     "threshold is too low for this corpus (or min_size too small)")
                s = torch.empty((t_slice,), dtype=torch.float32, device=dev)
                i = torch.empty((t_slice,), dtype=torch.int64, device=dev)
                if t_slice:
                    fill = L.tsim_range_fill if tau_q is None else L.tsim_range_fill_tau
                    _lib.check(fill(space, qf, ldq, nq, ec_f32.data_ptr(), ldc, N, d, tau_arg, sl.data_ptr(), s.data_ptr(),
                                    i.data_ptr(), idx_offset, ws.data_ptr(), ws.numel(), st), what)
                lims[q0 + 1:q0 + nq + 1] = sl[1:] + total
                total += t_slice
                parts_s.append(s)
                parts_i.append(i)
    if len(parts_s) == 1:
        scores, idx = parts_s[0], parts_i[0]
    elif parts_s:
        scores, idx = torch.cat(parts_s), torch.cat(parts_i)
    else:
        scores = torch.empty((0,), dtype=torch.float32, device=dev)
        idx = torch.empty((0,), dtype=torch.int64, device=dev)
    return (lims, scores, idx, status) if return_status else (lims, scores, idx)


def cosine_range(eq_unit: torch.Tensor, ec_unit: torch.Tensor, d: int, threshold, eq_f32: torch.Tensor,
                 ec_f32: torch.Tensor, rho_c: Optional[torch.Tensor] = None, idx_offset: int = 0, return_status: bool = False):
    """Exact range search by cosine: EVERY corpus row whose score against a query is >= ``threshold`` (faiss ``range_search``),
    the score being exactly what :func:`cosine_topk` returns for the pair with the float32 matrices given (which are required
    here).  Returns ``(lims int64 [Q+1], scores float32 [T], idx int64 [T])`` on the device, the CSR layout of faiss: the hits
    of query q are ``scores[lims[q]:lims[q+1]]`` / ``idx[...]`` (= corpus row + ``idx_offset``), ordered by (score desc, index
    asc).  Nothing is truncated, whatever the threshold and the data: ``-inf`` returns every row.  One MFMA pass over the corpus
    collects the candidates, an exact re-score decides; a query that collects more than RANGE_SLOT_CAP rows is answered by an
    exact pass over the float32 rows instead (``return_status`` adds int32 [Q]: 1 = collected, 2 = exact pass; include/tsim.h).
    The total T is read back once between the two halves of the call (the output is allocated from it); query sets above
    MAX_RANGE_QUERIES_PER_CALL rows are processed in slices.  Q = 0 or N = 0: empty results, no launch.
    ``threshold`` may also be a tensor (or array) [Q], one threshold per query (converted to float32 on the queries' device; a
    wrong length is a ValueError): query q is answered exactly as by the call with the float ``threshold[q]``, in the same single
    pass over the corpus.  ``-inf`` there returns every row, ``+inf`` none; a NaN there — which a float argument refuses — gives
    that query no hit and status 2."""
    if eq_f32 is None or ec_f32 is None:
        raise ValueError("cosine_range needs the float32 matrices eq_f32 and ec_f32")
    return _range("cosine_range", _lib.SPACE_COSINE, eq_unit, ec_unit, d, threshold, eq_f32, ec_f32, rho_c, None, idx_offset,
                  return_status)


def dot_range(eq_unit: torch.Tensor, ec_scaled: torch.Tensor, d: int, threshold, eq_f32: torch.Tensor,
              ec_f32: torch.Tensor, rho_c: torch.Tensor, scale_c: torch.Tensor, idx_offset: int = 0, return_status: bool = False):
    """:func:`cosine_range` by inner product: every row with float32(q.c) >= ``threshold``, the score of :func:`dot_topk`.
    ``(ec_scaled, rho_c, scale_c)``: :func:`dot_scaled_rows` of ``ec_f32``; all are required.  A zero query scores 0 against
    every row: all rows for a threshold <= 0, none above."""
    if eq_f32 is None or ec_f32 is None or rho_c is None or scale_c is None:
        raise ValueError("dot_range needs eq_f32, ec_f32 and the corpus rows' rho_c and scale_c (dot_scaled_rows)")
    return _range("dot_range", _lib.SPACE_DOT, eq_unit, ec_scaled, d, threshold, eq_f32, ec_f32, rho_c, scale_c, idx_offset,
                  return_status)


def l2_range(eq_aug: torch.Tensor, ec_aug: torch.Tensor, d: int, threshold, eq_f32: torch.Tensor, ec_f32: torch.Tensor,
             rho_c: torch.Tensor, scale_c: torch.Tensor, idx_offset: int = 0, return_status: bool = False):
    """Exact range search by Euclidean distance: EVERY corpus row whose SQUARED distance to a query is <= ``threshold`` (the
    radius of faiss' ``range_search`` in the L2 space, which is on the squared distance too), the distance being exactly the
    float32 value :func:`l2_topk` returns for the pair.  Returns ``(lims int64 [Q+1], dist2 float32 [T], idx int64 [T])`` in the
    CSR layout of :func:`cosine_range`, every segment ordered by (distance asc, index asc); ``return_status`` adds int32 [Q] with
    the same meaning.  The comparison is ``<=`` (the counterpart of ``>=`` in the other spaces); faiss compares with ``<``, so a
    row AT the radius is a hit here and not there.  ``eq_aug``: :func:`l2_query_rows` of ``eq_f32`` under ``scale_c``;
    ``(ec_aug, rho_c, scale_c)``: :func:`l2_rows` of ``ec_f32``; all are required; d <= 767.
    ``threshold``: a float, or a tensor / array [Q], under the rules of :func:`cosine_range`.  A negative radius hits nothing, 0
    exactly the rows equal to the query, ``+inf`` every row (through the exact pass, status 2); a NaN in an array gives that query
    no hit and status 2.  Nothing is truncated.  Known: a corpus whose norms spread over decades (or one clustered far from the
    origin) puts every row inside the guard's window; such queries end in the exact pass — exact but slow."""
    if eq_f32 is None or ec_f32 is None or rho_c is None or scale_c is None:
        raise ValueError("l2_range needs eq_f32, ec_f32 and the corpus rows' rho_c and scale_c (l2_rows)")
    _l2_dim(d, "l2_range")
    return _range("l2_range", _lib.SPACE_L2, eq_aug, ec_aug, d, threshold, eq_f32, ec_f32, rho_c, scale_c, idx_offset,
                  return_status)


def range_merge(results, total: Optional[int] = None, ascending: bool = False):
    """Merge range results of the SAME queries over disjoint row sets (corpus shards or chunks searched with their own
    ``idx_offset``): ``results`` is a sequence of ``(lims [Q+1], scores [T_r], idx [T_r])`` as :func:`cosine_range` returns them
    (a payload may be longer than ``lims[-1]``, e.g. padded for an exchange; the excess is ignored), the return value one such
    triple whose segment q is the union of the lists' segments ordered by (score desc, index asc) — what one range search over
    the concatenated rows returns, bit for bit.  One kernel (tsim_range_merge): each entry finds its place by binary search in
    the other lists' segments, so segments may be of any length.  1 <= len(results) <= 64; one list comes back as a copy.
    ``total``: the number of entries over all lists when the caller knows it on the host (the sum of ``lims[-1]``); without it
    the total is read back once.  ``ascending``: the segments are ordered by (score asc, index asc) — the squared distances of
    :func:`l2_range` — and so is the result (tsim_range_merge_asc)."""
    results = [tuple(r) for r in results]
    R = len(results)
    if not 1 <= R <= _lib.RANGE_MERGE_MAX_LISTS:
        raise ValueError(f"range_merge takes 1 to {_lib.RANGE_MERGE_MAX_LISTS} results, got {R}")
    _need_gpu(*[t for r in results for t in r])
    Q = results[0][0].numel() - 1
    for lims, s, i in results:
        if lims.dtype != torch.int64 or lims.dim() != 1 or lims.numel() != Q + 1 or Q < 0:
            raise ValueError("range_merge: every lims must be int64 [Q+1] for one Q")
        if s.dtype != torch.float32 or i.dtype != torch.int64 or s.dim() != 1 or s.shape != i.shape:
            raise ValueError("range_merge: scores float32 [T] and idx int64 [T] of one length per result")
    dev = results[0][0].device
    base, bases = 0, []
    for _, s, _ in results:
        bases.append(base)
        base += s.numel()
    # absolute offsets of every segment in the concatenated payloads, and the output's prefix sum
    lims_in = torch.stack([r[0] for r in results]) + torch.tensor(bases, dtype=torch.int64, device=dev)[:, None]
    lims_out = torch.zeros((Q + 1,), dtype=torch.int64, device=dev)
    if Q > 0:
        torch.cumsum((lims_in[:, 1:] - lims_in[:, :-1]).sum(0), 0, out=lims_out[1:])
    T = int(lims_out[-1].item()) if total is None else int(total)
    out_s = torch.empty((T,), dtype=torch.float32, device=dev)
    out_i = torch.empty((T,), dtype=torch.int64, device=dev)
    if Q > 0 and T > 0:
        s_in = (results[0][1] if R == 1 else torch.cat([r[1] for r in results])).contiguous()
        i_in = (results[0][2] if R == 1 else torch.cat([r[2] for r in results])).contiguous()
        with torch.cuda.device(dev):
            merge = _lib.lib().tsim_range_merge_asc if ascending else _lib.lib().tsim_range_merge
            _lib.check(merge(lims_in.data_ptr(), s_in.data_ptr(), i_in.data_ptr(), R, Q,
                             lims_out.data_ptr(), T, out_s.data_ptr(), out_i.data_ptr(), _stream(out_s)),
                       "range_merge")
    return lims_out, out_s, out_i


# ------------------------------------------------------------------------------------------------- community detection
COMMUNITY_ST_ROW, COMMUNITY_ST_LIMS = _lib.COMMUNITY_ST_ROW, _lib.COMMUNITY_ST_LIMS      # include/tsim.h TSIM_COMMUNITY_ST_*
COMMUNITY_MAX_ROUNDS = 2048     # default round budget of community_select before the serial finish (DESIGN.md §7 has the counts)
COMMUNITY_ROUND_BATCH = 4       # rounds launched before the first host read of the undecided counts; every batch doubles ...
COMMUNITY_ROUND_BATCH_MAX = 64  # ... up to this many (the rounds past the deciding one find nothing to do)


def community_select(lims: torch.Tensor, members: torch.Tensor, N: int, min_size: int, max_rounds: Optional[int] = None):
    """The de-overlap of candidate communities (include/tsim.h): ``lims`` int64 [C+1] and ``members`` int32 [T] are a CSR in
    PRIORITY order over rows 0 .. N-1; walking it in order, a community is accepted iff at least ``min_size`` of its entries are
    rows no accepted community before it has taken, and it takes those.  Returns ``(accept int32 [C], keep uint8 [T],
    rounds_used, status)``: ``keep`` marks the entries that ended up in an accepted community, ``status`` is an int (0 or the
    COMMUNITY_ST_* bits: a member >= N, which is dropped; a non-monotone ``lims`` pair, which is an empty community).  A negative
    member is padding.  The parallel form runs in rounds — each decides at least the first community still undecided — in
    batches of COMMUNITY_ROUND_BATCH, doubling up to COMMUNITY_ROUND_BATCH_MAX, with one read of the device's undecided counts
    after each batch, until nothing is undecided or ``max_rounds`` (default COMMUNITY_MAX_ROUNDS) are used up; what is left then is finished by one workgroup in order.  ``max_rounds=0`` is
    that serial form alone.  The results do not depend on ``max_rounds``; ``rounds_used`` counts the rounds up to the one that
    decided the last community (``max_rounds`` when the serial finish ran)."""
    _need_gpu(lims, members)
    if lims.dtype != torch.int64 or lims.dim() != 1 or lims.numel() < 1 or not lims.is_contiguous():
        raise ValueError("community_select: lims must be a contiguous int64 [C+1]")
    if members.dtype != torch.int32 or members.dim() != 1 or not members.is_contiguous():
        raise ValueError("community_select: members must be a contiguous int32 [T]")
    max_rounds = COMMUNITY_MAX_ROUNDS if max_rounds is None else int(max_rounds)
    N, min_size = int(N), int(min_size)
    if N <= 0 or min_size < 1 or max_rounds < 0:
        raise ValueError(f"community_select: N={N} (> 0), min_size={min_size} (>= 1), max_rounds={max_rounds} (>= 0)")
    dev = lims.device
    C, T = lims.numel() - 1, members.numel()
    accept = torch.zeros((C,), dtype=torch.int32, device=dev)
    keep = torch.zeros((T,), dtype=torch.uint8, device=dev)
    if C == 0:
        return accept, keep, 0, 0
    L = _lib.lib()
    with torch.cuda.device(dev):
        status = torch.zeros((1,), dtype=torch.int32, device=dev)
        left = torch.zeros((COMMUNITY_ROUND_BATCH_MAX,), dtype=torch.int32, device=dev)
        ws = torch.empty((L.tsim_community_select_workspace_bytes(C, N),), dtype=torch.uint8, device=dev)
        st = _stream(lims)
        head = (lims.data_ptr(), members.data_ptr(), C, T, N, min_size)
        tail = (accept.data_ptr(), keep.data_ptr(), status.data_ptr(), left.data_ptr(), ws.data_ptr(), ws.numel(), st)
        rounds, undecided, batch = 0, C, COMMUNITY_ROUND_BATCH
        if max_rounds == 0:
            _lib.check(L.tsim_community_select_rounds(*head, 0, 0, *tail), "community_select")
        while undecided and rounds < max_rounds:
            n = min(batch, max_rounds - rounds)
            batch = min(2 * batch, COMMUNITY_ROUND_BATCH_MAX)
            _lib.check(L.tsim_community_select_rounds(*head, rounds, n, *tail), "community_select")
            for v in left[:n].tolist():      # the host read of the batch
                rounds += 1
                undecided = v
                if not v:
                    break
        if undecided:
            _lib.check(L.tsim_community_select_finish(*head, *tail), "community_select")
        return accept, keep, rounds, int(status.item())


def community_detection(eq_unit: Optional[torch.Tensor], eq_f32: torch.Tensor, d: int, threshold: float, min_size: int,
                        space: str = "cosine", rho: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
                        max_members: int = 1 << 27, max_rounds: Optional[int] = None, return_info: bool = False):
    """Community detection ("fast clustering", sentence-transformers' ``util.community_detection`` with its tie orders fixed)
    over the rows ``eq_f32`` [N, d]: every group of at least ``min_size`` rows scoring >= ``threshold`` against a centre row,
    largest first, no row in two groups; no cluster count is needed.  The score s(i, j) is exactly what :func:`cosine_range`
    (``space='cosine'``) or :func:`dot_range` (``'dot'``) reports for query row i against corpus row j.
      1. hits(i) = the rows j with s(i, j) >= threshold, ordered by (score desc, index asc); row i is a centre iff it has at
         least ``min_size`` hits, and hits(i) is its candidate community;
      2. the candidates are ordered by (size desc, centre index asc);
      3. in that order a candidate keeps the rows no accepted candidate before it took, and is accepted iff at least
         ``min_size`` are left (:func:`community_select`, on the device);
      4. the accepted ones are ordered by (size desc, position in 2 asc); members keep the order of 1.
    Returns, on the device, ``(lims int64 [K+1], members int64 [M], centres int64 [K], labels int64 [N])``: community c is
    ``members[lims[c]:lims[c+1]]`` around row ``centres[c]`` (which another community may have taken), ``labels[i]`` its number
    or -1.  ``return_info=True`` adds a dict: ``scores`` float32 [M] (each member's score against its centre), ``rounds`` (of
    the de-overlap), ``candidates`` (the number of centres) and ``candidate_members`` (their hits, what ``max_members`` bounds).
    ``eq_unit``: cosine — :func:`l2norm_rows` of the rows, with ``rho`` its residual word (optional); dot — the corpus operand,
    ``(eq_unit, rho, scale)`` = :func:`dot_scaled_rows` of the rows (the query operand is made here).  None: made here.
    Step 1 runs in slices of MAX_RANGE_QUERIES_PER_CALL rows; only the centres' hits are materialised, and their number is held
    against ``max_members`` before anything is allocated for them: a ValueError says the threshold is too low for the corpus
    (every row of a dense region lists the whole region: the candidates grow with the SQUARE of a cluster's size).  2 and 4
    are stable sorts on the device."""
    centre, plims, pmem, pscore = community_candidates(eq_unit, eq_f32, d, threshold, min_size, space, rho, scale, max_members)
    N, dev = eq_f32.shape[0], eq_f32.device
    i64 = dict(dtype=torch.int64, device=dev)
    C, T = centre.numel(), pmem.numel()
    seg = torch.repeat_interleave(torch.arange(C, **i64), plims[1:] - plims[:-1])      # priority position of every entry
    accept, keep, rounds, _ = community_select(plims, pmem.to(torch.int32), max(N, 1), int(min_size), max_rounds)
    keep = keep.bool()
    kseg = seg[keep]
    ksize = torch.zeros((C,), **i64).index_add_(0, kseg, torch.ones_like(kseg))
    acc = torch.nonzero(accept).reshape(-1)                                      # accepted, in priority order
    acc = acc[torch.sort(ksize[acc], stable=True, descending=True)[1]]           # (size desc, priority position asc)
    K = acc.numel()
    rank = torch.full((C,), -1, **i64)
    rank[acc] = torch.arange(K, **i64)
    o = torch.sort(rank[kseg], stable=True)[1]               # entries grouped by final community, their order kept
    members = pmem[keep][o]
    out_lims = torch.zeros((K + 1,), **i64)
    torch.cumsum(ksize[acc], 0, out=out_lims[1:])
    labels = torch.full((N,), -1, **i64)
    labels[members] = rank[kseg][o]
    out = (out_lims, members, centre[acc], labels)
    if return_info:
        out += ({"scores": pscore[keep][o], "rounds": rounds, "candidates": C, "candidate_members": T},)
    return out


def community_candidates(eq_unit: Optional[torch.Tensor], eq_f32: torch.Tensor, d: int, threshold: float, min_size: int,
                         space: str = "cosine", rho: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
                         max_members: int = 1 << 27):
    """Steps 1 and 2 of :func:`community_detection` (same arguments): ``(centres int64 [C], lims int64 [C+1], members int64
    [T], scores float32 [T])`` — the candidate communities in priority order, (size desc, centre index asc), as a CSR: what
    :func:`community_select` takes (with the members as int32)."""
    what = "community_detection"
    _need_gpu(eq_f32)
    if space not in ("cosine", "dot"):
        raise ValueError(f"{what}: space={space!r}: one of 'cosine', 'dot'")
    min_size = int(min_size)
    if min_size < 1:
        raise ValueError(f"{what}: min_size={min_size} < 1")
    if eq_f32.dim() != 2 or eq_f32.dtype != torch.float32:
        raise ValueError(f"{what}: eq_f32 must be float32 [N, d]")
    N, dev = eq_f32.shape[0], eq_f32.device
    if space == "cosine":
        if eq_unit is None:
            eq_unit, rho = l2norm_rows(eq_f32, return_rho=True)
        q_unit, scale = eq_unit, None
        sp = _lib.SPACE_COSINE
    else:
        if eq_unit is None:
            eq_unit, rho, scale = dot_scaled_rows(eq_f32)
        elif rho is None or scale is None:
            raise ValueError(f"{what}: space='dot' needs (eq_unit, rho, scale) from dot_scaled_rows, or none of them")
        q_unit = l2norm_rows(eq_f32)
        sp = _lib.SPACE_DOT
    lims, scores, idx = _range(what, sp, q_unit, eq_unit, d, threshold, eq_f32, eq_f32, rho, scale, 0, False,
                               centre_min=min_size, max_members=int(max_members))
    i64 = dict(dtype=torch.int64, device=dev)
    sizes = lims[1:] - lims[:-1]
    centre = torch.nonzero(sizes > 0).reshape(-1)           # (min_size >= 1: a centre has a hit; the others got no segment)
    order = torch.sort(sizes[centre], stable=True, descending=True)[1]
    centre = centre[order]                                   # priority order: (size desc, centre index asc)
    csize = sizes[centre]
    C, T = centre.numel(), idx.numel()
    plims = torch.zeros((C + 1,), **i64)
    torch.cumsum(csize, 0, out=plims[1:])
    seg = torch.repeat_interleave(torch.arange(C, **i64), csize)                 # priority position of every entry
    src = torch.arange(T, **i64) - plims[:-1][seg] + lims[:-1][centre][seg]      # where the range search left it
    return centre, plims, idx[src], scores[src]


# ------------------------------------------------------------------------------------------------- HDBSCAN
def mst_prim(rows: torch.Tensor, core2: Optional[torch.Tensor] = None):
    """Prim's minimum spanning tree over the float32 rows [N, d] from row 0 (include/tsim.h tsim_mst_prim), in SQUARED distances:
    the weight of a pair is ``max(d2(a, b), core2[a], core2[b])`` with d2 the float32 value :func:`l2_topk` returns for it, or d2
    alone without ``core2`` (float32 [N]).  Returns ``(from int32 [N-1], to int32 [N-1], w2 float32 [N-1])`` on the device, edge t
    joining row ``to[t]`` to the tree at its nearest endpoint ``from[t]`` (the earlier one on a tie; the lower row joins first on
    a tie).  The rows may be a strided view with unit inner stride.  d <= 767.  Nothing is read back."""
    _need_gpu(rows)
    if rows.dim() != 2 or rows.dtype != torch.float32 or rows.shape[0] < 1 or rows.shape[1] < 1:
        raise ValueError("mst_prim: rows must be float32 [N, d] with N >= 1")
    if rows.stride(1) != 1 and rows.shape[1] > 1:
        rows = rows.contiguous()
    N, d = rows.shape
    _l2_dim(d, "mst_prim")
    dev = rows.device
    if core2 is not None:
        _need_gpu(rows, core2)
        if core2.dtype != torch.float32 or core2.shape != (N,):
            raise ValueError(f"mst_prim: core2 must be float32 [{N}]")
        core2 = core2.contiguous()
    frm = torch.empty((N - 1,), dtype=torch.int32, device=dev)
    to = torch.empty((N - 1,), dtype=torch.int32, device=dev)
    w2 = torch.empty((N - 1,), dtype=torch.float32, device=dev)
    L = _lib.lib()
    with torch.cuda.device(dev):
        ws = _workspace(dev, L.tsim_mst_prim_workspace_bytes(N))
        _lib.check(L.tsim_mst_prim(rows.data_ptr(), _row_stride(rows), N, d, core2.data_ptr() if core2 is not None else 0,
                                   frm.data_ptr(), to.data_ptr(), w2.data_ptr(), ws.data_ptr(), ws.numel(), _stream(rows)), "mst_prim")
    return frm, to, w2


def hdbscan_tree_labels(frm, to, w2, N: int, min_cluster_size: int):
    """The host tree stage of HDBSCAN (include/tsim.h tsim_hdbscan_tree_labels) on numpy edges: ``(labels int32 [N], n_clusters)``.
    ValueError where the edges are no spanning tree of rows 0 .. N-1."""
    frm = np.ascontiguousarray(frm, dtype=np.int32)
    to = np.ascontiguousarray(to, dtype=np.int32)
    w2 = np.ascontiguousarray(w2, dtype=np.float32)
    N, min_cluster_size = int(N), int(min_cluster_size)
    if N < 1 or frm.shape != (N - 1,) or to.shape != (N - 1,) or w2.shape != (N - 1,):
        raise ValueError(f"hdbscan_tree_labels: N={N} needs {N - 1} edges, got {frm.shape}, {to.shape}, {w2.shape}")
    if min_cluster_size < 2:
        raise ValueError(f"hdbscan_tree_labels: min_cluster_size={min_cluster_size} < 2")
    labels = np.empty((N,), dtype=np.int32)
    n_clusters = np.zeros((1,), dtype=np.int32)
    rc = _lib.lib().tsim_hdbscan_tree_labels(frm.ctypes.data, to.ctypes.data, w2.ctypes.data, N, min_cluster_size, labels.ctypes.data,
                                             n_clusters.ctypes.data)
    if rc == 1:
        raise ValueError("hdbscan_tree_labels: the edges are not a spanning tree of rows 0 .. N-1 (an endpoint out of range or a cycle)")
    if rc != 0:
        raise _lib.TsimError(f"hdbscan_tree_labels failed (code {rc})")
    return labels, int(n_clusters[0])


def hdbscan_unit_rows(rows: torch.Tensor) -> torch.Tensor:
    """The float32 unit rows ``x / |x|.clamp(min=1e-12)`` that ``hdbscan(metric='cosine')`` clusters."""
    return (rows / rows.norm(dim=1, keepdim=True).clamp(min=1e-12)).contiguous()


def hdbscan(rows: torch.Tensor, min_cluster_size: int, min_samples: Optional[int] = None, metric: str = "euclidean",
            return_info: bool = False):
    """HDBSCAN (``hdbscan.HDBSCAN`` / ``sklearn.cluster.HDBSCAN`` with ``cluster_selection_method='eom'``) over the float32 rows
    [N, d]: ``labels`` int64 [N] on the device, -1 for noise; neither a cluster count nor a threshold is needed.
      1. ``core2`` = the squared distance of every row to its ``min_samples``-th nearest row, itself included: the last column of
         :func:`l2_topk` of the rows against themselves (``min_samples`` defaults to ``min_cluster_size``);
      2. the minimum spanning tree of the mutual-reachability graph, :func:`mst_prim` with ``core2``;
      3. the N - 1 edges are read back once and the tree stage runs on the host (:func:`hdbscan_tree_labels`).
    ``metric='cosine'`` runs the same on the float32 unit rows (:func:`hdbscan_unit_rows`): Euclidean distance on those is
    monotone in cosine.  ``return_info=True`` adds a dict: ``from``, ``to``, ``w2`` (the edges, on the device), ``core2`` and
    ``n_clusters``.  ValueError: ``min_cluster_size < 2``, ``min_samples`` outside 1 .. min(N, MAX_K), non-finite rows, d > 767,
    another metric.  include/tsim.h has the definition and its tie rules; tests/golden/hdbscan.npz pins parity with
    scikit-learn on separated clusters."""
    what = "hdbscan"
    _need_gpu(rows)
    if metric not in ("euclidean", "cosine"):
        raise ValueError(f"{what}: metric={metric!r}: 'euclidean' or 'cosine'")
    if rows.dim() != 2 or rows.shape[0] < 1 or rows.shape[1] < 1:
        raise ValueError(f"{what}: rows must be [N, d] with N >= 1")
    N, d = rows.shape
    _l2_dim(d, what)
    min_cluster_size = int(min_cluster_size)
    min_samples = min_cluster_size if min_samples is None else int(min_samples)
    if min_cluster_size < 2:
        raise ValueError(f"{what}: min_cluster_size={min_cluster_size} < 2")
    if not 1 <= min_samples <= min(N, MAX_K):
        raise ValueError(f"{what}: min_samples={min_samples} outside 1..min(N, {MAX_K}) = {min(N, MAX_K)}")
    x = rows.float().contiguous()
    if not bool(torch.isfinite(x).all()):
        raise ValueError(f"{what}: the rows hold a NaN or an infinity")
    if metric == "cosine":
        x = hdbscan_unit_rows(x)
    ec, rho, maxnorm = l2_rows(x)
    dist, _ = l2_topk(l2_query_rows(x, maxnorm), ec, d, min_samples, x, x, rho, maxnorm)
    core2 = dist[:, min_samples - 1].contiguous()
    frm, to, w2 = mst_prim(x, core2)
    labels, n_clusters = hdbscan_tree_labels(frm.cpu().numpy(), to.cpu().numpy(), w2.cpu().numpy(), N, min_cluster_size)
    out = torch.from_numpy(labels.astype(np.int64)).to(x.device)
    if return_info:
        return out, {"from": frm, "to": to, "w2": w2, "core2": core2, "n_clusters": n_clusters}
    return out


def packed_result_bytes(Q: int, k: int) -> int:
    """Bytes of one rank's result buffer: [Q,k] float32 scores, then (8-byte aligned) [Q,k] int64 indices."""
    return (Q * k * 4 + 7) // 8 * 8 + Q * k * 8


def packed_result_views(buf: torch.Tensor, Q: int, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(scores, idx) views of result buffers ``buf`` uint8 [..., packed_result_bytes(Q, k)] (one per leading index): what
    :func:`cosine_topk` writes through ``out=`` and what :func:`topk_merge` reads in place after an all-gather."""
    so = (Q * k * 4 + 7) // 8 * 8
    s = buf[..., :Q * k * 4].view(torch.float32)
    i = buf[..., so:so + Q * k * 8].view(torch.int64)
    return s.unflatten(-1, (Q, k)), i.unflatten(-1, (Q, k))


def _list_major(t: torch.Tensor) -> bool:
    """[nlists, Q, k] with each list contiguous (lists may be any distance apart)"""
    return t.dim() == 3 and t.stride(2) == 1 and t.stride(1) == t.shape[2] and (t.shape[0] == 1 or t.stride(0) >= t.shape[1] * t.shape[2])


def topk_merge(scores, idx, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Merge per-shard/per-chunk lists (global indices) into [Q,k].  ``scores`` / ``idx`` are either sequences of [Q,k_in]
    tensors or [nlists, Q, k_in] tensors; the latter are read in place when every list is contiguous, whatever the distance
    between lists (e.g. :func:`packed_result_views` of an all-gathered buffer)."""
    s = scores if isinstance(scores, torch.Tensor) else torch.stack([t.contiguous() for t in scores])
    i = idx if isinstance(idx, torch.Tensor) else torch.stack([t.contiguous() for t in idx])
    if not _list_major(s):
        s = s.contiguous()
    if not _list_major(i):
        i = i.contiguous()
    _need_gpu(s, i)
    if s.dtype != torch.float32 or i.dtype != torch.int64 or s.shape != i.shape or s.dim() != 3:
        raise ValueError("topk_merge expects float32 scores and int64 indices of one shape [nlists, Q, k_in]")
    nl, Q, k_in = s.shape
    out_s = torch.empty((Q, k), dtype=torch.float32, device=s.device)
    out_i = torch.empty((Q, k), dtype=torch.int64, device=s.device)
    with torch.cuda.device(s.device):
        _lib.check(_lib.lib().tsim_topk_merge_strided(s.data_ptr(), i.data_ptr(), nl, Q, k_in, k, s.stride(0), i.stride(0),
                                                      out_s.data_ptr(), out_i.data_ptr(), _stream(s)), "topk_merge")
    return out_s, out_i


def cos_sim_dense(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    _need_gpu(a, b)
    a = a.float().contiguous()
    b = b.float().contiguous()
    if a.shape[1] != b.shape[1]:
        raise ValueError("cos_sim: width mismatch")
    out = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().tsim_cos_sim(a.data_ptr(), a.shape[0], b.data_ptr(), b.shape[0], a.shape[1],
                                           out.data_ptr(), _stream(a)), "cos_sim")
    return out


def mean_pool(hidden: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    _need_gpu(hidden, mask)
    assert len(hidden.shape) == 3  # batch, seq_len, embed_size (modules.py:159)
    if hidden.dtype not in (torch.float32, torch.bfloat16):
        hidden = hidden.float()
    hidden = hidden.contiguous()
    m = mask.to(torch.int32).contiguous()
    B, S, H = hidden.shape
    out = torch.empty((B, H), dtype=torch.float32, device=hidden.device)
    dt = _lib.TSIM_F32 if hidden.dtype == torch.float32 else _lib.TSIM_BF16
    with torch.cuda.device(hidden.device):
        _lib.check(_lib.lib().tsim_mean_pool(hidden.data_ptr(), dt, m.data_ptr(), B, S, H, out.data_ptr(),
                                             _stream(hidden)), "mean_pool")
    return out


POOL_MODES = {"mean": _lib.POOL_MEAN, "cls": _lib.POOL_CLS, "max": _lib.POOL_MAX, "mean_sqrt_len": _lib.POOL_MEAN_SQRT_LEN}
ACTIVATIONS = {"identity": _lib.ACT_IDENTITY, "tanh": _lib.ACT_TANH}


def pool_mode_id(mode) -> int:
    """'mean' | 'cls' | 'max' | 'mean_sqrt_len' (or the TSIM_POOL_* integer) -> TSIM_POOL_*."""
    if isinstance(mode, str):
        if mode not in POOL_MODES:
            raise ValueError(f"unknown pooling mode {mode!r} (one of {sorted(POOL_MODES)})")
        return POOL_MODES[mode]
    if int(mode) not in POOL_MODES.values():
        raise ValueError(f"unknown pooling mode {mode!r}")
    return int(mode)


def activation_id(act) -> int:
    """'identity' | 'tanh' (or the TSIM_ACT_* integer) -> TSIM_ACT_*."""
    if isinstance(act, str):
        if act not in ACTIVATIONS:
            raise ValueError(f"unknown activation {act!r} (one of {sorted(ACTIVATIONS)})")
        return ACTIVATIONS[act]
    if int(act) not in ACTIVATIONS.values():
        raise ValueError(f"unknown activation {act!r}")
    return int(act)


def pool(hidden: torch.Tensor, mask: torch.Tensor, mode="mean") -> torch.Tensor:
    """Pooling of a padded [B, S, H] float32/bf16 tensor with an attention mask [B, S] -> float32 [B, H]
    (/root/reference/src/modules/modules.py:154-181; include/tsim.h tsim_pool).  ``mode`` 'mean' is :func:`mean_pool` bit for
    bit; 'cls' takes the first token whose mask is set, 'max' the elementwise max over those tokens, 'mean_sqrt_len' the
    masked sum over sqrt(sum of the mask).  A row without tokens pools to zeros."""
    _need_gpu(hidden, mask)
    m_id = pool_mode_id(mode)
    if hidden.dim() != 3:
        raise ValueError("pool expects hidden states [batch, seq_len, hidden]")
    if hidden.dtype not in (torch.float32, torch.bfloat16):
        hidden = hidden.float()
    hidden = hidden.contiguous()
    m = mask.to(torch.int32).contiguous()
    B, S, H = hidden.shape
    if tuple(m.shape) != (B, S):
        raise ValueError(f"mask shape {tuple(m.shape)} != {(B, S)}")
    out = torch.empty((B, H), dtype=torch.float32, device=hidden.device)
    dt = _lib.TSIM_F32 if hidden.dtype == torch.float32 else _lib.TSIM_BF16
    with torch.cuda.device(hidden.device):
        _lib.check(_lib.lib().tsim_pool(hidden.data_ptr(), dt, m.data_ptr(), B, S, H, m_id, out.data_ptr(), _stream(hidden)),
                   "pool")
    return out


def dense_rows(x: torch.Tensor, w: Optional[torch.Tensor], b: Optional[torch.Tensor] = None, act="identity",
               normalize: bool = False) -> torch.Tensor:
    """sentence-transformers Dense (+ Normalize) on float32 rows: act(x @ w.T + b), then x / max(|x|, 1e-12) when
    ``normalize``.  x [B, d_in], w [d_out, d_in] (nn.Linear layout) or None (no projection), b [d_out] or None; d_in, d_out
    multiples of 8 in [8, 1024].  Every output element is one float32 fma chain in an order fixed by d_in (include/tsim.h)."""
    ts = [t for t in (x, w, b) if t is not None]
    _need_gpu(*ts)
    a_id = activation_id(act)
    if x.dim() != 2:
        raise ValueError("dense_rows expects a 2-D tensor")
    x = x.float().contiguous()
    B, d_in = x.shape
    d_out = d_in
    if w is not None:
        w = w.detach().float().contiguous()
        if w.dim() != 2 or w.shape[1] != d_in:
            raise ValueError(f"dense_rows: weight shape {tuple(w.shape)} does not take rows of width {d_in}")
        d_out = w.shape[0]
    if b is not None:
        b = b.detach().float().contiguous()
        if tuple(b.shape) != (d_out,):
            raise ValueError(f"dense_rows: bias shape {tuple(b.shape)} != ({d_out},)")
    out = torch.empty((B, d_out), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().tsim_dense_rows(x.data_ptr(), B, d_in, w.data_ptr() if w is not None else None,
                                              b.data_ptr() if b is not None else None, d_out, a_id, int(bool(normalize)),
                                              out.data_ptr(), _stream(x)), "dense_rows")
    return out


def quantize_mxfp8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[rows, K] bf16 -> (e4m3 bytes uint8 [rows, K], E8M0 block scales uint8 [rows, K/32]) — the operand format of
    the fp8 encoder variant (``NativeEncoder(weight_dtype="mxfp8")``).  K % 32 == 0."""
    _need_gpu(x)
    if x.dim() != 2 or x.dtype != torch.bfloat16:
        raise ValueError("quantize_mxfp8 expects a 2-D bfloat16 tensor")
    rows, K = x.shape
    if K % 32 != 0:
        raise ValueError(f"K={K} is not a multiple of the 32-element MX block")
    x = x.contiguous()
    q = torch.empty((rows, K), dtype=torch.uint8, device=x.device)
    s = torch.empty((rows, K // 32), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.lib().tsim_quantize_mxfp8(x.data_ptr(), rows, K, q.data_ptr(), s.data_ptr(), _stream(x)),
                   "quantize_mxfp8")
    return q, s


def gemm_mxfp8(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """float32 [M, N] = dequant(xq, xs) @ dequant(wq, ws)^T + bias with the block-scaled fp8 MFMA.
    xq [M, K] / wq [N, K] uint8 e4m3 bytes, xs [M, K/32] / ws [N, K/32] uint8 E8M0 scales, bias float32 [N]."""
    _need_gpu(xq, xs, wq, ws, bias)
    M, K = xq.shape
    N = wq.shape[0]
    if wq.shape[1] != K or xs.shape != (M, K // 32) or ws.shape != (N, K // 32) or bias.shape != (N,):
        raise ValueError("gemm_mxfp8: inconsistent operand shapes")
    Mp = (M + 255) // 256 * 256                      # the kernel works on whole 256-row tiles
    xqp = torch.zeros((Mp, K), dtype=torch.uint8, device=xq.device)
    xsp = torch.full((Mp, K // 32), 127, dtype=torch.uint8, device=xq.device)
    xqp[:M], xsp[:M] = xq, xs
    out = torch.empty((Mp, N), dtype=torch.float32, device=xq.device)
    with torch.cuda.device(xq.device):
        _lib.check(_lib.lib().tsim_gemm_mxfp8(xqp.data_ptr(), xsp.data_ptr(), wq.contiguous().data_ptr(),
                                              ws.contiguous().data_ptr(), bias.contiguous().data_ptr(), out.data_ptr(),
                                              M, N, K, _stream(xq)), "gemm_mxfp8")
    return out[:M]
