"""The numpy restatement of the int8-embedding ops (text_similarity_amd/csrc/int8_search.h) and the cases the int8 tests share.
Everything here is exact: float32 quantiser arithmetic as numpy evaluates it, integer scores, the (-score, row) order, the
canonical float64 lane sum."""
import numpy as np

from oracle.search_ref import _lane_sum

INT32_MIN = -2 ** 31


def int8_bytes(d):
    return -(-d // 16) * 16 if 1 <= d <= 1024 else 0


def ranges_of(x):
    """float32 [2, d]: per-column minimum and maximum (sentence-transformers' calibration ranges)"""
    x = np.asarray(x, np.float32)
    return np.vstack([x.min(axis=0), x.max(axis=0)]).astype(np.float32)


def st_quantize(x, ranges):
    """the literal sentence-transformers expression (quantize_embeddings, precision="int8"); defined for in-range values only"""
    starts = ranges[0, :]
    steps = (ranges[1, :] - ranges[0, :]) / 255
    return ((x - starts) / steps - 128).astype(np.int8)


def quantize_t(x, ranges):
    """the float32 value t whose truncation is the code"""
    x, ranges = np.asarray(x, np.float32), np.asarray(ranges, np.float32)
    with np.errstate(all="ignore"):
        starts = ranges[0, :]
        steps = (ranges[1, :] - ranges[0, :]) / np.float32(255)
        t = (x - starts) / steps - np.float32(128)
    assert t.dtype == np.float32
    return t


def quantize_ref(x, ranges, d=None):
    """[rows, d] float32 -> int8 [rows, int8_bytes(d)]: trunc(t) towards zero with t saturated to [-128, 127] (+-inf included),
    NaN -> 0, and zero bytes from d up to the padded stride"""
    x = np.asarray(x, np.float32)
    d = x.shape[1] if d is None else d
    t = quantize_t(x, ranges)
    with np.errstate(invalid="ignore"):
        c = np.trunc(np.clip(t, np.float32(-128), np.float32(127)))
    c = np.where(np.isnan(t), np.float32(0), c).astype(np.int8)
    out = np.zeros((x.shape[0], int8_bytes(d)), np.int8)
    out[:, :d] = c
    return out


def pad_codes(c, d=None):
    """int8 [rows, d] -> the padded layout [rows, int8_bytes(d)]"""
    c = np.asarray(c, np.int8)
    d = c.shape[1] if d is None else d
    out = np.zeros((c.shape[0], int8_bytes(d)), np.int8)
    out[:, :d] = c[:, :d]
    return out


def ip_ref(q_codes, c_codes, d):
    """int64 [Q, N] inner products over the first d values"""
    return q_codes[:, :d].astype(np.int64) @ c_codes[:, :d].astype(np.int64).T


def ip_topk_ref(q_codes, c_codes, d, k, idx_offset=0):
    """(score int32 [Q, k], idx int64 [Q, k]) by (score desc, row asc), padded with (INT32_MIN, -1)"""
    score = ip_ref(q_codes, c_codes, d)
    Q, N = score.shape
    os_ = np.full((Q, k), INT32_MIN, np.int32)
    oi = np.full((Q, k), -1, np.int64)
    rows = np.arange(N)
    for q in range(Q):
        order = np.lexsort((rows, -score[q]))[:k]
        os_[q, :order.size] = score[q, order]
        oi[q, :order.size] = order + idx_offset
    return os_, oi


def rescore_ref(q_f32, c_codes, d, cand, k, idx_offset=0):
    """(scores f32 [Q, k], idx int64 [Q, k], status int32 [Q]): every usable entry of cand [Q, m] scored as
    float32(_lane_sum(q, codes)), ranked by (-score, row); negatives skipped, entries >= N skipped with status bit 1, a row
    listed twice returned twice; padded with (-inf, -1)"""
    q_f32 = np.asarray(q_f32, np.float32)
    cand = np.asarray(cand, np.int64)
    N = c_codes.shape[0]
    vals = c_codes[:, :d].astype(np.float64)
    Q = q_f32.shape[0]
    os_ = np.full((Q, k), -np.inf, np.float32)
    oi = np.full((Q, k), -1, np.int64)
    st = np.zeros((Q,), np.int32)
    for q in range(Q):
        c = cand[q]
        st[q] = 1 if (c >= N).any() else 0
        c = c[(c >= 0) & (c < N)]
        if c.size == 0:
            continue
        s = np.float32(_lane_sum(q_f32[q][None, :], vals[c]))
        order = np.lexsort((c, -s))[:k]
        os_[q, :order.size] = s[order]
        oi[q, :order.size] = c[order] + idx_offset
    return os_, oi, st


def random_rows(rng, n, d):
    return rng.standard_normal((n, d)).astype(np.float32)


def uniform_codes(rng, n, d):
    """int8 [n, int8_bytes(d)], uniform over [-128, 127]"""
    return pad_codes(rng.integers(-128, 128, size=(n, d), dtype=np.int64).astype(np.int8))


def ternary_codes(rng, n, d):
    """int8 [n, int8_bytes(d)] from {-1, 0, 1}: few distinct scores, so ties everywhere"""
    return pad_codes(rng.integers(-1, 2, size=(n, d), dtype=np.int64).astype(np.int8))


def quantiser_rows(rows, d, seed):
    """(x float32 [rows, d], ranges float32 [2, d]) with the inputs that need care: values below the start and above the maximum,
    exactly at both ends, t on integer boundaries and one float32 step either side of them, NaN and +-inf, and (d >= 3) a
    constant column, whose step is 0: x == start gives 0 / 0 = NaN -> 0, anything else +-inf -> saturated"""
    rng = np.random.default_rng(seed)
    lo = (rng.standard_normal(d) - 2.0).astype(np.float32)
    hi = (lo + np.float32(0.5) + rng.random(d).astype(np.float32) * np.float32(3.0)).astype(np.float32)
    ranges = np.vstack([lo, hi]).astype(np.float32)
    if d >= 3:
        ranges[1, 2] = ranges[0, 2]                                    # the constant column
    x = (lo + (hi - lo) * rng.random((rows, d)).astype(np.float32)).astype(np.float32)
    step = (ranges[1] - ranges[0]) / np.float32(255)
    kind = rng.integers(0, 12, size=(rows, d))
    n = rng.integers(0, 256, size=(rows, d)).astype(np.float32)
    with np.errstate(all="ignore"):
        edge = (ranges[0] + n * step).astype(np.float32)               # t near an integer
    x = np.where(kind == 0, edge, x)
    x = np.where(kind == 1, np.nextafter(edge, np.float32(np.inf)), x)
    x = np.where(kind == 2, np.nextafter(edge, np.float32(-np.inf)), x)
    x = np.where(kind == 3, ranges[0] - np.float32(0.75), x)           # below the start
    x = np.where(kind == 4, ranges[1] + np.float32(0.75), x)           # above the maximum
    x = np.where(kind == 5, ranges[0] + 0 * x, x)                      # exactly at the start
    x = np.where(kind == 6, ranges[1] + 0 * x, x)                      # exactly at the maximum
    x = x.astype(np.float32)
    flat = x.reshape(-1)
    special = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], np.float32)
    pick = rng.random(flat.size) < 0.05
    flat[pick] = special[rng.integers(0, special.size, size=int(pick.sum()))]
    if d >= 3:
        x[:, 2] = np.where(np.arange(rows) % 3 == 0, ranges[0, 2], x[:, 2])     # on the constant: 0 / 0
    flat[:min(special.size, flat.size)] = special[:flat.size]         # every special at least once where the shape allows
    return x, ranges
