// Exact scan of inverted lists (included by search.hip, after the helpers it uses): the rows are stored in LIST order, list l
// is rows [off[l], off[l+1]), and query q is scored against the nprobe lists probes[q, 0..nprobe) only — the contiguous form
// of list_search.h (no gather through row numbers, no CSR prep, no staircase).  Scores are those of the list entries, bit for
// bit: exact_load_query and wave_scores unchanged, the Euclidean rows read through l2_f32 (-dist^2 inside, the sign flipped
// by the merge).  The entry offered to the running list is (score, row_ids[position]): results are ordered by (score desc, id
// asc), so equal rows in different lists rank as they do in the flat search.  A negative id is a tombstone: the row is loaded
// and scored and the score dropped — never a branch around the row loads (row_elems_f64 says what a predicated load costs).
//
// Work.  A list is cut into segments of S = TSIM_IVF_SEG rows from its own start.  Workgroup (pair p = q nprobe + j, slot s)
// passes the segments s, s + nseg, s + 2 nseg, ... of list probes[p] through a running list (SlList, as bf_partial_kernel) in
// blocks of at most SL_NB rows and writes its first k entries, padding included, to slot p nseg + s; a pair without a list
// (a negative probe, one >= nlist, an empty list, a slot past the list's end) writes padding.  nseg comes from the caller's
// hint max_list_len and from IVF_BUDGET (ivf_nseg); a list longer than the hint is still scanned completely, because the slots
// stride.  The slots of a query are consecutive, so list_merge_kernel in its shared form (nch = nprobe nseg) is the merge:
// one workgroup per query, store_result<NEG>.
//
// Offsets.  The workspace is sized without nlist, so no cleaned copy of list_off exists.  ivf_prep_kernel (one workgroup)
// clears the status words and writes ONE word: whether list_off is non-decreasing within [0, N].  If it is (the ordinary
// case) a workgroup reads its two offsets as they stand.  If not, every workgroup computes what list_prep_kernel would have
// written for its list — the running maximum of list_off[0 .. l] and [0 .. l + 1], clamped to [0, N] — by a reduction over
// that prefix, and slot 0 of the pair sets TSIM_IVF_ST_OFF where either word changed.  Either way lo <= hi lie in [0, N].
#pragma once

namespace tsim {
constexpr int IVF_SEG = TSIM_IVF_SEG;
constexpr int IVF_MAX_NSEG = 256;   // slots of one pair: a single pair over a long list still reaches every CU
constexpr size_t IVF_BUDGET = (size_t)64 << 20;
constexpr int IVF_PREP_T = 1024;
static_assert(IVF_SEG % 64 == 0 && IVF_SEG > 0, "a segment is whole wave rounds");

__global__ __launch_bounds__(IVF_PREP_T) void ivf_prep_kernel(int64_t Q, int64_t N, const int64_t *__restrict__ off, int64_t nlist,
                                                              int32_t *__restrict__ dirty, int32_t *__restrict__ status) {
    __shared__ int bad_s;
    if (threadIdx.x == 0) bad_s = 0;
    __syncthreads();
    if (status)
        for (int64_t q = threadIdx.x; q < Q; q += IVF_PREP_T) status[q] = 0;
    bool bad = false;
    for (int64_t l = threadIdx.x; l <= nlist; l += IVF_PREP_T) {
        const int64_t v = off[l];
        bad |= v < 0 || v > N || (l > 0 && off[l - 1] > v);
    }
    if (bad) bad_s = 1;   // (every writer writes 1)
    __syncthreads();
    if (threadIdx.x == 0) *dirty = bad_s;
}

// [lo, hi) of list l (0 <= l < nlist), cleaned as list_prep_kernel cleans lims; `changed`: either word differs from list_off.
// Called by the whole workgroup; red: 8 words of LDS.
__device__ __forceinline__ void ivf_list_range(const int64_t *off, int64_t l, int64_t N, bool dirty, int64_t *red, int64_t &lo,
                                               int64_t &hi, bool &changed) {
    lo = off[l];
    hi = off[l + 1];
    changed = false;
    if (!dirty) return;   // workgroup-uniform
    const int64_t raw_lo = lo, raw_hi = hi;
    int64_t m = 0;   // (the clamp from below, too)
    for (int64_t j = threadIdx.x; j <= l; j += 256) m = off[j] > m ? off[j] : m;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t y = __shfl_xor(m, o, 64);
        m = y > m ? y : m;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) m = red[w] > m ? red[w] : m;
    __syncthreads();   // (red is free again)
    lo = m > N ? N : m;
    hi = raw_hi > m ? raw_hi : m;
    hi = hi > N ? N : hi;
    changed = lo != raw_lo || hi != raw_hi;
}

template <typename T, bool COS>
__global__ __launch_bounds__(256) void ivf_partial_kernel(int64_t N, const T *__restrict__ xq, int64_t ldq, const T *__restrict__ xr,
                                                          int64_t ldr, int d, const int64_t *__restrict__ off, int64_t nlist,
                                                          const int32_t *__restrict__ row_ids, const int64_t *__restrict__ probes,
                                                          int nprobe, int nseg, int k, int kp, const int32_t *__restrict__ dirty,
                                                          float *__restrict__ ws_s, int *__restrict__ ws_i,
                                                          int32_t *__restrict__ status) {
    SlList<int, false> top = sl_shared_list<int, false>();
    __shared__ int64_t red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t p = blockIdx.x, q = blockIdx.x / (unsigned)nprobe;
    const int s = blockIdx.y;
    const int64_t l = probes[p];   // workgroup-uniform, as everything derived from it
    int64_t lo = 0, hi = 0;
    bool changed = false;
    if (l >= 0 && l < nlist) ivf_list_range(off, l, N, *dirty != 0, red, lo, hi, changed);
    if (status && s == 0 && threadIdx.x == 0) {
        const int bits = (l >= nlist ? TSIM_IVF_ST_LIST : 0) | (changed ? TSIM_IVF_ST_OFF : 0);
        if (bits) atomicOr(status + q, bits);
    }
    top.reset(kp);
    const int64_t first = lo + (int64_t)s * IVF_SEG;
    if (first < hi) {
        ExactQuery<T> eqr;
        exact_load_query<T, COS>(eqr, xq + q * ldq, d, lane);
        for (int64_t g = first; g < hi; g += (int64_t)nseg * IVF_SEG) {
            const int64_t g1 = g + IVF_SEG < hi ? g + IVF_SEG : hi;
            for (int64_t b = g; b < g1; b += SL_NB) {
                const int nb = (int)(g1 - b < SL_NB ? g1 - b : SL_NB);
                const SlBound<int> w = top.bound(k);
                for (int g0 = wave * 64; g0 < nb; g0 += 256) {   // wave-uniform
                    const int e = g0 + lane;
                    const int nvalid = nb - g0 < 64 ? nb - g0 : 64;
                    const int row = (int)(b + (e < nb ? e : g0));   // in [lo, hi): inside the rows and inside row_ids
                    const int id = row_ids[row];
                    const float sc = wave_scores<T, COS>(eqr, xr, ldr, row, nvalid, d, lane);
                    if (e < nb && id >= 0) top.offer(sc, id, w);   // (a negative id: scored, dropped)
                }
                top.flush(kp);
            }
        }
    }
    top.store_raw(ws_s, ws_i, (p * nseg + s) * k, k);
}

// Slots per pair: the segments of the longest list the caller expects, at most IVF_MAX_NSEG, and no more than keep the slots
// (8 B an entry) of the call within IVF_BUDGET; at least one.  The workspace holds min(what the hint asks for, the budget or
// one slot per pair) — non-decreasing in every argument although nseg itself falls as Q nprobe k grows.
static inline int64_t ivf_nseg_wanted(int64_t max_list_len) {
    return std::max<int64_t>(1, std::min<int64_t>((max_list_len + IVF_SEG - 1) / IVF_SEG, IVF_MAX_NSEG));
}
static inline int ivf_nseg(int64_t Q, int nprobe, int64_t max_list_len, int k) {
    const size_t one = (size_t)Q * nprobe * k * 8;
    return (int)std::max<int64_t>(1, std::min<int64_t>(ivf_nseg_wanted(max_list_len), (int64_t)(IVF_BUDGET / one)));
}
struct IvfWs {
    size_t dirty, ws_s, ws_i, total;
};
static void plan_workspace_ivf(int64_t Q, int nprobe, int64_t max_list_len, int k, IvfWs *w) {
    const size_t one = (size_t)Q * nprobe * k * 8;
    const size_t half = std::min(one * (size_t)ivf_nseg_wanted(max_list_len), std::max(IVF_BUDGET, one)) / 2;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    w->dirty = take(4);
    w->ws_s = take(half);
    w->ws_i = take(half);
    w->total = o;
}
}  // namespace tsim

extern "C" size_t tsim_ivf_scan_workspace_bytes(int64_t Q, int nprobe, int64_t max_list_len, int k) {
    if (Q <= 0 || nprobe <= 0 || max_list_len < 0 || k <= 0 || k > tsim::TOPK_LARGE_MAX_K) return 0;
    tsim::IvfWs w;
    tsim::plan_workspace_ivf(Q, nprobe, max_list_len, k, &w);
    return w.total;
}

extern "C" int tsim_ivf_scan_topk(int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *rows_f32, int64_t ld_rows,
                                  int64_t N, int d, const int64_t *list_off, int64_t nlist, const int32_t *row_ids,
                                  const int64_t *probes, int nprobe, int64_t max_list_len, int k, float *out_scores, int64_t *out_idx,
                                  int64_t idx_offset, int32_t *out_status, void *workspace, size_t workspace_bytes, void *stream) {
    using namespace tsim;
    const char *what = "ivf_scan_topk";
    TSIM_REQUIRE(eq_f32 && rows_f32 && list_off && row_ids && probes && out_scores && out_idx, "%s: null pointer", what);
    TSIM_REQUIRE(space == TSIM_SPACE_COSINE || space == TSIM_SPACE_DOT || space == TSIM_SPACE_L2, "%s: unknown space %d", what, space);
    TSIM_REQUIRE(Q > 0 && N > 0 && nlist > 0 && max_list_len >= 0, "%s: bad shape Q=%lld N=%lld nlist=%lld max_list_len=%lld", what,
                 (long long)Q, (long long)N, (long long)nlist, (long long)max_list_len);
    TSIM_REQUIRE(nprobe >= 1, "%s: nprobe=%d < 1", what, nprobe);
    TSIM_REQUIRE(k >= 1 && k <= TOPK_LARGE_MAX_K, "%s: k=%d outside 1..%d", what, k, TOPK_LARGE_MAX_K);
    TSIM_REQUIRE(d >= 1 && d <= 64 * XS_MAXI, "%s: d=%d outside 1..%d", what, d, 64 * XS_MAXI);
    TSIM_REQUIRE(space != TSIM_SPACE_L2 || d < 64 * XS_MAXI, "%s: d=%d (the Euclidean space takes d <= %d)", what, d, 64 * XS_MAXI - 1);
    TSIM_REQUIRE(ldq_f32 >= d && ld_rows >= d, "%s: float32 row strides %lld/%lld < d=%d", what, (long long)ldq_f32, (long long)ld_rows,
                 d);
    TSIM_REQUIRE(N < (1ll << 31) - 64 && nlist < (1ll << 40) && Q < (1ll << 31) && Q * nprobe < (1ll << 31) - 1,
                 "%s: too large for one launch (N=%lld, Q nprobe=%lld)", what, (long long)N, (long long)(Q * nprobe));
    IvfWs w;
    plan_workspace_ivf(Q, nprobe, max_list_len, k, &w);
    if (!workspace || workspace_bytes < w.total) return fail(TSIM_ENOMEM, "%s: workspace %zu B < %zu B", what, workspace_bytes, w.total);
    hipStream_t st = as_stream(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    int32_t *dirty = reinterpret_cast<int32_t *>(ws + w.dirty);
    float *ws_s = reinterpret_cast<float *>(ws + w.ws_s);
    int *ws_i = reinterpret_cast<int *>(ws + w.ws_i);
    const int kp = sl_list_len(k);
    const int nseg = ivf_nseg(Q, nprobe, max_list_len, k);
    hipLaunchKernelGGL(ivf_prep_kernel, dim3(1), dim3(IVF_PREP_T), 0, st, Q, N, list_off, nlist, dirty, out_status);
    TSIM_HIP_CHECK(hipGetLastError());
    const dim3 grid((unsigned)(Q * nprobe), (unsigned)nseg);
    auto launch = [&](auto rows, auto cosc) {
        using RT = decltype(rows);
        hipLaunchKernelGGL((ivf_partial_kernel<RT, decltype(cosc)::value>), grid, dim3(256), 0, st, N, reinterpret_cast<const RT *>(eq_f32),
                           ldq_f32, reinterpret_cast<const RT *>(rows_f32), ld_rows, d, list_off, nlist, row_ids, probes, nprobe, nseg, k,
                           kp, dirty, ws_s, ws_i, out_status);
    };
    if (space == TSIM_SPACE_COSINE) launch(float{}, std::true_type{});
    else if (space == TSIM_SPACE_DOT) launch(float{}, std::false_type{});
    else launch(l2_f32{}, std::false_type{});   // (float32 rows read through l2_f32: with_score_mode says why)
    TSIM_HIP_CHECK(hipGetLastError());
    // the merge of the shared form of the list search: the query's nch = nprobe nseg slots are consecutive
    const unsigned mg = (unsigned)(Q < 4096 ? Q : 4096);
    const int64_t nch = (int64_t)nprobe * nseg;
    if (space == TSIM_SPACE_L2)
        hipLaunchKernelGGL(list_merge_kernel<true>, dim3(mg), dim3(256), 0, st, Q, (int64_t)1, (const int64_t *)nullptr, nch, k, kp, ws_s,
                           ws_i, out_scores, out_idx, idx_offset);
    else
        hipLaunchKernelGGL(list_merge_kernel<false>, dim3(mg), dim3(256), 0, st, Q, (int64_t)1, (const int64_t *)nullptr, nch, k, kp, ws_s,
                           ws_i, out_scores, out_idx, idx_offset);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}
