// Exact top-k within candidate lists (included by search.hip, after the helpers it uses): each query is scored against its OWN
// list of corpus rows — the indirect form of the brute-force pass.  No MFMA selection, no guard: every listed row is scored
// with the exact definitions above (wave_scores: cosine of the float32 rows, float32(q.c), -dist^2 through l2_f32).
//
// Corpus rows.  float32, or IEEE half (tsim_list_topk_f16: the row store of a refine stage).  The query is float32 either way
// and its type T carries the metric; the corpus element type C only says how an element is loaded.  A half is widened exactly
// (v_cvt_f32_f16, subnormals kept by the default mode), so a half row scores the bits the float32 kernel gives on the widened
// row.  A lane reads its elements j = lane + 64 i as SINGLE halves: a row stride may be odd, so a row is only 2-byte aligned and
// a pair load (4 bytes) would be misaligned for every other row; a wave's 64 halves are one contiguous 128-byte segment per
// load instruction either way, NI instructions a row as for float32 rows, and no regrouping of pairs across lanes is needed.
//
// Lists.  cand[0..T) holds row numbers (int32 or int64); query q owns cand[lims[q] .. lims[q+1]) (CSR), or every query owns
// cand[0..T) (shared).  A negative entry is padding; an entry >= N is never dereferenced and raises TSIM_LIST_ST_ROW in the
// query's status word.  The index is loaded, CLAMPED to a valid row and the score discarded afterwards — never a branch around
// the row loads (row_elems_f64 says what a predicated load costs).
//
// Work.  cand is cut at the absolute positions 0, S, 2S, ... (S = TSIM_LIST_SLICE = SL_NB: one slice is one block of the running
// list).  CSR: workgroup (slice g, y) serves the queries whose lists meet [gS, (g+1)S), found by binary search in the cleaned
// lims.  For each it passes the entries of the query inside the slice through a running list (SlList, as bf_partial_kernel)
// and writes its first k entries to the pair's slot.  The host knows T, not the list lengths: with monotone lims
// the pairs (g, q) that exist form a staircase, g + q is unique among them, and Q + ceil(T / S) slots hold them all.  Shared:
// workgroup (chunk c, q) walks a chunk of whole slices with the running list, slot q * nch + c (list_shared_chunks).
// list_merge_kernel, one workgroup per query, joins the query's slots in blocks of SL_NB entries (several slots per block when k
// is small: a query that owns all of a long cand has T / S slots).
//
// lims are made monotone before anything reads them: list_prep_kernel (one workgroup) writes L[j] = the running maximum of
// lims[0..j], clamped to [0, T].  A pair that was decreasing comes out empty, one that pointed outside [0, T] in range, and the
// query gets TSIM_LIST_ST_LIMS.  The kernel also clears the status words.
#pragma once

namespace tsim {
static_assert(TSIM_LIST_SLICE == SL_NB, "a CSR slice is one block of the running LDS list");
constexpr int LIST_PREP_T = 1024;

__global__ __launch_bounds__(LIST_PREP_T) void list_prep_kernel(int64_t Q, int64_t T, const int64_t *__restrict__ lims,
                                                                int64_t *__restrict__ clean, int32_t *__restrict__ status) {
    __shared__ int64_t wmax[LIST_PREP_T / 64];
    __shared__ int64_t carry_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (!lims) {   // shared list: only the status words
        if (status)
            for (int64_t q = threadIdx.x; q < Q; q += LIST_PREP_T) status[q] = 0;
        return;
    }
    if (threadIdx.x == 0) carry_s = 0;   // (the clamp from below, too)
    __syncthreads();
    for (int64_t j0 = 0; j0 <= Q; j0 += LIST_PREP_T) {
        const int64_t j = j0 + threadIdx.x;
        int64_t v = j <= Q ? lims[j] : INT64_MIN;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {   // inclusive running maximum within the wave
            const int64_t y = __shfl_up(v, o, 64);
            if (lane >= o) v = y > v ? y : v;
        }
        if (lane == 63) wmax[wave] = v;
        __syncthreads();
        int64_t m = carry_s;
        for (int w = 0; w < wave; ++w) m = wmax[w] > m ? wmax[w] : m;
        v = v > m ? v : m;
        v = v > T ? T : v;   // (>= 0 by the carry)
        if (j <= Q) clean[j] = v;
        __syncthreads();
        if (threadIdx.x == LIST_PREP_T - 1) carry_s = v;   // the maximum so far (clamped: max and clamp commute)
        __syncthreads();
    }
    if (status)   // a query's pair is clean when both of its words came through unchanged (clean[]: behind the barriers above)
        for (int64_t q = threadIdx.x; q < Q; q += LIST_PREP_T)
            status[q] = (clean[q] != lims[q] || clean[q + 1] != lims[q + 1]) ? TSIM_LIST_ST_LIMS : 0;
}

template <typename CI>
__device__ __forceinline__ int64_t list_entry(const void *cand, int64_t at) {
    return (int64_t) reinterpret_cast<const CI *>(cand)[at];
}

// first q in [0, Q] with L[q + B] > x (B = 1) / L[q] >= x (B = 0); L monotone
template <int B>
__device__ __forceinline__ int64_t list_first_q(const int64_t *L, int64_t Q, int64_t x) {
    int64_t lo = 0, hi = Q;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const bool before = B ? L[mid + 1] <= x : L[mid] < x;
        lo = before ? mid + 1 : lo;
        hi = before ? hi : mid;
    }
    return lo;
}

template <typename T, bool COS, typename CI, typename C>
__global__ __launch_bounds__(256) void list_partial_kernel(int64_t Q, int64_t N, int64_t Tn, const T *__restrict__ xq, int64_t ldq,
                                                           const C *__restrict__ xc, int64_t ldc, int d, const void *__restrict__ cand,
                                                           const int64_t *__restrict__ L, int64_t nch, int64_t spc, int k, int kp,
                                                           float *__restrict__ ls_s, int *__restrict__ ls_i,
                                                           int32_t *__restrict__ status) {
    SlList<int, false> top = sl_shared_list<int, false>();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c = blockIdx.x;   // chunk: spc slices (CSR: one)
    const int64_t s0 = c * spc * TSIM_LIST_SLICE, s1 = s0 + spc * TSIM_LIST_SLICE < Tn ? s0 + spc * TSIM_LIST_SLICE : Tn;
    int64_t qa = 0, qb = Q;
    if (L) {   // CSR: the queries whose lists meet [s0, s1)
        qa = list_first_q<1>(L, Q, s0);
        qb = list_first_q<0>(L, Q, s1);
    }
    for (int64_t q = qa + blockIdx.y; q < qb; q += gridDim.y) {   // workgroup-uniform
        int64_t e0 = s0, e1 = s1;
        if (L) {
            e0 = L[q] > s0 ? L[q] : s0;
            e1 = L[q + 1] < s1 ? L[q + 1] : s1;
            if (e0 >= e1) continue;   // an empty list between two others
        }
        ExactQuery<T> eqr;
        exact_load_query<T, COS>(eqr, xq + q * ldq, d, lane);
        top.reset(kp);
        bool beyond = false;
        for (int64_t b = e0; b < e1; b += SL_NB) {   // (CSR: once)
            const int nb = (int)(e1 - b < SL_NB ? e1 - b : SL_NB);
            const SlBound<int> w = top.bound(k);
            for (int g0 = wave * 64; g0 < nb; g0 += 256) {   // wave-uniform
                const int e = g0 + lane;
                const int nvalid = nb - g0 < 64 ? nb - g0 : 64;
                const int64_t r = list_entry<CI>(cand, b + (e < nb ? e : g0));
                const bool usable = r >= 0 && r < N;
                const int row = usable ? (int)r : 0;   // clamped: the row is loaded and scored, the score dropped
                const float s = wave_scores<T, COS, C>(eqr, xc, ldc, row, nvalid, d, lane);
                if (e < nb) {
                    if (usable) top.offer(s, row, w);
                    beyond |= r >= N;
                }
            }
            top.flush(kp);
        }
        if (status && __any(beyond) && lane == 0) atomicOr(status + q, TSIM_LIST_ST_ROW);
        const int64_t slot = L ? q + c : q * nch + c;
        top.store_raw(ls_s, ls_i, slot * k, k);
        __syncthreads();
    }
}

template <bool NEG>
__global__ __launch_bounds__(256) void list_merge_kernel(int64_t Q, int64_t Tn, const int64_t *__restrict__ L, int64_t nch, int k,
                                                         int kp, const float *__restrict__ ls_s, const int *__restrict__ ls_i,
                                                         float *__restrict__ out_s, int64_t *__restrict__ out_i,
                                                         int64_t idx_offset) {
    SlList<int, false> top = sl_shared_list<int, false>();
    for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
        int64_t slot0 = q * nch, ns = Tn > 0 ? nch : 0;
        if (L) {
            const int64_t lo = L[q], hi = L[q + 1];
            ns = hi > lo ? (hi - 1) / TSIM_LIST_SLICE - lo / TSIM_LIST_SLICE + 1 : 0;
            slot0 = q + lo / TSIM_LIST_SLICE;
        }
        top.reset(kp);
        const int64_t E = ns * k;   // the slots of a query are consecutive: E entries from slot0 * k on
        for (int64_t b0 = 0; b0 < E; b0 += SL_NB) {
            const SlBound<int> w = top.bound(k);
            for (int64_t e = b0 + threadIdx.x; e < E && e < b0 + SL_NB; e += 256) {
                const int i = ls_i[slot0 * k + e];
                if (i != sl_pad<int>()) top.offer(ls_s[slot0 * k + e], i, w);
            }
            top.flush(kp);
        }
        top.store_result<NEG>(out_s, out_i, q * k, k, idx_offset);
        __syncthreads();
    }
}

// Slots of one call.  CSR: Q + ceil(T / S), the staircase.  Shared: Q x nch, nch chunks of whole slices — as many as there are
// slices, up to 1 024, and no more than keep the chunk lists (8 B an entry) within LIST_BUDGET.  The workspace holds the larger
// of the two (the function is not told which form the call takes) and is non-decreasing in Q, T and k.
constexpr size_t LIST_BUDGET = (size_t)64 << 20;
static inline int64_t list_slices(int64_t T) { return (T + TSIM_LIST_SLICE - 1) / TSIM_LIST_SLICE; }
static inline int64_t list_shared_chunks(int64_t Q, int64_t T, int k) {
    const int64_t fit = (int64_t)(LIST_BUDGET / ((size_t)Q * k * 8));
    return std::max<int64_t>(1, std::min<int64_t>({list_slices(T), 1024, fit}));
}
struct ListWs {
    size_t clean, ls_s, ls_i, total;
};
static void plan_workspace_list(int64_t Q, int64_t T, int k, ListWs *w) {
    const int64_t nsl = list_slices(T);
    const size_t csr = (size_t)(Q + nsl) * k * 8;
    const size_t shared = std::min((size_t)Q * std::min<int64_t>(nsl, 1024) * k * 8, std::max(LIST_BUDGET, (size_t)Q * k * 8));
    const size_t half = std::max(csr, shared) / 2;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    w->clean = take((size_t)(Q + 1) * 8);
    w->ls_s = take(half);
    w->ls_i = take(half);
    w->total = o;
}

// ec: float32 rows, or rows of IEEE half when `half_rows` (ldc in elements of that type either way)
static int list_topk(int sm, const char *what, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec, bool half_rows,
                     int64_t ldc, int64_t N, int d, const void *cand, int cand_dtype, int64_t T, const int64_t *lims, int shared, int k,
                     float *out_scores, int64_t *out_idx, int64_t idx_offset, int32_t *out_status, void *workspace,
                     size_t workspace_bytes, void *stream) {
    TSIM_REQUIRE(eq_f32 && ec && out_scores && out_idx && (cand || T == 0), "%s: null pointer", what);
    TSIM_REQUIRE(Q > 0 && N > 0 && T >= 0, "%s: bad shape Q=%lld N=%lld T=%lld", what, (long long)Q, (long long)N, (long long)T);
    TSIM_REQUIRE(k >= 1 && k <= TOPK_LARGE_MAX_K, "%s: k=%d outside 1..%d", what, k, TOPK_LARGE_MAX_K);
    TSIM_REQUIRE(d >= 1 && d <= 64 * XS_MAXI, "%s: d=%d outside 1..%d", what, d, 64 * XS_MAXI);
    TSIM_REQUIRE(sm != SM_L2 || d < 64 * XS_MAXI, "%s: d=%d (the Euclidean space takes d <= %d)", what, d, 64 * XS_MAXI - 1);
    TSIM_REQUIRE(ldq_f32 >= d && ldc >= d, "%s: row strides %lld/%lld < d=%d", what, (long long)ldq_f32, (long long)ldc, d);
    TSIM_REQUIRE((lims != nullptr) != (shared != 0), "%s: pass lims (one list per query) or shared = 1 (one list for all), not %s", what,
                 lims ? "both" : "neither");
    TSIM_REQUIRE(cand_dtype == TSIM_I32 || cand_dtype == TSIM_I64, "%s: unknown index dtype %d (TSIM_I32, TSIM_I64)", what, cand_dtype);
    TSIM_REQUIRE(N < (1ll << 31) - 64 && Q < (1ll << 31) - 512 && T < (1ll << 40), "%s: too large for 32-bit row ids", what);
    const int64_t nsl = list_slices(T);
    TSIM_REQUIRE(nsl < (1ll << 31) - 1, "%s: T=%lld too long for one launch", what, (long long)T);
    ListWs w;
    plan_workspace_list(Q, T, k, &w);
    if (!workspace || workspace_bytes < w.total) return fail(TSIM_ENOMEM, "%s: workspace %zu B < %zu B", what, workspace_bytes, w.total);
    hipStream_t st = as_stream(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    int64_t *clean = lims ? reinterpret_cast<int64_t *>(ws + w.clean) : nullptr;
    float *ls_s = reinterpret_cast<float *>(ws + w.ls_s);
    int *ls_i = reinterpret_cast<int *>(ws + w.ls_i);
    const int kp = sl_list_len(k);
    if (lims || out_status) {
        hipLaunchKernelGGL(list_prep_kernel, dim3(1), dim3(LIST_PREP_T), 0, st, Q, T, lims, clean, out_status);
        TSIM_HIP_CHECK(hipGetLastError());
    }
    // CSR: one slice per workgroup column, and a slice meets 1 + S / (mean list length) queries: four workgroups share them.
    // Shared: nch chunks of spc slices, one workgroup per (chunk, query).
    const int64_t spc = lims || !nsl ? 1 : (nsl + list_shared_chunks(Q, T, k) - 1) / list_shared_chunks(Q, T, k);
    const int64_t nch = (nsl + spc - 1) / spc;   // (no more than list_shared_chunks: every chunk holds a slice)
    if (nsl > 0) {
        const dim3 grid((unsigned)nch, (unsigned)(lims ? std::min<int64_t>(Q, 4) : std::min<int64_t>(Q, 65535)));
        // (not with_score_mode: its unit-row branch would instantiate a kernel for half rows that no entry can reach)
        auto launch = [&](auto rows, auto cosc, auto ci, auto crow) {
            using RT = decltype(rows);
            using CI = decltype(ci);
            using CT = decltype(crow);
            hipLaunchKernelGGL((list_partial_kernel<RT, decltype(cosc)::value, CI, CT>), grid, dim3(256), 0, st, Q, N, T,
                               reinterpret_cast<const RT *>(eq_f32), ldq_f32, reinterpret_cast<const CT *>(ec), ldc, d, cand, clean, nch,
                               spc, k, kp, ls_s, ls_i, out_status);
        };
        auto by_dtype = [&](auto rows, auto cosc) {   // (the corpus rows: the query's type, or unit_t = IEEE half)
            if (half_rows) {
                if (cand_dtype == TSIM_I32) launch(rows, cosc, int32_t{}, unit_t{});
                else launch(rows, cosc, int64_t{}, unit_t{});
            } else {
                if (cand_dtype == TSIM_I32) launch(rows, cosc, int32_t{}, rows);
                else launch(rows, cosc, int64_t{}, rows);
            }
        };
        if (sm == SM_COS) by_dtype(float{}, std::true_type{});
        else if (sm == SM_DOT) by_dtype(float{}, std::false_type{});
        else by_dtype(l2_f32{}, std::false_type{});   // (float32 rows read through l2_f32: with_score_mode says why)
        TSIM_HIP_CHECK(hipGetLastError());
    }
    const unsigned mg = (unsigned)(Q < 4096 ? Q : 4096);
    if (sm == SM_L2)
        hipLaunchKernelGGL(list_merge_kernel<true>, dim3(mg), dim3(256), 0, st, Q, T, clean, nch, k, kp, ls_s, ls_i, out_scores, out_idx,
                           idx_offset);
    else
        hipLaunchKernelGGL(list_merge_kernel<false>, dim3(mg), dim3(256), 0, st, Q, T, clean, nch, k, kp, ls_s, ls_i, out_scores, out_idx,
                           idx_offset);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}
}  // namespace tsim

extern "C" size_t tsim_list_topk_workspace_bytes(int64_t Q, int64_t T, int k) {
    if (Q <= 0 || T < 0 || k <= 0 || k > tsim::TOPK_LARGE_MAX_K) return 0;
    tsim::ListWs w;
    tsim::plan_workspace_list(Q, T, k, &w);
    return w.total;
}

extern "C" int tsim_cosine_list_topk(const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *ec_f32, int64_t ldc_f32, int64_t N,
                                     int d, const void *cand, int cand_dtype, int64_t T, const int64_t *lims, int shared, int k,
                                     float *out_scores, int64_t *out_idx, int64_t idx_offset, int32_t *out_status, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    return tsim::list_topk(tsim::SM_COS, "cosine_list_topk", eq_f32, ldq_f32, Q, ec_f32, false, ldc_f32, N, d, cand, cand_dtype, T, lims, shared,
                           k, out_scores, out_idx, idx_offset, out_status, workspace, workspace_bytes, stream);
}

extern "C" int tsim_dot_list_topk(const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *ec_f32, int64_t ldc_f32, int64_t N,
                                  int d, const void *cand, int cand_dtype, int64_t T, const int64_t *lims, int shared, int k,
                                  float *out_scores, int64_t *out_idx, int64_t idx_offset, int32_t *out_status, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    return tsim::list_topk(tsim::SM_DOT, "dot_list_topk", eq_f32, ldq_f32, Q, ec_f32, false, ldc_f32, N, d, cand, cand_dtype, T, lims, shared, k,
                           out_scores, out_idx, idx_offset, out_status, workspace, workspace_bytes, stream);
}

extern "C" int tsim_l2_list_topk(const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *ec_f32, int64_t ldc_f32, int64_t N,
                                 int d, const void *cand, int cand_dtype, int64_t T, const int64_t *lims, int shared, int k,
                                 float *out_scores, int64_t *out_idx, int64_t idx_offset, int32_t *out_status, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    return tsim::list_topk(tsim::SM_L2, "l2_list_topk", eq_f32, ldq_f32, Q, ec_f32, false, ldc_f32, N, d, cand, cand_dtype, T, lims, shared, k,
                           out_scores, out_idx, idx_offset, out_status, workspace, workspace_bytes, stream);
}

extern "C" int tsim_list_topk_f16(int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const void *ec_f16, int64_t ldc_f16,
                                  int64_t N, int d, const void *cand, int cand_dtype, int64_t T, const int64_t *lims, int shared, int k,
                                  float *out_scores, int64_t *out_idx, int64_t idx_offset, int32_t *out_status, void *workspace,
                                  size_t workspace_bytes, void *stream) {
    TSIM_REQUIRE(space == TSIM_SPACE_COSINE || space == TSIM_SPACE_DOT || space == TSIM_SPACE_L2,
                 "list_topk_f16: unknown space %d (TSIM_SPACE_COSINE, TSIM_SPACE_DOT, TSIM_SPACE_L2)", space);
    const int sm = space == TSIM_SPACE_COSINE ? tsim::SM_COS : space == TSIM_SPACE_DOT ? tsim::SM_DOT : tsim::SM_L2;
    return tsim::list_topk(sm, "list_topk_f16", eq_f32, ldq_f32, Q, ec_f16, true, ldc_f16, N, d, cand, cand_dtype, T, lims, shared, k,
                           out_scores, out_idx, idx_offset, out_status, workspace, workspace_bytes, stream);
}
