// The frame the code searches share (included by search.hip before hamming_search.h and int8_search.h): a first stage that is an
// exact top-k over compressed code rows, and a re-score of its candidates with the float32 query against the codes.  What a code
// type brings is its partial kernel's compare loop, its group size and how a code row expands to values; the rest is here.
//
// First stage.  A partial kernel's workgroup (chunk c, group g) owns rows_per_chunk rows and the ng <= G queries g G .. g G +
// ng - 1, each with a running list (SlList) of its own carved from dynamic LDS (hm_list, i8_list: top_s, top_i of kp entries,
// blk_s, blk_i of bc, the counters behind all lists).  The block protocol is the one of bf_partial_kernel — the bound is read before anyone
// offers since the list's last flush (the list does not change until its flush), at most bc entries are offered between two
// flushes — with one difference: a block is bc OFFERS, not bc rows.  Once a list has its bound a step of 256 rows offers a
// handful of entries, and a flush costs a sort and a merge behind a dozen barriers whatever it holds; the sort of a chunk's first
// full block is the dearest of them.  So a list is flushed after the chunk's first step (that sets its bound), after the last,
// and in between only when its block could not take the offers of another step.  The carve and that decision are written out in
// each partial kernel: every shared form that was tried moved all 24 partial kernels off the instructions they compile to now
// (DESIGN.md section 7), and their loops are the hot ones.  Chunk lists go to the workspace raw; code_merge_kernel, one workgroup per query, passes the query's nch k consecutive entries through one list in blocks of
// SL_NB and writes int32 values and int64 indices.
// Chunks: enough that chunks x groups reaches CS_WGS = 1 024 workgroups (four per CU — a single query still spreads over all 256
// CUs), of at least max(SL_NB, 4 k) rows (every chunk pays one full sort of its first block per query), and no more than keep the
// chunk lists within CS_BUDGET.
//
// Re-score.  code_rescore_kernel: one workgroup per query.  Each lane holds the query's elements j = lane + 64 i, i < 16, as
// float64.  A wave takes one candidate at a time and adds q_j v_j, v the value of the row's element j, in the order i = 0, 1, ..
// (the first term starts the sum, groups at or beyond d add nothing, an element beyond d inside the last group adds +0), the xor
// butterfly 32 .. 1 joins the lanes and the sum is rounded once to float32: float32(oracle.search_ref._lane_sum(q, v)) — every
// product is exact.  Candidates pass through one SlList in blocks of SL_NB; negative entries are skipped, entries >= N never
// dereferenced and reported in the status word.
#pragma once

namespace tsim {
constexpr int CS_MAX_D = 1024;                    // elements of a code row at most
constexpr int CS_MAXI = CS_MAX_D / 64;            // elements a lane of the re-score holds
constexpr int CS_WGS = 1024;                      // workgroups the partial pass aims for
constexpr int CS_MAX_CHUNKS = 1024;
constexpr size_t CS_BUDGET = (size_t)64 << 20;    // chunk lists of one call (8 B an entry)

// One workgroup per query: the query's nch chunk lists are consecutive, E = nch k entries from q nch k on.  The lists hold
// -distance (DIST: the value written is the distance, padding INT32_MAX) or the score itself (padding INT32_MIN).
template <bool DIST>
__global__ __launch_bounds__(256) void code_merge_kernel(int64_t Q, int64_t nch, int k, int kp, const float *__restrict__ ws_s,
                                                         const int *__restrict__ ws_i, int32_t *__restrict__ out_v,
                                                         int64_t *__restrict__ out_i, int64_t idx_offset) {
    SlList<int, false> top = sl_shared_list<int, false>();
    const int64_t E = nch * k;
    for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
        top.reset(kp);
        for (int64_t b0 = 0; b0 < E; b0 += SL_NB) {
            const SlBound<int> w = top.bound(k);
            for (int64_t e = b0 + threadIdx.x; e < E && e < b0 + SL_NB; e += 256) {
                const int i = ws_i[q * E + e];
                if (i != sl_pad<int>()) top.offer(ws_s[q * E + e], i, w);
            }
            top.flush(kp);
        }
        for (int t = threadIdx.x; t < k; t += 256) {
            const int row = top.top_i[t];
            const bool pad = row == sl_pad<int>();
            if (DIST)
                out_v[q * k + t] = pad ? INT32_MAX : (int32_t)(-top.top_s[t]);
            else
                out_v[q * k + t] = pad ? INT32_MIN : (int32_t)top.top_s[t];
            out_i[q * k + t] = pad ? -1 : (int64_t)row + idx_offset;
        }
        __syncthreads();
    }
}

// SIGN: a code row is sign bits, element 8j at bit 7 of byte j, and v_j = +-1: every lane reads the 8 bytes that hold its element
// of group i (one address for the whole wave).  Otherwise a row is int8 values: lane l reads byte lane + 64 i (one 64-byte span a
// wave).
template <bool SIGN>
__global__ __launch_bounds__(256) void code_rescore_kernel(int64_t Q, int64_t N, const float *__restrict__ xq, int64_t ldq,
                                                           const uint8_t *__restrict__ c_codes, int64_t ldc, int d,
                                                           const int64_t *__restrict__ cand, int64_t m, int k, int kp,
                                                           float *__restrict__ out_s, int64_t *__restrict__ out_i,
                                                           int64_t idx_offset, int32_t *__restrict__ status) {
    SlList<int, false> top = sl_shared_list<int, false>();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int shift = 8 * (lane >> 3) + 7 - (lane & 7);   // (SIGN) this lane's element within the 8 bytes of a group
    for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
        double qv[CS_MAXI];
        row_elems_f64<float, CS_MAXI>(qv, xq + q * ldq, d, lane);
        top.reset(kp);
        int beyond = 0;
        for (int64_t b = 0; b < m; b += SL_NB) {
            const int nb = (int)(m - b < SL_NB ? m - b : SL_NB);
            const SlBound<int> w = top.bound(k);
            for (int e = wave; e < nb; e += 4) {   // wave-uniform
                const int64_t r = cand[q * m + b + e];
                beyond |= r >= N;
                if (r < 0 || r >= N) continue;
                double acc = 0.0;
                if constexpr (SIGN) {
                    const unsigned long long *rp = reinterpret_cast<const unsigned long long *>(c_codes + r * ldc);
#pragma unroll
                    for (int i = 0; i < CS_MAXI; ++i) {
                        if (64 * i < d) {   // wave-uniform
                            const bool set = (rp[i] >> shift) & 1;
                            const double term = lane + 64 * i < d ? (set ? qv[i] : -qv[i]) : 0.0;
                            acc = i == 0 ? term : acc + term;
                        }
                    }
                } else {
                    const int8_t *rp = reinterpret_cast<const int8_t *>(c_codes + r * ldc);
                    int c[CS_MAXI];
#pragma unroll
                    for (int i = 0; i < CS_MAXI; ++i) {   // (branch-free loads: the address of an element past d is clamped)
                        const int j = lane + 64 * i;
                        c[i] = 64 * i < d ? (int)rp[j < d ? j : d - 1] : 0;
                    }
#pragma unroll
                    for (int i = 0; i < CS_MAXI; ++i) {
                        if (64 * i < d) {   // wave-uniform
                            const double term = lane + 64 * i < d ? qv[i] * (double)c[i] : 0.0;
                            acc = i == 0 ? term : acc + term;
                        }
                    }
                }
                const float s = (float)wave_sum_f64(acc);
                if (lane == 0) top.offer(s, (int)r, w);
            }
            top.flush(kp);
        }
        const int any_beyond = __syncthreads_or(beyond);
        top.store_result<false>(out_s, out_i, q * k, k, idx_offset);
        if (status && threadIdx.x == 0) status[q] = any_beyond ? TSIM_LIST_ST_ROW : 0;
        __syncthreads();
    }
}

// ----------------------------------------------------------------------------------------------------- host side
// Chunks of one call whose workgroups take G queries each: at most CS_MAX_CHUNKS, of at least max(SL_NB, 4 k) rows, as many as
// bring chunks x groups to CS_WGS workgroups, and no more than keep the chunk lists within CS_BUDGET.
static inline int64_t cs_chunks(int64_t Q, int64_t N, int k, int G) {
    const int64_t groups = (Q + G - 1) / G;
    const int64_t min_rows = std::max<int64_t>(SL_NB, ((int64_t)4 * k + SL_NB - 1) / SL_NB * SL_NB);
    const int64_t fit = (int64_t)(CS_BUDGET / ((size_t)Q * k * 8));
    return std::max<int64_t>(1, std::min<int64_t>({CS_MAX_CHUNKS, (N + min_rows - 1) / min_rows, (CS_WGS + groups - 1) / groups, fit}));
}
// The workspace holds the chunk lists: Q x chunks x k entries of 8 B, scores in one half and rows in the other.  The chunk count
// falls as Q grows, so the size asked for is a bound that does not: with every chunk the corpus allows, capped where the budget
// caps the chunk count.
static inline size_t cs_workspace_half(int64_t Q, int64_t N, int k) {
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(CS_MAX_CHUNKS, (N + SL_NB - 1) / SL_NB));
    const size_t one = (size_t)Q * k * 8;
    return align256(std::min(one * (size_t)cap, std::max(CS_BUDGET, one)) / 2);
}
static inline size_t cs_workspace_bytes(int64_t Q, int64_t N, int k) {
    if (Q <= 0 || N < 0 || k <= 0 || k > TOPK_LARGE_MAX_K) return 0;
    return 2 * cs_workspace_half(Q, N, k);
}

// rows of `width` bytes (what the public function `width_fn` gives for d) read with 16-byte loads
static int cs_check_stride(const char *what, const char *name, const void *codes, int64_t ld, int d, int width, const char *width_fn) {
    TSIM_REQUIRE((reinterpret_cast<uintptr_t>(codes) & 15) == 0, "%s: the rows of %s do not start on a 16-byte boundary", what, name);
    TSIM_REQUIRE(ld % 16 == 0, "%s: %s=%lld is not a multiple of 16", what, name, (long long)ld);
    TSIM_REQUIRE(ld >= width, "%s: %s=%lld < %s(%d)=%d", what, name, (long long)ld, width_fn, d, width);
    return TSIM_OK;
}

// what cs_topk hands the callable that launches the partial kernel
struct CsLaunch {
    dim3 grid;       // (chunks, query groups)
    size_t lds;
    hipStream_t st;
    int64_t rpc;     // rows per chunk
    int G, kp, bc;
    float *ws_s;
    int *ws_i;
};
template <auto KERN, typename... Args>
static int cs_launch_partial(const CsLaunch &l, Args... args) {
    static DevOnce once;
    TSIM_MAX_LDS(once, KERN, 160 * 1024);
    hipLaunchKernelGGL(KERN, l.grid, dim3(256), l.lds, l.st, args...);
    return TSIM_OK;
}

// A top-k entry: the argument checks, the workspace split, the chunks and the grid, `partial(CsLaunch)` and the merge.  `width`
// and `width_fn` as in cs_check_stride; `group(Q, k, d)` the queries of a workgroup, `block_cap(kp)` the entries of a list's block.
template <bool DIST, typename Partial>
static int cs_topk(const char *what, int width, const char *width_fn, int (*group)(int64_t, int, int), int (*block_cap)(int),
                   const void *q_codes, int64_t ldq, int64_t Q, const void *c_codes, int64_t ldc, int64_t N, int d, int k,
                   int32_t *out_v, int64_t *out_idx, int64_t idx_offset, void *workspace, size_t workspace_bytes, void *stream,
                   Partial partial) {
    TSIM_REQUIRE(q_codes && out_v && out_idx && (c_codes || N == 0), "%s: null pointer", what);
    TSIM_REQUIRE(d >= 1 && d <= CS_MAX_D, "%s: d=%d outside 1..%d", what, d, CS_MAX_D);
    TSIM_REQUIRE(k >= 1 && k <= TOPK_LARGE_MAX_K, "%s: k=%d outside 1..%d", what, k, TOPK_LARGE_MAX_K);
    TSIM_REQUIRE(Q > 0 && N >= 0, "%s: bad shape Q=%lld N=%lld", what, (long long)Q, (long long)N);
    TSIM_REQUIRE(N < (1ll << 31) - 64 && Q < (1ll << 31) - 512, "%s: too large for 32-bit row ids", what);
    if (int rc = cs_check_stride(what, "ldq", q_codes, ldq, d, width, width_fn)) return rc;
    if (int rc = cs_check_stride(what, "ldc", c_codes, ldc, d, width, width_fn)) return rc;
    const size_t half = cs_workspace_half(Q, N, k);
    if (!workspace || workspace_bytes < 2 * half) return fail(TSIM_ENOMEM, "%s: workspace %zu B < %zu B", what, workspace_bytes, 2 * half);
    CsLaunch l{};
    l.st = as_stream(stream);
    l.ws_s = reinterpret_cast<float *>(workspace);
    l.ws_i = reinterpret_cast<int *>(reinterpret_cast<char *>(workspace) + half);
    l.kp = sl_list_len(k);
    int64_t nch = 0;
    if (N > 0) {
        l.G = group(Q, k, d);
        const int64_t want = cs_chunks(Q, N, k, l.G);
        l.rpc = ((N + want - 1) / want + SL_NB - 1) / SL_NB * SL_NB;   // whole blocks
        nch = (N + l.rpc - 1) / l.rpc;                                 // (<= want: every chunk holds a row)
        const int64_t groups = (Q + l.G - 1) / l.G;
        TSIM_REQUIRE(groups <= 65535, "%s: Q=%lld needs more than 65535 query groups: slice the queries", what, (long long)Q);
        l.grid = dim3((unsigned)nch, (unsigned)groups);
        l.bc = block_cap(l.kp);
        l.lds = (size_t)l.G * ((size_t)l.kp * 8 + (size_t)l.bc * 8) + (size_t)l.G * 4;   // G lists (hm_list, i8_list), G counters
        if (int rc = partial(l)) return rc;
        TSIM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(code_merge_kernel<DIST>, dim3((unsigned)std::min<int64_t>(Q, 4096)), dim3(256), 0, l.st, Q, nch, k, l.kp, l.ws_s,
                       l.ws_i, out_v, out_idx, idx_offset);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

// a re-score entry
template <bool SIGN>
static int cs_rescore(const char *what, int width, const char *width_fn, const float *eq_f32, int64_t ldq_f32, int64_t Q,
                      const void *c_codes, int64_t ldc, int64_t N, int d, const int64_t *cand, int64_t m, int k, float *out_scores,
                      int64_t *out_idx, int64_t idx_offset, int32_t *out_status, void *stream) {
    TSIM_REQUIRE(eq_f32 && out_scores && out_idx && (c_codes || N == 0) && (cand || m == 0), "%s: null pointer", what);
    TSIM_REQUIRE(d >= 1 && d <= CS_MAX_D, "%s: d=%d outside 1..%d", what, d, CS_MAX_D);
    TSIM_REQUIRE(k >= 1 && k <= TOPK_LARGE_MAX_K, "%s: k=%d outside 1..%d", what, k, TOPK_LARGE_MAX_K);
    TSIM_REQUIRE(Q > 0 && N >= 0 && m >= 0, "%s: bad shape Q=%lld N=%lld m=%lld", what, (long long)Q, (long long)N, (long long)m);
    TSIM_REQUIRE(N < (1ll << 31) - 64, "%s: too large for 32-bit row ids", what);
    TSIM_REQUIRE(ldq_f32 >= d, "%s: ldq_f32=%lld < d=%d", what, (long long)ldq_f32, d);
    if (int rc = cs_check_stride(what, "ldc", c_codes, ldc, d, width, width_fn)) return rc;
    hipLaunchKernelGGL(code_rescore_kernel<SIGN>, dim3((unsigned)std::min<int64_t>(Q, 1 << 20)), dim3(256), 0, as_stream(stream), Q, N,
                       eq_f32, ldq_f32, reinterpret_cast<const uint8_t *>(c_codes), ldc, d, cand, m, k, sl_list_len(k), out_scores,
                       out_idx, idx_offset, out_status);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}
}  // namespace tsim
