// IVF-PQ (included by search.hip, after pq_search.h and ivf_search.h, whose pieces it joins): PQ codes of each row's RESIDUAL to
// its list centroid, stored in inverted lists, and the exact ADC top-k over the lists a query probes; faiss' IndexIVFPQ with 8-bit
// codes (the IVFADC of the PQ paper) is the model.  tests/ivfpq_cases.py restates everything in numpy, bit for bit.
//
// Lists: GpuIVFIndex's packed form (ivf_search.h) — list_off int64 [nlist + 1], row_ids int32 [N] (negative: a tombstone), the
// code rows in list order, tsim_pq_code_bytes(M) or more apart.  probes int64 [Q, nprobe]; an entry < 0 or >= nlist is padding.
//
// Tables.  by_residual = false needs nothing new: tsim_pq_tables, one table a query, no bias.  With residuals:
//   ip:  <q, c_l + r~> = <q, c_l> + <q, r~>: per query L[m][j] as pq_tables' ip table, per probe B[j] = sum_{i < d} (double)q_i
//        (double)c_{l_j},i (pq_dot's ordered, uncontracted sum).  A = max(max |L|, max over valid probes |B|), x = ilogb(A) + 1,
//        e = 23 - ceil(log2(M + 1)) - x, T = rint(L 2^e), bias[q][j] = rint(B[j] 2^e).  |bias| + sum_m max_j |T| < 2^24 (M + 1
//        terms of at most 2^23 / (M + 1) each, plus half a unit of rounding each), so bias + sum_m T[m][code[m]] is an exact int32.
//        ivfpq_tables_ip_kernel: one workgroup per query, two passes over the same arithmetic as pq_tables_kernel; thread t owns
//        the probes t, t + 256, ...
//   l2:  |q - c_l - r~|^2: one table per valid (query, probe) pair, L_p[m][j] = -sqdist(rq_m, cb_mj), rq_i = float32(q_i - c_l,i).
//        A = max |L_p| over all valid pairs of the QUERY: one exponent per query, so the pairs' integer scores compare in the
//        merge; e = 23 - ceil(log2 M) - x.  ivfpq_tables_l2_max_kernel (a workgroup per pair) leaves max |L_p| (+inf for a NaN or an
//        infinity) per pair in the workspace; ivfpq_tables_l2_kernel (a workgroup per pair) reduces its query's nprobe words, then scales,
//        rounds and writes its table.  A maximum does not depend on the order it is taken in.
//   Either: a query with a NaN or an infinity among its entries (valid pairs only), or with A == 0, gets zero tables, zero biases and
//   e = 0.  Tables of padding probes are not written; their bias is 0.
//
// Scan.  score(q, r in probe j) = bias[q][j] + sum_m T[m][code_r[m]], T the table of pair p = q nprobe + j (tables_per_pair) or of
// query q.  ivfpq_scan_partial_kernel<NW>: workgroup (pair p, slot s) copies its table into LDS (M KiB), reads the list's bounds
// through ivf_list_range and walks the segments s, s + nseg, ... (TSIM_IVFPQ_SEG rows each, from the list's own start) as
// pq_adc_partial_kernel walks a chunk: a code row per lane with NW 16-byte loads, the next step's row (and id) loaded before this
// step's lookups, bytes taken with a compile-time index, one ds_read_b32 per sub-quantiser.  (float)(bias + sum) and
// row_ids[position] are offered when the id is >= 0 (a tombstone is loaded and scored and its score dropped); the flush rule is
// the code-search frame's: after the workgroup's first step, after its last, and in between when the block could not take another
// step.  store_raw to slot p nseg + s; a pair without rows for this slot writes padding and copies no table.  The query's
// nprobe nseg slots are consecutive: code_merge_kernel<DIST> is the merge.
//
// Segment length.  A workgroup pays M KiB of table copy for M S bytes of codes: S / 1024 code bytes per table byte, which is
// why TSIM_IVFPQ_SEG is not TSIM_IVF_SEG (at 512 rows a workgroup would read twice as much table as code).
// LDS: M KiB + 32 (ivf_list_range's words) + 8 kp + 8 bc + 4, all dynamic and every carve a multiple of 16.
#pragma once

namespace tsim {
constexpr int IVFPQ_SEG = TSIM_IVFPQ_SEG;
constexpr int IVFPQ_MAX_NSEG = 256;   // slots of one pair
constexpr size_t IVFPQ_BUDGET = (size_t)64 << 20;
static_assert(IVFPQ_SEG % 256 == 0 && IVFPQ_SEG > 0, "a segment is whole steps of 256 rows");

// ceil(log2 n), n >= 1
__host__ __device__ inline int ivfpq_clog(int n) {
    int c = 0;
    while ((1 << c) < n) ++c;
    return c;
}
// the workgroup's maximum of a non-negative double, +inf when any thread saw a NaN or an infinity (`bad`: a maximum carries the
// flag, so no second reduction); red: 4 doubles of LDS, free again on return
__device__ __forceinline__ double ivfpq_block_max(double amax, int bad, double *red) {
    if (bad) amax = (double)INFINITY;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double other = __shfl_xor(amax, o, 64);
        amax = other > amax ? other : amax;
    }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
    __syncthreads();
    amax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return amax;
}
// 2^e for the exponent of a query whose largest entry is A (a normal double: sums of products of float32 values), e itself in `e`
__device__ __forceinline__ double ivfpq_scale(double A, int clog, int &e) {
    const int x = (int)((__double_as_longlong(A) >> 52) & 0x7ff) - 1022;   // ilogb(A) + 1
    e = 23 - clog - x;
    return __longlong_as_double((long long)(e + 1023) << 52);
}

// B[j] of one probe: the ordered sum over the whole row
__device__ __forceinline__ double ivfpq_bias(const float *qs, const float *__restrict__ c, int d) {
    double acc = 0.0;
    for (int i = 0; i < d; ++i) acc = pq_dot(acc, qs[i], c[i]);
    return acc;
}

__global__ __launch_bounds__(256) void ivfpq_tables_ip_kernel(int64_t Q, const float *__restrict__ xq, int64_t ldq,
                                                              const float *__restrict__ cent, int64_t ld_cent, int64_t nlist,
                                                              const int64_t *__restrict__ probes, int nprobe,
                                                              const float *__restrict__ codebooks, int d, int M,
                                                              int32_t *__restrict__ tables, int32_t *__restrict__ bias,
                                                              int32_t *__restrict__ exps) {
    __shared__ float qs[CS_MAX_D];
    __shared__ double red[4];
    const int dsub = d / M, j = threadIdx.x;
    const int clog = ivfpq_clog(M + 1);
    for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {   // workgroup-uniform
        for (int t = j; t < d; t += 256) qs[t] = xq[q * ldq + t];
        __syncthreads();
        double amax = 0.0;
        int bad = 0;
        for (int m = 0; m < M; ++m) {
            const double v = fabs(pq_entry<false>(qs + m * dsub, codebooks + ((int64_t)m * 256 + j) * dsub, dsub));
            bad |= !(v < (double)INFINITY);
            amax = v > amax ? v : amax;
        }
        for (int t = j; t < nprobe; t += 256) {
            const int64_t l = probes[q * nprobe + t];
            if (l < 0 || l >= nlist) continue;
            const double v = fabs(ivfpq_bias(qs, cent + l * ld_cent, d));
            bad |= !(v < (double)INFINITY);
            amax = v > amax ? v : amax;
        }
        amax = ivfpq_block_max(amax, bad, red);
        const bool zero = !(amax < (double)INFINITY) || amax == 0.0;
        int e = 0;
        double scale = 1.0;
        if (!zero) scale = ivfpq_scale(amax, clog, e);
        for (int m = 0; m < M; ++m) {
            int32_t t = 0;
            if (!zero) t = (int32_t)rint(pq_entry<false>(qs + m * dsub, codebooks + ((int64_t)m * 256 + j) * dsub, dsub) * scale);
            tables[(q * M + m) * 256 + j] = t;
        }
        for (int t = j; t < nprobe; t += 256) {
            const int64_t l = probes[q * nprobe + t];
            int32_t b = 0;
            if (!zero && l >= 0 && l < nlist) b = (int32_t)rint(ivfpq_bias(qs, cent + l * ld_cent, d) * scale);
            bias[q * nprobe + t] = b;
        }
        if (j == 0) exps[q] = e;
        __syncthreads();   // qs is rewritten for the next query
    }
}

// the residual query of pair p in LDS; false when the pair has no list (workgroup-uniform)
__device__ __forceinline__ bool ivfpq_residual_query(float *qs, int64_t p, const float *__restrict__ xq, int64_t ldq,
                                                     const float *__restrict__ cent, int64_t ld_cent, int64_t nlist,
                                                     const int64_t *__restrict__ probes, int nprobe, int d) {
    const int64_t l = probes[p];
    if (l < 0 || l >= nlist) return false;
    const int64_t q = p / nprobe;
    for (int t = threadIdx.x; t < d; t += 256) qs[t] = xq[q * ldq + t] - cent[l * ld_cent + t];   // one rounded float32 subtraction
    __syncthreads();
    return true;
}

__global__ __launch_bounds__(256) void ivfpq_tables_l2_max_kernel(int64_t P, const float *__restrict__ xq, int64_t ldq,
                                                                  const float *__restrict__ cent, int64_t ld_cent, int64_t nlist,
                                                                  const int64_t *__restrict__ probes, int nprobe,
                                                                  const float *__restrict__ codebooks, int d, int M,
                                                                  double *__restrict__ pair_max) {
    __shared__ float qs[CS_MAX_D];
    __shared__ double red[4];
    const int dsub = d / M, j = threadIdx.x;
    for (int64_t p = blockIdx.x; p < P; p += gridDim.x) {   // workgroup-uniform
        double amax = 0.0;
        int bad = 0;
        if (ivfpq_residual_query(qs, p, xq, ldq, cent, ld_cent, nlist, probes, nprobe, d)) {
            for (int m = 0; m < M; ++m) {
                const double v = fabs(pq_entry<true>(qs + m * dsub, codebooks + ((int64_t)m * 256 + j) * dsub, dsub));
                bad |= !(v < (double)INFINITY);
                amax = v > amax ? v : amax;
            }
        }
        amax = ivfpq_block_max(amax, bad, red);   // (its barriers also free qs)
        if (j == 0) pair_max[p] = amax;   // +inf: a NaN or an infinity; a padding pair: 0, neutral in the query's reduction
    }
}

__global__ __launch_bounds__(256) void ivfpq_tables_l2_kernel(int64_t P, const float *__restrict__ xq, int64_t ldq,
                                                              const float *__restrict__ cent, int64_t ld_cent, int64_t nlist,
                                                              const int64_t *__restrict__ probes, int nprobe,
                                                              const float *__restrict__ codebooks, int d, int M,
                                                              const double *__restrict__ pair_max,
                                                              int32_t *__restrict__ tables, int32_t *__restrict__ exps) {
    __shared__ float qs[CS_MAX_D];
    __shared__ double red[4];
    const int dsub = d / M, j = threadIdx.x;
    const int clog = ivfpq_clog(M);
    for (int64_t p = blockIdx.x; p < P; p += gridDim.x) {   // workgroup-uniform
        const int64_t q = p / nprobe;
        double amax = 0.0;   // the query's pairs, an infinity among them included
        for (int t = j; t < nprobe; t += 256) {
            const double v = pair_max[q * nprobe + t];
            amax = v > amax ? v : amax;
        }
        amax = ivfpq_block_max(amax, 0, red);
        const bool zero = !(amax < (double)INFINITY) || amax == 0.0;
        int e = 0;
        double scale = 1.0;
        if (!zero) scale = ivfpq_scale(amax, clog, e);
        if (p == q * nprobe && j == 0) exps[q] = e;
        if (ivfpq_residual_query(qs, p, xq, ldq, cent, ld_cent, nlist, probes, nprobe, d)) {
            for (int m = 0; m < M; ++m) {
                int32_t t = 0;
                if (!zero) t = (int32_t)rint(pq_entry<true>(qs + m * dsub, codebooks + ((int64_t)m * 256 + j) * dsub, dsub) * scale);
                tables[(p * M + m) * 256 + j] = t;
            }
        }
        __syncthreads();   // qs is rewritten for the next pair
    }
}

// =====================================================================================================
// the scan
// =====================================================================================================
template <int NW>
__global__ __launch_bounds__(256) void ivfpq_scan_partial_kernel(int64_t N, const int32_t *__restrict__ tables, int per_pair,
                                                                 const int32_t *__restrict__ bias, const uint8_t *__restrict__ c_codes,
                                                                 int64_t ldc, int M, const int64_t *__restrict__ off, int64_t nlist,
                                                                 const int32_t *__restrict__ row_ids,
                                                                 const int64_t *__restrict__ probes, int nprobe, int nseg, int k, int kp,
                                                                 int bc, const int32_t *__restrict__ dirty, float *__restrict__ ws_s,
                                                                 int *__restrict__ ws_i, int32_t *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char ivfpq_smem[];   // the table [M][256] int32, 4 words, the list, its counter
    int *tab = reinterpret_cast<int *>(ivfpq_smem);
    int64_t *red = reinterpret_cast<int64_t *>(ivfpq_smem + (size_t)M * 1024);
    char *lists = ivfpq_smem + (size_t)M * 1024 + 32;
    int *counter = reinterpret_cast<int *>(lists + pq_list_bytes(kp, bc));
    SlList<int, false> list = pq_list(lists, 0, kp, bc, counter);
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
    const int64_t first = lo + (int64_t)s * IVFPQ_SEG, stride = (int64_t)nseg * IVFPQ_SEG;
    if (first < hi) {   // M x 64 16-byte words
        const uint4 *src = reinterpret_cast<const uint4 *>(tables + (per_pair ? p : q) * M * 256);
        for (int t = threadIdx.x; t < M * 64; t += 256) reinterpret_cast<uint4 *>(tab)[t] = src[t];
    }
    list.reset(kp);   // (ends in a barrier: the table is in place)
    if (first < hi) {
        const int b0 = bias ? bias[p] : 0;
        // positions stay in [lo, hi): inside the code rows and inside row_ids
        auto load_row = [&](uint4 (&dst)[NW], int &id, int64_t b, int64_t r1) {
            const int64_t row = b + (int)threadIdx.x < r1 ? b + (int)threadIdx.x : r1 - 1;   // (clamped: loaded and scored, never offered)
            const uint4 *rp = reinterpret_cast<const uint4 *>(c_codes + row * ldc);
#pragma unroll
            for (int w = 0; w < NW; ++w) dst[w] = rp[w];
            id = row_ids[row];
        };
        uint4 rn[NW];
        int idn;
        load_row(rn, idn, first, first + IVFPQ_SEG < hi ? first + IVFPQ_SEG : hi);
        for (int64_t g = first; g < hi; g += stride) {
            const int64_t g1 = g + IVFPQ_SEG < hi ? g + IVFPQ_SEG : hi;
            const bool last_seg = g + stride >= hi;
            for (int64_t b = g; b < g1; b += 256) {   // one step: a row a thread
                const int nb = (int)(g1 - b < 256 ? g1 - b : 256);
                const int e = (int)threadIdx.x;
                uint4 r[NW];
#pragma unroll
                for (int w = 0; w < NW; ++w) r[w] = rn[w];
                const int id = idn;
                // the next step: of this segment, else the first of the workgroup's next segment, else this one again
                const bool more = b + 256 < g1;
                const int64_t nxt = more ? b + 256 : (last_seg ? b : g + stride);
                const int64_t nxt1 = more || last_seg ? g1 : (g + stride + IVFPQ_SEG < hi ? g + stride + IVFPQ_SEG : hi);
                load_row(rn, idn, nxt, nxt1);
                const SlBound<int> bound = list.bound(k);
                int score = b0;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const uint32_t dw[4] = {r[w].x, r[w].y, r[w].z, r[w].w};
#pragma unroll
                    for (int t = 0; t < 16; ++t) {
                        const int m = 16 * w + t;
                        if (w < NW - 1 || m < M) score += tab[m * 256 + (int)((dw[t >> 2] >> (8 * (t & 3))) & 0xffu)];
                    }
                }
                if (e < nb && id >= 0) list.offer((float)score, id, bound);   // (a negative id: scored, dropped)
                // Whether to flush (workgroup-uniform; the counter is read between two barriers): after the workgroup's first step
                // and after its last, otherwise when the block could not take another step's 256 offers.
                bool need = b == first || (last_seg && !more);
                if (!need) {
                    __syncthreads();
                    need = *counter > bc - 256;
                    __syncthreads();
                }
                if (need) list.flush(kp);
            }
        }
    }
    list.store_raw(ws_s, ws_i, (p * nseg + s) * k, k);
}

// Slots per pair, as ivf_nseg: the segments of the longest list the caller expects, at most IVFPQ_MAX_NSEG, and no more than keep
// the slots (8 B an entry) of the call within IVFPQ_BUDGET; at least one.  The workspace holds min(what the hint asks for, the
// budget or one slot per pair): non-decreasing in every argument although nseg itself falls as Q nprobe k grows.
static inline int64_t ivfpq_nseg_wanted(int64_t max_list_len) {
    return std::max<int64_t>(1, std::min<int64_t>((max_list_len + IVFPQ_SEG - 1) / IVFPQ_SEG, IVFPQ_MAX_NSEG));
}
static inline int ivfpq_nseg(int64_t Q, int nprobe, int64_t max_list_len, int k) {
    const size_t one = (size_t)Q * nprobe * k * 8;
    return (int)std::max<int64_t>(1, std::min<int64_t>(ivfpq_nseg_wanted(max_list_len), (int64_t)(IVFPQ_BUDGET / one)));
}
static void plan_workspace_ivfpq(int64_t Q, int nprobe, int64_t max_list_len, int k, IvfWs *w) {
    const size_t one = (size_t)Q * nprobe * k * 8;
    const size_t half = std::min(one * (size_t)ivfpq_nseg_wanted(max_list_len), std::max(IVFPQ_BUDGET, one)) / 2;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    w->dirty = take(4);
    w->ws_s = take(half);
    w->ws_i = take(half);
    w->total = o;
}
static inline bool ivfpq_pairs_ok(int64_t Q, int nprobe) { return Q > 0 && nprobe >= 1 && Q < (1ll << 31) && Q * nprobe < (1ll << 31) - 1; }
}  // namespace tsim

extern "C" size_t tsim_ivfpq_tables_workspace_bytes(int64_t Q, int nprobe) {
    if (!tsim::ivfpq_pairs_ok(Q, nprobe)) return 0;
    return tsim::align256((size_t)Q * nprobe * 8);
}

extern "C" int tsim_ivfpq_tables(int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *centroids, int64_t ld_cent,
                                 int64_t nlist, const int64_t *probes, int nprobe, const float *codebooks, int d, int M,
                                 int32_t *tables, int32_t *bias, int32_t *exps, void *workspace, size_t workspace_bytes,
                                 void *stream) {
    using namespace tsim;
    const char *what = "ivfpq_tables";
    TSIM_REQUIRE(space == TSIM_SPACE_DOT || space == TSIM_SPACE_L2, "%s: space=%d is neither TSIM_SPACE_DOT nor TSIM_SPACE_L2", what, space);
    TSIM_REQUIRE(eq_f32 && centroids && probes && codebooks && tables && exps, "%s: null pointer", what);
    TSIM_REQUIRE(space == TSIM_SPACE_L2 || bias, "%s: the inner product needs bias", what);
    TSIM_REQUIRE(pq_shape_ok(d, M), "%s: d=%d M=%d: needs 1 <= d <= %d, 1 <= M <= %d, d %% M == 0 and d / M <= %d", what, d, M, CS_MAX_D,
                 PQ_MAX_M, PQ_MAX_DSUB);
    TSIM_REQUIRE(nprobe >= 1, "%s: nprobe=%d < 1", what, nprobe);
    TSIM_REQUIRE(Q >= 0 && nlist > 0 && ldq_f32 >= d && ld_cent >= d, "%s: bad shape Q=%lld nlist=%lld d=%d ldq_f32=%lld ld_cent=%lld", what,
                 (long long)Q, (long long)nlist, d, (long long)ldq_f32, (long long)ld_cent);
    TSIM_REQUIRE(Q == 0 || ivfpq_pairs_ok(Q, nprobe), "%s: too large for one launch (Q nprobe=%lld)", what, (long long)(Q * nprobe));
    TSIM_REQUIRE((reinterpret_cast<uintptr_t>(tables) & 15) == 0, "%s: tables do not start on a 16-byte boundary", what);
    if (Q == 0) return TSIM_OK;
    hipStream_t st = as_stream(stream);
    if (space == TSIM_SPACE_DOT) {
        hipLaunchKernelGGL(ivfpq_tables_ip_kernel, dim3((unsigned)std::min<int64_t>(Q, 1 << 16)), dim3(256), 0, st, Q, eq_f32, ldq_f32,
                           centroids, ld_cent, nlist, probes, nprobe, codebooks, d, M, tables, bias, exps);
        TSIM_HIP_CHECK(hipGetLastError());
        return TSIM_OK;
    }
    const int64_t P = Q * nprobe;
    const size_t need = tsim_ivfpq_tables_workspace_bytes(Q, nprobe);
    if (!workspace || workspace_bytes < need) return fail(TSIM_ENOMEM, "%s: workspace %zu B < %zu B", what, workspace_bytes, need);
    double *pair_max = reinterpret_cast<double *>(workspace);
    const dim3 grid((unsigned)std::min<int64_t>(P, 1 << 20));
    hipLaunchKernelGGL(ivfpq_tables_l2_max_kernel, grid, dim3(256), 0, st, P, eq_f32, ldq_f32, centroids, ld_cent, nlist, probes, nprobe,
                       codebooks, d, M, pair_max);
    TSIM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ivfpq_tables_l2_kernel, grid, dim3(256), 0, st, P, eq_f32, ldq_f32, centroids, ld_cent, nlist, probes, nprobe,
                       codebooks, d, M, pair_max, tables, exps);
    TSIM_HIP_CHECK(hipGetLastError());
    if (bias) TSIM_HIP_CHECK(hipMemsetAsync(bias, 0, (size_t)P * 4, st));
    return TSIM_OK;
}

extern "C" size_t tsim_ivfpq_scan_workspace_bytes(int64_t Q, int nprobe, int64_t max_list_len, int k) {
    if (Q <= 0 || nprobe <= 0 || max_list_len < 0 || k <= 0 || k > tsim::TOPK_LARGE_MAX_K) return 0;
    tsim::IvfWs w;
    tsim::plan_workspace_ivfpq(Q, nprobe, max_list_len, k, &w);
    return w.total;
}

extern "C" int tsim_ivfpq_scan_topk(int space, const int32_t *tables, int tables_per_pair, const int32_t *bias, int64_t Q,
                                    const uint8_t *c_codes, int64_t ldc, int64_t N, int M, const int64_t *list_off, int64_t nlist,
                                    const int32_t *row_ids, const int64_t *probes, int nprobe, int64_t max_list_len, int k,
                                    int32_t *out_val, int64_t *out_idx, int64_t idx_offset, int32_t *out_status, void *workspace,
                                    size_t workspace_bytes, void *stream) {
    using namespace tsim;
    const char *what = "ivfpq_scan_topk";
    TSIM_REQUIRE(space == TSIM_SPACE_DOT || space == TSIM_SPACE_L2, "%s: space=%d is neither TSIM_SPACE_DOT nor TSIM_SPACE_L2", what, space);
    TSIM_REQUIRE(tables && c_codes && list_off && row_ids && probes && out_val && out_idx, "%s: null pointer", what);
    TSIM_REQUIRE(M >= 1 && M <= PQ_MAX_M, "%s: M=%d outside 1..%d", what, M, PQ_MAX_M);
    TSIM_REQUIRE(nprobe >= 1, "%s: nprobe=%d < 1", what, nprobe);
    TSIM_REQUIRE(k >= 1 && k <= TOPK_LARGE_MAX_K, "%s: k=%d outside 1..%d", what, k, TOPK_LARGE_MAX_K);
    TSIM_REQUIRE(Q > 0 && N > 0 && nlist > 0 && max_list_len >= 0, "%s: bad shape Q=%lld N=%lld nlist=%lld max_list_len=%lld", what,
                 (long long)Q, (long long)N, (long long)nlist, (long long)max_list_len);
    TSIM_REQUIRE(N < (1ll << 31) - 64 && nlist < (1ll << 40) && ivfpq_pairs_ok(Q, nprobe),
                 "%s: too large for one launch (N=%lld, Q nprobe=%lld)", what, (long long)N, (long long)(Q * nprobe));
    TSIM_REQUIRE((reinterpret_cast<uintptr_t>(tables) & 15) == 0, "%s: tables do not start on a 16-byte boundary", what);
    if (int rc = cs_check_stride(what, "ldc", c_codes, ldc, M, pq_code_bytes(M), "tsim_pq_code_bytes")) return rc;
    IvfWs w;
    plan_workspace_ivfpq(Q, nprobe, max_list_len, k, &w);
    if (!workspace || workspace_bytes < w.total) return fail(TSIM_ENOMEM, "%s: workspace %zu B < %zu B", what, workspace_bytes, w.total);
    CsLaunch l{};
    l.st = as_stream(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    int32_t *dirty = reinterpret_cast<int32_t *>(ws + w.dirty);
    l.ws_s = reinterpret_cast<float *>(ws + w.ws_s);
    l.ws_i = reinterpret_cast<int *>(ws + w.ws_i);
    l.kp = sl_list_len(k);
    l.bc = pq_block_cap(l.kp);
    const int nseg = ivfpq_nseg(Q, nprobe, max_list_len, k);
    hipLaunchKernelGGL(ivf_prep_kernel, dim3(1), dim3(IVF_PREP_T), 0, l.st, Q, N, list_off, nlist, dirty, out_status);
    TSIM_HIP_CHECK(hipGetLastError());
    l.grid = dim3((unsigned)(Q * nprobe), (unsigned)nseg);
    l.lds = (size_t)M * 1024 + 32 + pq_list_bytes(l.kp, l.bc) + 4;
    const int per_pair = tables_per_pair ? 1 : 0;
    switch (pq_code_bytes(M) / 16) {
#define TSIM_IVFPQ_CASE(NW)                                                                                                        \
    case NW:                                                                                                                       \
        cs_launch_partial<ivfpq_scan_partial_kernel<NW>>(l, N, tables, per_pair, bias, c_codes, ldc, M, list_off, nlist, row_ids,  \
                                                         probes, nprobe, nseg, k, l.kp, l.bc, (const int32_t *)dirty, l.ws_s,     \
                                                         l.ws_i, out_status);                                                      \
        break;
        TSIM_IVFPQ_CASE(1) TSIM_IVFPQ_CASE(2) TSIM_IVFPQ_CASE(3) TSIM_IVFPQ_CASE(4)
#undef TSIM_IVFPQ_CASE
    }
    TSIM_HIP_CHECK(hipGetLastError());
    const int64_t nch = (int64_t)nprobe * nseg;
    const dim3 mg((unsigned)std::min<int64_t>(Q, 4096));
    if (space == TSIM_SPACE_L2)
        hipLaunchKernelGGL(code_merge_kernel<true>, mg, dim3(256), 0, l.st, Q, nch, k, l.kp, l.ws_s, l.ws_i, out_val, out_idx, idx_offset);
    else
        hipLaunchKernelGGL(code_merge_kernel<false>, mg, dim3(256), 0, l.st, Q, nch, k, l.kp, l.ws_s, l.ws_i, out_val, out_idx, idx_offset);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}
