// Product quantisation (included by search.hip, after code_search.h, whose frame it fills in): the PQ encoder, the per-query
// lookup tables and the exact ADC (asymmetric distance computation) top-k; faiss' IndexPQ with 8-bit codes is the model.
//
// Codebooks.  float32 [M, 256, dsub] contiguous, dsub = d / M: 1 <= d <= 1024, 1 <= M <= 64, d % M == 0, dsub <= 64; finite (the
// callers check that where codebooks enter).  A code row is M bytes, byte m the centroid number of sub-vector m.  Rows lie
// tsim_pq_code_bytes(M) = M rounded up to 16 bytes apart (or more: every stride is a multiple of 16), so a row is read with 16-byte
// loads; the bytes from M to tsim_pq_code_bytes(M) are zero in everything written here and are never read as sub-quantisers.
//
// Everything is defined bit for bit (tests/pq_cases.py restates it in numpy):
//   dist(x, c) in float64: dist = 0; for i = 0 .. dsub - 1: t = (double)x_i - (double)c_i, p = t t, dist = dist + p, each one
//     rounded IEEE operation, never contracted to an FMA (pq_sqdist, pq_dot: #pragma clang fp contract(off)).
//   code = the first j with dist_j < best, best = +inf at the start: ties go to the lower j, a sub-vector with a NaN or an infinity
//     gets code 0 (no comparison with +inf or NaN holds).
//   L[m][j] = sum_i q_i c_i (ip; the same ordered sum, the products are exact) or -dist (l2).  A = max |L| over the query's table.
//     A zero, NaN or infinite: the table is all zero and e = 0.  Otherwise x = ilogb(A) + 1 (A < 2^x), e = 23 - ceil(log2 M) - x,
//     T[m][j] = (int32) rint(L[m][j] 2^e), half to even.  Then sum_m max_j |T[m][j]| <= 2^23 + M / 2 < 2^24.
//   score(q, r) = sum_m T_q[m][code_r[m]], an int32 that no order of the additions changes, exact as a float32: the running list
//     (SlList: score desc, index asc) carries it unchanged, and "exact" is the true top-k under (score desc, row asc).  For l2 the
//     scores are <= 0 and the same list order is (-score asc, row asc); code_merge_kernel<true> writes -score.
//
// Work.
//   pq_encode_rows_kernel: workgroup (row block, sub-space m) holds sub-space m's codebook in LDS (256 dsub floats, <= 64 KiB); a
//     lane owns one row at a time, its dsub elements in registers, and walks the 256 centroids (every lane reads the same LDS
//     word: a broadcast).  Once per corpus.
//   pq_tables_kernel: one workgroup per query, thread j owns centroid j of every sub-space.  Two passes over the same arithmetic:
//     the first finds A (wave butterfly, then LDS), the second scales, rounds and writes — no M entries a thread to keep.
//   pq_adc_partial_kernel<NW> (NW = ceil(M / 16) 16-byte words per code row), in the frame of code_search.h with ONE query a
//     workgroup: workgroup (chunk c, query q) copies the query's int32 table into LDS (M KiB), then walks its rows as
//     hamming_partial_kernel does: every lane loads one row ONCE with 16-byte loads (the next step's row before this step's
//     lookups) and sums M ds_read_b32 lookups; byte m comes out of a register with a compile-time index (the loop over m is
//     unrolled; the last word's bytes are guarded by the workgroup-uniform m < M).  The list (pq_list) and its flushes follow the
//     frame's protocol; a step is 256 rows.
//
// G = 1 (pq_group).  LDS of a workgroup: M KiB + 8 kp + 8 bc + 4 — 52.6 KiB at (M, k) = (48, 10), three workgroups a CU; at most
// 81 924 B, at (64, 1 024), within the 160 KiB that cs_launch_partial opts every partial kernel in to.  The lookups, Q N M of
// them, and the table copies (chunks x Q) do not depend on G; a group would only spare re-reading the code rows, 16 NW bytes
// against M lookups.  Tried and dropped (profiles/pq_ab.txt): the entries of TWO queries side by side, one
// ds_read_b64 for both (64 banks instead of 32, address arithmetic paid once) — two tables leave a CU one workgroup where one
// table leaves three, and with the row prefetch in both it lost at every size measured: N = 1 M, k = 10, one table / two, ms:
// M = 48: Q = 256 3.84 / 4.25, Q = 4096 59.0 / 61.9; M = 64: Q = 256 4.46 / 4.78, Q = 4096 68.5 / 70.0 (Q = 16, before the
// prefetch: 0.43 / 0.54).  So bank conflicts are not what bounds the scan; what does was not profiled.
#pragma once

namespace tsim {
constexpr int PQ_MAX_M = 64;       // sub-quantisers at most
constexpr int PQ_MAX_DSUB = 64;    // elements of a sub-vector at most: a codebook of 256 x 64 floats is 64 KiB of LDS

__host__ __device__ inline int pq_code_bytes(int M) { return M >= 1 && M <= PQ_MAX_M ? (M + 15) / 16 * 16 : 0; }
static inline bool pq_shape_ok(int d, int M) {
    return d >= 1 && d <= CS_MAX_D && M >= 1 && M <= PQ_MAX_M && d % M == 0 && d / M <= PQ_MAX_DSUB;
}
// Entries of a list's block: 512 for short lists, SL_NB for long ones — the rule i8_block_cap measured (a copy, like pq_list below:
// a helper shared with the int8 kernels moved all 16 of them off the instructions they compiled to).
static inline int pq_block_cap(int kp) { return kp <= 128 ? 512 : SL_NB; }
// one running list per query in dynamic LDS, laid out as i8_list's (top_s, top_i: kp entries; blk_s, blk_i: bc), the counters
// behind all lists
__host__ __device__ inline size_t pq_list_bytes(int kp, int bc) { return (size_t)kp * 8 + (size_t)bc * 8; }
__device__ __forceinline__ SlList<int, false> pq_list(char *lists, int g, int kp, int bc, int *counters) {
    char *base = lists + (size_t)g * pq_list_bytes(kp, bc);
    float *top_s = reinterpret_cast<float *>(base);
    int *top_i = reinterpret_cast<int *>(top_s + kp);
    float *blk_s = reinterpret_cast<float *>(top_i + kp);
    int *blk_i = reinterpret_cast<int *>(blk_s + bc);
    return {top_s, blk_s, nullptr, top_i, blk_i, nullptr, counters + g, nullptr};
}
static inline int pq_group(int64_t, int, int) { return 1; }   // one query a workgroup (above)

// one step of the ordered float64 sums (above)
__device__ __forceinline__ double pq_sqdist(double dist, float x, float c) {
#pragma clang fp contract(off)
    const double t = (double)x - (double)c;
    const double p = t * t;
    return dist + p;
}
__device__ __forceinline__ double pq_dot(double acc, float x, float c) {
#pragma clang fp contract(off)
    const double p = (double)x * (double)c;
    return acc + p;
}

// =====================================================================================================
// pq_encode_rows
// =====================================================================================================
template <typename T>
__global__ __launch_bounds__(256) void pq_encode_rows_kernel(const T *__restrict__ x, int64_t rows, int d, int64_t ld_in,
                                                             const float *__restrict__ codebooks, int M,
                                                             uint8_t *__restrict__ codes, int64_t ld_code) {
    extern __shared__ __attribute__((aligned(16))) char pq_enc_smem[];
    float *cs = reinterpret_cast<float *>(pq_enc_smem);   // [256][dsub]
    const int dsub = d / M, m = blockIdx.y;
    for (int t = threadIdx.x; t < 256 * dsub; t += 256) cs[t] = codebooks[(int64_t)m * 256 * dsub + t];
    __syncthreads();
    const int cb = pq_code_bytes(M);
    for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < rows; row += (int64_t)gridDim.x * 256) {
        const T *xp = x + row * ld_in + m * dsub;
        float xv[PQ_MAX_DSUB];
#pragma unroll
        for (int i = 0; i < PQ_MAX_DSUB; ++i) xv[i] = i < dsub ? load_as_f32<T>(xp + i) : 0.f;
        double best = INFINITY;
        int code = 0;
        for (int j = 0; j < 256; ++j) {
            const float *c = cs + j * dsub;
            double dist = 0.0;
#pragma unroll
            for (int i = 0; i < PQ_MAX_DSUB; ++i)
                if (i < dsub) dist = pq_sqdist(dist, xv[i], c[i]);   // (workgroup-uniform; a constant trip count keeps xv in registers)
            if (dist < best) {
                best = dist;
                code = j;
            }
        }
        uint8_t *out = codes + row * ld_code;
        out[m] = (uint8_t)code;
        if (m == M - 1)
            for (int b = M; b < cb; ++b) out[b] = 0;   // the pad bytes, by the last sub-space's workgroup
    }
}

// =====================================================================================================
// pq_tables
// =====================================================================================================
template <bool L2>
__device__ __forceinline__ double pq_entry(const float *q, const float *__restrict__ c, int dsub) {
    double acc = 0.0;
    for (int i = 0; i < dsub; ++i) acc = L2 ? pq_sqdist(acc, q[i], c[i]) : pq_dot(acc, q[i], c[i]);
    return L2 ? -acc : acc;
}

template <bool L2>
__global__ __launch_bounds__(256) void pq_tables_kernel(int64_t Q, const float *__restrict__ xq, int64_t ldq,
                                                        const float *__restrict__ codebooks, int d, int M,
                                                        int32_t *__restrict__ tables, int32_t *__restrict__ exps) {
    __shared__ float qs[CS_MAX_D];
    __shared__ double red[4];
    const int dsub = d / M, j = threadIdx.x, lane = j & 63, wave = j >> 6;
    int clog = 0;   // ceil(log2 M)
    while ((1 << clog) < M) ++clog;
    for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {   // workgroup-uniform
        for (int t = j; t < d; t += 256) qs[t] = xq[q * ldq + t];
        __syncthreads();
        double amax = 0.0;
        int bad = 0;
        for (int m = 0; m < M; ++m) {
            const double v = fabs(pq_entry<L2>(qs + m * dsub, codebooks + ((int64_t)m * 256 + j) * dsub, dsub));
            bad |= !(v < (double)INFINITY);   // NaN or infinite
            amax = v > amax ? v : amax;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double other = __shfl_xor(amax, o, 64);
            amax = other > amax ? other : amax;
        }
        if (lane == 0) red[wave] = amax;
        const bool any_bad = __syncthreads_or(bad) != 0;   // (the barrier also publishes red)
        amax = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
        const bool zero_table = any_bad || amax == 0.0;
        int e = 0;
        if (!zero_table) {
            // A is a sum of products of float32 values: a normal double, its biased exponent field is ilogb(A) + 1023
            const int x = (int)((__double_as_longlong(amax) >> 52) & 0x7ff) - 1022;
            e = 23 - clog - x;
        }
        const double scale = __longlong_as_double((long long)(e + 1023) << 52);   // 2^e: |e| stays far below 1023
        for (int m = 0; m < M; ++m) {
            int32_t t = 0;
            if (!zero_table) t = (int32_t)rint(pq_entry<L2>(qs + m * dsub, codebooks + ((int64_t)m * 256 + j) * dsub, dsub) * scale);
            tables[(q * M + m) * 256 + j] = t;
        }
        if (j == 0) exps[q] = e;
        __syncthreads();   // qs and red are rewritten for the next query
    }
}

// =====================================================================================================
// ADC top-k
// =====================================================================================================
template <int NW>
__global__ __launch_bounds__(256) void pq_adc_partial_kernel(int64_t N, int64_t rows_per_chunk, const int32_t *__restrict__ tables,
                                                             const uint8_t *__restrict__ c_codes, int64_t ldc, int M, int k, int kp,
                                                             int bc, float *__restrict__ ws_s, int *__restrict__ ws_i) {
    extern __shared__ __attribute__((aligned(16))) char pq_smem[];   // the query's table [M][256] int32, its list, its counter
    int *tab = reinterpret_cast<int *>(pq_smem);
    char *lists = pq_smem + (size_t)M * 1024;
    int *counter = reinterpret_cast<int *>(lists + pq_list_bytes(kp, bc));
    SlList<int, false> list = pq_list(lists, 0, kp, bc, counter);
    const int64_t nch = gridDim.x, chunk = blockIdx.x, q = blockIdx.y;
    const int64_t r0 = chunk * rows_per_chunk;
    const int64_t r1 = r0 + rows_per_chunk < N ? r0 + rows_per_chunk : N;
    {   // M x 64 16-byte words
        const uint4 *src = reinterpret_cast<const uint4 *>(tables + q * M * 256);
        for (int t = threadIdx.x; t < M * 64; t += 256) reinterpret_cast<uint4 *>(tab)[t] = src[t];
    }
    list.reset(kp);   // (ends in a barrier: the table is in place)
    // the row of the NEXT step is loaded before this step's lookups, so the load is in flight under them (N = 1 M, M = 48, k = 10:
    // Q = 16 0.37 ms against 0.43 without, Q = 4096 59.0 against 71.0)
    auto load_row = [&](uint4 (&dst)[NW], int64_t b) {
        const int64_t row = b + (int)threadIdx.x < r1 ? b + (int)threadIdx.x : r1 - 1;   // (clamped: loaded and scored, never offered)
        const uint4 *rp = reinterpret_cast<const uint4 *>(c_codes + row * ldc);
#pragma unroll
        for (int w = 0; w < NW; ++w) dst[w] = rp[w];
    };
    uint4 rn[NW];
    load_row(rn, r0);
    for (int64_t b = r0; b < r1; b += 256) {   // one step: a row a thread
        const int nb = (int)(r1 - b < 256 ? r1 - b : 256);
        const int e = (int)threadIdx.x;
        uint4 r[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) r[w] = rn[w];
        load_row(rn, b + 256 < r1 ? b + 256 : b);
        const SlBound<int> bound = list.bound(k);
        int score = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const uint32_t dw[4] = {r[w].x, r[w].y, r[w].z, r[w].w};
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int m = 16 * w + t;
                if (w < NW - 1 || m < M) score += tab[m * 256 + (int)((dw[t >> 2] >> (8 * (t & 3))) & 0xffu)];
            }
        }
        if (e < nb) list.offer((float)score, (int)(b + e), bound);
        // Whether to flush (workgroup-uniform; the counter is read between two barriers): after the chunk's first step and after
        // the last, otherwise when the block could not take another step's 256 offers.
        bool need = b == r0 || b + 256 >= r1;
        if (!need) {
            __syncthreads();
            need = *counter > bc - 256;
            __syncthreads();
        }
        if (need) list.flush(kp);
    }
    list.store_raw(ws_s, ws_i, (q * nch + chunk) * k, k);
}
}  // namespace tsim

extern "C" int tsim_pq_code_bytes(int M) { return tsim::pq_code_bytes(M); }

extern "C" int tsim_pq_encode_rows(const void *x, int x_dtype, int64_t rows, int d, int64_t ld_in, const float *codebooks, int M,
                                   uint8_t *codes, int64_t ld_code, void *stream) {
    using namespace tsim;
    const char *what = "pq_encode_rows";
    TSIM_REQUIRE(x && codebooks && codes, "%s: null pointer", what);
    TSIM_REQUIRE(pq_shape_ok(d, M), "%s: d=%d M=%d: needs 1 <= d <= %d, 1 <= M <= %d, d %% M == 0 and d / M <= %d", what, d, M, CS_MAX_D,
                 PQ_MAX_M, PQ_MAX_DSUB);
    TSIM_REQUIRE(rows >= 0 && rows < (1ll << 31) - 64 && ld_in >= d, "%s: bad shape rows=%lld d=%d ld_in=%lld", what, (long long)rows, d,
                 (long long)ld_in);
    TSIM_REQUIRE(x_dtype == TSIM_F32 || x_dtype == TSIM_BF16, "%s: unknown x_dtype %d", what, x_dtype);
    if (int rc = cs_check_stride(what, "ld_code", codes, ld_code, M, pq_code_bytes(M), "tsim_pq_code_bytes")) return rc;
    if (rows == 0) return TSIM_OK;
    const dim3 grid((unsigned)std::min<int64_t>((rows + 255) / 256, 256), (unsigned)M);
    const size_t lds = (size_t)256 * (d / M) * 4;
    if (x_dtype == TSIM_F32) {
        static DevOnce once;
        TSIM_MAX_LDS(once, pq_encode_rows_kernel<float>, 64 * 1024);
        hipLaunchKernelGGL(pq_encode_rows_kernel<float>, grid, dim3(256), lds, as_stream(stream), (const float *)x, rows, d, ld_in,
                           codebooks, M, codes, ld_code);
    } else {
        static DevOnce once;
        TSIM_MAX_LDS(once, pq_encode_rows_kernel<bf16_t>, 64 * 1024);
        hipLaunchKernelGGL(pq_encode_rows_kernel<bf16_t>, grid, dim3(256), lds, as_stream(stream), (const bf16_t *)x, rows, d, ld_in,
                           codebooks, M, codes, ld_code);
    }
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

extern "C" int tsim_pq_tables(int space, const float *eq_f32, int64_t ldq_f32, int64_t Q, const float *codebooks, int d, int M,
                              int32_t *tables, int32_t *exps, void *stream) {
    using namespace tsim;
    const char *what = "pq_tables";
    TSIM_REQUIRE(eq_f32 && codebooks && tables && exps, "%s: null pointer", what);
    TSIM_REQUIRE(space == TSIM_SPACE_DOT || space == TSIM_SPACE_L2, "%s: space=%d is neither TSIM_SPACE_DOT nor TSIM_SPACE_L2", what, space);
    TSIM_REQUIRE(pq_shape_ok(d, M), "%s: d=%d M=%d: needs 1 <= d <= %d, 1 <= M <= %d, d %% M == 0 and d / M <= %d", what, d, M, CS_MAX_D,
                 PQ_MAX_M, PQ_MAX_DSUB);
    TSIM_REQUIRE(Q >= 0 && Q < (1ll << 31) - 512 && ldq_f32 >= d, "%s: bad shape Q=%lld d=%d ldq_f32=%lld", what, (long long)Q, d,
                 (long long)ldq_f32);
    TSIM_REQUIRE((reinterpret_cast<uintptr_t>(tables) & 15) == 0, "%s: tables do not start on a 16-byte boundary", what);
    if (Q == 0) return TSIM_OK;
    const dim3 grid((unsigned)std::min<int64_t>(Q, 1 << 16));
    if (space == TSIM_SPACE_L2)
        hipLaunchKernelGGL(pq_tables_kernel<true>, grid, dim3(256), 0, as_stream(stream), Q, eq_f32, ldq_f32, codebooks, d, M, tables, exps);
    else
        hipLaunchKernelGGL(pq_tables_kernel<false>, grid, dim3(256), 0, as_stream(stream), Q, eq_f32, ldq_f32, codebooks, d, M, tables, exps);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

extern "C" size_t tsim_pq_adc_topk_workspace_bytes(int64_t Q, int64_t N, int M, int k) {
    return tsim::pq_code_bytes(M) ? tsim::cs_workspace_bytes(Q, N, k) : 0;
}

extern "C" int tsim_pq_adc_topk(int space, const int32_t *tables, int64_t Q, const uint8_t *c_codes, int64_t ldc, int64_t N, int M, int k,
                                int32_t *out_val, int64_t *out_idx, int64_t idx_offset, void *workspace, size_t workspace_bytes,
                                void *stream) {
    using namespace tsim;
    const char *what = "pq_adc_topk";
    TSIM_REQUIRE(space == TSIM_SPACE_DOT || space == TSIM_SPACE_L2, "%s: space=%d is neither TSIM_SPACE_DOT nor TSIM_SPACE_L2", what, space);
    TSIM_REQUIRE(M >= 1 && M <= PQ_MAX_M, "%s: M=%d outside 1..%d", what, M, PQ_MAX_M);
    // the frame sees the tables as the "query codes": rows of M x 1024 bytes, a multiple of 16 whatever M
    auto partial = [&](const CsLaunch &frame) {
        CsLaunch l = frame;
        l.lds += (size_t)M * 1024;   // the table in front of the list (G = 1)
        switch (pq_code_bytes(M) / 16) {
#define TSIM_PQ_CASE(NW)                                                                                                          \
    case NW:                                                                                                                      \
        return cs_launch_partial<pq_adc_partial_kernel<NW>>(l, N, l.rpc, tables, c_codes, ldc, M, k, l.kp, l.bc, l.ws_s, l.ws_i);
            TSIM_PQ_CASE(1) TSIM_PQ_CASE(2) TSIM_PQ_CASE(3) TSIM_PQ_CASE(4)
#undef TSIM_PQ_CASE
        }
        return (int)TSIM_OK;
    };
    if (space == TSIM_SPACE_L2)
        return cs_topk<true>(what, pq_code_bytes(M), "tsim_pq_code_bytes", pq_group, pq_block_cap, tables, (int64_t)M * 1024, Q, c_codes, ldc,
                             N, M, k, out_val, out_idx, idx_offset, workspace, workspace_bytes, stream, partial);
    return cs_topk<false>(what, pq_code_bytes(M), "tsim_pq_code_bytes", pq_group, pq_block_cap, tables, (int64_t)M * 1024, Q, c_codes, ldc, N,
                          M, k, out_val, out_idx, idx_offset, workspace, workspace_bytes, stream, partial);
}
