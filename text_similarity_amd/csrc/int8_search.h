// int8 embeddings (included by search.hip, after hamming_search.h, whose chunk budget and workspace rule it uses): the calibrated
// scalar quantiser, exact inner-product top-k on the int8 matrix pipe, and the re-score of its candidates with the float32 query
// against the code values.
//
// Codes.  A code row is d int8 values, 1 <= d <= 1024.  Rows lie tsim_int8_bytes(d) = d rounded up to 16 bytes apart (or more:
// every stride is a multiple of 16), so a row is read with 16-byte loads; the bytes from d to tsim_int8_bytes(d) are zero in
// everything written here.  No kernel relies on that: the QUERY bytes at positions >= d are zeroed in registers, and in integers
// 0 x junk = 0, so the corpus side needs no mask at all.
//
// The score sum_j q_j c_j is an integer with |score| <= 128 x 128 x 1024 = 2^24: exact in int32 and exact as a float32, so the
// running list (SlList: score desc, index asc) carries it unchanged and "exact" is the true top-k under (score desc, row asc).
//
// Work.  int8_ip_partial_kernel<KS> (KS = ceil(d / 64) k-steps of v_mfma_i32_16x16x64_i8): workgroup (chunk c, group g) owns
// rows_per_chunk rows and the ng <= G queries g G .. g G + ng - 1.  Every wave keeps the group's queries resident as the B
// fragments: in k-step s lane l holds bytes 64 s + 16 (l >> 4) .. + 15 of query l & 15 (KS x 4 VGPRs).  A wave takes 16 corpus
// rows at a time: lane l loads THE SAME 16-byte slice of row l & 15 straight from global memory as the A fragment — no LDS
// staging: a row is used once per workgroup.  Both operands follow one byte -> (lane, element) rule, so whatever order the
// hardware gives the 64 k values inside a step, each corpus byte meets the query byte of its own position and the sum over k is
// right; tests/test_int8_gpu.py checks that with asymmetric one-hot data, it is not assumed.  C/D: column l & 15 is the
// query, row 4 (l >> 4) + reg the corpus row (the map of every 16x16 MFMA on gfx950): each lane offers its four scores to the
// list of its query.  The tile of the NEXT 16 rows is loaded before the current one is multiplied and offered, so a wave has two
// tiles of loads in flight (16 lists leave room for two workgroups a CU at the most).
//
// Lists and flushes: those of hamming_partial_kernel.  One SlList per query in dynamic LDS (i8_list), a step is 256 rows (four
// tiles a wave), a list is flushed after the chunk's first step, after the last, and in between only when its block could not
// take the 256 offers of another step.  A block holds bc = 512 or SL_NB entries (i8_block_cap).  G (i8_group): at most 16
// while k <= 64, else 8 (the other eight columns of the tile are zero and never offered).  Chunks and workspace: hm_chunks'
// rules with this G.
// int8_ip_merge_kernel is hamming_merge_kernel writing int32 scores, padding (INT32_MIN, -1).
#pragma once

namespace tsim {
constexpr int I8_MAX_D = 1024;
constexpr int I8_STEP = 256;   // rows of one step of the partial kernel: 4 waves x 4 tiles x 16 rows

__host__ __device__ inline int i8_bytes(int d) { return d >= 1 && d <= I8_MAX_D ? (d + 15) / 16 * 16 : 0; }
// Queries of one workgroup: at most 16 while k <= 64, else 8, and for a small query set fewer, so that several groups exist:
// ceil(Q / 4) a group for rows up to 512 bytes, ceil(Q / 2) beyond (every group reads the whole corpus once more, and a wide row
// makes that pass dearer than the lists it spares: at Q = 16, N = 1 M, d = 1024 two groups took 0.64 ms, four 0.81, one 0.76; at
// d = 384 four groups 0.41, two 0.46, one 0.69).
static inline int i8_group_cap(int k) { return k <= 64 ? 16 : 8; }
static inline int i8_group(int64_t Q, int k, int d) {
    const int D = i8_bytes(d) > 512 ? 2 : 4;
    return (int)std::max<int64_t>(1, std::min<int64_t>(i8_group_cap(k), (Q + D - 1) / D));
}
// Entries of a list's block (what is offered between two flushes).  Short lists take 512, not SL_NB: 16 lists of k <= 64 then
// take 73 KiB instead of 136, two workgroups share a CU and one's flushes hide behind the other's loads — at N = 1 M, d = 384,
// k = 10: Q = 256 1.65 ms against 3.36, Q = 4096 11.3 against 16.9; k = 100 (eight lists): 2.18 against 2.50.  Long lists (k = 1024:
// 12.0 ms against 10.2 at Q = 256) keep SL_NB: they fill a block of 512 every other step whatever their bound.
static inline int i8_block_cap(int kp) { return kp <= 128 ? 512 : SL_NB; }

typedef int i8x16_t __attribute__((ext_vector_type(4)));   // 16 int8 values: one A or B fragment of a k-step
typedef int i32x4_t __attribute__((ext_vector_type(4)));   // the C/D fragment

// =====================================================================================================
// quantize_int8_rows: sentence-transformers' quantize_embeddings(precision="int8") in float32,
//   start = ranges[0], step = (ranges[1] - ranges[0]) / 255, t = (x - start) / step - 128, code = trunc(t),
// with t saturated to [-128, 127] (+-inf included) and NaN -> 0, where numpy's cast is undefined.  One wave per row: lane l
// quantises elements l, l + 64, .. (coalesced reads; the columns' start and step stay in registers across the rows of a wave),
// the bytes pass through LDS, and lane w < stride / 16 stores word w of the code row with one 16-byte store — the pad bytes are
// zero codes written by the same store.  HBM-bound on the input.
// =====================================================================================================
__device__ __forceinline__ int i8_quantize_one(float x, float start, float step) {
#pragma clang fp contract(off)
    const float t = (x - start) / step - 128.f;
    if (t != t) return 0;
    return (int)fminf(fmaxf(t, -128.f), 127.f);   // (int) truncates towards zero
}

__global__ __launch_bounds__(256) void quantize_int8_rows_kernel(const float *__restrict__ x, int64_t rows, int d, int64_t ld_in,
                                                                 const float *__restrict__ ranges, int8_t *__restrict__ codes,
                                                                 int64_t ld_code) {
    __shared__ __attribute__((aligned(16))) int8_t stage[4][I8_MAX_D];
    constexpr int NI = I8_MAX_D / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cb = i8_bytes(d);
    float start[NI], step[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int j = lane + 64 * i;
        const int jc = j < d ? j : d - 1;
        start[i] = ranges[jc];
        step[i] = (ranges[d + jc] - start[i]) / 255.f;
    }
    for (int64_t r0 = (int64_t)blockIdx.x * 4; r0 < rows; r0 += (int64_t)gridDim.x * 4) {   // workgroup-uniform
        const int64_t row = r0 + wave < rows ? r0 + wave : rows - 1;   // (clamped: quantised again, not stored)
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (64 * i < cb) {   // uniform
                const int j = lane + 64 * i;
                const float v = x[row * ld_in + (j < d ? j : d - 1)];
                stage[wave][j] = j < d ? (int8_t)i8_quantize_one(v, start[i], step[i]) : (int8_t)0;
            }
        }
        __syncthreads();
        if (r0 + wave < rows && 16 * lane < cb)
            *reinterpret_cast<uint4 *>(codes + row * ld_code + 16 * lane) = *reinterpret_cast<const uint4 *>(&stage[wave][16 * lane]);
        __syncthreads();
    }
}

// =====================================================================================================
// int8 inner-product top-k
// =====================================================================================================
// one running list per query in dynamic LDS, laid out as hamming_partial_kernel's (top_s, top_i: kp entries; blk_s, blk_i: bc),
// the counters behind all lists
__host__ __device__ inline size_t i8_list_bytes(int kp, int bc) { return (size_t)kp * 8 + (size_t)bc * 8; }
__device__ __forceinline__ SlList<int, false> i8_list(char *smem, int g, int kp, int bc, int *counters) {
    char *base = smem + (size_t)g * i8_list_bytes(kp, bc);
    float *top_s = reinterpret_cast<float *>(base);
    int *top_i = reinterpret_cast<int *>(top_s + kp);
    float *blk_s = reinterpret_cast<float *>(top_i + kp);
    int *blk_i = reinterpret_cast<int *>(blk_s + bc);
    return {top_s, blk_s, nullptr, top_i, blk_i, nullptr, counters + g, nullptr};
}

// dword t (0..3) of the 16-byte word at byte offset `off` of a code row, with the bytes at positions >= d cleared
__device__ __forceinline__ uint32_t i8_dword_mask(int off, int t, int d) {
    int n = d - (off + 4 * t);
    n = n < 0 ? 0 : n > 4 ? 4 : n;
    return n == 4 ? 0xffffffffu : (1u << (8 * n)) - 1u;
}

// the 16-byte slices of one row that this lane holds, k-step by k-step: bytes 64 s + 16 (lane >> 4) .. + 15.  A slice at or
// beyond the row's cb = tsim_int8_bytes(d) bytes is not loaded: its address is clamped to the row's last word (what arrives
// there meets zero query bytes on the corpus side, and is masked to zero on the query side).
template <int KS>
__device__ __forceinline__ void i8_load_slices(i8x16_t (&f)[KS], const int8_t *row, int cb, int lane) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int off = 64 * s + 16 * (lane >> 4);
        f[s] = *reinterpret_cast<const i8x16_t *>(row + (off < cb ? off : cb - 16));
    }
}

template <int KS>
__global__ __launch_bounds__(256) void int8_ip_partial_kernel(int64_t Q, int64_t N, int64_t rows_per_chunk, int G,
                                                              const int8_t *__restrict__ q_codes, int64_t ldq,
                                                              const int8_t *__restrict__ c_codes, int64_t ldc, int d, int k, int kp,
                                                              int bc, float *__restrict__ ws_s, int *__restrict__ ws_i) {
    extern __shared__ __attribute__((aligned(16))) char i8_smem[];
    int *counters = reinterpret_cast<int *>(i8_smem + (size_t)G * i8_list_bytes(kp, bc));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, quad = lane >> 4;
    const int cb = i8_bytes(d);
    const int64_t nch = gridDim.x, chunk = blockIdx.x;
    const int64_t q0 = (int64_t)blockIdx.y * G;
    const int ng = (int)(Q - q0 < G ? Q - q0 : G);
    const int64_t r0 = chunk * rows_per_chunk;
    const int64_t r1 = r0 + rows_per_chunk < N ? r0 + rows_per_chunk : N;   // (r0 < r1: every chunk holds a row)
    const bool live = col < ng;              // this lane's column of the tile is a query of the group
    const int mine = live ? col : ng - 1;    // (the list whose bound a dead column reads and never uses)

    // B fragments: the group's queries, bytes at positions >= d and the columns beyond the group zero
    i8x16_t bq[KS];
    i8_load_slices<KS>(bq, q_codes + (q0 + mine) * ldq, cb, lane);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        const int off = 64 * s + 16 * quad;
#pragma unroll
        for (int t = 0; t < 4; ++t) bq[s][t] = live ? (int)((uint32_t)bq[s][t] & i8_dword_mask(off, t, d)) : 0;
    }
    for (int g = 0; g < ng; ++g) i8_list(i8_smem, g, kp, bc, counters).reset(kp);

    // tile (b, t) of this wave: rows b + 64 wave + 16 t .. + 15; the row of this lane's A slices is clamped to the chunk
    auto tile_row = [&](int64_t base) {
        const int64_t r = base + col;
        return r < r1 ? r : r1 - 1;
    };
    i8x16_t an[KS];
    i8_load_slices<KS>(an, c_codes + tile_row(r0 + 64 * wave) * ldc, cb, lane);
    for (int64_t b = r0; b < r1; b += I8_STEP) {
        SlList<int, false> list = i8_list(i8_smem, mine, kp, bc, counters);
        const SlBound<int> bound = list.bound(k);   // (behind the barrier that ends the last flush, reset or counter check)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int64_t base = b + 64 * wave + 16 * t;
            i8x16_t a[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) a[s] = an[s];
            // the next tile of this wave: the next of this step, or the first of the next step (clamped past the chunk's end)
            const int64_t next = t < 3 ? base + 16 : b + I8_STEP + 64 * wave;
            i8_load_slices<KS>(an, c_codes + tile_row(next) * ldc, cb, lane);
            i32x4_t acc = {0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < KS; ++s) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[s], bq[s], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = base + 4 * quad + r;
                if (live && row < r1) list.offer((float)acc[r], (int)row, bound);
            }
        }
        // Which lists to flush (workgroup-uniform; the counters are read between two barriers): all after the chunk's first
        // step and after the last, otherwise those whose block could not take another step's offers.
        const bool all = b == r0 || b + I8_STEP >= r1;
        uint32_t need = all ? 0xffffffffu : 0u;
        if (!all) {
            __syncthreads();
            for (int g = 0; g < ng; ++g) need |= (uint32_t)(counters[g] > bc - I8_STEP) << g;
            __syncthreads();
        }
        for (int g = 0; g < ng; ++g)
            if ((need >> g) & 1) i8_list(i8_smem, g, kp, bc, counters).flush(kp);
    }
    for (int g = 0; g < ng; ++g) i8_list(i8_smem, g, kp, bc, counters).store_raw(ws_s, ws_i, ((q0 + g) * nch + chunk) * k, k);
}

// one workgroup per query: the query's nch chunk lists are consecutive, E = nch k entries from q nch k on
__global__ __launch_bounds__(256) void int8_ip_merge_kernel(int64_t Q, int64_t nch, int k, int kp, const float *__restrict__ ws_s,
                                                            const int *__restrict__ ws_i, int32_t *__restrict__ out_s,
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
            out_s[q * k + t] = pad ? INT32_MIN : (int32_t)top.top_s[t];
            out_i[q * k + t] = pad ? -1 : (int64_t)row + idx_offset;
        }
        __syncthreads();
    }
}

// =====================================================================================================
// int8_rescore: sign_rescore_kernel with the code value in place of +-1.  One workgroup per query; each lane holds the query's
// elements j = lane + 64 i as float64; a wave takes one candidate at a time, lane l reads byte lane + 64 i of the code row (one
// 64-byte span a wave) and adds q_j c_j in the order i = 0, 1, .. (the first product starts the sum, groups at or beyond d add
// nothing, an element beyond d inside the last group adds +0), the xor butterfly joins the lanes and the sum is rounded once:
// float32(oracle.search_ref._lane_sum(q, codes)) — every product of a float32 and an int8 is exact in float64.
// =====================================================================================================
__global__ __launch_bounds__(256) void int8_rescore_kernel(int64_t Q, int64_t N, const float *__restrict__ xq, int64_t ldq,
                                                           const int8_t *__restrict__ c_codes, int64_t ldc, int d,
                                                           const int64_t *__restrict__ cand, int64_t m, int k, int kp,
                                                           float *__restrict__ out_s, int64_t *__restrict__ out_i,
                                                           int64_t idx_offset, int32_t *__restrict__ status) {
    SlList<int, false> top = sl_shared_list<int, false>();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t q = blockIdx.x; q < Q; q += gridDim.x) {
        double qv[SR_MAXI];
        row_elems_f64<float, SR_MAXI>(qv, xq + q * ldq, d, lane);
        top.reset(kp);
        int beyond = 0;
        for (int64_t b = 0; b < m; b += SL_NB) {
            const int nb = (int)(m - b < SL_NB ? m - b : SL_NB);
            const SlBound<int> w = top.bound(k);
            for (int e = wave; e < nb; e += 4) {   // wave-uniform
                const int64_t r = cand[q * m + b + e];
                beyond |= r >= N;
                if (r < 0 || r >= N) continue;
                const int8_t *rp = c_codes + r * ldc;
                int c[SR_MAXI];
#pragma unroll
                for (int i = 0; i < SR_MAXI; ++i) {   // (branch-free loads: the address of an element past d is clamped)
                    const int j = lane + 64 * i;
                    c[i] = 64 * i < d ? (int)rp[j < d ? j : d - 1] : 0;
                }
                double acc = 0.0;
#pragma unroll
                for (int i = 0; i < SR_MAXI; ++i) {
                    if (64 * i < d) {   // wave-uniform
                        const double term = lane + 64 * i < d ? qv[i] * (double)c[i] : 0.0;
                        acc = i == 0 ? term : acc + term;
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
// hm_chunks with this kernel's group size
static inline int64_t i8_chunks(int64_t Q, int64_t N, int k, int d) {
    const int G = i8_group(Q, k, d);
    const int64_t groups = (Q + G - 1) / G;
    const int64_t min_rows = std::max<int64_t>(SL_NB, ((int64_t)4 * k + SL_NB - 1) / SL_NB * SL_NB);
    const int64_t fit = (int64_t)(HM_BUDGET / ((size_t)Q * k * 8));
    return std::max<int64_t>(1, std::min<int64_t>({HM_MAX_CHUNKS, (N + min_rows - 1) / min_rows, (HM_WGS + groups - 1) / groups, fit}));
}

static int check_int8_stride(const char *what, const char *name, const void *codes, int64_t ld, int d) {
    TSIM_REQUIRE((reinterpret_cast<uintptr_t>(codes) & 15) == 0, "%s: the rows of %s do not start on a 16-byte boundary", what, name);
    TSIM_REQUIRE(ld % 16 == 0, "%s: %s=%lld is not a multiple of 16", what, name, (long long)ld);
    TSIM_REQUIRE(ld >= i8_bytes(d), "%s: %s=%lld < tsim_int8_bytes(%d)=%d", what, name, (long long)ld, d, i8_bytes(d));
    return TSIM_OK;
}

template <int KS>
static int int8_ip_partial_launch(dim3 grid, size_t lds, hipStream_t st, int64_t Q, int64_t N, int64_t rpc, int G, const int8_t *q_codes,
                                  int64_t ldq, const int8_t *c_codes, int64_t ldc, int d, int k, int kp, int bc, float *ws_s, int *ws_i) {
    static DevOnce once;
    TSIM_MAX_LDS(once, int8_ip_partial_kernel<KS>, 160 * 1024);
    hipLaunchKernelGGL(int8_ip_partial_kernel<KS>, grid, dim3(256), lds, st, Q, N, rpc, G, q_codes, ldq, c_codes, ldc, d, k, kp, bc, ws_s,
                       ws_i);
    return TSIM_OK;
}
}  // namespace tsim

extern "C" int tsim_int8_bytes(int d) { return tsim::i8_bytes(d); }

extern "C" int tsim_quantize_int8_rows(const float *x, int64_t rows, int d, int64_t ld_in, const float *ranges, int8_t *codes,
                                       int64_t ld_code, void *stream) {
    using namespace tsim;
    const char *what = "quantize_int8_rows";
    TSIM_REQUIRE(x && ranges && codes, "%s: null pointer", what);
    TSIM_REQUIRE(d >= 1 && d <= I8_MAX_D, "%s: d=%d outside 1..%d", what, d, I8_MAX_D);
    TSIM_REQUIRE(rows >= 0 && rows < (1ll << 31) - 64 && ld_in >= d, "%s: bad shape rows=%lld d=%d ld_in=%lld", what, (long long)rows, d,
                 (long long)ld_in);
    if (int rc = check_int8_stride(what, "ld_code", codes, ld_code, d)) return rc;
    if (rows == 0) return TSIM_OK;
    const dim3 grid((unsigned)std::min<int64_t>((rows + 3) / 4, 256 * 16));
    hipLaunchKernelGGL(quantize_int8_rows_kernel, grid, dim3(256), 0, as_stream(stream), x, rows, d, ld_in, ranges, codes, ld_code);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

extern "C" size_t tsim_int8_ip_topk_workspace_bytes(int64_t Q, int64_t N, int k) {
    if (Q <= 0 || N < 0 || k <= 0 || k > tsim::TOPK_LARGE_MAX_K) return 0;
    return 2 * tsim::hm_workspace_half(Q, N, k);
}

extern "C" int tsim_int8_ip_topk(const int8_t *q_codes, int64_t ldq, int64_t Q, const int8_t *c_codes, int64_t ldc, int64_t N, int d,
                                 int k, int32_t *out_score, int64_t *out_idx, int64_t idx_offset, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    using namespace tsim;
    const char *what = "int8_ip_topk";
    TSIM_REQUIRE(q_codes && out_score && out_idx && (c_codes || N == 0), "%s: null pointer", what);
    TSIM_REQUIRE(d >= 1 && d <= I8_MAX_D, "%s: d=%d outside 1..%d", what, d, I8_MAX_D);
    TSIM_REQUIRE(k >= 1 && k <= TOPK_LARGE_MAX_K, "%s: k=%d outside 1..%d", what, k, TOPK_LARGE_MAX_K);
    TSIM_REQUIRE(Q > 0 && N >= 0, "%s: bad shape Q=%lld N=%lld", what, (long long)Q, (long long)N);
    TSIM_REQUIRE(N < (1ll << 31) - 64 && Q < (1ll << 31) - 512, "%s: too large for 32-bit row ids", what);
    if (int rc = check_int8_stride(what, "ldq", q_codes, ldq, d)) return rc;
    if (int rc = check_int8_stride(what, "ldc", c_codes, ldc, d)) return rc;
    const size_t half = hm_workspace_half(Q, N, k);
    if (!workspace || workspace_bytes < 2 * half) return fail(TSIM_ENOMEM, "%s: workspace %zu B < %zu B", what, workspace_bytes, 2 * half);
    hipStream_t st = as_stream(stream);
    float *ws_s = reinterpret_cast<float *>(workspace);
    int *ws_i = reinterpret_cast<int *>(reinterpret_cast<char *>(workspace) + half);
    const int kp = sl_list_len(k);
    int64_t nch = 0;
    if (N > 0) {
        const int64_t want = i8_chunks(Q, N, k, d);
        const int64_t rpc = ((N + want - 1) / want + SL_NB - 1) / SL_NB * SL_NB;   // whole blocks
        nch = (N + rpc - 1) / rpc;                                                // (<= want: every chunk holds a row)
        const int G = i8_group(Q, k, d);
        const int64_t groups = (Q + G - 1) / G;
        TSIM_REQUIRE(groups <= 65535, "%s: Q=%lld needs more than 65535 query groups: slice the queries", what, (long long)Q);
        const dim3 grid((unsigned)nch, (unsigned)groups);
        const int bc = i8_block_cap(kp);
        const size_t lds = (size_t)G * i8_list_bytes(kp, bc) + (size_t)G * 4;
        int rc = TSIM_OK;
        switch ((d + 63) / 64) {
#define TSIM_I8_CASE(KS)                                                                                                          \
    case KS:                                                                                                                      \
        rc = int8_ip_partial_launch<KS>(grid, lds, st, Q, N, rpc, G, q_codes, ldq, c_codes, ldc, d, k, kp, bc, ws_s, ws_i);         \
        break;
            TSIM_I8_CASE(1) TSIM_I8_CASE(2) TSIM_I8_CASE(3) TSIM_I8_CASE(4) TSIM_I8_CASE(5) TSIM_I8_CASE(6) TSIM_I8_CASE(7) TSIM_I8_CASE(8)
            TSIM_I8_CASE(9) TSIM_I8_CASE(10) TSIM_I8_CASE(11) TSIM_I8_CASE(12) TSIM_I8_CASE(13) TSIM_I8_CASE(14) TSIM_I8_CASE(15)
            TSIM_I8_CASE(16)
#undef TSIM_I8_CASE
        }
        if (rc) return rc;
        TSIM_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(int8_ip_merge_kernel, dim3((unsigned)std::min<int64_t>(Q, 4096)), dim3(256), 0, st, Q, nch, k, kp, ws_s, ws_i,
                       out_score, out_idx, idx_offset);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

extern "C" int tsim_int8_rescore_topk(const float *eq_f32, int64_t ldq_f32, int64_t Q, const int8_t *c_codes, int64_t ldc, int64_t N,
                                      int d, const int64_t *cand, int64_t m, int k, float *out_scores, int64_t *out_idx,
                                      int64_t idx_offset, int32_t *out_status, void *stream) {
    using namespace tsim;
    const char *what = "int8_rescore_topk";
    TSIM_REQUIRE(eq_f32 && out_scores && out_idx && (c_codes || N == 0) && (cand || m == 0), "%s: null pointer", what);
    TSIM_REQUIRE(d >= 1 && d <= I8_MAX_D, "%s: d=%d outside 1..%d", what, d, I8_MAX_D);
    TSIM_REQUIRE(k >= 1 && k <= TOPK_LARGE_MAX_K, "%s: k=%d outside 1..%d", what, k, TOPK_LARGE_MAX_K);
    TSIM_REQUIRE(Q > 0 && N >= 0 && m >= 0, "%s: bad shape Q=%lld N=%lld m=%lld", what, (long long)Q, (long long)N, (long long)m);
    TSIM_REQUIRE(N < (1ll << 31) - 64, "%s: too large for 32-bit row ids", what);
    TSIM_REQUIRE(ldq_f32 >= d, "%s: ldq_f32=%lld < d=%d", what, (long long)ldq_f32, d);
    if (int rc = check_int8_stride(what, "ldc", c_codes, ldc, d)) return rc;
    hipLaunchKernelGGL(int8_rescore_kernel, dim3((unsigned)std::min<int64_t>(Q, 1 << 20)), dim3(256), 0, as_stream(stream), Q, N, eq_f32,
                       ldq_f32, c_codes, ldc, d, cand, m, k, sl_list_len(k), out_scores, out_idx, idx_offset, out_status);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}
