// int8 embeddings (included by search.hip, after code_search.h, whose frame it fills in): the calibrated scalar quantiser, exact
// inner-product top-k on the int8 matrix pipe, and the re-score of its candidates with the float32 query against the code values
// (code_rescore_kernel<false>).
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
// Lists (i8_list) and flushes follow the frame's protocol.  A step is 256 rows (four tiles a wave); a list's block holds bc = 512
// or SL_NB entries (i8_block_cap).  G (i8_group): at most 16 while k <= 64, else 8 (the other eight columns of the tile are zero
// and never offered).
#pragma once

namespace tsim {
constexpr int I8_STEP = 256;   // rows of one step of the partial kernel: 4 waves x 4 tiles x 16 rows

__host__ __device__ inline int i8_bytes(int d) { return d >= 1 && d <= CS_MAX_D ? (d + 15) / 16 * 16 : 0; }
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
    __shared__ __attribute__((aligned(16))) int8_t stage[4][CS_MAX_D];
    constexpr int NI = CS_MAX_D / 64;
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
}  // namespace tsim

extern "C" int tsim_int8_bytes(int d) { return tsim::i8_bytes(d); }

extern "C" int tsim_quantize_int8_rows(const float *x, int64_t rows, int d, int64_t ld_in, const float *ranges, int8_t *codes,
                                       int64_t ld_code, void *stream) {
    using namespace tsim;
    const char *what = "quantize_int8_rows";
    TSIM_REQUIRE(x && ranges && codes, "%s: null pointer", what);
    TSIM_REQUIRE(d >= 1 && d <= CS_MAX_D, "%s: d=%d outside 1..%d", what, d, CS_MAX_D);
    TSIM_REQUIRE(rows >= 0 && rows < (1ll << 31) - 64 && ld_in >= d, "%s: bad shape rows=%lld d=%d ld_in=%lld", what, (long long)rows, d,
                 (long long)ld_in);
    if (int rc = cs_check_stride(what, "ld_code", codes, ld_code, d, i8_bytes(d), "tsim_int8_bytes")) return rc;
    if (rows == 0) return TSIM_OK;
    const dim3 grid((unsigned)std::min<int64_t>((rows + 3) / 4, 256 * 16));
    hipLaunchKernelGGL(quantize_int8_rows_kernel, grid, dim3(256), 0, as_stream(stream), x, rows, d, ld_in, ranges, codes, ld_code);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

extern "C" size_t tsim_int8_ip_topk_workspace_bytes(int64_t Q, int64_t N, int k) { return tsim::cs_workspace_bytes(Q, N, k); }

extern "C" int tsim_int8_ip_topk(const int8_t *q_codes, int64_t ldq, int64_t Q, const int8_t *c_codes, int64_t ldc, int64_t N, int d,
                                 int k, int32_t *out_score, int64_t *out_idx, int64_t idx_offset, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    using namespace tsim;
    return cs_topk<false>(
        "int8_ip_topk", i8_bytes(d), "tsim_int8_bytes", i8_group, i8_block_cap, q_codes, ldq, Q, c_codes, ldc, N, d, k, out_score, out_idx,
        idx_offset, workspace, workspace_bytes, stream, [&](const CsLaunch &l) {
            switch ((d + 63) / 64) {
#define TSIM_I8_CASE(KS)                                                                                                          \
    case KS:                                                                                                                      \
        return cs_launch_partial<int8_ip_partial_kernel<KS>>(l, Q, N, l.rpc, l.G, q_codes, ldq, c_codes, ldc, d, k, l.kp, l.bc,      \
                                                             l.ws_s, l.ws_i);
                TSIM_I8_CASE(1) TSIM_I8_CASE(2) TSIM_I8_CASE(3) TSIM_I8_CASE(4) TSIM_I8_CASE(5) TSIM_I8_CASE(6) TSIM_I8_CASE(7) TSIM_I8_CASE(8)
                TSIM_I8_CASE(9) TSIM_I8_CASE(10) TSIM_I8_CASE(11) TSIM_I8_CASE(12) TSIM_I8_CASE(13) TSIM_I8_CASE(14) TSIM_I8_CASE(15)
                TSIM_I8_CASE(16)
#undef TSIM_I8_CASE
            }
            return (int)TSIM_OK;
        });
}

extern "C" int tsim_int8_rescore_topk(const float *eq_f32, int64_t ldq_f32, int64_t Q, const int8_t *c_codes, int64_t ldc, int64_t N,
                                      int d, const int64_t *cand, int64_t m, int k, float *out_scores, int64_t *out_idx,
                                      int64_t idx_offset, int32_t *out_status, void *stream) {
    return tsim::cs_rescore<false>("int8_rescore_topk", tsim::i8_bytes(d), "tsim_int8_bytes", eq_f32, ldq_f32, Q, c_codes, ldc, N, d,
                                   cand, m, k, out_scores, out_idx, idx_offset, out_status, stream);
}

