// Binary embeddings (included by search.hip, after code_search.h, whose frame it fills in): sign-bit codes, exact Hamming top-k,
// and the re-score of Hamming candidates with the float32 query against the +-1 expansion of the codes (code_rescore_kernel<true>).
//
// Codes.  A code row is np.packbits(x > 0, axis=1) of the float row: element 8j is bit 7 of byte j, the last byte is zero-filled.
// Rows lie tsim_code_bytes(d) = ceil(d / 8) rounded up to 16 bytes apart (or more: every stride is a multiple of 16), so a row is
// read with 16-byte loads; the bytes from ceil(d / 8) to tsim_code_bytes(d) are zero in everything written here.  No kernel
// relies on that: bits at positions >= d are masked out of both operands before they are counted.
//
// Hamming distance is an integer, so "exact" is the true top-k under (dist asc, row asc).  A lane offers (-float(dist), row) to
// the running list (SlList): dist <= 1024 is exact in float32 and the list's key order (score desc, index asc) is that order.
//
// Work.  hamming_partial_kernel<NW> (NW 16-byte words per code row), in the frame of code_search.h: workgroup (chunk c, group g)
// owns rows_per_chunk rows and the ng <= G queries g G .. g G + ng - 1.  Every lane owns one row at a time, loads it ONCE with
// 16-byte loads (consecutive lanes read consecutive rows: a wave reads one contiguous span) and compares it with each of the
// group's queries in turn — the query's dwords are workgroup-uniform, so they come through scalar loads and sit in SGPRs: one
// v_xor and one accumulating v_bcnt per dword.  Lists (hm_list: blocks of SL_NB offers) and flushes follow the frame's protocol.
// At Q = 16, N = 1 M the first version (every list flushed once per 1 024 rows, eight queries a workgroup) took 0.62 ms, this one
// 0.19 ms.
//
// G = min(8, ceil(Q / 4)) (hm_group).  Per (row, query) pair the loop issues 8 NW VALU instructions plus about ten for the offer; the row costs 16 NW
// bytes of HBM once per group.  At d = 384 that is 34 lane-instructions against 48 / G bytes: with the chip's 39 T
// lane-instructions/s and 6.3 TB/s the two meet near G = 9, so eight queries per pass bring a large query set to the VALU
// bound, while eight lists of k = 1024 (8 x 16 KiB + counters) still fit the 160 KiB of a workgroup and eight of k <= 64
// (68 KiB) leave room for two workgroups per CU.  A larger G buys nothing once the loop is VALU-bound and costs occupancy.
// A small query set takes fewer queries per workgroup — at least four groups while Q allows: the sorts of a flush are bound by
// barriers and LDS latency, not by bandwidth, so they want many small workgroups resident per CU (8.5 KiB a list for k <= 64),
// and the codes of a million rows (48 MB) are re-read from the cache, not from HBM.
#pragma once

namespace tsim {
constexpr int HM_G = 8;                           // queries of one workgroup at most (above)
static inline int hm_group(int64_t Q) { return (int)std::max<int64_t>(1, std::min<int64_t>(HM_G, (Q + 3) / 4)); }

__host__ __device__ inline int hm_code_bytes(int d) { return d >= 1 && d <= CS_MAX_D ? ((d + 7) / 8 + 15) / 16 * 16 : 0; }

// =====================================================================================================
// pack_sign_rows: one wave per 64 elements.  The ballot of x > 0 holds element e of the wave's 64 at bit e; numpy's order wants
// element 8j at bit 7 of byte j: the bits of every byte reversed (all 64 bits reversed, then the bytes swapped back).  Lane 0
// stores the 8 bytes.  A row takes tsim_code_bytes(d) / 8 waves, so the pad bytes are written (zero) by the same code.
// x > 0 is decided on the bit pattern (0 < bits <= 0x7f800000): +0, -0, NaN, -inf and everything negative give 0, positive
// subnormals 1, whatever the denormal mode of the compare.  HBM-bound on the input.
// =====================================================================================================
template <typename T>
__device__ __forceinline__ bool sign_bit_set(const T *p);
template <>
__device__ __forceinline__ bool sign_bit_set<float>(const float *p) {
    const int b = __float_as_int(*p);
    return b > 0 && b <= 0x7f800000;
}
template <>
__device__ __forceinline__ bool sign_bit_set<bf16_t>(const bf16_t *p) {
    const int b = (int)((uint32_t)*p << 16);
    return b > 0 && b <= 0x7f800000;
}

template <typename T>
__global__ __launch_bounds__(256) void pack_sign_rows_kernel(const T *__restrict__ x, int64_t rows, int d, int64_t ld_in,
                                                             uint8_t *__restrict__ codes, int64_t ld_code) {
    const int lane = threadIdx.x & 63;
    const int wpr = hm_code_bytes(d) / 8;   // waves (8-byte words) per row
    const int64_t units = rows * wpr;
    for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < units; u += (int64_t)gridDim.x * 4) {   // wave-uniform
        const int64_t row = u / wpr;
        const int w = (int)(u - row * wpr);
        const int j = w * 64 + lane;
        const bool bit = j < d ? sign_bit_set<T>(x + row * ld_in + j) : false;
        const unsigned long long m = __ballot(bit);
        if (lane == 0)
            *reinterpret_cast<unsigned long long *>(codes + row * ld_code + 8 * w) = __builtin_bswap64(__brevll(m));
    }
}

// =====================================================================================================
// Hamming top-k
// =====================================================================================================
// dword t of a code row with the bits of elements >= d cleared: byte b of the dword holds elements 32 t + 8 b .. + 7, the first
// of them at bit 7
__device__ __forceinline__ uint32_t hm_dword_mask(int t, int d) {
    uint32_t m = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        int n = d - (32 * t + 8 * b);
        n = n < 0 ? 0 : n > 8 ? 8 : n;
        m |= ((0xff00u >> n) & 0xffu) << (8 * b);
    }
    return m;
}

// bytes of one running list in dynamic LDS (top_s, top_i: kp entries; blk_s, blk_i: SL_NB), the counters behind all lists
__host__ __device__ inline size_t hm_list_bytes(int kp) { return (size_t)kp * 8 + (size_t)SL_NB * 8; }
__device__ __forceinline__ SlList<int, false> hm_list(char *smem, int g, int kp, int *counters) {
    char *base = smem + (size_t)g * hm_list_bytes(kp);
    float *top_s = reinterpret_cast<float *>(base);
    int *top_i = reinterpret_cast<int *>(top_s + kp);
    float *blk_s = reinterpret_cast<float *>(top_i + kp);
    int *blk_i = reinterpret_cast<int *>(blk_s + SL_NB);
    return {top_s, blk_s, nullptr, top_i, blk_i, nullptr, counters + g, nullptr};
}

template <int NW>
__device__ __forceinline__ void hm_load_query(uint4 (&q)[NW], const uint8_t *row) {
    const uint4 *qp = reinterpret_cast<const uint4 *>(row);
#pragma unroll
    for (int w = 0; w < NW; ++w) q[w] = qp[w];
}

template <int NW>
__global__ __launch_bounds__(256) void hamming_partial_kernel(int64_t Q, int64_t N, int64_t rows_per_chunk, int G,
                                                              const uint8_t *__restrict__ q_codes, int64_t ldq,
                                                              const uint8_t *__restrict__ c_codes, int64_t ldc, int d, int k, int kp,
                                                              float *__restrict__ ws_s, int *__restrict__ ws_i) {
    extern __shared__ __attribute__((aligned(16))) char hm_smem[];
    int *counters = reinterpret_cast<int *>(hm_smem + (size_t)G * hm_list_bytes(kp));
    const int64_t nch = gridDim.x, chunk = blockIdx.x;
    const int64_t q0 = (int64_t)blockIdx.y * G;
    const int ng = (int)(Q - q0 < G ? Q - q0 : G);
    const int64_t r0 = chunk * rows_per_chunk;
    const int64_t r1 = r0 + rows_per_chunk < N ? r0 + rows_per_chunk : N;
    uint32_t lastm[4];   // the masks of the row's last four dwords (every dword before them lies below d)
#pragma unroll
    for (int t = 0; t < 4; ++t) lastm[t] = hm_dword_mask(4 * (NW - 1) + t, d);
    for (int g = 0; g < ng; ++g) hm_list(hm_smem, g, kp, counters).reset(kp);
    for (int64_t b = r0; b < r1; b += 256) {   // one step: a row a thread
        const int nb = (int)(r1 - b < 256 ? r1 - b : 256);
        const int e = (int)threadIdx.x;
        const int64_t row = b + (e < nb ? e : 0);   // (clamped: the row is loaded and compared, the distance dropped)
        const uint4 *rp = reinterpret_cast<const uint4 *>(c_codes + row * ldc);
        uint4 r[NW];
#pragma unroll
        for (int w = 0; w < NW; ++w) r[w] = rp[w];
        r[NW - 1].x &= lastm[0];
        r[NW - 1].y &= lastm[1];
        r[NW - 1].z &= lastm[2];
        r[NW - 1].w &= lastm[3];
        // The queries in turn (workgroup-uniform).  The words and the bound of query g + 1 are fetched before query g is
        // compared, so the scalar loads and the two LDS reads are in flight under the popcounts instead of in front of them.
        uint4 qn[NW];
        hm_load_query<NW>(qn, q_codes + q0 * ldq);
        SlBound<int> wn = hm_list(hm_smem, 0, kp, counters).bound(k);
        for (int g = 0; g < ng; ++g) {
            uint4 qw[NW];
#pragma unroll
            for (int w = 0; w < NW; ++w) qw[w] = qn[w];
            const SlBound<int> bound = wn;
            const int gn = g + 1 < ng ? g + 1 : g;
            hm_load_query<NW>(qn, q_codes + (q0 + gn) * ldq);
            wn = hm_list(hm_smem, gn, kp, counters).bound(k);
            qw[NW - 1].x &= lastm[0];
            qw[NW - 1].y &= lastm[1];
            qw[NW - 1].z &= lastm[2];
            qw[NW - 1].w &= lastm[3];
            uint32_t dist = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                dist += __popc(r[w].x ^ qw[w].x);
                dist += __popc(r[w].y ^ qw[w].y);
                dist += __popc(r[w].z ^ qw[w].z);
                dist += __popc(r[w].w ^ qw[w].w);
            }
            if (e < nb) hm_list(hm_smem, g, kp, counters).offer(-(float)dist, (int)row, bound);
        }
        // Which lists to flush (workgroup-uniform: the counters are read between two barriers, so no offer of the next step
        // moves them under a reader): all after the chunk's first step, which gives every list its bound, and after the last;
        // otherwise those whose block could not take another step's 256 offers.
        const bool all = b == r0 || b + 256 >= r1;
        uint32_t need = all ? 0xffffffffu : 0u;
        if (!all) {
            __syncthreads();
            for (int g = 0; g < ng; ++g) need |= (uint32_t)(counters[g] > SL_NB - 256) << g;
            __syncthreads();
        }
        for (int g = 0; g < ng; ++g)
            if ((need >> g) & 1) hm_list(hm_smem, g, kp, counters).flush(kp);
    }
    for (int g = 0; g < ng; ++g) hm_list(hm_smem, g, kp, counters).store_raw(ws_s, ws_i, ((q0 + g) * nch + chunk) * k, k);
}
}  // namespace tsim

extern "C" int tsim_code_bytes(int d) { return tsim::hm_code_bytes(d); }

extern "C" int tsim_pack_sign_rows(const void *x, int x_dtype, int64_t rows, int d, int64_t ld_in, uint8_t *codes, int64_t ld_code,
                                   void *stream) {
    using namespace tsim;
    TSIM_REQUIRE(x && codes, "pack_sign_rows: null pointer");
    TSIM_REQUIRE(d >= 1 && d <= CS_MAX_D, "pack_sign_rows: d=%d outside 1..%d", d, CS_MAX_D);
    TSIM_REQUIRE(rows >= 0 && rows < (1ll << 31) - 64 && ld_in >= d, "pack_sign_rows: bad shape rows=%lld d=%d ld_in=%lld", (long long)rows,
                 d, (long long)ld_in);
    if (int rc = cs_check_stride("pack_sign_rows", "ld_code", codes, ld_code, d, hm_code_bytes(d), "tsim_code_bytes")) return rc;
    if (rows == 0) return TSIM_OK;
    const int64_t blocks = (rows * (hm_code_bytes(d) / 8) + 3) / 4;
    const dim3 grid((unsigned)std::min<int64_t>(blocks, 1 << 22));
    if (x_dtype == TSIM_F32)
        hipLaunchKernelGGL(pack_sign_rows_kernel<float>, grid, dim3(256), 0, as_stream(stream), (const float *)x, rows, d, ld_in, codes,
                           ld_code);
    else if (x_dtype == TSIM_BF16)
        hipLaunchKernelGGL(pack_sign_rows_kernel<bf16_t>, grid, dim3(256), 0, as_stream(stream), (const bf16_t *)x, rows, d, ld_in, codes,
                           ld_code);
    else
        return fail(TSIM_EINVAL, "pack_sign_rows: unknown x_dtype %d", x_dtype);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}


extern "C" size_t tsim_hamming_topk_workspace_bytes(int64_t Q, int64_t N, int k) { return tsim::cs_workspace_bytes(Q, N, k); }

extern "C" int tsim_hamming_topk(const uint8_t *q_codes, int64_t ldq, int64_t Q, const uint8_t *c_codes, int64_t ldc, int64_t N, int d,
                                 int k, int32_t *out_dist, int64_t *out_idx, int64_t idx_offset, void *workspace,
                                 size_t workspace_bytes, void *stream) {
    using namespace tsim;
    return cs_topk<true>(
        "hamming_topk", hm_code_bytes(d), "tsim_code_bytes", [](int64_t nq, int, int) { return hm_group(nq); }, [](int) { return SL_NB; },
        q_codes, ldq, Q, c_codes, ldc, N, d, k, out_dist, out_idx, idx_offset, workspace, workspace_bytes, stream, [&](const CsLaunch &l) {
            switch (hm_code_bytes(d) / 16) {
#define TSIM_HM_CASE(NW)                                                                                                          \
    case NW:                                                                                                                      \
        return cs_launch_partial<hamming_partial_kernel<NW>>(l, Q, N, l.rpc, l.G, q_codes, ldq, c_codes, ldc, d, k, l.kp, l.ws_s,    \
                                                             l.ws_i);
                TSIM_HM_CASE(1) TSIM_HM_CASE(2) TSIM_HM_CASE(3) TSIM_HM_CASE(4) TSIM_HM_CASE(5) TSIM_HM_CASE(6) TSIM_HM_CASE(7) TSIM_HM_CASE(8)
#undef TSIM_HM_CASE
            }
            return (int)TSIM_OK;
        });
}

extern "C" int tsim_sign_rescore_topk(const float *eq_f32, int64_t ldq_f32, int64_t Q, const uint8_t *c_codes, int64_t ldc, int64_t N,
                                      int d, const int64_t *cand, int64_t m, int k, float *out_scores, int64_t *out_idx,
                                      int64_t idx_offset, int32_t *out_status, void *stream) {
    return tsim::cs_rescore<true>("sign_rescore_topk", tsim::hm_code_bytes(d), "tsim_code_bytes", eq_f32, ldq_f32, Q, c_codes, ldc, N, d,
                                  cand, m, k, out_scores, out_idx, idx_offset, out_status, stream);
}
