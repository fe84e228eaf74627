// Transformer encoder forward for gfx950 (MI355X) on PACKED tokens: BERT (DistilBERT, RoBERTa / XLM-R / CamemBERT) and MPNet families.
//
// Replaces `context_embedder(**features)[0]` + mean-pool of the reference
// (/root/reference/src/models/sentence_encoder.py:33-38; layer arithmetic as stated in
// /root/reference/src/models/bert_of_theseus.py:185-211 embeddings, :244-336 attention,
// :346-350 / :411-414 / :424-428 projections + residual LayerNorm + GELU).
//
// Layout in HBM (per encoder handle): activations are [tokens, features] bf16 row-major over the packed
// token axis (no padding rows between sequences; the token axis is rounded up to 128 rows of slack):
//   x0, x1 [Tp, H]   residual stream (LayerNorm outputs)      qkv [Tp, 3H]   fused Q|K|V projections
//   ctx    [Tp, H]   attention output                         h1  [Tp, F]    GELU(FFN1)
// Weights bf16 in nn.Linear layout [out, in] (K contiguous for both GEMM operands); embedding tables,
// biases and LayerNorm parameters float32.  (Hidden 384, BERT family: qkv, h1 and, between the layers, x0 / x1 are block-packed,
// see packed_off / group_off.)
#include <math.h>
#include <cmath>

#include <stdlib.h>
#include <string.h>

#include <vector>

#include <type_traits>
#include <utility>

#include "common.h"
#include "gemm_pp.h"

namespace tsim {

// =====================================================================================================
// BLOCK-PACKED activation layout (round 3) for the wide intermediates of the hidden-384 path, qkv [T, 3H] and h1 [T, F]:
//     element (token t, feature f)  ->  ((t >> 5) * (W / 8) + (f >> 3)) * 256 + (t & 31) * 8 + (f & 7)      (W = row width)
// i.e. per block of 32 tokens and group of 8 features one contiguous 512-byte run of [token][8 features].  Why: a wave of the
// projection kernels owns 32 tokens x 32 features and stores 16 bytes per lane; in the row-major layout one store instruction
// touches 32 rows x 32 B, and such a store costs its wave ~400 cycles of issue (tools/microbench/mfma_loop: two of them per
// step 2 598 cycles against 1 780 without and 1 913 with two CONTIGUOUS 1-KiB stores; in-kernel stamps 650-750 per step).  In
// the packed layout the same instruction writes 1 KiB of contiguous memory.  The readers gain too: attention's q / k / v loads
// (16 B per lane of 32 consecutive tokens: two runs instead of 32 pieces) and the LDS-DMA pieces of the FFN2 operand (256-byte
// runs instead of 64-byte ones).  A block of 32 tokens occupies 32 * W elements in both layouts, so block-aligned row offsets
// are the same.  Token counts are padded to 128 (+128) rows by the encoder's buffers.
// =====================================================================================================
__device__ __forceinline__ int64_t packed_off(int64_t t, int f, int W) {   // element offset of (t, f), f a multiple of 8 here
    return ((t >> 5) * (W >> 3) + (f >> 3)) * 256 + (t & 31) * 8 + (f & 7);
}
// The residual stream x0 / x1 [T, 384] moves in 16-byte groups of 8 features per lane (the resident fragments of gemm_xres2, the
// residual reads and result stores of the LayerNorm GEMMs).  BYTE offset of group g (features 8 g .. 8 g + 7) of token row t in a
// [rows, W] bf16 buffer, row-major or block-packed: the one address rule of every such access.  Linear in g, so a lane computes
// group_off(t, g0) once and adds multiples of the wave-uniform group_off(0, 1): in the packed layout the 32 rows x 2 groups
// of one wave instruction are one contiguous KiB instead of 32 pieces of 32 B.
__device__ __forceinline__ int64_t group_off(int64_t t, int g, int W, int packed) {
    return packed ? packed_off(t, 8 * g, W) * 2 : (t * W + 8 * g) * 2;
}

// =====================================================================================================
// embeddings: x[t] = LayerNorm(word[id] + pos[pos_id] (+ type[type_id]))        one wave per token, fp32 math
// HBM-bound: reads 2-3 rows of H floats, writes H bf16.
// TYPED: tok_type [T] picks the token-type row (BERT sentence pairs); untyped, row 0 is added (type_tab = the table, or
// NULL for MPNet).  Both forms issue the same row loads before the sums, and a typed call whose ids are all 0 computes the
// untyped call's bits.
// =====================================================================================================
template <int VPL, bool TYPED = false>  // values per lane = H / 64
__global__ __launch_bounds__(256) void embed_ln_kernel(const int32_t *__restrict__ ids,
                                                       const int32_t *__restrict__ pos,
                                                       const float *__restrict__ word,
                                                       const float *__restrict__ pos_emb,
                                                       const float *__restrict__ type_tab,
                                                       const float *__restrict__ gamma,
                                                       const float *__restrict__ beta, float eps, int T, int H,
                                                       bf16_t *__restrict__ out, int vocab, int max_pos,
                                                       const int32_t *__restrict__ col, int max_len,
                                                       int *__restrict__ err_flags,
                                                       const int32_t *__restrict__ tok_type = nullptr, int n_types = 0) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    // HF raises IndexError on an id / position outside its table; a kernel cannot, so the index is clamped (no read
    // outside the tables) and an error bit is left for tsim_encoder_error_flags.  A token whose column is >= the max_len
    // the caller promised would be skipped by the attention grid: flagged as well.
    int id = ids[t], ps = pos[t];
    int ty = 0;
    if constexpr (TYPED) ty = tok_type[t];
    int bad = 0;
    if (id < 0 || id >= vocab) { bad |= TSIM_ENC_ERR_TOKEN_ID; id = id < 0 ? 0 : vocab - 1; }
    if (ps < 0 || ps >= max_pos) { bad |= TSIM_ENC_ERR_POSITION; ps = ps < 0 ? 0 : max_pos - 1; }
    if (col[t] >= max_len || col[t] < 0) bad |= TSIM_ENC_ERR_MAX_LEN;
    if constexpr (TYPED) {
        if (ty < 0 || ty >= n_types) { bad |= TSIM_ENC_ERR_TOKEN_TYPE; ty = ty < 0 ? 0 : n_types - 1; }
    }
    if (bad && lane == 0) atomicOr(err_flags, bad);
    const float *w = word + (int64_t)id * H;
    const float *p = pos_emb + (int64_t)ps * H;
    const float *type_row = TYPED ? type_tab + (int64_t)ty * H : type_tab;
    // all row loads first, the sums after them: with `if (type_row)` inside the loop every iteration was a branch with its own
    // s_waitcnt vmcnt(0) — six dependent memory round trips per token (50 us per forward for a kernel that moves 155 MB)
    float v[VPL], pv[VPL], tv[VPL];
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        v[i] = w[lane + i * 64];
        pv[i] = p[lane + i * 64];
    }
    if (type_row) {   // wave-uniform
#pragma unroll
        for (int i = 0; i < VPL; ++i) tv[i] = type_row[lane + i * 64];
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        float a = v[i];
        if (type_row) a += tv[i];   // HF order: (word + token_type) + position
        a += pv[i];
        v[i] = a;
        s += a;
    }
    const float mean = wave_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const float dlt = v[i] - mean;
        q = fmaf(dlt, dlt, q);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)H + eps);
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
        const int j = lane + i * 64;
        out[(int64_t)t * H + j] = f32_to_bf16((v[i] - mean) * rstd * gamma[j] + beta[j]);
    }
}

// =====================================================================================================
// GEMM  out[m, n] = epilogue( sum_k X[m,k] * W[n,k] + bias[n] )          bf16 in, fp32 accumulate (MFMA)
//
// MFMA orientation: A = W tile (rows = output features), B = X tile (columns = tokens), so a lane owns
// ONE token (column lane&31) and 16 features per 32x32 tile.  Row-wise epilogues (LayerNorm statistics,
// packed stores of 4 consecutive features) then need almost no cross-lane traffic.
// Staging: both operands are K-contiguous; tiles stream HBM/L2 -> LDS with global_load_lds_dwordx4 into
// a 2-stage ring (one barrier per K-step: wait -> barrier -> issue next -> compute).  LDS image: rows of
// BK*2 bytes packed into 256-byte super-rows, 16-byte slot index XORed with (super-row & 15) so that the
// ds_read_b128 of a fragment (32 lanes = 32 rows, same K chunk) is bank-conflict free; the permutation is
// applied on the SOURCE address because LDS-DMA writes lane-linearly.
// Epilogues: BIAS | BIAS+GELU(erf) | BIAS+RESIDUAL+LAYERNORM (requires BN == N: a workgroup owns whole rows).
// Roofline: MFMA-bound when K is large; at K = 384 (MiniLM) 288 FLOP per byte moved, i.e. at the
// HBM/MFMA balance point, so operand reuse through L2 (XCD-aware tile order) matters.
// =====================================================================================================
enum { EPI_BIAS = 0, EPI_GELU = 1, EPI_RES_LN = 2 };

template <int BM, int BN, int BK, int WAVES_M, int WAVES_N, int NST = 2>
constexpr int gemm_lds_bytes() {
    return NST * (BM + BN) * BK * 2;
}

// NST = ring slots.  2: wait vmcnt(0) -> barrier -> issue next -> compute (prefetch distance one k-tile).  > 2: counted
// vmcnt, prefetch distance NST-1 k-tiles (needs the stage's 1-KiB pieces to split evenly over the waves).
template <int BM, int BN, int BK, int WAVES_M, int WAVES_N, int EPI, int NST = 2>
__global__ __launch_bounds__(WAVES_M *WAVES_N * 64) void gemm_bf16_kernel(
    const bf16_t *__restrict__ X, const bf16_t *__restrict__ W, const float *__restrict__ bias,
    const bf16_t *__restrict__ res, const float *__restrict__ gamma, const float *__restrict__ beta, float eps,
    bf16_t *__restrict__ out, int M, int N, int K, int mtiles, int ntiles, const bf16_t *__restrict__ Wimg, int xpacked,
    int respacked, int opacked) {
    // xpacked: X is in the block-packed layout (packed_off; BM is a multiple of 32, so a tile starts on a block)
    // respacked / opacked (EPI_RES_LN): so is the residual / goes the output (group_off)
    // Wimg (optional, BN == N): W re-laid at load time as the LDS images of its k-tiles (pack_gemm_w_kernel), so that every
    // DMA piece of the W operand is 1 KiB of CONTIGUOUS memory.  From row-major W a piece gathers 8 rows x 128 B, and that
    // shape streams from L2 at half the rate (tools/microbench/dma_stream: 60 vs 115-128 GB/s per CU); W is 3/4 of the bytes
    // this kernel stages at BM = 128, BN = 384.
    constexpr int NW = WAVES_M * WAVES_N;
    constexpr int TM = BM / WAVES_M, TN = BN / WAVES_N, MT = TM / 32, NT = TN / 32;
    constexpr int RB = BK * 2;       // bytes per tile row
    constexpr int CPR = RB / 16;     // 16-byte chunks per row
    constexpr int RPS = 256 / RB;    // rows per 256-byte super-row
    constexpr int X_BYTES = BM * RB, W_BYTES = BN * RB, STAGE = X_BYTES + W_BYTES;
    constexpr int PIECES = STAGE / 1024, XPIECES = X_BYTES / 1024;
    constexpr int KSTEPS = BK / 16;
    static_assert(TM % 32 == 0 && TN % 32 == 0 && X_BYTES % 1024 == 0 && W_BYTES % 1024 == 0, "tile shape");
    static_assert(NST == 2 || PIECES % NW == 0, "a deep ring needs equal DMA counts per wave");
    constexpr int PPW = (PIECES + NW - 1) / NW;
    extern __shared__ __attribute__((aligned(16))) char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int r = lane & 31, h = lane >> 5;

    // tile order: the ntiles feature tiles of one token tile share blockIdx%8, i.e. one XCD's L2 (speed only)
    const int b = blockIdx.x, xcd = b & 7, jj = b >> 3;
    const int nt_id = jj % ntiles;
    const int mt_id = (jj / ntiles) * 8 + xcd;
    if (mt_id >= mtiles) return;
    const int m0 = mt_id * BM, n0 = nt_id * BN;

    // ---- LDS-DMA sources: per piece handled by this wave, the byte offset of this lane's 16 B inside the operand
    // (computed once: per k-tile only kt * BK * 2 is added)
    constexpr int PPW_MAX = (PIECES + NW - 1) / NW;
    int src_off[PPW_MAX];
#pragma unroll
    for (int i = 0; i < PPW_MAX; ++i) {
        const int p = wave + i * NW;
        const bool isx = p < XPIECES;
        const int sl = (isx ? p : p - XPIECES) * 64 + lane;
        const int sr = sl >> 4, chp = sl & 15;
        const int ch = chp ^ (sr & 15);
        const int row = sr * RPS + ch / CPR, c = ch % CPR;
        src_off[i] = (isx && xpacked) ? (row >> 5) * K * 64 + (row & 31) * 16 + c * 512 : row * K * 2 + c * 16;
    }
    const int xkstride = xpacked ? (BK / 8) * 512 : BK * 2;   // bytes per k-tile along a row of X
    const char *xbase = reinterpret_cast<const char *>(X + (int64_t)m0 * K);
    const char *wbase = reinterpret_cast<const char *>(W + (int64_t)n0 * K);
    const char *wimg = reinterpret_cast<const char *>(Wimg);
    // source of piece p (this wave's i-th) for k-tile kt
    auto piece_src = [&](int i, int p, int kt) __attribute__((always_inline)) -> const char * {
        if (p < XPIECES) return xbase + src_off[i] + kt * xkstride;
        if (wimg) return wimg + (int64_t)kt * W_BYTES + (p - XPIECES) * 1024 + lane * 16;
        return wbase + src_off[i] + kt * (BK * 2);
    };
    auto issue = [&](int kt, int stage) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < PPW_MAX; ++i) {
            const int p = wave + i * NW;
            if (p < PIECES) glds16(piece_src(i, p, kt), smem + stage * STAGE + p * 1024);
        }
    };
    // fragment address inside a region for tile row `row`, k-step s, lane half h
    auto frag_off = [&](int row, int s) {
        const int sr = row / RPS;
        const int ch = (row % RPS) * CPR + 2 * s + h;
        return sr * 256 + ((ch ^ (sr & 15)) << 4);
    };

    // accumulators START from the bias (acc[i][j][g]: feature n0 + wn*TN + i*32 + (g&3) + 8*(g>>2) + 4*h): no bias pass in the
    // epilogue, and the same arithmetic as ln_rows_gemm_kernel below, whose rows must carry the same bits
    f32x16 acc[NT][MT];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const float4 bv = *reinterpret_cast<const float4 *>(bias + n0 + wn * TN + 4 * h + i * 32 + 8 * gq);
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                acc[i][j][4 * gq + 0] = bv.x;
                acc[i][j][4 * gq + 1] = bv.y;
                acc[i][j][4 * gq + 2] = bv.z;
                acc[i][j][4 * gq + 3] = bv.w;
            }
        }
#if defined(TSIM_LN_DIAG) && TSIM_LN_DIAG == 3
    const int nk = 1;   // TIMING-ONLY: prologue + epilogue alone
#else
    const int nk = K / BK;
#endif
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) asm volatile("" : "+v"(acc[i][j]));   // retire the bias loads before any LDS-DMA is in flight
    // (Reading the residual tile here, under the first tiles' LDS-DMA latency, instead of in the epilogue measured +0.15 ms per
    // forward: reverted.)
    if constexpr (NST == 2) {
        issue(0, 0);
    } else {
#pragma unroll
        for (int i = 0; i < NST - 1; ++i) issue(i < nk ? i : nk - 1, i);   // past-the-end: re-read (uniform vmcnt)
    }
    for (int kt = 0; kt < nk; ++kt) {
        const char *xs = smem + (kt % NST) * STAGE;
        const char *ws = xs + X_BYTES;
        auto load_frags = [&](int s, bf16x8 (&bx)[MT], bf16x8 (&aw)[NT]) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < MT; ++j)
                bx[j] = *reinterpret_cast<const bf16x8 *>(xs + frag_off(wm * TM + j * 32 + r, s));
#pragma unroll
            for (int i = 0; i < NT; ++i)
                aw[i] = *reinterpret_cast<const bf16x8 *>(ws + frag_off(wn * TN + i * 32 + r, s));
        };
        if constexpr (NST == 2) {
            // tile kt landed for everyone; everyone finished reading tile kt-1.  The next tile's DMA pieces are issued
            // a k-step's worth at a time BEHIND that k-step's MFMAs (a piece costs its wave ~100 issue cycles: all of
            // them up front would leave the matrix pipe idle), and the fragments of k-step s+1 are read before the
            // MFMAs of k-step s.
            wait_vmcnt<0>();
            __builtin_amdgcn_s_barrier();
            bf16x8 bx[2][MT], aw[2][NT];
#if defined(TSIM_LN_DIAG) && (TSIM_LN_DIAG == 1 || TSIM_LN_DIAG == 4 || TSIM_LN_DIAG == 5)   // TIMING-ONLY: staging alone (no fragment reads, no MFMAs); 4: X pieces only, 5: W pieces only
            for (int s = 0; s < KSTEPS; ++s)
                if (kt + 1 < nk) {
#pragma unroll
                    for (int i = s * PPW_MAX / KSTEPS; i < (s + 1) * PPW_MAX / KSTEPS; ++i) {
                        const int p = wave + i * NW;
                        if (TSIM_LN_DIAG == 4 && p >= XPIECES) continue;
                        if (TSIM_LN_DIAG == 5 && p < XPIECES) continue;
                        if (p < PIECES) glds16(piece_src(i, p, kt + 1), smem + ((kt + 1) & 1) * STAGE + p * 1024);
                    }
                }
            continue;
#endif
            load_frags(0, bx[0], aw[0]);
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s) {
                if (s + 1 < KSTEPS) load_frags(s + 1, bx[(s + 1) & 1], aw[(s + 1) & 1]);
                // (issuing the next k-tile's pieces behind the first one or two k-steps only, instead of all four: measured equal)
#if defined(TSIM_LN_DIAG) && TSIM_LN_DIAG == 2   // TIMING-ONLY: no staging inside the loop (stale tiles)
                if (false) {
#else
                if (kt + 1 < nk) {
#endif
#pragma unroll
                    for (int i = s * PPW_MAX / KSTEPS; i < (s + 1) * PPW_MAX / KSTEPS; ++i) {
                        const int p = wave + i * NW;
                        if (p < PIECES) glds16(piece_src(i, p, kt + 1), smem + ((kt + 1) & 1) * STAGE + p * 1024);
                    }
                }
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j < MT; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aw[s & 1][i], bx[s & 1][j], acc[i][j], 0, 0, 0);
            }
        } else {
            wait_vmcnt<(NST - 2) * PPW>();  // tile kt landed (NST-2 younger tiles may be in flight)
            __builtin_amdgcn_s_barrier();
            const int nx = kt + NST - 1;
            issue(nx < nk ? nx : nk - 1, nx % NST);
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s) {
                bf16x8 bx[MT], aw[NT];
                load_frags(s, bx, aw);
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int j = 0; j < MT; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aw[i], bx[j], acc[i][j], 0, 0, 0);
            }
        }
    }

    if constexpr (NST > 2) wait_vmcnt<0>();   // the re-read tiles of the tail must land before LDS is reused / freed
    // ---- epilogue.  acc[i][j][g]: feature n = n0 + wn*TN + i*32 + (g&3) + 8*(g>>2) + 4*h, token m = m0 + wm*TM + j*32 + r
    const int nbase = n0 + wn * TN + 4 * h;
    const int mbase = m0 + wm * TM + r;

    if constexpr (EPI == EPI_RES_LN) {
        // Residual add + LayerNorm over the N = BN features of each token (two-pass statistics, fp32).
        // DIRECT form (end of round 2): the residual comes in and the result goes out as 16-byte accesses per lane with a
        // v_permlane32_swap between the half-waves (lane (r, h) touches features 8 (gq + h) .. + 7 of its token's row: 32
        // contiguous bytes per row and instruction pair), the way gemm_xres2 stores.  No residual tile DMA, no output tile in
        // LDS; only the row statistics cross the four feature waves through LDS.  (The first form moved both tiles through LDS
        // because 8-byte groups per lane touched 32 cache lines per instruction; timing-only builds put prologue + epilogue at
        // 43 % of this kernel.)
        float *red = reinterpret_cast<float *>(smem);            // [2][WAVES_N][BM] partial sums
        __builtin_amdgcn_s_barrier();                            // every wave is past its last fragment read
        const int g0 = (n0 + wn * TN) / 8 + h;                   // the lane's first 8-feature group
        const int rgs = (int)group_off(0, 1, N, respacked), ogs = (int)group_off(0, 1, N, opacked);
#pragma unroll
        for (int j = 0; j < MT; ++j) {
            const int64_t m = m0 + wm * TM + j * 32 + r;
            const int64_t mr = m < M ? m : M - 1;
            const char *rp = reinterpret_cast<const char *>(res) + group_off(mr, g0, N, respacked);
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int gq = 0; gq < 4; gq += 2) {
                    const uint4 o = *reinterpret_cast<const uint4 *>(rp + (i * 4 + gq) * rgs);
                    auto s0 = __builtin_amdgcn_permlane32_swap(o.x, o.z, false, false);
                    auto s1 = __builtin_amdgcn_permlane32_swap(o.y, o.w, false, false);
                    const uint32_t a0 = s0[0], c0 = s0[1], a1 = s1[0], c1 = s1[1];
                    acc[i][j][4 * gq + 0] += __uint_as_float(a0 << 16);
                    acc[i][j][4 * gq + 1] += __uint_as_float(a0 & 0xffff0000u);
                    acc[i][j][4 * gq + 2] += __uint_as_float(a1 << 16);
                    acc[i][j][4 * gq + 3] += __uint_as_float(a1 & 0xffff0000u);
                    acc[i][j][4 * gq + 4] += __uint_as_float(c0 << 16);
                    acc[i][j][4 * gq + 5] += __uint_as_float(c0 & 0xffff0000u);
                    acc[i][j][4 * gq + 6] += __uint_as_float(c1 << 16);
                    acc[i][j][4 * gq + 7] += __uint_as_float(c1 & 0xffff0000u);
                }
        }
        float mean[MT], rstd[MT];
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < NT; ++i)
#pragma unroll
                    for (int g = 0; g < 16; ++g) {
                        // explicit operations, nothing left to contraction: ln_rows_gemm_kernel repeats them literally
                        if (pass == 0) {
                            s += acc[i][j][g];
                        } else {
                            const float dlt = acc[i][j][g] - mean[j];
                            s = fmaf(dlt, dlt, s);
                        }
                    }
                s += __shfl_xor(s, 32, 64);
                if (h == 0) red[(pass * WAVES_N + wn) * BM + wm * TM + j * 32 + r] = s;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                float s = 0.f;
#pragma unroll
                for (int w = 0; w < WAVES_N; ++w) s += red[(pass * WAVES_N + w) * BM + wm * TM + j * 32 + r];
                if (pass == 0)
                    mean[j] = s / (float)N;
                else
                    rstd[j] = 1.0f / sqrtf(s / (float)N + eps);
            }
        }
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            float4 gv[4], be[4];
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                gv[gq] = *reinterpret_cast<const float4 *>(gamma + nbase + i * 32 + 8 * gq);
                be[gq] = *reinterpret_cast<const float4 *>(beta + nbase + i * 32 + 8 * gq);
            }
#pragma unroll
            for (int j = 0; j < MT; ++j) {
                uint32_t pk[8];
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const float y0 = fmaf((acc[i][j][4 * gq + 0] - mean[j]) * rstd[j], gv[gq].x, be[gq].x);
                    const float y1 = fmaf((acc[i][j][4 * gq + 1] - mean[j]) * rstd[j], gv[gq].y, be[gq].y);
                    const float y2 = fmaf((acc[i][j][4 * gq + 2] - mean[j]) * rstd[j], gv[gq].z, be[gq].z);
                    const float y3 = fmaf((acc[i][j][4 * gq + 3] - mean[j]) * rstd[j], gv[gq].w, be[gq].w);
                    pk[2 * gq] = pack_bf16x2(y0, y1);
                    pk[2 * gq + 1] = pack_bf16x2(y2, y3);
                }
                const int64_t m = m0 + wm * TM + j * 32 + r;
                char *op = reinterpret_cast<char *>(out) + group_off(m, g0, N, opacked);
#pragma unroll
                for (int gq = 0; gq < 4; gq += 2) {
                    auto s0 = __builtin_amdgcn_permlane32_swap(pk[2 * gq], pk[2 * gq + 2], false, false);
                    auto s1 = __builtin_amdgcn_permlane32_swap(pk[2 * gq + 1], pk[2 * gq + 3], false, false);
                    if (m < M) *reinterpret_cast<uint4 *>(op + (i * 4 + gq) * ogs) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
                }
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const int n = nbase + i * 32 + 8 * gq;
#pragma unroll
                for (int j = 0; j < MT; ++j) {
                    const int64_t m = mbase + j * 32;
                    float y0 = acc[i][j][4 * gq + 0], y1 = acc[i][j][4 * gq + 1];
                    float y2 = acc[i][j][4 * gq + 2], y3 = acc[i][j][4 * gq + 3];
                    if constexpr (EPI == EPI_GELU) {
                        gelu2(y0, y1);
                        gelu2(y2, y3);
                    }
                    uint2 o;
                    o.x = pack_bf16x2(y0, y1);
                    o.y = pack_bf16x2(y2, y3);
                    *reinterpret_cast<uint2 *>(out + m * N + n) = o;
                }
            }
    }
}

// encoder_plan sends row-major K = 384 projections whose width is a multiple of XR_BN to gemm_xres2 (below).  (192 is the feature tile of
// the first form of that kernel; the predicate is kept as it was so that every shape keeps its kernel.)
constexpr int XR_BN = 192;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

#ifdef TSIM_PP_STAMPS
// DIAGNOSTIC build only (python -m text_similarity_amd.build --stamps; tools/x2_stamps.py): cycles of wave 0 of gemm_xres2 per
// workgroup: [0] steps, [1] wait (vmcnt + barrier), [2] workgroups, [3] fragment reads + MFMAs, [4] stores, [5] activation
// fragment (re)loads, [6] items, [7] number of (re)loads.  Slots 0-7: EPI_BIAS (QKV), 8-15: EPI_GELU (FFN1).
__device__ unsigned long long g_xr_stamps[16];
#define XR_T() __builtin_amdgcn_s_memtime()
#ifndef TSIM_XR_STAMP_TID
#define TSIM_XR_STAMP_TID 0   // 256: wave 4, the SIMD partner of wave 0
#endif
#define XR_ACC(i, v) do { if (threadIdx.x == TSIM_XR_STAMP_TID) atomicAdd(&g_xr_stamps[(i) + (EPI == EPI_GELU ? 8 : 0)], (unsigned long long)(v)); } while (0)
#else
#define XR_T() 0ull
#define XR_ACC(i, v) do { } while (0)
#endif

template <int... I, class Fn>
__device__ __forceinline__ void ff_static_for(std::integer_sequence<int, I...>, Fn &&f) {   // f(integral_constant<I>) for each I
    (f(std::integral_constant<int, I>{}), ...);
}

// =====================================================================================================
// gemm_xres2: the register-resident K = 384 projection with the EPILOGUE OVERLAPPED.
//
// In the first form of this kernel (192-feature items; removed) every sixth tile-step all eight waves stop feeding the matrix
// pipe and run the epilogue of a 192-feature item together (bias, GELU, packing, stores): 28 % of the kernel's time with the MFMA pipe idle, plus the
// activation reloads (profiles/README.md).  Here an item is 96 features (three 32-feature sub-tiles, W tiles of 96 x 128 k:
// the same 24 KiB per step, three steps per item) and there are TWO accumulator sets (2 x 48 VGPRs beside the 96 of the
// resident activations): while the 24 MFMAs of a step accumulate item i, the wave finishes one sub-tile of item i-1 in
// their shadow — two accumulator registers (GELU, bf16 pack) after every k-step, the half-wave swap and the two 16-byte
// stores at the end of the step.  The bias is not added in the epilogue: the accumulators START from it.
// k order per output ascending, so rows stay batch-invariant bit for bit.
// =====================================================================================================
// TWO STEPS PER BARRIER.  Stamps (tools/x2_stamps.py): of a step's ~3 200 cycles a wave spends ~1 000 in the ring wait
// + workgroup barrier and both waves of a SIMD sit there together — a cost per BARRIER, not per MFMA.  With six ring slots the
// tiles are synchronised in pairs: one vmcnt wait + barrier in front of every even step covers the tiles of steps st and st + 1
// (both issued four steps earlier), the odd step runs straight on; a step issues the tile of step st + 4 into the slot the pair
// before the current one has left (everyone is past that pair: they passed this pair's barrier).
// MEASURED: QKV 73.1 -> 71.2 us, FFN1 119.6 -> 115.3 us (-3 %): the wait is mostly not a per-barrier constant.
// The item loop is X2Loop below; gemm_xres2_kernel runs it on a contiguous range of items, ln_rows_xres2_kernel behind its
// LayerNorm phase on the items of its own token block and its share of the remainder blocks'.
constexpr int X2_BN = 96, X2_BK = 128, X2_NSTAGE = 6, X2_PD = 4, X2_KG = 3, X2_NSUB = 3;

// One 16-byte result store in the SGPR-base + 32-bit-offset form, as inline asm: inside the MFMA stream there is no room for a
// 64-bit address per store (the output is < 4 GiB, checked by the launchers), and an asm statement is exactly ONE store
// instruction, which the manual vmcnt bookkeeping of these kernels counts.
// (s_nop: a store of more than 64 bits needs one wait state before a VALU may overwrite its data registers; hipcc pads its own
// stores but cannot see into an asm statement — without it the next instruction now and then replaced the data under the store:
// a corrupted 16-byte group, non-finite rows after the LayerNorm, the whole sequence after the next attention, in ~20 % of the
// forwards on some boxes and none on others)
__device__ __forceinline__ void x2_store16(uint32_t voff, const u32x4 &o, uint64_t base) {
    asm volatile("global_store_dwordx4 %0, %1, %2\n\ts_nop 1" ::"v"(voff), "v"(o), "s"(base) : "memory");
}

// item i of a workgroup -> block * ntiles + feature tile: a contiguous range (ln_rows_xres2_kernel: X2Chain)
struct X2Range {
    int it0;
    __device__ __forceinline__ int operator()(int i) const { return it0 + i; }
};

// The item loop of the K = 384 projection for one workgroup of eight waves: items map(0) .. map(n_items - 1), W tiles through
// the six-slot ring at smem, the bias at smem + bias_off.  A kernel constructs it, loads the bias, then prime() (the first
// X2_PD W tiles), start() (lane-derived addresses and the loop's state) and run().  Nothing here reads threadIdx: the lane id
// comes in as an argument, so that a caller can hand prime() and start() separately derived copies of it.
//   PK / XPK  the output goes out / the activations come in the block-packed layout (packed_off, group_off)
//   CARRY     24 stores issued between prime() and start() (ln_rows_xres2_kernel's LayerNorm rows) are younger than the primed
//             tiles and are counted in the ring waits of steps 0 and 2, which would otherwise wait for the whole burst; a
//             compile-time flag, so that the wait chain grows no branch without them
//   resident  the token block whose fragments bx[] the caller has filled before run() (-1: none)
template <int EPI, bool PK, bool XPK, bool CARRY, class Map>
struct X2Loop {
    static constexpr int K = 384, KSTEPS = K / 16, NW = 8, BMX = NW * 32;
    static constexpr int STAGE = X2_BN * X2_BK * 2;                 // 24 KiB
    static constexpr int PIECES = STAGE / 1024, PPW = PIECES / NW;  // 24 pieces, 3 per wave
    static_assert(PIECES % NW == 0 && X2_KG * X2_BK == K, "tile shape");
    static_assert(PPW == 3, "the issue schedule of a step places three pieces");

    const char *X, *W;
    char *smem;
    uint64_t out_base;
    uint32_t lbase, bias_lds;
    int M, N, ntiles, n_items, wave;
    Map map;
    int pi, pg, pj;     // the next W tile to issue: k-group pg of item pi, feature tile pj (past the end: the last tile again)
    int r, h, src_off[PPW], cks[8];
    bf16x8 bx[KSTEPS];  // the resident activation fragments of token block cur_mb
    f32x16 accA[X2_NSUB], accB[X2_NSUB];
    int cur_mb, m0, old_m0, old_n0;
    int st;             // steps done
    int ring;           // st % X2_NSTAGE, kept as a counter
    int young1, young2, young3;   // global stores issued in the last three steps, youngest first (-1: unknown)
    int carry;
    uint32_t old_rowoff;          // byte offset of this lane's 16-byte column group in its token row of the PREVIOUS item's block
    bool old_live;                // ... and whether that row exists (one compare per item: the mask guards its six stores per step)
    unsigned x2_n, x2_w, x2_c, x2_e, x2_r, x2_nr;   // (diagnostic build only; 32-bit sums: a workgroup runs < 2^32 cycles)

    __device__ __forceinline__ X2Loop(const void *X_, const bf16_t *W_, bf16_t *out_, char *smem_, int bias_off, int M_, int N_,
                                      int wave_, const Map &map_, int n_items_, int resident)
        : X(reinterpret_cast<const char *>(X_)), W(reinterpret_cast<const char *>(W_)), smem(smem_),
          out_base((uint64_t)(uintptr_t)out_), lbase((uint32_t)(uintptr_t)((__attribute__((address_space(3))) char *)smem_)),
          bias_lds(lbase + bias_off), M(M_), N(N_), ntiles(N_ / X2_BN), n_items(n_items_), wave(wave_), map(map_),
          cur_mb(resident), m0(resident * BMX + wave_ * 32) {
        // (pinned in its SGPR pair here: left alone hipcc sinks the kernel-argument load into the loop's first block and then
        // waits lgkmcnt(0) in front of every store, on the paths where it cannot tell that the load has long landed)
        asm volatile("" : "+s"(out_base));
    }

    // LDS image of a W tile: 96 rows of 256 B (128 k), 16-byte slot c of row rr holds source chunk c ^ (rr & 15); piece i of
    // this wave is 1 KiB of it, the lane's 16 bytes come from this offset in the tile's first row
    __device__ __forceinline__ int piece_off(int lane, int i) const {
        const int sl = (wave * PPW + i) * 64 + lane;
        const int row = sl >> 4, ch = (sl & 15) ^ (row & 15);
        return row * K * 2 + ch * 16;
    }
    __device__ __forceinline__ const char *tile_base() const { return W + ((int64_t)pj * X2_BN * K + pg * X2_BK) * 2; }
    __device__ __forceinline__ void advance() {
        if (++pg == X2_KG) {
            if (pi + 1 < n_items) {
                pg = 0;
                ++pi;
                pj = map(pi) % ntiles;
            } else {
                pg = X2_KG - 1;       // past-the-end: re-read the last tile (uniform vmcnt)
            }
        }
    }
    __device__ __forceinline__ void issue_piece(const char *src, int stage, int i) const {
#if defined(TSIM_X2_DIAG) && (TSIM_X2_DIAG & 4)   // TIMING-ONLY: no W stream (stale tiles)
        (void)src;
#else
        glds16(src, smem + stage * STAGE + (wave * PPW + i) * 1024);
#endif
    }
    // the first X2_PD tiles (offsets from the lane id given here, not kept: start() computes them again from its own)
    __device__ __forceinline__ void prime(int lane) {
        pi = 0, pg = 0, pj = map(0) % ntiles;
#pragma unroll
        for (int s = 0; s < X2_PD; ++s) {
            const char *base = tile_base();
#pragma unroll
            for (int i = 0; i < PPW; ++i) issue_piece(base + piece_off(lane, i), s, i);
            advance();
        }
    }
    __device__ __forceinline__ void start(int lane) {
        r = lane & 31, h = lane >> 5;
#pragma unroll
        for (int i = 0; i < PPW; ++i) src_off[i] = piece_off(lane, i);
        // fragment of sub-tile i, k-step ks (of 8 in a tile): row i*32 + r, source chunk 2 ks + h -> slot (2 ks + h) ^ (r & 15)
#pragma unroll
        for (int ks = 0; ks < 8; ++ks) cks[ks] = r * 256 + (((2 * ks + h) ^ (r & 15)) << 4);
        old_m0 = old_n0 = 0;
        st = ring = 0;
        young1 = young2 = young3 = 0;
        carry = CARRY;
        old_rowoff = 0;
        old_live = false;
        x2_n =x2_w = x2_c = x2_e = x2_r = x2_nr = 0;
    }

    // epilogue of ONE finished sub-tile whose 16 registers have been packed into pk[8] (pk[2gq], pk[2gq+1] = the lane's four
    // features 8gq + 4h .. +3 of group gq): swap half-waves so that every lane owns 8 contiguous features, two 16-byte stores
    // at the end of the step.  (Issuing them inside the MFMA stream instead measured equal: what costs is the store's PATTERN.)
    template <int gq>
    __device__ __forceinline__ void store_half(const uint32_t (&pk)[8], int ncol) const {
        uint32_t a0 = pk[2 * gq], a1 = pk[2 * gq + 1], b0 = pk[2 * gq + 2], b1 = pk[2 * gq + 3];
        auto s0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
        auto s1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
        const u32x4 o = {s0[0], s1[0], s0[1], s1[1]};
        const uint32_t voff = old_rowoff + (uint32_t)(ncol + 8 * gq) * (PK ? 64u : 2u);
#if !(defined(TSIM_X2_DIAG) && (TSIM_X2_DIAG & 1))   // (bit 1: TIMING-ONLY, no output stores)
        if (old_live) x2_store16(voff, o, out_base);
#else
        asm volatile("" ::"v"(voff), "v"(o));
#endif
    }
    __device__ __forceinline__ uint32_t finish2(float y0, float y1) const {
#if !(defined(TSIM_X2_DIAG) && (TSIM_X2_DIAG & 2))   // (bit 2: TIMING-ONLY, no activation function)
        // (two independent scalar Horner chains instead of the packed one: measured equal, 2.633 vs 2.632 ms per forward)
        if constexpr (EPI == EPI_GELU) gelu2(y0, y1);
#endif
        return pack_bf16x2(y0, y1);
    }

    // one item into cur; OLD: the previous item, finished in old, goes out in the shadow of this one's MFMAs
    template <bool OLD>
    __device__ __forceinline__ void run_item(f32x16 (&cur)[X2_NSUB], f32x16 (&old)[X2_NSUB], int item) {
        const int gi = map(item);
        if (gi / ntiles != cur_mb) {                          // wave-uniform: new token block -> reload fragments
            [[maybe_unused]] const unsigned long long xr0 = XR_T();
            cur_mb = gi / ntiles;
            m0 = cur_mb * BMX + wave * 32;
            // fragment s = groups 2 s + h of row m0 + r (packed: rows past M of the last block are the buffer's padding)
            const char *xp = X + group_off(m0 + r, h, K, XPK);
            constexpr int xgs = XPK ? 512 : 16;               // group_off(0, 1, ..)
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s) bx[s] = *reinterpret_cast<const bf16x8 *>(xp + 2 * s * xgs);
#pragma unroll
            for (int s = 0; s < KSTEPS; ++s) asm volatile("" : "+v"(bx[s]));   // retire these ordinary loads here
            young1 = young2 = young3 = 0;                     // ... and with them (vmcnt(0)) everything older
            carry = 0;
#ifdef TSIM_PP_STAMPS
            x2_r += (unsigned)(XR_T() - xr0); x2_nr += 1;
#endif
        }
        const int n0 = (gi % ntiles) * X2_BN;
        // accumulators start from the bias (in LDS: an ordinary global load inside the loop would drain the W ring at its first
        // use): cur[i][q] belongs to feature n0 + 32 i + (q & 3) + 8 (q >> 2) + 4 h
        // (ONE address register + immediates: twelve separately computed addresses were hoisted out of the loop and spilled)
        const uint32_t baddr = bias_lds + (n0 + 4 * h) * 4;
        ff_static_for(std::make_integer_sequence<int, X2_NSUB>{}, [&](auto ic) __attribute__((always_inline)) {
            constexpr int i = decltype(ic)::value;
            f32x4 bv[4];
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bv[0]) : "v"(baddr), "n"((i * 32 + 0) * 4) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bv[1]) : "v"(baddr), "n"((i * 32 + 8) * 4) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bv[2]) : "v"(baddr), "n"((i * 32 + 16) * 4) : "memory");
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(bv[3]) : "v"(baddr), "n"((i * 32 + 24) * 4) : "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(bv[0]), "+v"(bv[1]), "+v"(bv[2]), "+v"(bv[3])::"memory");
#pragma unroll
            for (int q = 0; q < 16; ++q) cur[i][q] = bv[q >> 2][q & 3];
        });
#pragma unroll
        for (int g = 0; g < X2_KG; ++g) {
            // (opaque on purpose: with six steps per loop trip and six slots hipcc knows the slot of every unrolled step, hoists the
            // 6 x 8 fragment addresses out of the loop as invariants and spills all 48 of them)
            asm volatile("" : "+s"(ring));
            const int stage = ring;
            [[maybe_unused]] const unsigned long long xs0 = XR_T();
            // ring wait, even step: the tiles of this step and the next must have landed.  Younger than the next step's pieces:
            // the pieces of steps st + 2 and st + 3 and the stores of the last three steps
            if ((st & 1) == 0) {
                const int ys = (young1 >= 0 && young2 >= 0 && young3 >= 0) ? young1 + young2 + young3 : 0;
                if (CARRY && carry) wait_vmcnt<2 * PPW + 24>();   // (no store of the loop has been issued yet: ys = 0)
                else if (ys == 6) wait_vmcnt<2 * PPW + 6>();
                else if (ys == 4) wait_vmcnt<2 * PPW + 4>();
                else if (ys == 2) wait_vmcnt<2 * PPW + 2>();
                else wait_vmcnt<2 * PPW>();               // none, or unknown store count: always safe
                __builtin_amdgcn_s_barrier();
            }
            __builtin_amdgcn_sched_barrier(0);            // (the odd step has no barrier to fence hipcc's scheduler either)
            [[maybe_unused]] const unsigned long long xs1 = XR_T();
            // Right behind the barrier all eight waves have LDS-DMA to issue and queue at the CU's one address path while the
            // matrix pipe idles; the tile is not needed for two steps, so its three pieces are dropped between the k-steps'
            // MFMAs instead.
            uint32_t pk[8];
            // The step's 24 fragment reads (n = 3 ks + i) roll PF reads ahead of their MFMAs with COUNTED lgkmcnt waits, as in the
            // search kernel's tile loop: hipcc's own schedule of plain loads waits lgkmcnt(0) in front of every k-step, i.e. for
            // the three reads it has just issued (timing-only builds: the bare loop without stores, activation and W stream ran
            // at 43 % of the MFMA rate).  No other LDS instruction is issued between these reads (LDS-DMA counts in vmcnt), so the
            // counts are exact.
            {
                constexpr int PF = 3, NRD = 8 * X2_NSUB;
                lds_u32x4 fr[PF + 1];
                const uint32_t wsl = lbase + stage * STAGE;
                auto rd = [&](auto nc) __attribute__((always_inline)) {
                    constexpr int n = decltype(nc)::value;
                    lds_read_b128_imm<(n % X2_NSUB) * 8192>(fr[n % (PF + 1)], wsl + cks[n / X2_NSUB]);
                };
                ff_static_for(std::make_integer_sequence<int, PF>{}, rd);
                ff_static_for(std::make_integer_sequence<int, NRD>{}, [&](auto nc) __attribute__((always_inline)) {
                    constexpr int n = decltype(nc)::value;
                    constexpr int ks = n / X2_NSUB, i = n % X2_NSUB;
                    if constexpr (n + PF < NRD) rd(std::integral_constant<int, n + PF>{});
                    constexpr int younger = n + PF < NRD ? PF : NRD - 1 - n;
                    lgkm_wait_counted<younger>(fr[n % (PF + 1)]);
                    cur[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fr[n % (PF + 1)]), bx[g * 8 + ks], cur[i], 0, 0, 0);
                    if constexpr (i == X2_NSUB - 1) {
                        if constexpr (ks == 1 || ks == 3 || ks == 5) {       // one piece of the tile of step st + X2_PD
                            const int ns = stage + X2_PD;
                            issue_piece(tile_base() + src_off[ks >> 1], ns >= X2_NSTAGE ? ns - X2_NSTAGE : ns, ks >> 1);
                            if constexpr (ks == 5) advance();
                        }
                        if constexpr (OLD) pk[ks] = finish2(old[g][2 * ks], old[g][2 * ks + 1]);   // in the MFMAs' shadow
                    }
                });
            }
#ifdef TSIM_PP_STAMPS
#pragma unroll
            for (int i = 0; i < X2_NSUB; ++i) asm volatile("" : "+v"(cur[i]));
#endif
            [[maybe_unused]] const unsigned long long xs2 = XR_T();
            young3 = young2;
            young2 = young1;
            young1 = 0;
            if constexpr (OLD) {
                store_half<0>(pk, old_n0 + g * 32);
                store_half<2>(pk, old_n0 + g * 32);
#if defined(TSIM_X2_DIAG) && (TSIM_X2_DIAG & 1)
                young1 = 0;
#else
                young1 = old_m0 + 32 <= M ? 2 : -1;      // both stores of this step were issued for certain / unknown
#endif
            }
            ++st;
            ring = ring + 1 == X2_NSTAGE ? 0 : ring + 1;
            if constexpr (CARRY)
                if (st >= 3) carry = 0;   // the wait of step 4 is for tiles issued after the carried stores
#ifdef TSIM_PP_STAMPS
            { const unsigned long long xs3 = XR_T(); x2_n += 1; x2_w += (unsigned)(xs1 - xs0); x2_c += (unsigned)(xs2 - xs1); x2_e += (unsigned)(xs3 - xs2); }
#endif
        }
        old_m0 = m0;
        old_n0 = n0;
        old_live = m0 + r < M;
        old_rowoff = PK ? (uint32_t)(m0 >> 5) * (uint32_t)(N * 64) + 16u * r + 512u * h     // m0 is a multiple of 32
                        : (uint32_t)(m0 + r) * (uint32_t)(N * 2) + 16u * h;
    }
    // the last item's three sub-tiles
    __device__ __forceinline__ void flush(f32x16 (&acc)[X2_NSUB]) const {
#pragma unroll
        for (int g = 0; g < X2_NSUB; ++g) {
            uint32_t pk[8];
#pragma unroll
            for (int ks = 0; ks < 8; ++ks) pk[ks] = finish2(acc[g][2 * ks], acc[g][2 * ks + 1]);
            store_half<0>(pk, old_n0 + g * 32);
            store_half<2>(pk, old_n0 + g * 32);
        }
    }
    // all items: the two accumulator sets alternate, the last item is flushed
    __device__ __forceinline__ void run() {
        int item = 0;
        run_item<false>(accA, accB, item++);
        for (; item + 2 <= n_items; item += 2) {
            run_item<true>(accB, accA, item);
            run_item<true>(accA, accB, item + 1);
        }
        const bool lastA = item >= n_items;      // the last finished item sits in accA, unless one more item goes into accB
        if (!lastA) run_item<true>(accB, accA, item);
        wait_vmcnt<0>();                         // no LDS-DMA may outlive the workgroup (past-the-end tiles)
        if (lastA) flush(accA); else flush(accB);
    }
};

// PK: the output goes out in the block-packed layout (see packed_off); XPK: X comes in it (group_off)
template <int EPI, bool PK, bool XPK>
__global__ __launch_bounds__(512) void gemm_xres2_kernel(const bf16_t *__restrict__ X, const bf16_t *__restrict__ W,
                                                         const float *__restrict__ bias, bf16_t *__restrict__ out,
                                                         int M, int N, int items_total) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int it0 = (int)((int64_t)items_total * blockIdx.x / gridDim.x);
    const int it1 = (int)((int64_t)items_total * (blockIdx.x + 1) / gridDim.x);
    if (it1 <= it0) return;
    typedef X2Loop<EPI, PK, XPK, false, X2Range> Loop;
    Loop x2(X, W, out, smem, X2_NSTAGE * Loop::STAGE, M, N, wave, X2Range{it0}, it1 - it0, -1);
    // bias -> LDS once per workgroup, above the ring
    for (int p = wave; p * 256 < N; p += Loop::NW)
        if (p * 256 + lane * 4 < N) glds16(bias + p * 256 + lane * 4, smem + X2_NSTAGE * Loop::STAGE + p * 1024);
    wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    x2.prime(lane);
    x2.start(lane);
    x2.run();
    XR_ACC(0, x2.x2_n); XR_ACC(1, x2.x2_w); XR_ACC(3, x2.x2_c); XR_ACC(4, x2.x2_e); XR_ACC(6, x2.x2_n / 3); XR_ACC(2, 1); XR_ACC(5, x2.x2_r); XR_ACC(7, x2.x2_nr);
}

// W [BN rows, K] -> per k-tile of BK the W-region LDS image of gemm_bf16_kernel<.., BN, BK, ..>: 16-byte slot sl of the image
// (super-row sr = sl >> 4 of 256 B = 256 / (2 BK) tile rows, slot chp = sl & 15) holds chunk ch = chp ^ (sr & 15) of the super-row.
__global__ __launch_bounds__(256) void pack_gemm_w_kernel(const uint4 *__restrict__ W, uint4 *__restrict__ img, int BN, int BK, int K) {
    const int slots = BN * BK * 2 / 16;                             // 16-byte slots per k-tile image
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= (int64_t)slots * (K / BK)) return;
    const int kt = (int)(u / slots), sl = (int)(u % slots);
    const int cpr = BK * 2 / 16, rps = 256 / (BK * 2);
    const int sr = sl >> 4, ch = (sl & 15) ^ (sr & 15);
    const int row = sr * rps + ch / cpr, c = ch % cpr;
    img[u] = W[((int64_t)row * K + (int64_t)kt * BK) * 2 / 16 + c];
}
// W [N rows, K] -> MFMA A-fragment images: 1-KiB block (k-step s, 32-feature sub-tile j) at (s * (N / 32) + j) * 1024, lane (r, h)'s
// 16 bytes = W[32 j + r][16 s + 8 h .. + 8).  Two consecutive k-steps (24 KiB at N = 384) are ln_rows_gemm_kernel's W region of a
// 32-k tile — LDS-DMA copies it verbatim, a fragment read is lane-linear (conflict-free, one address register) — and
// ln_tail_gemm_kernel loads the same blocks straight into registers, one contiguous KiB per load.
__global__ __launch_bounds__(256) void pack_frag_w_kernel(const uint4 *__restrict__ W, uint4 *__restrict__ img, int N, int K) {
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;      // 16-byte unit of the image
    if (u >= (int64_t)N * K / 8) return;
    const int lane = (int)(u & 63), blk = (int)(u >> 6);
    const int nt = N / 32, s = blk / nt, j = blk % nt, r = lane & 31, h = lane >> 5;
    img[u] = W[((int64_t)(32 * j + r) * K + 16 * s + 8 * h) / 8];
}
// =====================================================================================================
// ln_rows_gemm: out = LayerNorm(X W^T + bias + res) for hidden 384 with 256 tokens per workgroup — the O-projection and FFN2 of
// a MiniLM layer wherever whole rounds of 256-token tiles exist (the rest of the tokens goes through ln_tail_gemm_kernel or
// gemm_bf16_kernel<128 / 64, 384, ..>, whose rows carry the same bits: same k order, same MFMA shape, accumulators from the
// bias, the same statistics).
//
// Why (round 3).  LDS is the binding resource of the LayerNorm GEMM: an LDS-DMA write moves 64 B per LDS cycle, a ds_read_b128
// 256 B, and at BM = 128, BK = 64 a k-tile stages 64 KiB (1 024 LDS cycles) and is read 160 KiB (640) for 1 536 cycles of MFMA
// per SIMD — measured: staging alone 71 of 80 us (profiles/README.md).  The W tile is 3/4 of the staged bytes and is re-staged for
// every token tile, so the tile must hold more tokens; gemm_bf16_kernel's 2 x 4 wave grid at BM = 256 needs 192 accumulator
// registers beside ~110 others and spills (measured 115 us per launch instead of 80).  Here every WAVE owns 32 token rows and ALL
// 384 features (12 accumulator tiles = 192 VGPRs): LayerNorm statistics never leave the
// wave — no barrier, no LDS round trip, no parameter staging in the epilogue — and the k loop is the asm-pipelined form of the
// other kernels: 32-k tiles (16 KiB of X + 24 KiB of W as packed images) through a three-slot LDS-DMA ring with counted vmcnt (two
// tiles in flight across the barrier), fragment reads rolling four ahead with counted lgkmcnt, 24 MFMAs per wave and tile.
// Per k-tile: 40 KiB staged (640 LDS cycles) + 208 KiB read (832) for 1 536 MFMA cycles per SIMD.
// =====================================================================================================
// NW = waves = 32-token row blocks per workgroup, LR_NST = ring slots: <8, 3> (256 tokens, 120 KiB).
// The phases are the ln384_* functions below; ln_rows_xres2_kernel runs the same ones in front of its projection.  They take the
// lane id (and r = lane & 31, h = lane >> 5) as arguments and never read threadIdx, so a caller short of registers can hand each
// phase a freshly derived copy.
constexpr int LR_BK = 32, LR_WBYTES = 384 * LR_BK * 2;

// accumulators start from the bias: acc[t][q] = output feature 32 t + (q & 3) + 8 (q >> 2) + 4 h of the lane's token row
__device__ __forceinline__ void ln384_bias_start(f32x16 (&acc)[12], const float *bias, int h) {
#pragma unroll
    for (int t = 0; t < 12; ++t)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const f32x4 bv = *reinterpret_cast<const f32x4 *>(bias + 32 * t + 8 * gq + 4 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[t][4 * gq + e] = bv[e];
        }
}

// The k loop of a workgroup of NW waves on token rows m0 .. m0 + 32 NW - 1 through LR_NST ring slots at smem (a stage is the X
// tile of 32 NW rows plus the W tile).  CLAMP: rows past M repeat row M - 1 (never stored); without it all rows exist.
// On return the last tiles (past-the-end ones too) are still in flight: the caller waits vmcnt(0).
template <int NW, int LR_NST, bool CLAMP>
__device__ __forceinline__ void ln384_kloop(f32x16 (&acc)[12], const bf16_t *X, const bf16_t *Wimg, char *smem, int wave, int lane,
                                            int r, int h, int m0, int M, int K, int xpacked) {
    constexpr int XBYTES = NW * 32 * LR_BK * 2, STAGE = XBYTES + LR_WBYTES;
    constexpr int XP = XBYTES / 1024, PIECES = STAGE / 1024, PPW = PIECES / NW;   // pieces 0..XP-1: X, the rest: W
    static_assert(PIECES % NW == 0 && XP == 2 * NW, "every wave issues two X pieces and PPW - 2 W pieces per k-tile");
    const int nk = K / LR_BK;
    // LDS image of the X region (as gemm_bf16_kernel at BK = 32): rows of 64 B, four to a 256-byte super-row; 16-byte slot (sr, chp)
    // holds chunk ch = chp ^ (sr & 15) of the super-row = chunk ch & 3 of row 4 sr + (ch >> 2).  The permutation goes on the SOURCE
    // address (LDS-DMA writes lane-linearly).  The W region is the tile's 24 fragment blocks (pack_frag_w_kernel), copied verbatim.
    const char *xsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int sl = (wave + i * NW) * 64 + lane;
        const int sr = sl >> 4, ch = (sl & 15) ^ (sr & 15);
        const int row = sr * 4 + (ch >> 2);
        const int64_t m = !CLAMP || m0 + row < M ? m0 + row : M - 1;
        xsrc[i] = xpacked ? reinterpret_cast<const char *>(X + packed_off(m, (ch & 3) * 8, K))
                          : reinterpret_cast<const char *>(X) + m * K * 2 + (ch & 3) * 16;
    }
    const int xkstride = xpacked ? (LR_BK / 8) * 512 : LR_BK * 2;   // bytes per k-tile along a row
    const char *wsrc = reinterpret_cast<const char *>(Wimg) + lane * 16;
    auto issue = [&](int kt, int stage) __attribute__((always_inline)) {
        const int k2 = kt < nk ? kt : nk - 1;                  // past-the-end: re-read the last tile (uniform vmcnt)
        char *dst = smem + stage * STAGE;
#pragma unroll
        for (int i = 0; i < 2; ++i) glds16(xsrc[i] + k2 * xkstride, dst + (wave + i * NW) * 1024);
#pragma unroll
        for (int i = 2; i < PPW; ++i)
            glds16(wsrc + (int64_t)k2 * LR_WBYTES + (wave + i * NW - XP) * 1024, dst + (wave + i * NW) * 1024);
    };
    // fragment read addresses inside a stage.  X: row rho = 32 wave + r, k-step s, lane half h -> super-row rho >> 2, chunk
    // (rho & 3) * 4 + 2 s + h.  W: block 12 s + t of the region, this lane's 16 bytes: one address register and an immediate.
    const uint32_t lbase = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char *)smem);
    uint32_t xo[2];
#pragma unroll
    for (int sk = 0; sk < 2; ++sk) {
        const int ch = (r & 3) * 4 + 2 * sk + h;
        xo[sk] = lbase + wave * 2048 + (r >> 2) * 256 + ((ch ^ ((((wave & 1) << 3) + (r >> 2)) & 15)) << 4);
    }
    const uint32_t wl = lbase + XBYTES + lane * 16;

    static_assert(LR_NST >= 3 && (LR_NST - 2) * PPW <= 63, "ring depth");
#pragma unroll
    for (int i = 0; i < LR_NST - 1; ++i) issue(i, i);
#pragma unroll
    for (int t = 0; t < 12; ++t) asm volatile("" : "+v"(acc[t]));   // retire the bias loads here (and with them the first tiles)
    auto do_tile = [&](int kt, auto stc) __attribute__((always_inline)) {
        constexpr int stage = decltype(stc)::value;
        wait_vmcnt<(LR_NST - 2) * PPW>();  // my pieces of tile kt (those of kt + 1 .. kt + NST - 2 stay in flight)
        __builtin_amdgcn_s_barrier();      // everyone's landed; everyone is past tile kt - 1
        issue(kt + LR_NST - 1, (stage + LR_NST - 1) % LR_NST);
        constexpr int PF = 4, NRD = 24;
        lds_u32x4 bfr[2], fr[PF + 1];
        const uint32_t so = stage * STAGE;
        lds_read_b128_imm<0>(bfr[0], xo[0] + so);
        lds_read_b128_imm<0>(bfr[1], xo[1] + so);
        const uint32_t wa = wl + so;
        auto rd = [&](auto nc) __attribute__((always_inline)) {            // read n: k-step n / 12, tile n % 12 = block n
            constexpr int n = decltype(nc)::value;
            lds_read_b128_imm<n * 1024>(fr[n % (PF + 1)], wa);
        };
        ff_static_for(std::make_integer_sequence<int, PF>{}, rd);
        ff_static_for(std::make_integer_sequence<int, NRD>{}, [&](auto nc) __attribute__((always_inline)) {
            constexpr int n = decltype(nc)::value;
            if constexpr (n + PF < NRD) rd(std::integral_constant<int, n + PF>{});
            constexpr int younger = n + PF < NRD ? PF : NRD - 1 - n;
            lgkm_wait_counted<younger>(fr[n % (PF + 1)]);                  // ... and everything older: both X fragments
            if constexpr (n == 0) { asm volatile("" : "+v"(bfr[0])); asm volatile("" : "+v"(bfr[1])); }
            acc[n % 12] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, fr[n % (PF + 1)]),
                                                                   __builtin_bit_cast(bf16x8, bfr[n / 12]), acc[n % 12], 0, 0, 0);
        });
    };
    int kt = 0;
    for (; kt + LR_NST <= nk; kt += LR_NST)
        ff_static_for(std::make_integer_sequence<int, LR_NST>{}, [&](auto sc) __attribute__((always_inline)) {
            do_tile(kt + decltype(sc)::value, sc);
        });
    ff_static_for(std::make_integer_sequence<int, LR_NST - 1>{}, [&](auto sc) __attribute__((always_inline)) {
        if (kt + decltype(sc)::value < nk) do_tile(kt + decltype(sc)::value, sc);
    });
}

// + residual: the lane's 16 bytes at res + ro + group * rgs are the 8 features of group gq + h; the swap turns them into the
// accumulator layout (one base and 32-bit offsets: M * 768 < 4 GiB, checked by the launchers)
__device__ __forceinline__ void ln384_add_residual(f32x16 (&acc)[12], const bf16_t *res, uint32_t ro, uint32_t rgs) {
#pragma unroll
    for (int t = 0; t < 12; ++t)
#pragma unroll
        for (int gq = 0; gq < 4; gq += 2) {
            const uint4 o = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(res) + (ro + (4 * t + gq) * rgs));
            auto s0 = __builtin_amdgcn_permlane32_swap(o.x, o.z, false, false);
            auto s1 = __builtin_amdgcn_permlane32_swap(o.y, o.w, false, false);
            const uint32_t a0 = s0[0], c0 = s0[1], a1 = s1[0], c1 = s1[1];
            acc[t][4 * gq + 0] += __uint_as_float(a0 << 16);
            acc[t][4 * gq + 1] += __uint_as_float(a0 & 0xffff0000u);
            acc[t][4 * gq + 2] += __uint_as_float(a1 << 16);
            acc[t][4 * gq + 3] += __uint_as_float(a1 & 0xffff0000u);
            acc[t][4 * gq + 4] += __uint_as_float(c0 << 16);
            acc[t][4 * gq + 5] += __uint_as_float(c0 & 0xffff0000u);
            acc[t][4 * gq + 6] += __uint_as_float(c1 << 16);
            acc[t][4 * gq + 7] += __uint_as_float(c1 & 0xffff0000u);
        }
}

// two-pass statistics of the lane's row (wave-local: no barrier, no LDS round trip) in the association order of
// gemm_bf16_kernel<.., 384, .., WAVES_N = 4, ..>, which is what makes rows bit-equal across the kernels: four groups of three
// sub-tiles (there: one wave each), each summed tile by tile, register by register, then across the half-waves, then
// ((0 + g0) + g1) + g2) + g3
__device__ __forceinline__ void ln384_stats(const f32x16 (&acc)[12], float eps, float &mean, float &rstd) {
    constexpr int N = 384;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            float sg = 0.f;
#pragma unroll
            for (int t = 3 * w; t < 3 * w + 3; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    if (pass == 0) {
                        sg += acc[t][q];
                    } else {
                        const float dlt = acc[t][q] - mean;
                        sg = fmaf(dlt, dlt, sg);
                    }
                }
            sg += __shfl_xor(sg, 32, 64);
            tot += sg;
        }
        if (pass == 0)
            mean = tot / (float)N;
        else
            rstd = 1.0f / sqrtf(tot / (float)N + eps);
    }
}

// normalise, pack to bf16, swap half-waves so that every lane owns 8 contiguous features: sink(4 t + gq, o) gets the 16-byte
// group 4 t + gq + h of the lane's row.  gamma / beta: global memory or LDS
template <class Sink>
__device__ __forceinline__ void ln384_normalise(const f32x16 (&acc)[12], float mean, float rstd, const float *gamma,
                                                const float *beta, int h, Sink &&sink) {
#pragma unroll
    for (int t = 0; t < 12; ++t) {
        uint32_t pk[8];
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const int n = 32 * t + 8 * gq + 4 * h;
            const f32x4 gv = *reinterpret_cast<const f32x4 *>(gamma + n), bv = *reinterpret_cast<const f32x4 *>(beta + n);
            const float o0 = fmaf((acc[t][4 * gq + 0] - mean) * rstd, gv[0], bv[0]);
            const float o1 = fmaf((acc[t][4 * gq + 1] - mean) * rstd, gv[1], bv[1]);
            const float o2 = fmaf((acc[t][4 * gq + 2] - mean) * rstd, gv[2], bv[2]);
            const float o3 = fmaf((acc[t][4 * gq + 3] - mean) * rstd, gv[3], bv[3]);
            pk[2 * gq] = pack_bf16x2(o0, o1);
            pk[2 * gq + 1] = pack_bf16x2(o2, o3);
        }
#pragma unroll
        for (int gq = 0; gq < 4; gq += 2) {
            auto s0 = __builtin_amdgcn_permlane32_swap(pk[2 * gq], pk[2 * gq + 2], false, false);
            auto s1w = __builtin_amdgcn_permlane32_swap(pk[2 * gq + 1], pk[2 * gq + 3], false, false);
            const u32x4 o = {s0[0], s1w[0], s0[1], s1w[1]};
            sink(4 * t + gq, o);
        }
    }
}

template <int NW, int LR_NST>
__global__ __launch_bounds__(NW * 64) void ln_rows_gemm_kernel(const bf16_t *__restrict__ X, const bf16_t *__restrict__ Wimg,
                                                               const float *__restrict__ bias, const bf16_t *__restrict__ res,
                                                               const float *__restrict__ gamma, const float *__restrict__ beta,
                                                               float eps, bf16_t *__restrict__ out, int M, int K, int xpacked,
                                                               int respacked, int opacked) {
    // xpacked: X is in the block-packed layout (packed_off): FFN2's operand h1.  respacked / opacked: so is the residual / goes the
    // output (group_off)
    constexpr int N = 384;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 31, h = lane >> 5;
    const int m0 = blockIdx.x * (NW * 32);

    f32x16 acc[12];
    ln384_bias_start(acc, bias, h);
    ln384_kloop<NW, LR_NST, true>(acc, X, Wimg, smem, wave, lane, r, h, m0, M, K, xpacked);
    wait_vmcnt<0>();   // past-the-end tiles must not outlive the workgroup

    // ---------------------------------------------------------------- epilogue: + residual, LayerNorm, store
    const int64_t m = m0 + wave * 32 + r;
    const bool live = m < M;
    const int64_t mr = live ? m : M - 1;
    ln384_add_residual(acc, res, (uint32_t)group_off(mr, h, N, respacked), (uint32_t)group_off(0, 1, N, respacked));
    float mean, rstd;
    ln384_stats(acc, eps, mean, rstd);
    const uint32_t oo = (uint32_t)group_off(m, h, N, opacked), ogs = (uint32_t)group_off(0, 1, N, opacked);
    ln384_normalise(acc, mean, rstd, gamma, beta, h, [&](int g, const u32x4 &o) __attribute__((always_inline)) {
        if (live) *reinterpret_cast<u32x4 *>(reinterpret_cast<char *>(out) + (oo + g * ogs)) = o;
    });
}

// =====================================================================================================
// ln_rows_xres2: the LayerNorm GEMM of a 256-token block and the K = 384 projection that follows it, in the SAME workgroup —
// O-projection -> FFN1 (EPI_GELU) and FFN2 -> the next layer's QKV (EPI_BIAS) of the block-packed hidden-384 path.
//
// ln_rows_gemm_kernel<8, 3> and gemm_xres2_kernel<EPI, true, true> use one decomposition (a workgroup owns 256 tokens, a wave 32
// token rows and all 384 features), and the 16-byte groups the LayerNorm epilogue stores after its half-wave swap ARE the resident
// fragments bx[24] of the projection (group 4 t + gq + h = 2 s + h for s = 2 t + gq / 2).  So the workgroup keeps them, and the
// projection starts without the store drain, the kernel boundary, the W-ring prologue and the fragment load in between.  No
// arithmetic changes: the first phase is ln_rows_gemm_kernel's (the ln384_* functions: k order, accumulators from the bias,
// residual add, two-pass statistics), the second gemm_xres2_kernel's item loop (X2Loop): the same code in both places.
//
// Hand-over:
//   LDS     the three 40-KiB slots of the LayerNorm ring and the six 24-KiB slots of the W ring overlap (one barrier after the last
//           k-tile, W pieces only behind it); the projection's bias and gamma / beta sit above both (144 KiB ..), loaded once.
//   vmcnt   the W ring is primed (X2_PD tiles) right behind that barrier, BEFORE the epilogue's 24 result stores; the stores are
//           inline asm (an exact count) and are carried as `carry` in the ring waits of steps 0 and 2, which would otherwise wait
//           for the whole burst.  gamma / beta come from LDS so that no load of the epilogue waits behind a store either.
//           The epilogue's residual loads are ordinary loads issued behind the primed tiles, so the first wait on a residual row
//           also waits for the four W tiles (they come from L2 and are needed next anyway): part of the hand-over's cost.
//   rows    the row is still stored (x1 / x0 is the next LayerNorm's residual).
// Items: workgroup b takes the N / 96 items of its own block, then its share of the remainder blocks' items (chain_part), whose
// fragments it loads from memory as gemm_xres2 does: their rows were written by the remainder launch BEFORE this kernel.
// =====================================================================================================
struct ChainPart { int own, r0, n; };   // own items, first remainder item, items in all
// The item-assignment rule (host and device: tsim_chain_items_host).  Workgroup b of G owns whole block b (the grid is the whole
// blocks), the R = rem_blocks * ntiles items of the blocks behind them are cut into G contiguous shares.
__host__ __device__ inline ChainPart chain_part(int G, int rem_blocks, int ntiles, int b) {
    const long long R = (long long)rem_blocks * ntiles;
    const int r0 = (int)(R * b / G), r1 = (int)(R * (b + 1) / G);
    return {ntiles, r0, ntiles + r1 - r0};
}
// the workgroup's i-th item as block * ntiles + feature tile
__host__ __device__ inline int chain_item(const ChainPart &p, int G, int ntiles, int b, int i) {
    return i < p.own ? b * ntiles + i : G * ntiles + p.r0 + (i - p.own);
}
struct X2Chain {   // X2Loop's item map of workgroup b
    ChainPart part;
    int G, ntiles, b;
    __device__ __forceinline__ int operator()(int i) const { return chain_item(part, G, ntiles, b, i); }
};

template <int EPI>
__global__ __launch_bounds__(512) void ln_rows_xres2_kernel(const bf16_t *__restrict__ X, const bf16_t *__restrict__ Wimg,
                                                            const float *__restrict__ lbias, const bf16_t *__restrict__ res,
                                                            const float *__restrict__ gamma, const float *__restrict__ beta,
                                                            float eps, bf16_t *xout, int K, int xpacked, int respacked,
                                                            const bf16_t *__restrict__ W2, const float *__restrict__ bias2,
                                                            bf16_t *__restrict__ out2, int M, int N2, int rem_blocks) {
    // grid = the whole blocks (all of their rows exist); M = all token rows, the remainder blocks included; xout and out2 packed
    constexpr int NW = 8, N = 384, LR_NST = 3;
    constexpr int LSTAGE = NW * 32 * LR_BK * 2 + LR_WBYTES;   // a stage of the LayerNorm ring
    typedef X2Loop<EPI, true, true, true, X2Chain> Loop;   // the projection phase: packed in and out, the 24 row stores carried
    constexpr int BMX = Loop::BMX;
    constexpr int BIAS_OFF = X2_NSTAGE * Loop::STAGE, GB_OFF = BIAS_OFF + 6144;   // bias2 (N2 <= 1536) | gamma | beta
    static_assert(LR_NST * LSTAGE <= BIAS_OFF && Loop::NW == NW && 2 * Loop::PPW + 24 <= 63, "hand-over layout");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m0l = blockIdx.x * BMX;

    // the projection's bias and the LayerNorm parameters -> LDS, above both rings
    for (int p = wave; p * 256 < N2; p += NW)
        if (p * 256 + lane * 4 < N2) glds16(bias2 + p * 256 + lane * 4, smem + BIAS_OFF + p * 1024);
    if (wave < 2 && wave * 256 + lane * 4 < N) {
        glds16(gamma + wave * 256 + lane * 4, smem + GB_OFF + wave * 1024);
        glds16(beta + wave * 256 + lane * 4, smem + GB_OFF + N * 4 + wave * 1024);
    }

    // ---------------------------------------------------------------- LayerNorm phase: all rows of the block exist, no clamp
    f32x16 acc[12];
    ln384_bias_start(acc, lbias, lane >> 5);
    ln384_kloop<NW, LR_NST, false>(acc, X, Wimg, smem, wave, lane, lane & 31, lane >> 5, m0l, M, K, xpacked);
    wait_vmcnt<0>();                    // the last tiles (past-the-end ones too) have landed in my slots ...
    __builtin_amdgcn_s_barrier();       // ... and in everyone's, and everyone has read its last fragments: the LayerNorm ring is free

    // ---------------------------------------------------------------- hand-over: prime the W ring
    const int ntiles = N2 / X2_BN, G = (int)gridDim.x, wg = (int)blockIdx.x;
    const X2Chain items{chain_part(G, rem_blocks, ntiles, wg), G, ntiles, wg};
    // the block's own fragments are resident: the epilogue below leaves them in x2.bx
    Loop x2(xout, W2, out2, smem, BIAS_OFF, M, N2, wave, items, items.part.n, wg);
    // (the piece offsets are computed again behind the epilogue: held across it they cost registers the epilogue has not got)
    x2.prime(__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)));

    // ---------------------------------------------------------------- LayerNorm epilogue: + residual, statistics, store AND keep
    {
        // (lane ids from mbcnt, not from threadIdx: nothing lane-derived has to live through the k loop or the residual phase)
        const int lane1 = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        ln384_add_residual(acc, res, (uint32_t)group_off(m0l + wave * 32 + (lane1 & 31), lane1 >> 5, N, respacked),
                           (uint32_t)group_off(0, 1, N, respacked));
        float mean, rstd;
        ln384_stats(acc, eps, mean, rstd);
        int lane3 = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
        asm volatile("" : "+v"(lane3));
        const uint32_t oo = (uint32_t)group_off(m0l + wave * 32 + (lane3 & 31), lane3 >> 5, N, 1);
        constexpr uint32_t ogs = 512;   // group_off(0, 1, N, 1)
        const uint64_t xb = (uint64_t)(uintptr_t)xout;
        // gamma / beta from LDS; the row is stored (exactly one store instruction per group: the 24 that the item loop carries) AND
        // kept: group 4 t + gq + h is fragment s = 2 t + gq / 2 of the projection
        const float *gl = reinterpret_cast<const float *>(smem + GB_OFF);
        ln384_normalise(acc, mean, rstd, gl, gl + N, lane3 >> 5, [&](int g, const u32x4 &o) __attribute__((always_inline)) {
            x2_store16(oo + g * ogs, o, xb);
            x2.bx[g / 2] = __builtin_bit_cast(bf16x8, o);
        });
    }

    // ---------------------------------------------------------------- projection phase
    // (lane-derived values of this phase start from an opaque copy of the lane id, so that none of them is computed early and
    // carried through the epilogue, where every register is taken)
    int lane2 = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    asm volatile("" : "+v"(lane2));
    x2.start(lane2);
    x2.run();
}

// =====================================================================================================
// attention on packed tokens (MFMA).  One wave per (sequence, head, block of 32 queries); a workgroup = 4 heads.
//   S^T = K Q^T   v_mfma_f32_32x32x16_bf16 with A = K rows, B = Q rows: the QUERY lands on the lane (column), 16 keys
//                 in the accumulator registers -> softmax statistics are lane-local plus one cross-half shuffle;
//   O^T = V^T P^T the score accumulator, converted pairwise to bf16, IS the B operand of the second product
//                 (cdna_hip_programming.md §3 "An accumulator tile as the next MFMA's operand"); the k order inside a
//                 k-step is then key = 16s + 8(j>>2) + 4h + (j&3), and the V^T fragment is gathered in that order.
// fp32 online softmax over key blocks of 32 (scores = q.k/sqrt(dh) [+ MPNet relative-position bias]).  No mask is
// needed: the packed layout holds valid tokens only, which equals the reference's additive (1-m)*-10000 mask in fp32
// (exp underflows to exactly 0).  Operands come straight from HBM/L2 (each byte of qkv is read once per query block);
// FLOPs are ~S/(6H) of the layer's (<1 % at the benchmark's 16-token mean length): HBM/latency-bound.
// =====================================================================================================
template <int DH, bool REL, bool PK = false>   // PK: qkv is in the block-packed layout (packed_off); ctx stays row-major
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DH <= 32 ? 6 : 4))) void attention_kernel(const bf16_t *__restrict__ qkv,
                                                        const int32_t *__restrict__ cu, const int32_t *__restrict__ col,
                                                        const float *__restrict__ relb, int relw, int H,
                                                        int heads, float scale, bf16_t *__restrict__ ctx, int B, int xcd_map) {
    constexpr int KS = DH / 16;            // k-steps of the QK^T product
    constexpr int OT = (DH + 31) / 32;     // 32-row blocks of O^T
    constexpr int ROWB = DH * 2 < 64 ? 64 : DH * 2;   // bytes per key row of the V image (>= 32 dims, so block reads stay inside)
    __shared__ __attribute__((aligned(16))) char vimg[4 * 32 * ROWB];
    typedef __attribute__((ext_vector_type(4))) short s16x4;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // XCD-aware order: workgroup b runs on XCD b % 8, so sequence = (b % 8) * ceil(B / 8) + b / 8 gives every XCD one contiguous
    // range of sequences: neighbours in the packed token axis share cache lines (a sequence's slice of a 512-byte chunk or of a
    // row rarely starts on a line boundary), and with the plain order the two halves of such a line were fetched by two L2s
    int seq = blockIdx.x;
    if (xcd_map) {
        seq = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
        if (seq >= B) return;
    }
    const int head = blockIdx.y * 4 + wave, qb = blockIdx.z;
    const int t0 = cu[seq], S = cu[seq + 1] - t0;
    if (qb * 32 >= S || head >= heads) return;  // wave-uniform
    const int r = lane & 31, h = lane >> 5;
    const int64_t H3 = 3 * (int64_t)H;
    const int qi = qb * 32 + r;
    const int tq = t0 + (qi < S ? qi : S - 1);

    bf16x8 qf[KS];
    {
        // element (token, feature) of qkv; every access below is 8 features (16 bytes) at a feature offset that is a multiple of 8
        const bf16_t *qp = PK ? qkv + packed_off(tq, head * DH + 8 * h, (int)H3) : qkv + tq * H3 + head * DH + 8 * h;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            qf[s] = *reinterpret_cast<const bf16x8 *>(qp + (PK ? 2 * 256 : 16) * s);   // +16 features = two groups of 8
        }
    }
    const int qcol = REL ? col[tq] : 0;
    f32x16 o[OT];
#pragma unroll
    for (int ob = 0; ob < OT; ++ob)
#pragma unroll
        for (int g = 0; g < 16; ++g) o[ob][g] = 0.f;
    float m = -INFINITY, l = 0.f;

    for (int k0 = 0; k0 < S; k0 += 32) {
        const int kr = k0 + r;
        const int tk = t0 + (kr < S ? kr : S - 1);
        f32x16 sc;
#pragma unroll
        for (int g = 0; g < 16; ++g) sc[g] = 0.f;
        // the key block's V rows are requested together with its K rows (measured equal to requesting them after the softmax)
        constexpr int CH = DH / 16;                          // 16-byte chunks per half row of V
        uint4 vr[CH];
        {
            const bf16_t *kp = PK ? qkv + packed_off(tk, H + head * DH + 8 * h, (int)H3) : qkv + tk * H3 + H + head * DH + 8 * h;
            const bf16_t *vsrc = PK ? qkv + packed_off(tk, 2 * H + head * DH + h * (DH / 2), (int)H3)
                                    : qkv + tk * H3 + 2 * H + head * DH + h * (DH / 2);
            bf16x8 kf[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) kf[s] = *reinterpret_cast<const bf16x8 *>(kp + (PK ? 2 * 256 : 16) * s);
#pragma unroll
            for (int c = 0; c < CH; ++c) vr[c] = *reinterpret_cast<const uint4 *>(vsrc + (PK ? 256 : 8) * c);
#pragma unroll
            for (int s = 0; s < KS; ++s) sc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[s], qf[s], sc, 0, 0, 0);
        }
        // sc[g]: key k0 + (g&3) + 8(g>>2) + 4h, query qi
        float bm = -INFINITY;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int key = k0 + (g & 3) + 8 * (g >> 2) + 4 * h;
            float v = sc[g] * scale;
            if (REL) {
                const int kc = col[t0 + (key < S ? key : S - 1)];
                v += relb[head * relw + (kc - qcol) + (relw >> 1)];
            }
            v = key < S ? v : -INFINITY;
            sc[g] = v;
            bm = fmaxf(bm, v);
        }
        bm = fmaxf(bm, __shfl_xor(bm, 32, 64));
        const float mn = fmaxf(m, bm);
        const float corr = __expf(m - mn);     // first block: exp(-inf) = 0
        float ps = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            sc[g] = __expf(sc[g] - mn);
            ps += sc[g];
        }
        ps += __shfl_xor(ps, 32, 64);
        l = l * corr + ps;
        m = mn;
#pragma unroll
        for (int ob = 0; ob < OT; ++ob)
#pragma unroll
            for (int g = 0; g < 16; ++g) o[ob][g] *= corr;
        // P^T fragments: k-step s takes accumulator registers 8s..8s+7
        bf16x8 pf[2];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int j = 0; j < 8; ++j) pf[s][j] = (__bf16)sc[8 * s + j];
        // V^T fragments in the matching k order.  V rows (keys) are row-major in memory; the MFMA wants, per lane, 8 keys of one
        // head dimension.  Each lane loads half a V row with 16-byte loads into a wave-private [32 keys][ROWB] LDS image and
        // ds_read_b64_tr_b16 hands every lane 4 keys of its dimension (a 16-lane group reads a 4-key x 16-dim block column-
        // major; lane 4q+p of the group supplies the address of key q, dims 4p..4p+3): 2-byte gathers from global memory
        // (16 load instructions per k-step pair) were the kernel's largest cost.  EXEC is full here (out-of-range keys and
        // queries are clamped, not masked), as the instruction requires.
        {
            char *vrow = vimg + wave * (32 * ROWB) + r * ROWB + h * DH;
#pragma unroll
            for (int c = 0; c < CH; ++c) *reinterpret_cast<uint4 *>(vrow + 16 * c) = vr[c];
        }
        __builtin_amdgcn_wave_barrier();                     // wave-private image: LDS ops of one wave execute in order
#pragma unroll
        for (int ob = 0; ob < OT; ++ob) {
            const bool iv = ob * 32 + r < DH;
            const int grp16 = (lane >> 4) & 1, q4 = (lane & 15) >> 2, p4 = lane & 3;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                bf16x8 vf;
#pragma unroll
                for (int half = 0; half < 2; ++half) {
                    const int key = 16 * s + 8 * half + 4 * h + q4;              // row of the block this lane addresses
                    const char *ad = vimg + wave * (32 * ROWB) + key * ROWB + (ob * 32 + grp16 * 16 + 4 * p4) * 2;
                    const s16x4 t = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)ad);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        vf[4 * half + e] = __builtin_bit_cast(__bf16, (bf16_t)(iv ? (bf16_t)t[e] : (bf16_t)0));
                }
                o[ob] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[s], o[ob], 0, 0, 0);
            }
        }
        __builtin_amdgcn_wave_barrier();                     // the next key block overwrites the image
    }
    if (qi < S) {
        const float inv = 1.0f / l;
        bf16_t *op = ctx + (int64_t)(t0 + qi) * H + head * DH + 4 * h;
#pragma unroll
        for (int ob = 0; ob < OT; ++ob)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const int i = ob * 32 + 8 * gq;  // + 4h + (0..3)
                if (i + 4 * h < DH) {
                    uint2 w;
                    w.x = pack_bf16x2(o[ob][4 * gq] * inv, o[ob][4 * gq + 1] * inv);
                    w.y = pack_bf16x2(o[ob][4 * gq + 2] * inv, o[ob][4 * gq + 3] * inv);
                    *reinterpret_cast<uint2 *>(op + i) = w;
                }
            }
    }
}

// =====================================================================================================
// masked mean-pool over the packed layout (A4) + optional fused L2-normalise to half precision (search operand).
// One wave per sequence: pooled[b] = sum_t x[t] / max(len, 1e-9).  HBM-bound: T*H*2 B in.
// A lane owns 16-byte pieces of the row (features 8c .. 8c+7 for c = lane, lane + 64): one 16-byte load per token and
// piece (the first form read 2 bytes per lane and load: 48 us for 52 MB).  Per feature the sum still runs over the
// tokens in ascending order in float32, and the squared norm is taken in the canonical element order of
// tsim_l2norm_rows (element j on lane j % 64, ascending, then the xor butterfly) from a wave-private LDS copy of the
// pooled row, so pooled and unit rows keep their bits.
// MODE (TSIM_POOL_*, the head of tsim_encoder_forward_head): MEAN is the kernel above, unchanged; CLS takes the first token's
// row, MAX the elementwise max over the tokens, MEAN_SQRT_LEN the MEAN sum divided by sqrt(len).  An empty sequence pools to
// a zero row in every mode.  NORM: sentence-transformers' Normalize on the pooled row, x / max(|x|, 1e-12) with the
// canonical order and float64 scale of tsim_l2norm_rows, rounded once to float32; the unit rows are then taken from the
// normalised row (a second canonical pass), so they are tsim_l2norm_rows(final rows) bit for bit.
// =====================================================================================================
template <int NP, int MODE = TSIM_POOL_MEAN, bool NORM = false>   // NP: 16-byte pieces per lane = ceil(H / 512)
__global__ __launch_bounds__(256) void pool_packed_kernel(const bf16_t *__restrict__ x,
                                                          const int32_t *__restrict__ cu, int B, int H,
                                                          float *__restrict__ pooled, unit_t *__restrict__ unit,
                                                          int ld_unit, float *__restrict__ rho_max) {
    __shared__ __attribute__((aligned(16))) float rows[4][NP * 512];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + w;
    if (b >= B) return;
    const int t0 = cu[b], t1 = cu[b + 1];
    float s[NP][8];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int e = 0; e < 8; ++e) s[p][e] = MODE == TSIM_POOL_MAX ? -INFINITY : 0.f;
    // the loop is latency-bound (one dependent-free load per token): four tokens' loads are issued together, the adds stay in
    // token order
    auto add_row = [&](int p, const uint4 &v) __attribute__((always_inline)) {
        const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            s[p][2 * q] += __uint_as_float(wv[q] << 16);
            s[p][2 * q + 1] += __uint_as_float(wv[q] & 0xffff0000u);
        }
    };
    if constexpr (MODE == TSIM_POOL_CLS) {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int f0 = (lane + 64 * p) * 8;
            if (f0 >= H || t1 <= t0) continue;
            const uint4 v = *reinterpret_cast<const uint4 *>(x + (int64_t)t0 * H + f0);
            const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                s[p][2 * q] = __uint_as_float(wv[q] << 16);
                s[p][2 * q + 1] = __uint_as_float(wv[q] & 0xffff0000u);
            }
        }
    } else if constexpr (MODE == TSIM_POOL_MAX) {
        // same round trips as the sums; re-reading the last row past the ragged end leaves a max unchanged
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int f0 = (lane + 64 * p) * 8;
            if (f0 >= H) continue;
            const bf16_t *xp = x + f0;
            for (int t = t0; t < t1; t += 8) {
                uint4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const uint4 *>(xp + (int64_t)(t + u < t1 ? t + u : t1 - 1) * H);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const uint32_t wv[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        s[p][2 * q] = fmaxf(s[p][2 * q], __uint_as_float(wv[q] << 16));
                        s[p][2 * q + 1] = fmaxf(s[p][2 * q + 1], __uint_as_float(wv[q] & 0xffff0000u));
                    }
                }
            }
        }
    } else {
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int f0 = (lane + 64 * p) * 8;
            if (f0 >= H) continue;
            const bf16_t *xp = x + f0;
            // eight tokens per round trip, the ragged end included: a token past the end re-reads the last row (no branch around a
            // load: that would put a full wait behind it) and adds zeros — most sequences of the benchmark are one or two round trips
            for (int t = t0; t < t1; t += 8) {
                uint4 v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const uint4 *>(xp + (int64_t)(t + u < t1 ? t + u : t1 - 1) * H);
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    if (t + u >= t1) v[u] = make_uint4(0u, 0u, 0u, 0u);
                    add_row(p, v[u]);
                }
            }
        }
    }
    const float den = MODE == TSIM_POOL_MEAN_SQRT_LEN ? sqrtf(fmaxf((float)(t1 - t0), 1e-9f)) : fmaxf((float)(t1 - t0), 1e-9f);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int f0 = (lane + 64 * p) * 8;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if constexpr (MODE == TSIM_POOL_MEAN || MODE == TSIM_POOL_MEAN_SQRT_LEN) s[p][e] = s[p][e] / den;
            else if constexpr (MODE == TSIM_POOL_MAX) s[p][e] = t1 > t0 ? s[p][e] : 0.f;
        }
        if (f0 < H) {
            const float4 lo = make_float4(s[p][0], s[p][1], s[p][2], s[p][3]), hi = make_float4(s[p][4], s[p][5], s[p][6], s[p][7]);
            if (!NORM && pooled) {
                *reinterpret_cast<float4 *>(pooled + (int64_t)b * H + f0) = lo;
                *reinterpret_cast<float4 *>(pooled + (int64_t)b * H + f0 + 4) = hi;
            }
            *reinterpret_cast<float4 *>(&rows[w][f0]) = lo;
            *reinterpret_cast<float4 *>(&rows[w][f0 + 4]) = hi;
        }
    }
    if constexpr (NORM) {   // Normalize: the final row replaces the pooled one in registers, in LDS and in `pooled`
        __builtin_amdgcn_wave_barrier();
        double ss = 0.0;
        for (int jx = lane; jx < H; jx += 64) {
            const float v = rows[w][jx];
            ss = fma((double)v, (double)v, ss);
        }
        const double inv = canonical_inv_norm(ss, 1e-12f);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int f0 = (lane + 64 * p) * 8;
#pragma unroll
            for (int e = 0; e < 8; ++e) s[p][e] = canonical_scale_f32(s[p][e], inv);
            if (f0 < H) {
                const float4 lo = make_float4(s[p][0], s[p][1], s[p][2], s[p][3]), hi = make_float4(s[p][4], s[p][5], s[p][6], s[p][7]);
                if (pooled) {
                    *reinterpret_cast<float4 *>(pooled + (int64_t)b * H + f0) = lo;
                    *reinterpret_cast<float4 *>(pooled + (int64_t)b * H + f0 + 4) = hi;
                }
                *reinterpret_cast<float4 *>(&rows[w][f0]) = lo;
                *reinterpret_cast<float4 *>(&rows[w][f0 + 4]) = hi;
            }
        }
    }
    if (unit) {  // identical bits to tsim_l2norm_rows(pooled): same element order, same float64 scale
        __builtin_amdgcn_wave_barrier();   // wave-private row: LDS operations of one wave execute in order
        double ss = 0.0;
        for (int jx = lane; jx < H; jx += 64) {
            const float v = rows[w][jx];
            ss = fma((double)v, (double)v, ss);
        }
        const double inv = canonical_inv_norm(ss, 1e-8f);
        double r2 = 0.0;   // squared rounding residual of the row (the search guard's rho, see tsim_l2norm_rows)
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int f0 = (lane + 64 * p) * 8;
            if (f0 < H) {
                f16x8 u;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    u[e] = canonical_unit_elem(s[p][e], inv);
                    const double de = (double)(float)u[e] - (double)s[p][e] * inv;
                    r2 = fma(de, de, r2);
                }
                *reinterpret_cast<f16x8 *>(unit + (int64_t)b * ld_unit + f0) = u;
            }
        }
        for (int jx = H + lane; jx < ld_unit; jx += 64) unit[(int64_t)b * ld_unit + jx] = 0;
        if (rho_max) {
            const float rho = rho_round_up(sqrt(wave_sum_f64(r2)));
            if (lane == 0) rho_publish(rho_max, rho);
        }
    }
}

// =====================================================================================================
// sequence-classification head (HF BertPooler + classifier):  pooled = tanh(W_p x + b_p),  logits = W_c pooled + b_c
// with x the CLS row (first token) of each sequence in the final hidden state.  One workgroup of H threads per CLS_ROWS
// sequences: the rows are staged in LDS as float32 ([feature][row], so a thread reads its k-th inputs of all rows with two
// 16-byte LDS loads); thread j owns pooled feature j and sums k = 0 .. H-1 in ascending order with one fma per term (W_p
// is stored transposed: one coalesced row of W_p^T per k).  Each logit is one wave's dot product: lane l takes features
// l, l+64, ... in ascending order, then the xor butterfly of wave_sum.  Every sum therefore runs in an order fixed by H
// alone — not by B nor by the sequence's slot in the batch — so rows are batch-composition invariant bit for bit.
// A zero-length sequence reads a zero row.  VALU only: per sequence 2 H^2 + 2 H L FLOP against the encoder's ~24 H^2
// per token and layer.
// =====================================================================================================
constexpr int CLS_ROWS = 8;
constexpr int CLS_MAX_H = 768;
constexpr int CLS_WIDE_H = 1024;   // hidden-1024 encoders: an instance of their own (the launch bound fixes the register budget)
constexpr int CLS_MAX_LABELS = 32;

__global__ __launch_bounds__(CLS_MAX_H) void cls_head_kernel(const bf16_t *__restrict__ x, const int32_t *__restrict__ cu,
                                                             int B, int H, const float *__restrict__ wpT,
                                                             const float *__restrict__ bp, const float *__restrict__ wc,
                                                             const float *__restrict__ bc, int n_labels,
                                                             float *__restrict__ logits) {
    __shared__ __attribute__((aligned(16))) float xs[CLS_MAX_H][CLS_ROWS];   // CLS rows, [feature][row]
    __shared__ float ps[CLS_ROWS][CLS_MAX_H];                               // pooled rows
    const int j = threadIdx.x;   // blockDim.x == H
    const int b0 = blockIdx.x * CLS_ROWS;
#pragma unroll
    for (int r = 0; r < CLS_ROWS; ++r) {
        const int b = b0 + r;
        float v = 0.f;
        if (b < B) {
            const int t0 = cu[b];
            if (cu[b + 1] > t0) v = bf16_to_f32(x[(int64_t)t0 * H + j]);
        }
        xs[j][r] = v;
    }
    __syncthreads();
    float acc[CLS_ROWS];
#pragma unroll
    for (int r = 0; r < CLS_ROWS; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < H; k0 += 8) {   // H % 64 == 0
        float w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) w[u] = wpT[(int64_t)(k0 + u) * H + j];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float4 lo = *reinterpret_cast<const float4 *>(&xs[k0 + u][0]);
            const float4 hi = *reinterpret_cast<const float4 *>(&xs[k0 + u][4]);
            const float xv[CLS_ROWS] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
            for (int r = 0; r < CLS_ROWS; ++r) acc[r] = fmaf(w[u], xv[r], acc[r]);
        }
    }
    const float bj = bp[j];
#pragma unroll
    for (int r = 0; r < CLS_ROWS; ++r) ps[r][j] = tanhf(acc[r] + bj);
    __syncthreads();
    const int lane = j & 63, wave = j >> 6, n_waves = H >> 6;
    const int n_out = CLS_ROWS * n_labels;
    for (int o = wave; o < n_out; o += n_waves) {   // wave-uniform
        const int r = o / n_labels, c = o - r * n_labels;
        const int b = b0 + r;
        if (b >= B) break;   // o grows with r: every later output of this wave is past B as well
        float s = 0.f;
        for (int i = lane; i < H; i += 64) s = fmaf(wc[(int64_t)c * H + i], ps[r][i], s);
        s = wave_sum(s);
        if (lane == 0) logits[(int64_t)b * n_labels + c] = s + bc[c];
    }
}

// The same head for hidden 1024 (1 024 threads; MAXH sits in the launch bound) and for the ReLU between the two layers
// (ACT = TSIM_ACT_RELU, DistilBERT's pre_classifier; TSIM_ACT_TANH also serves RoBERTa's classifier.dense).  A copy, not a
// shared body: the instance above keeps its instructions (through a shared inline body hipcc schedules its index arithmetic
// differently).
template <int MAXH, int ACT>
__global__ __launch_bounds__(MAXH) void cls_head_wide_kernel(const bf16_t *__restrict__ x, const int32_t *__restrict__ cu,
                                                             int B, int H, const float *__restrict__ wpT,
                                                             const float *__restrict__ bp, const float *__restrict__ wc,
                                                             const float *__restrict__ bc, int n_labels,
                                                             float *__restrict__ logits) {
    __shared__ __attribute__((aligned(16))) float xs[MAXH][CLS_ROWS];   // CLS rows, [feature][row]
    __shared__ float ps[CLS_ROWS][MAXH];                               // pooled rows
    const int j = threadIdx.x;   // blockDim.x == H
    const int b0 = blockIdx.x * CLS_ROWS;
#pragma unroll
    for (int r = 0; r < CLS_ROWS; ++r) {
        const int b = b0 + r;
        float v = 0.f;
        if (b < B) {
            const int t0 = cu[b];
            if (cu[b + 1] > t0) v = bf16_to_f32(x[(int64_t)t0 * H + j]);
        }
        xs[j][r] = v;
    }
    __syncthreads();
    float acc[CLS_ROWS];
#pragma unroll
    for (int r = 0; r < CLS_ROWS; ++r) acc[r] = 0.f;
    for (int k0 = 0; k0 < H; k0 += 8) {   // H % 64 == 0
        float w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) w[u] = wpT[(int64_t)(k0 + u) * H + j];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const float4 lo = *reinterpret_cast<const float4 *>(&xs[k0 + u][0]);
            const float4 hi = *reinterpret_cast<const float4 *>(&xs[k0 + u][4]);
            const float xv[CLS_ROWS] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
            for (int r = 0; r < CLS_ROWS; ++r) acc[r] = fmaf(w[u], xv[r], acc[r]);
        }
    }
    const float bj = bp[j];
#pragma unroll
    for (int r = 0; r < CLS_ROWS; ++r) ps[r][j] = ACT == TSIM_ACT_RELU ? fmaxf(acc[r] + bj, 0.f) : tanhf(acc[r] + bj);
    __syncthreads();
    const int lane = j & 63, wave = j >> 6, n_waves = H >> 6;
    const int n_out = CLS_ROWS * n_labels;
    for (int o = wave; o < n_out; o += n_waves) {   // wave-uniform
        const int r = o / n_labels, c = o - r * n_labels;
        const int b = b0 + r;
        if (b >= B) break;   // o grows with r: every later output of this wave is past B as well
        float s = 0.f;
        for (int i = lane; i < H; i += 64) s = fmaf(wc[(int64_t)c * H + i], ps[r][i], s);
        s = wave_sum(s);
        if (lane == 0) logits[(int64_t)b * n_labels + c] = s + bc[c];
    }
}

// =====================================================================================================
// Dense + Normalize of a sentence-transformers head (tsim_dense_rows, tsim_encoder_forward_head):
//   y[b] = act(W x[b] + bias), then y / max(|y|, 1e-12) when `normalize`, then (optional) unit rows of y.
// A workgroup owns DN_ROWS = 16 rows and all d_out columns; its DN_WAVES = 8 waves (two per SIMD, so one wave's loads hide
// behind the other's MFMAs) split the 16-column tiles: wave v computes tiles v, v + 8, ... with
// v_mfma_f32_16x16x4_f32 (A = 16 rows x 4 k of x, B = 4 k x 16 columns of W^T, one float per lane each).  That MFMA is bit for
// bit a k-ordered fmaf chain from C, so every output element is ONE fmaf chain from +0 over its d_in products, in the order
// k = k0 + 4g + j for k0 = 0, 16, ..; j = 0..3; g = 0..3 (lane group g holds k0 + 4g .. k0 + 4g + 3 of a 16-byte load) — fixed
// by d_in alone, so rows are batch-composition invariant.  A half chunk (d_in % 16 == 8) adds fmaf(0, 0, acc) = acc.
// x and W come straight from L2 (W is read once per workgroup: 0.6 MB at 384 x 384), the next chunk's loads are issued before
// the current chunk's MFMAs.  The tiles go through LDS ([row][column], float32) so the row epilogue (bias, tanh, the canonical
// Normalize and unit rows of tsim_l2norm_rows) runs one wave per row with element j on lane j % 64 — the order of
// tsim_l2norm_rows, so unit rows equal tsim_l2norm_rows(out) bit for bit.  w == NULL: no projection (d_out == d_in).
// =====================================================================================================
constexpr int DN_ROWS = 16;
constexpr int DN_MAX = 1024;
constexpr int DN_WAVES = 8;

// 16 bytes at p when ok, else zeros (a `ok ? *p : zero` of two lvalues selects an ADDRESS and puts the zero on the stack)
__device__ __forceinline__ float4 load4_or_zero(const float *p, bool ok) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) v = *reinterpret_cast<const float4 *>(p);
    return v;
}

template <int NT>   // 16-column tiles per wave: d_out <= 16 DN_WAVES NT
__global__ __launch_bounds__(64 * DN_WAVES) void dense_rows_kernel(const float *__restrict__ x, int B, int d_in, const float *__restrict__ wt,
                                                         const float *__restrict__ bias, int d_out, int act, int normalize,
                                                         float *__restrict__ out, unit_t *__restrict__ unit, int ld_unit,
                                                         float *__restrict__ rho_max) {
    extern __shared__ __attribute__((aligned(16))) float ys[];   // [DN_ROWS][d_out]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r0 = blockIdx.x * DN_ROWS;
    if (wt) {
        const int i = lane & 15, g = lane >> 4;
        const int ntt = (d_out + 15) >> 4;
        const float *xp = x + (int64_t)min(r0 + i, B - 1) * d_in + 4 * g;   // rows past B re-read the last row, never stored
        const float *wp[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) wp[t] = wt + (int64_t)min((wv + DN_WAVES * t) * 16 + i, d_out - 1) * d_in + 4 * g;
        f32x4 acc[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        float4 a = load4_or_zero(xp, 4 * g < d_in), bw[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t) bw[t] = load4_or_zero(wp[t], wv + DN_WAVES * t < ntt && 4 * g < d_in);
        for (int k0 = 0; k0 < d_in; k0 += 16) {
            const int k1 = k0 + 16;
            const bool kin = k1 + 4 * g < d_in;
            const float4 an = load4_or_zero(xp + k1, kin);
            float4 bn[NT];
#pragma unroll
            for (int t = 0; t < NT; ++t) bn[t] = load4_or_zero(wp[t] + k1, wv + DN_WAVES * t < ntt && kin);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (wv + DN_WAVES * t < ntt) {   // wave-uniform
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, bw[t].x, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, bw[t].y, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, bw[t].z, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, bw[t].w, acc[t], 0, 0, 0);
                }
            }
            a = an;
#pragma unroll
            for (int t = 0; t < NT; ++t) bw[t] = bn[t];
        }
        // C/D: column lane & 15 of the tile, rows 4g .. 4g + 3
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const int col = (wv + DN_WAVES * t) * 16 + i;
            if (col < d_out) {
#pragma unroll
                for (int r = 0; r < 4; ++r) ys[(4 * g + r) * d_out + col] = acc[t][r];
            }
        }
    } else {   // no projection: the rows themselves
        for (int k = threadIdx.x; k < DN_ROWS * d_out; k += 64 * DN_WAVES) {
            const int r = k / d_out;
            ys[k] = r0 + r < B ? x[(int64_t)(r0 + r) * d_in + (k - r * d_out)] : 0.f;
        }
    }
    __syncthreads();
    for (int r = wv; r < DN_ROWS; r += DN_WAVES) {   // wave-uniform; every lane touches only its own elements j = lane + 64 m
        const int b = r0 + r;
        if (b >= B) break;
        float *y = ys + r * d_out;
        for (int j = lane; j < d_out; j += 64) {
            float v = y[j];
            if (bias) v += bias[j];
            if (act == TSIM_ACT_TANH) v = tanhf(v);
            y[j] = v;
        }
        if (normalize) {
            double ss = 0.0;
            for (int j = lane; j < d_out; j += 64) ss = fma((double)y[j], (double)y[j], ss);
            const double inv = canonical_inv_norm(ss, 1e-12f);
            for (int j = lane; j < d_out; j += 64) y[j] = canonical_scale_f32(y[j], inv);
        }
        if (out)
            for (int j = lane; j < d_out; j += 64) out[(int64_t)b * d_out + j] = y[j];
        if (unit) {   // tsim_l2norm_rows(y, eps 1e-8), element for element
            double ss = 0.0;
            for (int j = lane; j < d_out; j += 64) ss = fma((double)y[j], (double)y[j], ss);
            const double inv = canonical_inv_norm(ss, 1e-8f);
            double r2 = 0.0;
            for (int j = lane; j < ld_unit; j += 64) {
                unit_t hv = (unit_t)0;
                if (j < d_out) {
                    hv = canonical_unit_elem(y[j], inv);
                    const double de = (double)(float)hv - (double)y[j] * inv;
                    r2 = fma(de, de, r2);
                }
                unit[(int64_t)b * ld_unit + j] = hv;
            }
            if (rho_max) {
                const float rho = rho_round_up(sqrt(wave_sum_f64(r2)));
                if (lane == 0) rho_publish(rho_max, rho);
            }
        }
    }
}

static int dense_rows_launch(const float *x, int B, int d_in, const float *w, const float *bias, int d_out, int act, int normalize,
                             float *out, unit_t *unit, int ld_unit, float *rho_max, hipStream_t st) {
    if (B <= 0) return TSIM_OK;
    const dim3 grid((unsigned)((B + DN_ROWS - 1) / DN_ROWS));
    const size_t lds = (size_t)DN_ROWS * d_out * sizeof(float);
#define DENSE(NT) hipLaunchKernelGGL(dense_rows_kernel<NT>, grid, dim3(64 * DN_WAVES), lds, st, x, B, d_in, w, bias, d_out, act, normalize, out, unit, ld_unit, rho_max)
    const int nt = ((d_out + 15) / 16 + DN_WAVES - 1) / DN_WAVES;   // tiles per wave
    if (nt <= 1) DENSE(1); else if (nt <= 2) DENSE(2); else if (nt <= 3) DENSE(3); else if (nt <= 4) DENSE(4);
    else if (nt <= 6) DENSE(6); else DENSE(8);
#undef DENSE
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

// shared argument checks of tsim_dense_rows and the head of tsim_encoder_forward_head
static int dense_check(int d_in, int d_out, int act, const float *w) {
    TSIM_REQUIRE(d_in >= 8 && d_in <= DN_MAX && d_in % 8 == 0, "dense: d_in=%d outside [8, %d] or not a multiple of 8", d_in, DN_MAX);
    TSIM_REQUIRE(d_out >= 8 && d_out <= DN_MAX && d_out % 8 == 0, "dense: d_out=%d outside [8, %d] or not a multiple of 8", d_out,
                 DN_MAX);
    TSIM_REQUIRE(w || d_out == d_in, "dense: without a weight matrix d_out (%d) must equal d_in (%d)", d_out, d_in);
    TSIM_REQUIRE(act == TSIM_ACT_IDENTITY || act == TSIM_ACT_TANH, "dense: unknown activation %d (TSIM_ACT_IDENTITY, TSIM_ACT_TANH)",
                 act);
    TSIM_REQUIRE(((uintptr_t)w & 15) == 0, "dense: the weight matrix must be 16-byte aligned");
    return TSIM_OK;
}

// =====================================================================================================
// host side
// =====================================================================================================
static uint16_t host_f32_to_bf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

}  // namespace tsim

#include "encoder_plan.h"   // EncoderPlan, encoder_plan, chain_blocks, ln384_segments: which kernels run

using namespace tsim;

struct tsim_encoder {
    tsim_encoder_config cfg;
    EncoderPlan plan;   // (of cfg: tsim_encoder_create builds its images and buffers, the forward runs its forms)
    int Tp = 0;
    // weights
    float *word = nullptr, *pos = nullptr, *type0 = nullptr, *emb_g = nullptr, *emb_b = nullptr, *relb = nullptr;
    int relw = 0;
    int n_types = 0;   // rows of the token-type table at type0 (tsim_encoder_set_token_types); 0: row 0 only, untyped calls only
    // sequence-classification head (tsim_encoder_set_cls_head), float32: W_p transposed [in][out], b_p, W_c [labels][H], b_c
    float *head_wpT = nullptr, *head_bp = nullptr, *head_wc = nullptr, *head_bc = nullptr;
    int n_labels = 0;
    int head_act = TSIM_ACT_TANH;   // TSIM_ACT_TANH | TSIM_ACT_RELU (tsim_encoder_set_cls_head_act)
    struct Layer {
        bf16_t *wqkv, *wo, *w1, *w2;
        bf16_t *pqkv = nullptr, *po = nullptr;     // tile-major copies for the ping-pong GEMM (QKV and O-projection)
        bf16_t *lo = nullptr, *l2 = nullptr;   // H = 384: O-proj / FFN2 weights as the k-tile LDS images of the LayerNorm GEMM
        bf16_t *lo32 = nullptr, *l232 = nullptr;   // ... and as MFMA fragment images (pack_frag_w_kernel) for ln_rows_gemm / ln_tail_gemm
        uint8_t *qqkv = nullptr, *qo = nullptr, *q1 = nullptr, *q2 = nullptr;   // MXFP8 weights: e4m3 bytes (tile-major) ...
        uint8_t *sqkv = nullptr, *so = nullptr, *s1 = nullptr, *s2 = nullptr;   // ... and E8M0 block scales [out, in/32]
        float *bqkv, *bo, *b1, *b2, *g1, *be1, *g2, *be2;
    };
    std::vector<Layer> layers;
    std::vector<void *> allocs;
    // activations
    bf16_t *x0 = nullptr, *x1 = nullptr, *qkv = nullptr, *ctx = nullptr, *h1 = nullptr;
    float *ybuf = nullptr;   // fp32 pre-LayerNorm sums (wide models only)
    float *lnimg = nullptr;  // hidden 384: ln_split's accumulator images (LS_MAX_BLOCKS row blocks at most)
    // pre-Dense rows of a sentence head (tsim_encoder_forward_head) [max_seqs, H] float32: only when qkv, dead after the last
    // layer and used for them otherwise, is too small (max_seqs > 1.5 Tp: batches of mostly empty sequences)
    float *head_x = nullptr;
    uint8_t *aq = nullptr, *as = nullptr, *hq = nullptr, *hs = nullptr;   // MXFP8 images of a projection's input ([Tp,H] / [Tp,F])
    int *err_flags = nullptr;   // TSIM_ENC_ERR_* bits raised by kernels since the last tsim_encoder_error_flags
};

namespace tsim {

static int dev_alloc(tsim_encoder *e, size_t bytes, void **out) {
    void *p = nullptr;
    hipError_t err = hipMalloc(&p, bytes);
    if (err != hipSuccess) return fail(TSIM_ENOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(err));
    e->allocs.push_back(p);
    *out = p;
    return TSIM_OK;
}

static int upload_f32(tsim_encoder *e, const float *h, size_t n, float **out) {
    int rc = dev_alloc(e, n * 4, (void **)out);
    if (rc) return rc;
    TSIM_HIP_CHECK(hipMemcpy(*out, h, n * 4, hipMemcpyHostToDevice));
    return TSIM_OK;
}

static int upload_bf16(tsim_encoder *e, const std::vector<const float *> &parts, size_t n_each, bf16_t **out) {
    std::vector<uint16_t> tmp(n_each * parts.size());
    for (size_t p = 0; p < parts.size(); ++p)
        for (size_t i = 0; i < n_each; ++i) tmp[p * n_each + i] = host_f32_to_bf16(parts[p][i]);
    int rc = dev_alloc(e, tmp.size() * 2, (void **)out);
    if (rc) return rc;
    TSIM_HIP_CHECK(hipMemcpy(*out, tmp.data(), tmp.size() * 2, hipMemcpyHostToDevice));
    return TSIM_OK;
}

// MPNet relative_position_bucket (transformers mpnet/modeling_mpnet.py relative_position_bucket):
// rel = key_col - query_col, n = -rel.
// fp32 -> e4m3 byte, nearest even, |v| <= 448 (oracle/fp8_ref.f32_to_e4m3)
static uint8_t host_f32_to_e4m3(float v) {
    const uint8_t sign = std::signbit(v) ? 0x80 : 0;
    const double a = std::fabs((double)v);
    if (a == 0.0) return sign;
    int exp;
    const double mant = std::frexp(a, &exp);          // a = mant * 2^exp, mant in [0.5, 1)
    long byte;
    if (a >= std::ldexp(1.0, -6))
        byte = ((long)(exp - 1 + 7) << 3) + std::lrint((mant * 2.0 - 1.0) * 8.0);   // a carry of 8 bumps the exponent
    else
        byte = std::lrint(std::ldexp(a, 9));
    if (byte > 0x7e) byte = 0x7e;
    return (uint8_t)byte | sign;
}

// parts: row blocks of n_rows x K fp32 (nn.Linear [out, in]) -> MXFP8 along K (oracle/fp8_ref.mx_quantize)
static int upload_mxfp8(tsim_encoder *e, const std::vector<const float *> &parts, size_t n_rows, size_t K, uint8_t **q,
                        uint8_t **sc) {
    const size_t rows = n_rows * parts.size(), nb = K / 32;
    std::vector<uint8_t> hq(rows * K), hs(rows * nb);
    for (size_t p = 0; p < parts.size(); ++p)
        for (size_t r = 0; r < n_rows; ++r)
            for (size_t b = 0; b < nb; ++b) {
                const float *src = parts[p] + r * K + b * 32;
                float amax = 0.f;
                for (int i = 0; i < 32; ++i) amax = std::fmax(amax, std::fabs(src[i]));
                int sexp = 0;
                if (amax > 0.f) {
                    int ex;
                    (void)std::frexp((double)amax, &ex);
                    sexp = ex - 1 - 8;
                    sexp = sexp < -127 ? -127 : (sexp > 127 ? 127 : sexp);
                }
                uint8_t *dst = hq.data() + (p * n_rows + r) * K + b * 32;
                for (int i = 0; i < 32; ++i) {
                    double y = std::ldexp((double)src[i], -sexp);
                    y = y > 448.0 ? 448.0 : (y < -448.0 ? -448.0 : y);
                    dst[i] = host_f32_to_e4m3((float)y);
                }
                hs[(p * n_rows + r) * nb + b] = (uint8_t)(sexp + 127);
            }
    int rc = dev_alloc(e, hq.size(), (void **)q);
    if (rc) return rc;
    if ((rc = dev_alloc(e, hs.size(), (void **)sc))) return rc;
    TSIM_HIP_CHECK(hipMemcpy(*q, hq.data(), hq.size(), hipMemcpyHostToDevice));
    TSIM_HIP_CHECK(hipMemcpy(*sc, hs.data(), hs.size(), hipMemcpyHostToDevice));
    return TSIM_OK;
}

static int mpnet_bucket(int rel, int num_buckets) {
    int ret = 0;
    int n = -rel;
    const int nb = num_buckets / 2;
    if (n < 0) {
        ret += nb;
        n = -n;
    }
    const int max_exact = nb / 2;
    if (n < max_exact) return ret + n;
    // float32 arithmetic like torch: log(n / max_exact) / log(128 / max_exact) * (nb - max_exact)
    const float v = logf((float)n / (float)max_exact) / (float)log(128.0 / max_exact) * (float)(nb - max_exact);
    int large = max_exact + (int)v;
    if (large > nb - 1) large = nb - 1;
    return ret + large;
}

// Where the rows of a hidden-384 LayerNorm GEMM's operands live: row-major, or the block-packed layout (packed_off) that qkv, h1
// and the residual stream have between the kernels of the packed family.  (The kernels take them as 0 / 1.)
enum Layout : int { ROW_MAJOR = 0, BLOCK_PACKED = 1 };
struct Layouts { Layout x, res, out; };
constexpr Layouts ALL_ROW_MAJOR = {ROW_MAJOR, ROW_MAJOR, ROW_MAJOR};

// A hidden-384 LayerNorm GEMM: out = LayerNorm(X W^T + bias + res) gamma + beta, X [rows, K], W [384, K] row-major, as k-tile LDS
// images (Wk: pack_gemm_w_kernel) and as MFMA fragment images (Wf: pack_frag_w_kernel)
struct LnGemm {
    const bf16_t *X, *W, *Wk, *Wf;
    const float *bias;
    const bf16_t *res;
    const float *gamma, *beta;
    float eps;
    bf16_t *out;
    int K;
    Layouts lay;
};

template <int BM, int BN, int BK, int WM, int WN, int EPI, int NST = 2>
static int launch_gemm(const bf16_t *X, const bf16_t *W, const float *bias, const bf16_t *res, const float *gamma,
                       const float *beta, float eps, bf16_t *out, int M, int N, int K, hipStream_t st,
                       const bf16_t *Wimg, Layouts lay) {
    constexpr int lds = gemm_lds_bytes<BM, BN, BK, WM, WN, NST>();
    static_assert(lds <= 160 * 1024, "LDS budget");
    auto kern = gemm_bf16_kernel<BM, BN, BK, WM, WN, EPI, NST>;
    static DevOnce lds_once;
    TSIM_MAX_LDS(lds_once, kern, lds);
    if (N % BN != 0 || K % BK != 0) return fail(TSIM_EUNSUPPORTED, "gemm: N=%d K=%d not tileable by %dx%d", N, K, BN, BK);
    const int mtiles = (M + BM - 1) / BM, ntiles = N / BN;
    const int grid = ((mtiles + 7) / 8) * 8 * ntiles;
    if (Wimg && ntiles != 1) return fail(TSIM_EINVAL, "gemm: a packed W image needs BN == N");
    hipLaunchKernelGGL(kern, dim3(grid), dim3(WM * WN * 64), lds, st, X, W, bias, res, gamma, beta, eps, out, M, N, K,
                       mtiles, ntiles, Wimg, (int)lay.x, (int)lay.res, (int)lay.out);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

template <int EPI, bool PK, bool XPK>
static int gemm_xres2(const bf16_t *X, const bf16_t *W, const float *bias, bf16_t *out, int M, int N, hipStream_t st) {
    constexpr int lds = X2_NSTAGE * X2_BN * X2_BK * 2 + 8192;   // ring | bias (N <= 2048)
    if (N > 2048) return fail(TSIM_EUNSUPPORTED, "gemm_xres2: N=%d > 2048", N);
    if (((int64_t)M + 256) * N * 2 >= (1ll << 32)) return fail(TSIM_EUNSUPPORTED, "gemm_xres2: output of %d x %d exceeds 4 GiB", M, N);
    auto kern = gemm_xres2_kernel<EPI, PK, XPK>;
    static DevOnce lds_once;
    TSIM_MAX_LDS(lds_once, kern, lds);
    const int items = ((M + 255) / 256) * (N / X2_BN);
    const int grid = items < 256 ? items : 256;             // persistent workgroups, one per CU
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), lds, st, X, W, bias, out, M, N, items);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

// =====================================================================================================
// ln_tail_gemm: the LayerNorm GEMM of width 384 for FEW rows (the remainder behind ln_rows_gemm's whole rounds, and small batches).
//
// A remainder launch has far fewer workgroups than CUs, and every workgroup has to see ALL of W whatever its token count: its cost is
// the latency of its k loop.  Through an LDS ring that loop paid, per 64-k tile, a workgroup barrier, seven LDS-DMA issues per wave
// (~100-150 cycles each) and the DMA's own latency for twelve MFMAs per wave: 1.7 us per tile, 40 us for FFN2's 24 tiles and 1 657
// rows (against 90 us for the 65 536 rows of the main launch) — 13 % of a MiniLM forward for 2.5 % of its rows.
// Here nothing is shared, so nothing goes through LDS: a workgroup is 32 token rows x 4 waves, wave w owns features 96 w .. + 95
// (three accumulator tiles) and streams ITS slice of W straight from L2 into MFMA A fragments, and the token rows likewise into B
// fragments (the four waves read the same rows: L1 hits).  W is stored as MFMA fragment blocks (pack_frag_w_kernel): a wave's load
// is one contiguous KiB — and the image is the one ln_rows_gemm has just streamed through every XCD's L2.  (Reading a swizzled
// LDS image instead, 16-byte chunks scattered over 2 KiB per load, measured 38 us against 27 for FFN2's remainder.)  Loads roll PF
// k-steps ahead of their MFMAs with counted vmcnt waits; no barrier until the LayerNorm statistics cross the four feature waves (gemm_bf16_kernel's direct
// epilogue, operation for operation).
// Same arithmetic as the other two forms — accumulators start from the bias, k ascending in 32x32x16 steps, statistics in the order
// (wave's 48 values, half-wave partner, waves 0..3) — so a row has the same bits whichever kernel produced it.
// Bound: 12 KiB of W + 4 KiB of rows per k-step and workgroup at the CU's 64 B/clk L2 path = 256 cycles per k-step.
// =====================================================================================================
typedef __attribute__((ext_vector_type(4))) uint32_t lt_u32x4;

// The GEMM part of one ln_tail wave: acc = bias + X W^T + res for token rows m0 .. m0 + 31 and features 96 wn .. + 95, in the
// calling wave's registers (lane = token row r + 32 h, as the MFMA leaves them).
template <int PF>
__device__ __forceinline__ void lt_gemm_slice(const bf16_t *__restrict__ X, const bf16_t *__restrict__ Wimg32,
                                              const float *__restrict__ bias, const bf16_t *__restrict__ res, int M, int K,
                                              int xpacked, int respacked, int wn, int m0, f32x16 (&acc)[3]) {
    constexpr int N = 384, NT = 3;
    const int lane = threadIdx.x & 63;
    const int r = lane & 31, h = lane >> 5;
    const int ksteps = K / 16;                                   // a multiple of PF (launcher)

    // per-lane source addresses at k-step 0; per k-step the W pointer advances 12 KiB, the row pointer 1 KiB (packed) or 32 B
    const int64_t mrow = (int64_t)(m0 + r < M ? m0 + r : M - 1);
    const char *xp = reinterpret_cast<const char *>(X) +
                     (xpacked ? (int64_t)(m0 >> 5) * K * 64 + h * 512 + r * 16          // (rows of a partial block exist: padding)
                              : (mrow * K + 8 * h) * 2);
    const int xstep = xpacked ? 1024 : 32;
    const char *wp = reinterpret_cast<const char *>(Wimg32) + (int64_t)(NT * wn) * 1024 + lane * 16;
    constexpr int WSTEP = (N / 32) * 1024;                       // fragment blocks of one k-step

#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const float4 bv = *reinterpret_cast<const float4 *>(bias + wn * 96 + 4 * h + i * 32 + 8 * gq);
            acc[i][4 * gq + 0] = bv.x;
            acc[i][4 * gq + 1] = bv.y;
            acc[i][4 * gq + 2] = bv.z;
            acc[i][4 * gq + 3] = bv.w;
        }
#pragma unroll
    for (int i = 0; i < NT; ++i) asm volatile("" : "+v"(acc[i]));   // retire the bias loads: the vmcnt counts below are exact

    lt_u32x4 fw[PF][NT], fx[PF];
    // (the three W loads of a step use immediate offsets 0 / 1024 / 2048 from one address register)
    auto issue = [&](auto slotc, int s) __attribute__((always_inline)) {
        constexpr int slot = decltype(slotc)::value;
        const int sc = s < ksteps ? s : ksteps - 1;              // past the end: re-read the last step (uniform vmcnt)
        const char *w = wp + (int64_t)sc * WSTEP;
        const char *x = xp + (int64_t)sc * xstep;
        // (references: an asm operand alone does not make a generic lambda capture the arrays)
        lt_u32x4 &f0 = fw[slot][0], &f1 = fw[slot][1], &f2 = fw[slot][2], &f3 = fx[slot];
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(f0) : "v"(w) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, off offset:1024" : "=v"(f1) : "v"(w) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, off offset:2048" : "=v"(f2) : "v"(w) : "memory");
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(f3) : "v"(x) : "memory");
    };
    ff_static_for(std::make_integer_sequence<int, PF>{}, [&](auto sc) __attribute__((always_inline)) { issue(sc, decltype(sc)::value); });
    for (int s0 = 0; s0 < ksteps; s0 += PF) {
        ff_static_for(std::make_integer_sequence<int, PF>{}, [&](auto sc) __attribute__((always_inline)) {
            constexpr int slot = decltype(sc)::value;
            // the 4 (PF - 1) loads of the PF - 1 younger steps may stay in flight
            lt_u32x4 &f0 = fw[slot][0], &f1 = fw[slot][1], &f2 = fw[slot][2], &f3 = fx[slot];
            asm volatile("s_waitcnt vmcnt(%4)" : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3) : "n"(4 * (PF - 1)) : "memory");
            const bf16x8 bx = __builtin_bit_cast(bf16x8, f3);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f0), bx, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f1), bx, acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, f2), bx, acc[2], 0, 0, 0);
            // the slot's registers are free once the MFMAs have READ them: the reload below is ordered behind them by its
            // dependency on the same registers
            asm volatile("" : "+v"(f0), "+v"(f1), "+v"(f2), "+v"(f3));
            issue(sc, s0 + slot + PF);
        });
    }
    wait_vmcnt<0>();

    // ---- residual: gemm_bf16_kernel<.., WAVES_N = 4, ..>'s direct epilogue with MT = 1, operation for operation
    {
        const int64_t m = m0 + r;
        const int64_t mr = m < M ? m : M - 1;
        const uint32_t ro = (uint32_t)group_off(mr, wn * 12 + h, N, respacked), rgs = (uint32_t)group_off(0, 1, N, respacked);
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int gq = 0; gq < 4; gq += 2) {
                const uint4 o = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(res) + (ro + (4 * i + gq) * rgs));
                auto s0 = __builtin_amdgcn_permlane32_swap(o.x, o.z, false, false);
                auto s1 = __builtin_amdgcn_permlane32_swap(o.y, o.w, false, false);
                const uint32_t a0 = s0[0], c0 = s0[1], a1 = s1[0], c1 = s1[1];
                acc[i][4 * gq + 0] += __uint_as_float(a0 << 16);
                acc[i][4 * gq + 1] += __uint_as_float(a0 & 0xffff0000u);
                acc[i][4 * gq + 2] += __uint_as_float(a1 << 16);
                acc[i][4 * gq + 3] += __uint_as_float(a1 & 0xffff0000u);
                acc[i][4 * gq + 4] += __uint_as_float(c0 << 16);
                acc[i][4 * gq + 5] += __uint_as_float(c0 & 0xffff0000u);
                acc[i][4 * gq + 6] += __uint_as_float(c1 << 16);
                acc[i][4 * gq + 7] += __uint_as_float(c1 & 0xffff0000u);
            }
    }
}

// The LayerNorm part: statistics in the order (wave's 48 values, half-wave partner, waves 0..3) and the normalised bf16 rows.  All
// four feature waves of the row block call it in one workgroup (red: its 2 x 4 x 32 floats of LDS).
__device__ __forceinline__ void lt_layernorm(f32x16 (&acc)[3], float *red, const float *__restrict__ gamma,
                                             const float *__restrict__ beta, float eps, bf16_t *__restrict__ out, int M, int wn,
                                             int m0, int opacked) {
    constexpr int N = 384, NT = 3, WAVES_N = 4, BM = 32;
    const int lane = threadIdx.x & 63;
    const int r = lane & 31, h = lane >> 5;
    const int nbase = wn * 96 + 4 * h;
    float mean = 0.f, rstd = 0.f;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                if (pass == 0) {
                    s += acc[i][g];
                } else {
                    const float dlt = acc[i][g] - mean;
                    s = fmaf(dlt, dlt, s);
                }
            }
        s += __shfl_xor(s, 32, 64);
        if (h == 0) red[(pass * WAVES_N + wn) * BM + r] = s;
        __syncthreads();
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < WAVES_N; ++w) t += red[(pass * WAVES_N + w) * BM + r];
        if (pass == 0)
            mean = t / (float)N;
        else
            rstd = 1.0f / sqrtf(t / (float)N + eps);
    }
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        float4 gv[4], be[4];
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            gv[gq] = *reinterpret_cast<const float4 *>(gamma + nbase + i * 32 + 8 * gq);
            be[gq] = *reinterpret_cast<const float4 *>(beta + nbase + i * 32 + 8 * gq);
        }
        uint32_t pk[8];
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const float y0 = fmaf((acc[i][4 * gq + 0] - mean) * rstd, gv[gq].x, be[gq].x);
            const float y1 = fmaf((acc[i][4 * gq + 1] - mean) * rstd, gv[gq].y, be[gq].y);
            const float y2 = fmaf((acc[i][4 * gq + 2] - mean) * rstd, gv[gq].z, be[gq].z);
            const float y3 = fmaf((acc[i][4 * gq + 3] - mean) * rstd, gv[gq].w, be[gq].w);
            pk[2 * gq] = pack_bf16x2(y0, y1);
            pk[2 * gq + 1] = pack_bf16x2(y2, y3);
        }
        const int64_t m = m0 + r;
        const uint32_t oo = (uint32_t)group_off(m, wn * 12 + h, N, opacked), ogs = (uint32_t)group_off(0, 1, N, opacked);
#pragma unroll
        for (int gq = 0; gq < 4; gq += 2) {
            auto s0 = __builtin_amdgcn_permlane32_swap(pk[2 * gq], pk[2 * gq + 2], false, false);
            auto s1 = __builtin_amdgcn_permlane32_swap(pk[2 * gq + 1], pk[2 * gq + 3], false, false);
            if (m < M)
                *reinterpret_cast<uint4 *>(reinterpret_cast<char *>(out) + (oo + (4 * i + gq) * ogs)) = make_uint4(s0[0], s1[0], s0[1], s1[1]);
        }
    }
}

template <int PF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1))) void ln_tail_gemm_kernel(
    const bf16_t *__restrict__ X, const bf16_t *__restrict__ Wimg32, const float *__restrict__ bias, const bf16_t *__restrict__ res,
    const float *__restrict__ gamma, const float *__restrict__ beta, float eps, bf16_t *__restrict__ out, int M, int K, int xpacked,
    int respacked, int opacked) {
    __shared__ float red[2 * 4 * 32];
    const int wn = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m0 = blockIdx.x * 32;
    f32x16 acc[3];
    lt_gemm_slice<PF>(X, Wimg32, bias, res, M, K, xpacked, respacked, wn, m0, acc);
    lt_layernorm(acc, red, gamma, beta, eps, out, M, wn, m0, opacked);
}

// =====================================================================================================
// ln_split: ln_tail with the 384 features of a row block split over S workgroups (S = 2: two feature waves each, S = 4: one),
// for remainders of few blocks.  ln_tail's k loop is bound by the CU's L2 path — every workgroup streams ALL of W, 16 KiB per
// k-step — on as many CUs as there are row blocks; with S slices per block, S times as many CUs stream 1/S of W each (at S = 4:
// 3 KiB of W + 1 KiB of rows = 64 cycles against 96 of MFMA per k-step).  Each wave runs ln_tail's loop and residual add
// unchanged and stores its accumulators as an fp32 register image (lane and register order kept); ln_split_finish_kernel then
// reloads the four images of a row block into the registers of four waves and runs ln_tail's LayerNorm, so a row carries the
// same bits as from every other form.
// Image: [row block][wave wn][i * 4 + gq][lane] float4 = acc[i][4 gq .. 4 gq + 3] (48 KiB per row block, coalesced KiB stores).
// =====================================================================================================
template <int PF, int S>
__global__ __launch_bounds__(256 / S) __attribute__((amdgpu_waves_per_eu(1, 1))) void ln_split_gemm_kernel(
    const bf16_t *__restrict__ X, const bf16_t *__restrict__ Wimg32, const float *__restrict__ bias, const bf16_t *__restrict__ res,
    float4 *__restrict__ img, int M, int K, int xpacked, int respacked) {
    const int blk = blockIdx.x / S, sl = blockIdx.x % S;
    const int wn = __builtin_amdgcn_readfirstlane(sl * (4 / S) + (threadIdx.x >> 6));
    const int m0 = blk * 32;
    f32x16 acc[3];
    lt_gemm_slice<PF>(X, Wimg32, bias, res, M, K, xpacked, respacked, wn, m0, acc);
    float4 *dst = img + (int64_t)(blk * 4 + wn) * 12 * 64 + (threadIdx.x & 63);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
            dst[(i * 4 + gq) * 64] = make_float4(acc[i][4 * gq + 0], acc[i][4 * gq + 1], acc[i][4 * gq + 2], acc[i][4 * gq + 3]);
}

__global__ __launch_bounds__(256) void ln_split_finish_kernel(const float4 *__restrict__ img, const float *__restrict__ gamma,
                                                              const float *__restrict__ beta, float eps, bf16_t *__restrict__ out,
                                                              int M, int opacked) {
    __shared__ float red[2 * 4 * 32];
    const int wn = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int m0 = blockIdx.x * 32;
    const float4 *src = img + (int64_t)(blockIdx.x * 4 + wn) * 12 * 64 + (threadIdx.x & 63);
    f32x16 acc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const float4 v = src[(i * 4 + gq) * 64];
            acc[i][4 * gq + 0] = v.x;
            acc[i][4 * gq + 1] = v.y;
            acc[i][4 * gq + 2] = v.z;
            acc[i][4 * gq + 3] = v.w;
        }
    lt_layernorm(acc, red, gamma, beta, eps, out, M, wn, m0, opacked);
}

// Rows [0, M) of g (M <= 8 192) as one TSIM_SEG_LN_TAIL / _SPLIT2 / _SPLIT4 segment.  img: ln_split's accumulator images
static int ln_tail_gemm(const LnGemm &g, int M, int form, float *img, hipStream_t st) {
    if (g.K % (16 * LT_PF) != 0) return fail(TSIM_EUNSUPPORTED, "ln_tail_gemm: K=%d", g.K);
    const int nb = (M + 31) / 32, xpk = g.lay.x, rpk = g.lay.res, opk = g.lay.out;
    if (form == TSIM_SEG_LN_TAIL) {
        hipLaunchKernelGGL(ln_tail_gemm_kernel<LT_PF>, dim3((unsigned)nb), dim3(256), 0, st, g.X, g.Wf, g.bias, g.res, g.gamma, g.beta,
                           g.eps, g.out, M, g.K, xpk, rpk, opk);
        TSIM_HIP_CHECK(hipGetLastError());
        return TSIM_OK;
    }
    float4 *im = reinterpret_cast<float4 *>(img);
    if (form == TSIM_SEG_LN_SPLIT4)
        hipLaunchKernelGGL((ln_split_gemm_kernel<LT_PF, 4>), dim3((unsigned)(nb * 4)), dim3(64), 0, st, g.X, g.Wf, g.bias, g.res, im, M,
                           g.K, xpk, rpk);
    else
        hipLaunchKernelGGL((ln_split_gemm_kernel<LT_PF, 2>), dim3((unsigned)(nb * 2)), dim3(128), 0, st, g.X, g.Wf, g.bias, g.res, im, M,
                           g.K, xpk, rpk);
    TSIM_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ln_split_finish_kernel, dim3((unsigned)nb), dim3(256), 0, st, im, g.gamma, g.beta, g.eps, g.out, M, opk);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

// Rows [0, M) of g in workgroups of NW * 32 token rows (the last one may be partial)
template <int NW, int NST>
static int ln_rows_gemm(const LnGemm &g, int M, hipStream_t st) {
    constexpr int lds = NST * (NW * 32 * LR_BK * 2 + LR_WBYTES);   // <8, 3>: 120 KiB
    static_assert(lds <= 160 * 1024, "LDS budget");
    auto kern = ln_rows_gemm_kernel<NW, NST>;
    static DevOnce lds_once;
    TSIM_MAX_LDS(lds_once, kern, lds);
    if (g.K % LR_BK != 0 || g.K < NST * LR_BK) return fail(TSIM_EUNSUPPORTED, "ln_rows_gemm: K=%d", g.K);
    if (((int64_t)M + 256) * 768 >= (1ll << 32)) return fail(TSIM_EUNSUPPORTED, "ln_rows_gemm: %d rows of 384 exceed 4 GiB", M);
    hipLaunchKernelGGL(kern, dim3((unsigned)((M + NW * 32 - 1) / (NW * 32))), dim3(NW * 64), lds, st, g.X, g.Wf, g.bias, g.res, g.gamma,
                       g.beta, g.eps, g.out, M, g.K, (int)g.lay.x, (int)g.lay.res, (int)g.lay.out);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

// ln_rows_xres2: the first `blocks` 256-token blocks of g (output block-packed) + the projection [M, 384] x W2^T -> out2 [M, N2] of
// ALL M rows (the rows behind the whole blocks must have been written to g.out before: ln384_gemm runs those segments first)
template <int EPI>
static int ln_rows_xres2(const LnGemm &g, int blocks, const bf16_t *W2, const float *bias2, bf16_t *out2, int M, int N2, hipStream_t st) {
    constexpr int lds = X2_NSTAGE * X2_BN * X2_BK * 2 + 6144 + 2 * 384 * 4;   // W ring (over the LayerNorm ring) | bias2 | gamma | beta
    static_assert(lds <= 160 * 1024, "LDS budget");
    if (N2 % X2_BN != 0 || N2 > 1536) return fail(TSIM_EUNSUPPORTED, "ln_rows_xres2: N=%d", N2);
    if (g.K % LR_BK != 0 || g.K < 3 * LR_BK) return fail(TSIM_EUNSUPPORTED, "ln_rows_xres2: K=%d", g.K);
    if (blocks <= 0 || (int64_t)blocks * 256 > M) return fail(TSIM_EINVAL, "ln_rows_xres2: %d blocks of %d rows", blocks, M);
    if (((int64_t)M + 256) * N2 * 2 >= (1ll << 32) || ((int64_t)M + 256) * 768 >= (1ll << 32))
        return fail(TSIM_EUNSUPPORTED, "ln_rows_xres2: output of %d x %d exceeds 4 GiB", M, N2);
    auto kern = ln_rows_xres2_kernel<EPI>;
    static DevOnce lds_once;
    TSIM_MAX_LDS(lds_once, kern, lds);
    const int rem_blocks = (M - blocks * 256 + 255) / 256;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(512), lds, st, g.X, g.Wf, g.bias, g.res, g.gamma, g.beta, g.eps, g.out, g.K,
                       (int)g.lay.x, (int)g.lay.res, W2, bias2, out2, M, N2, rem_blocks);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

// T rows of g, segment by segment (ln384_segments).  chained: the whole blocks are left to the caller's ln_rows_xres2 launch,
// which needs the rows behind them written first: only those run here.
static int ln384_gemm(const LnGemm &g, int T, bool chained, float *lnimg, hipStream_t st) {
    tsim_route_segment seg[TSIM_ROUTE_MAX_SEGS];
    const int n = ln384_segments(T, g.K, chained, seg);
    for (int i = 0; i < n; ++i) {
        const int r0 = seg[i].row0, rows = seg[i].rows;   // (r0 is a multiple of 32: a row block starts at the same element in both layouts)
        LnGemm s = g;
        s.X += (int64_t)r0 * g.K, s.res += (int64_t)r0 * 384, s.out += (int64_t)r0 * 384;
        int rc = TSIM_OK;
        switch (seg[i].form) {
            case TSIM_SEG_LN_ROWS_CHAINED: break;
            // (a four-slot ring with the second half of the waves issuing behind their MFMAs measured equal, 68.5 vs 66-68 us per launch)
            case TSIM_SEG_LN_ROWS: rc = ln_rows_gemm<8, 3>(s, rows, st); break;
            // (four 32-k ring slots instead of two 64-k ones — prefetch distance 3 — measured 2.5 % SLOWER per forward: the deep
            // path issues a k-tile's DMA pieces in one burst ahead of the MFMAs instead of behind each k-step's)
            case TSIM_SEG_BF16_128x384:
                rc = launch_gemm<128, 384, 64, 2, 4, EPI_RES_LN>(s.X, s.W, s.bias, s.res, s.gamma, s.beta, s.eps, s.out, rows, 384, s.K, st, s.Wk, s.lay);
                break;
            // 64 token rows (eight waves) per workgroup.  (A three-slot ring measured no different: 2.744-2.751 vs 2.751-2.752 ms per forward.)
            case TSIM_SEG_BF16_64x384:
                rc = launch_gemm<64, 384, 64, 2, 4, EPI_RES_LN>(s.X, s.W, s.bias, s.res, s.gamma, s.beta, s.eps, s.out, rows, 384, s.K, st, s.Wk, s.lay);
                break;
            default: rc = ln_tail_gemm(s, rows, seg[i].form, lnimg, st);
        }
        if (rc) return rc;
    }
    return TSIM_OK;
}

// =====================================================================================================
// The forward's stages: embedding, one layer function per family of the plan, pooling, classification head
// =====================================================================================================
template <int V>
using int_c = std::integral_constant<int, V>;

static int embed_rows(tsim_encoder *e, const int32_t *tok_ids, const int32_t *tok_type, const int32_t *tok_pos, const int32_t *tok_col,
                      int T, int max_len, hipStream_t st) {
    const tsim_encoder_config &c = e->cfg;
    // column of a token inside its sequence: tok_col when given (MPNet), else tok_pos (BERT: position == column)
    const int32_t *colp = tok_col ? tok_col : tok_pos;
    const int col_limit = tok_col || c.arch == TSIM_ARCH_BERT ? max_len : c.max_pos;   // MPNet / RoBERTa without tok_col: pos is not a column
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)((T + 3) / 4)), dim3(256), 0, st, tok_ids, tok_pos, e->word, e->pos, e->type0, e->emb_g, e->emb_b,
                           c.ln_eps, T, c.hidden, e->x0, c.vocab, c.max_pos, colp, col_limit, e->err_flags, tok_type, tok_type ? e->n_types : 0);
    };
    auto go = [&](auto v) { tok_type ? launch(embed_ln_kernel<decltype(v)::value, true>) : launch(embed_ln_kernel<decltype(v)::value, false>); };
    c.hidden == 64 ? go(int_c<1>{}) : c.hidden == 384 ? go(int_c<6>{}) : c.hidden == 768 ? go(int_c<12>{}) : go(int_c<16>{});   // values per lane
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

struct Forward {   // the layers of one call: what they share, and one function per family of the plan
    tsim_encoder *e;
    const int32_t *cu_seqlens, *col;   // col: MPNet's token columns (relative-position bias); null otherwise
    int T, B, H, F, chain;             // chain: chain_blocks of T
    float eps;
    dim3 agrid;                        // attention: (sequences, groups of four heads, blocks of 32 queries), xcd_map = 1
    hipStream_t st;
    using Layer = tsim_encoder::Layer;

    int attention() const {
        const int heads = e->cfg.heads, dh = H / heads;
        auto launch = [&](auto kern) {
            hipLaunchKernelGGL(kern, agrid, dim3(256), 0, st, e->qkv, cu_seqlens, col, e->relb, e->relw, H, heads, 1.0f / sqrtf((float)dh), e->ctx, B, 1);
        };
        auto go = [&](auto d) {
            constexpr int D = decltype(d)::value;
            if (e->cfg.arch == TSIM_ARCH_MPNET) launch(attention_kernel<D, true, false>);
            else if (e->plan.family == TSIM_FAMILY_H384_PACKED) launch(attention_kernel<D, false, true>);
            else launch(attention_kernel<D, false, false>);
        };
        dh == 16 ? go(int_c<16>{}) : dh == 32 ? go(int_c<32>{}) : go(int_c<64>{});
        TSIM_HIP_CHECK(hipGetLastError());
        return TSIM_OK;
    }

    int ffn1_rowmajor(const Layer &L) const {   // FFN1 of the families whose h1 is row-major
        switch (const int form = e->plan.form[TSIM_ROUTE_FFN1]) {
            case TSIM_FORM_XRES2: return gemm_xres2<EPI_GELU, false, false>(e->x1, L.w1, L.b1, e->h1, T, F, st);
            case TSIM_FORM_PP_256: case TSIM_FORM_PP_128: return gemm_pp(PP_EPI_GELU, e->x1, L.w1, 0, L.b1, e->h1, T, F, H, st);   // (the tile: gemm_pp_tile_width)
            case TSIM_FORM_BF16_128x128:
                return launch_gemm<128, 128, 64, 2, 2, EPI_GELU>(e->x1, L.w1, L.b1, nullptr, nullptr, nullptr, 0.f, e->h1, T, F, H, st, nullptr, ALL_ROW_MAJOR);
            case TSIM_FORM_BF16_128x64:
                return launch_gemm<128, 64, 64, 2, 2, EPI_GELU>(e->x1, L.w1, L.b1, nullptr, nullptr, nullptr, 0.f, e->h1, T, F, H, st, nullptr, ALL_ROW_MAJOR);
            default: return fail(TSIM_EINVAL, "encoder: FFN1 form %d is not a row-major one", form);
        }
    }

    // Projections on MXFP8 operands (v_mfma_scale_f32_32x32x64_f8f6f4); x0's image comes fused from the previous layer's LayerNorm
    // kernel, for layer 0 from the stand-alone quantiser
    int layer_mx(int l) const {
        const Layer &L = e->layers[l];
        int rc;
        if (l == 0 && (rc = quant_mx(e->x0, T, H, e->aq, e->as, st))) return rc;
        if ((rc = gemm_pp_mx(PP_EPI_BIAS, e->aq, e->as, L.qqkv, 1, L.sqkv, L.bqkv, e->qkv, nullptr, T, 3 * H, H, st))) return rc;
        if ((rc = attention()) || (rc = quant_mx(e->ctx, T, H, e->aq, e->as, st))) return rc;
        if ((rc = gemm_pp_mx(PP_EPI_F32, e->aq, e->as, L.qo, 1, L.so, L.bo, e->ybuf, nullptr, T, H, H, st))) return rc;
        if ((rc = res_ln_rows(e->ybuf, e->x0, L.g1, L.be1, eps, e->x1, e->aq, e->as, T, H, st))) return rc;
        if ((rc = gemm_pp_mx(PP_EPI_GELU_MX, e->aq, e->as, L.q1, 1, L.s1, L.b1, e->hq, e->hs, T, F, H, st))) return rc;
        if ((rc = gemm_pp_mx(PP_EPI_F32, e->hq, e->hs, L.q2, 1, L.s2, L.b2, e->ybuf, nullptr, T, H, F, st))) return rc;
        return res_ln_rows(e->ybuf, e->x1, L.g2, L.be2, eps, e->x0, e->aq, e->as, T, H, st);
    }

    // Hidden 768 / 1024 in bf16.  Wide rows: a workgroup cannot own whole 768-feature rows at a 256-token tile, so the O and FFN2
    // projections write fp32 sums and a row kernel adds the residual and normalises (HBM-bound, 8 B per element)
    int layer_pp(int l) const {
        const Layer &L = e->layers[l];
        const bool pq = e->plan.form[TSIM_ROUTE_QKV] == TSIM_FORM_PP_256_PACKED_W, po = e->plan.form[TSIM_ROUTE_O] == TSIM_FORM_PP_RES_LN_PACKED_W;
        int rc;
        if ((rc = gemm_pp(PP_EPI_BIAS, e->x0, pq ? L.pqkv : L.wqkv, pq, L.bqkv, e->qkv, T, 3 * H, H, st)) || (rc = attention())) return rc;
        if ((rc = gemm_pp(PP_EPI_F32, e->ctx, po ? L.po : L.wo, po, L.bo, e->ybuf, T, H, H, st))) return rc;
        if ((rc = res_ln_rows(e->ybuf, e->x0, L.g1, L.be1, eps, e->x1, nullptr, nullptr, T, H, st)) || (rc = ffn1_rowmajor(L))) return rc;
        if ((rc = gemm_pp(PP_EPI_F32, e->h1, L.w2, 0, L.b2, e->ybuf, T, H, F, st))) return rc;
        return res_ln_rows(e->ybuf, e->x1, L.g2, L.be2, eps, e->x0, nullptr, nullptr, T, H, st);
    }

    // Hidden 384, both families.  chain > 0 (packed family only): the O-projection's launch runs FFN1 too, and FFN2's the next
    // layer's QKV; the rows behind the whole blocks go first (their LayerNorm launches as ever), the projection's items of those
    // rows are shared out.
    int layer_384(int l) const {
        const Layer &L = e->layers[l];
        const bool pk = e->plan.family == TSIM_FAMILY_H384_PACKED, last = l + 1 == e->cfg.num_layers, chain_qkv = chain > 0 && !last;
        // The residual stream is block-packed between the layers of the packed family (group_off): x1 always, x0 except as the
        // embedding kernel leaves it (layer 0 reads it row-major) and as the last layer leaves it (pooling, heads and the
        // last_hidden copy read it row-major).
        const Layout packed = pk ? BLOCK_PACKED : ROW_MAJOR, x0_in = pk && l > 0 ? BLOCK_PACKED : ROW_MAJOR, x0_out = pk && !last ? BLOCK_PACKED : ROW_MAJOR;
        int rc;
        if (chain > 0 && l > 0) rc = TSIM_OK;   // the previous layer's FFN2 launch has written this layer's qkv
        else if (!pk) rc = gemm_xres2<EPI_BIAS, false, false>(e->x0, L.wqkv, L.bqkv, e->qkv, T, 3 * H, st);
        else if (x0_in == BLOCK_PACKED) rc = gemm_xres2<EPI_BIAS, true, true>(e->x0, L.wqkv, L.bqkv, e->qkv, T, 3 * H, st);
        else rc = gemm_xres2<EPI_BIAS, true, false>(e->x0, L.wqkv, L.bqkv, e->qkv, T, 3 * H, st);
        if (rc || (rc = attention())) return rc;
        const LnGemm o = {e->ctx, L.wo, L.lo, L.lo32, L.bo, e->x0, L.g1, L.be1, eps, e->x1, H, {ROW_MAJOR, x0_in, packed}};
        if ((rc = ln384_gemm(o, T, chain > 0, e->lnimg, st))) return rc;
        if (chain > 0) rc = ln_rows_xres2<EPI_GELU>(o, chain, L.w1, L.b1, e->h1, T, F, st);
        else rc = pk ? gemm_xres2<EPI_GELU, true, true>(e->x1, L.w1, L.b1, e->h1, T, F, st) : ffn1_rowmajor(L);
        if (rc) return rc;
        const LnGemm f2 = {e->h1, L.w2, L.l2, L.l232, L.b2, e->x1, L.g2, L.be2, eps, e->x0, F, {packed, packed, x0_out}};
        if ((rc = ln384_gemm(f2, T, chain_qkv, e->lnimg, st)) || !chain_qkv) return rc;
        return ln_rows_xres2<EPI_BIAS>(f2, chain, e->layers[l + 1].wqkv, e->layers[l + 1].bqkv, e->qkv, T, 3 * H, st);
    }

    int layer_h64(int l) const {   // hidden 64: gemm_bf16's 128-token tiles throughout
        const Layer &L = e->layers[l];
        int rc;
        if ((rc = launch_gemm<128, 64, 64, 2, 2, EPI_BIAS>(e->x0, L.wqkv, L.bqkv, nullptr, nullptr, nullptr, 0.f, e->qkv, T, 3 * H, H, st, nullptr, ALL_ROW_MAJOR))) return rc;
        if ((rc = attention()) || (rc = launch_gemm<128, 64, 64, 4, 2, EPI_RES_LN>(e->ctx, L.wo, L.bo, e->x0, L.g1, L.be1, eps, e->x1, T, H, H, st, nullptr, ALL_ROW_MAJOR))) return rc;
        if ((rc = ffn1_rowmajor(L))) return rc;
        return launch_gemm<128, 64, 64, 4, 2, EPI_RES_LN>(e->h1, L.w2, L.b2, e->x1, L.g2, L.be2, eps, e->x0, T, H, F, st, nullptr, ALL_ROW_MAJOR);
    }
};

// pool_packed_kernel<NP, MODE, NORM> over the final hidden state (x0): NP by the width, MODE = TSIM_POOL_*, NORM = Normalize fused
static int pool_rows(const tsim_encoder *e, const int32_t *cu_seqlens, int B, int mode, bool norm, float *px, unit_t *pu, int ld_unit,
                     float *unit_rho_max, hipStream_t st) {
    const int H = e->cfg.hidden;
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)((B + 3) / 4)), dim3(256), 0, st, e->x0, cu_seqlens, B, H, px, pu, ld_unit, pu ? unit_rho_max : nullptr);
    };
    auto by_width = [&](auto m, auto n) {
        H <= 512 ? launch(pool_packed_kernel<1, decltype(m)::value, decltype(n)::value>) : launch(pool_packed_kernel<2, decltype(m)::value, decltype(n)::value>);
    };
    auto by_mode = [&](auto n) {
        mode == TSIM_POOL_MEAN ? by_width(int_c<TSIM_POOL_MEAN>{}, n) : mode == TSIM_POOL_CLS ? by_width(int_c<TSIM_POOL_CLS>{}, n)
        : mode == TSIM_POOL_MAX ? by_width(int_c<TSIM_POOL_MAX>{}, n) : by_width(int_c<TSIM_POOL_MEAN_SQRT_LEN>{}, n);
    };
    norm ? by_mode(std::true_type{}) : by_mode(std::false_type{});
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

// Sequence-classification logits from the CLS rows of the final hidden state (x0); sequences without tokens read zeros
static int cls_head(const tsim_encoder *e, const int32_t *cu_seqlens, int B, float *logits_f32, hipStream_t st) {
    const int H = e->cfg.hidden;
    auto launch = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3((unsigned)((B + CLS_ROWS - 1) / CLS_ROWS)), dim3((unsigned)H), 0, st, e->x0, cu_seqlens, B, H, e->head_wpT,
                           e->head_bp, e->head_wc, e->head_bc, e->n_labels, logits_f32);
    };
    if (e->head_act == TSIM_ACT_RELU) H <= CLS_MAX_H ? launch(cls_head_wide_kernel<CLS_MAX_H, TSIM_ACT_RELU>) : launch(cls_head_wide_kernel<CLS_WIDE_H, TSIM_ACT_RELU>);
    else H <= CLS_MAX_H ? launch(cls_head_kernel) : launch(cls_head_wide_kernel<CLS_WIDE_H, TSIM_ACT_TANH>);
    TSIM_HIP_CHECK(hipGetLastError());
    return TSIM_OK;
}

}  // namespace tsim

// Introspection (host only, no launch): the items workgroup b of G takes in a chained launch (chain_part / chain_item as
// ln_rows_xres2_kernel evaluates them), as block * ntiles + feature tile.  Returns the count (< 0: bad arguments); fills at most cap.
extern "C" int tsim_chain_items_host(int blocks, int rem_blocks, int ntiles, int G, int b, int32_t *items, int cap) {
    if (blocks != G || rem_blocks < 0 || ntiles <= 0 || G <= 0 || b < 0 || b >= G || (cap > 0 && !items)) return -1;
    const ChainPart p = chain_part(G, rem_blocks, ntiles, b);
    for (int i = 0; i < p.n && i < cap; ++i) items[i] = chain_item(p, G, ntiles, b, i);
    return p.n;
}

extern "C" int tsim_encoder_route_host(const tsim_encoder_config *cfg, int32_t T, int32_t layer, tsim_encoder_route *out) {
    TSIM_REQUIRE(cfg && out, "encoder_route_host: null pointer");
    TSIM_REQUIRE(T >= 0 && layer >= 0 && layer < cfg->num_layers, "encoder_route_host: T=%d layer=%d of %d", T, layer, cfg->num_layers);
    if (int rc = encoder_plan(*cfg, out)) return rc;
    out->chain_blocks = chain_blocks(*out, cfg->ffn, T);
    out->qkv_chained = out->chain_blocks > 0 && layer > 0;
    if (out->form[TSIM_ROUTE_O] == TSIM_FORM_LN384) {   // (as layer_384 asks for them)
        out->n_seg[0] = ln384_segments(T, cfg->hidden, out->chain_blocks > 0, out->seg[0]);
        out->n_seg[1] = ln384_segments(T, cfg->ffn, out->chain_blocks > 0 && layer + 1 < cfg->num_layers, out->seg[1]);
    }
    return TSIM_OK;
}

extern "C" int tsim_encoder_create(const tsim_encoder_config *cfg, const tsim_encoder_weights_host *w,
                                   tsim_encoder **out) {
    TSIM_REQUIRE(cfg && w && out, "encoder_create: null pointer");
    EncoderPlan plan;
    if (int rc = encoder_plan(*cfg, &plan)) return rc;
    const int H = cfg->hidden, F = cfg->ffn, L = cfg->num_layers;
    TSIM_REQUIRE(w->word_emb && w->pos_emb && w->emb_ln_g && w->emb_ln_b && w->layers, "encoder_create: missing weights");
    TSIM_REQUIRE(cfg->arch != TSIM_ARCH_MPNET || w->rel_bias, "encoder_create: MPNet needs rel_bias");
    const bool mx = plan.images & TSIM_IMG_MXFP8;
    tsim_encoder *e = new tsim_encoder();
    e->cfg = *cfg;
    e->plan = plan;
    e->Tp = (cfg->max_tokens + 127) / 128 * 128 + 128;
    int rc = TSIM_OK;
    auto bail = [&](int code) {
        tsim_encoder_destroy(e);
        return code;
    };
    if ((rc = upload_f32(e, w->word_emb, (size_t)cfg->vocab * H, &e->word))) return bail(rc);
    if ((rc = upload_f32(e, w->pos_emb, (size_t)cfg->max_pos * H, &e->pos))) return bail(rc);
    if (w->type_emb && (rc = upload_f32(e, w->type_emb, H, &e->type0))) return bail(rc);
    if ((rc = upload_f32(e, w->emb_ln_g, H, &e->emb_g))) return bail(rc);
    if ((rc = upload_f32(e, w->emb_ln_b, H, &e->emb_b))) return bail(rc);
    if (cfg->arch == TSIM_ARCH_MPNET) {
        const int maxp = cfg->max_pos;
        e->relw = 2 * maxp - 1;
        std::vector<float> tab((size_t)cfg->heads * e->relw);
        for (int d = -(maxp - 1); d <= maxp - 1; ++d) {
            const int bk = mpnet_bucket(d, cfg->rel_buckets);
            for (int hh = 0; hh < cfg->heads; ++hh) tab[(size_t)hh * e->relw + d + maxp - 1] = w->rel_bias[bk * cfg->heads + hh];
        }
        if ((rc = upload_f32(e, tab.data(), tab.size(), &e->relb))) return bail(rc);
    }
    e->layers.resize(L);
    for (int l = 0; l < L; ++l) {
        const tsim_layer_weights_host &lw = w->layers[l];
        tsim_encoder::Layer &d = e->layers[l];
        if ((rc = upload_bf16(e, {lw.wq, lw.wk, lw.wv}, (size_t)H * H, &d.wqkv))) return bail(rc);
        if ((rc = upload_bf16(e, {lw.wo}, (size_t)H * H, &d.wo))) return bail(rc);
        if ((rc = upload_bf16(e, {lw.w1}, (size_t)F * H, &d.w1))) return bail(rc);
        if ((rc = upload_bf16(e, {lw.w2}, (size_t)H * F, &d.w2))) return bail(rc);
        if (mx) {
            if ((rc = upload_mxfp8(e, {lw.wq, lw.wk, lw.wv}, H, H, &d.qqkv, &d.sqkv))) return bail(rc);
            if ((rc = upload_mxfp8(e, {lw.wo}, H, H, &d.qo, &d.so))) return bail(rc);
            if ((rc = upload_mxfp8(e, {lw.w1}, F, H, &d.q1, &d.s1))) return bail(rc);
            if ((rc = upload_mxfp8(e, {lw.w2}, H, F, &d.q2, &d.s2))) return bail(rc);
        }
        // tile-major copies for the ping-pong projections (contiguous 1-KiB DMA pieces): [feature tile][k-tile][LDS image]
        auto repack = [&](const void *src, int n_rows, int kbytes, void **dst) {
            int r2 = dev_alloc(e, (size_t)n_rows * kbytes, dst);
            return r2 ? r2 : pack_w(src, *dst, n_rows, kbytes, gemm_pp_tile_width(n_rows), nullptr);
        };
        if (mx) {
            void *t;
            if ((rc = repack(d.qqkv, 3 * H, H, &t))) return bail(rc); d.qqkv = (uint8_t *)t;
            if ((rc = repack(d.qo, H, H, &t))) return bail(rc); d.qo = (uint8_t *)t;
            if ((rc = repack(d.q1, F, H, &t))) return bail(rc); d.q1 = (uint8_t *)t;
            if ((rc = repack(d.q2, H, F, &t))) return bail(rc); d.q2 = (uint8_t *)t;
        } else if (plan.images & TSIM_IMG_PP_QKV_O) {
            if ((rc = repack(d.wqkv, 3 * H, H * 2, (void **)&d.pqkv))) return bail(rc);
            if ((rc = repack(d.wo, H, H * 2, (void **)&d.po))) return bail(rc);
        }
        // hidden-384 LayerNorm GEMM: the O and FFN2 matrices [H, K] as contiguous k-tile LDS images (BN = 384, BK = 64) ...
        auto image = [&](auto kern, const bf16_t *src, int K, bf16_t **dst, auto... tile) {
            const int r2 = dev_alloc(e, (size_t)H * K * 2, (void **)dst);
            if (!r2) hipLaunchKernelGGL(kern, dim3((unsigned)((H * K / 8 + 255) / 256)), dim3(256), 0, 0, reinterpret_cast<const uint4 *>(src),
                                        reinterpret_cast<uint4 *>(*dst), tile..., K);
            return r2;
        };
        if ((plan.images & TSIM_IMG_LN_KTILE) && ((rc = image(pack_gemm_w_kernel, d.wo, H, &d.lo, 384, 64)) || (rc = image(pack_gemm_w_kernel, d.w2, F, &d.l2, 384, 64))))
            return bail(rc);
        if ((plan.images & TSIM_IMG_LN_FRAG) && ((rc = image(pack_frag_w_kernel, d.wo, H, &d.lo32, 384)) || (rc = image(pack_frag_w_kernel, d.w2, F, &d.l232, 384))))
            return bail(rc);   // ... and as MFMA fragment images
        if (hipGetLastError() != hipSuccess) return bail(fail(TSIM_EHIP, "LayerNorm GEMM weight packing failed"));
        std::vector<float> bq(3 * (size_t)H);
        memcpy(bq.data(), lw.bq, H * 4);
        memcpy(bq.data() + H, lw.bk, H * 4);
        memcpy(bq.data() + 2 * H, lw.bv, H * 4);
        if ((rc = upload_f32(e, bq.data(), bq.size(), &d.bqkv))) return bail(rc);
        if ((rc = upload_f32(e, lw.bo, H, &d.bo))) return bail(rc);
        if ((rc = upload_f32(e, lw.b1, F, &d.b1))) return bail(rc);
        if ((rc = upload_f32(e, lw.b2, H, &d.b2))) return bail(rc);
        if ((rc = upload_f32(e, lw.ln1_g, H, &d.g1))) return bail(rc);
        if ((rc = upload_f32(e, lw.ln1_b, H, &d.be1))) return bail(rc);
        if ((rc = upload_f32(e, lw.ln2_g, H, &d.g2))) return bail(rc);
        if ((rc = upload_f32(e, lw.ln2_b, H, &d.be2))) return bail(rc);
    }
    const size_t Tp = e->Tp;
    struct { bf16_t **p; size_t n; } acts[] = {{&e->x0, Tp * H}, {&e->x1, Tp * H}, {&e->qkv, Tp * 3 * H},
                                               {&e->ctx, Tp * H}, {&e->h1, Tp * F}};
    for (auto &a : acts) {
        if ((rc = dev_alloc(e, a.n * 2, (void **)a.p))) return bail(rc);
        if (hipMemset(*a.p, 0, a.n * 2) != hipSuccess) return bail(fail(TSIM_EHIP, "hipMemset failed"));
    }
    if (plan.buffers & TSIM_BUF_YBUF) {
        if ((rc = dev_alloc(e, Tp * H * 4, (void **)&e->ybuf))) return bail(rc);
        if (hipMemset(e->ybuf, 0, Tp * H * 4) != hipSuccess) return bail(fail(TSIM_EHIP, "hipMemset failed"));
    }
    if (plan.buffers & TSIM_BUF_LNIMG) {   // ln_split's accumulator images: every row block a forward can hand to ln_tail_gemm
        const size_t blocks = (Tp + 31) / 32 < (size_t)LS_MAX_BLOCKS ? (Tp + 31) / 32 : (size_t)LS_MAX_BLOCKS;   // (a forward has T <= max_tokens < Tp rows)
        const size_t bytes = blocks * 4 * 12 * 64 * 16;
        if ((rc = dev_alloc(e, bytes, (void **)&e->lnimg))) return bail(rc);
        if (hipMemset(e->lnimg, 0, bytes) != hipSuccess) return bail(fail(TSIM_EHIP, "hipMemset failed"));
    }
    if ((size_t)cfg->max_seqs * H * 4 > Tp * 3 * H * 2 && (rc = dev_alloc(e, (size_t)cfg->max_seqs * H * 4, (void **)&e->head_x)))
        return bail(rc);
    if (plan.buffers & TSIM_BUF_MX_ACT) {
        struct { uint8_t **p; size_t n; } qb[] = {{&e->aq, Tp * H}, {&e->as, Tp * H / 32}, {&e->hq, Tp * F}, {&e->hs, Tp * F / 32}};
        for (auto &a : qb) {
            if ((rc = dev_alloc(e, a.n, (void **)a.p))) return bail(rc);
            if (hipMemset(*a.p, 0, a.n) != hipSuccess) return bail(fail(TSIM_EHIP, "hipMemset failed"));
        }
    }
    if ((rc = dev_alloc(e, 256, (void **)&e->err_flags))) return bail(rc);
    if (hipMemset(e->err_flags, 0, 256) != hipSuccess) return bail(fail(TSIM_EHIP, "hipMemset failed"));
    if (hipDeviceSynchronize() != hipSuccess) return bail(fail(TSIM_EHIP, "sync after upload failed"));
    *out = e;
    return TSIM_OK;
}

extern "C" int tsim_encoder_error_flags(tsim_encoder *e, int32_t *flags_host, void *stream) {
    TSIM_REQUIRE(e && flags_host, "encoder_error_flags: null pointer");
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    TSIM_HIP_CHECK(hipMemcpyAsync(flags_host, e->err_flags, 4, hipMemcpyDeviceToHost, st));
    TSIM_HIP_CHECK(hipMemsetAsync(e->err_flags, 0, 4, st));
    TSIM_HIP_CHECK(hipStreamSynchronize(st));
    return TSIM_OK;
}

extern "C" int tsim_quantize_mxfp8(const void *x_bf16, int64_t rows, int K, void *q_out, void *scale_out, void *stream) {
    TSIM_REQUIRE(x_bf16 && q_out && scale_out, "quantize_mxfp8: null pointer");
    TSIM_REQUIRE(rows >= 0 && K > 0, "quantize_mxfp8: bad shape rows=%lld K=%d", (long long)rows, K);
    return quant_mx(static_cast<const bf16_t *>(x_bf16), rows, K, static_cast<uint8_t *>(q_out),
                    static_cast<uint8_t *>(scale_out), reinterpret_cast<hipStream_t>(stream));
}

extern "C" int tsim_gemm_mxfp8(const void *xq, const void *xs, const void *wq, const void *ws, const float *bias,
                               float *out_f32, int M, int N, int K, void *stream) {
    TSIM_REQUIRE(xq && xs && wq && ws && bias && out_f32, "gemm_mxfp8: null pointer");
    TSIM_REQUIRE(M >= 0 && N > 0 && K > 0, "gemm_mxfp8: bad shape M=%d N=%d K=%d", M, N, K);
    return gemm_pp_mx(PP_EPI_F32, static_cast<const uint8_t *>(xq), static_cast<const uint8_t *>(xs),
                      static_cast<const uint8_t *>(wq), 0, static_cast<const uint8_t *>(ws), bias, out_f32, nullptr, M, N, K,
                      reinterpret_cast<hipStream_t>(stream));
}

#ifdef TSIM_PP_STAMPS
extern "C" int tsim_debug_xr_stamps(unsigned long long *out16, int reset) {
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(tsim::g_xr_stamps), 128) != hipSuccess) return 1;
    if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(tsim::g_xr_stamps), z, 128) != hipSuccess) return 1; }
    return 0;
}
#endif

extern "C" void tsim_encoder_destroy(tsim_encoder *e) {
    if (!e) return;
    for (void *p : e->allocs) (void)hipFree(p);
    delete e;
}

extern "C" int tsim_encoder_set_token_types(tsim_encoder *e, const float *type_emb_host, int32_t n_types) {
    TSIM_REQUIRE(e && type_emb_host, "encoder_set_token_types: null pointer");
    TSIM_REQUIRE(e->cfg.arch != TSIM_ARCH_MPNET, "encoder_set_token_types: BERT only (MPNet has no token-type table)");
    TSIM_REQUIRE(n_types >= 1, "encoder_set_token_types: n_types=%d < 1", n_types);
    float *tab = nullptr;
    if (int rc = upload_f32(e, type_emb_host, (size_t)n_types * e->cfg.hidden, &tab)) return rc;
    e->type0 = tab;   // row 0 serves the untyped calls from now on (the previous one-row copy stays allocated until destroy)
    e->n_types = n_types;
    return TSIM_OK;
}

extern "C" int tsim_encoder_set_cls_head(tsim_encoder *e, const float *pool_w_host, const float *pool_b_host,
                                         const float *cls_w_host, const float *cls_b_host, int32_t num_labels) {
    return tsim_encoder_set_cls_head_act(e, pool_w_host, pool_b_host, cls_w_host, cls_b_host, num_labels, TSIM_ACT_TANH);
}

extern "C" int tsim_encoder_set_cls_head_act(tsim_encoder *e, const float *pool_w_host, const float *pool_b_host,
                                             const float *cls_w_host, const float *cls_b_host, int32_t num_labels, int32_t act) {
    TSIM_REQUIRE(e && pool_w_host && pool_b_host && cls_w_host && cls_b_host, "encoder_set_cls_head: null pointer");
    TSIM_REQUIRE(e->cfg.arch != TSIM_ARCH_MPNET, "encoder_set_cls_head: BERT only");
    TSIM_REQUIRE(act == TSIM_ACT_TANH || act == TSIM_ACT_RELU, "encoder_set_cls_head: activation %d (TSIM_ACT_TANH, TSIM_ACT_RELU)", act);
    TSIM_REQUIRE(num_labels >= 1 && num_labels <= CLS_MAX_LABELS, "encoder_set_cls_head: num_labels=%d outside [1, %d]", num_labels,
                 CLS_MAX_LABELS);
    const int H = e->cfg.hidden;
    TSIM_REQUIRE(H % 64 == 0 && H <= CLS_WIDE_H, "encoder_set_cls_head: hidden=%d unsupported", H);
    std::vector<float> wT((size_t)H * H);
    for (int o = 0; o < H; ++o)
        for (int k = 0; k < H; ++k) wT[(size_t)k * H + o] = pool_w_host[(size_t)o * H + k];
    int rc;
    if ((rc = upload_f32(e, wT.data(), wT.size(), &e->head_wpT))) return rc;
    if ((rc = upload_f32(e, pool_b_host, H, &e->head_bp))) return rc;
    if ((rc = upload_f32(e, cls_w_host, (size_t)num_labels * H, &e->head_wc))) return rc;
    if ((rc = upload_f32(e, cls_b_host, num_labels, &e->head_bc))) return rc;
    e->n_labels = num_labels;
    e->head_act = act;
    return TSIM_OK;
}

extern "C" int tsim_encoder_forward(tsim_encoder *e, const int32_t *tok_ids, const int32_t *tok_pos,
                                    const int32_t *tok_col, const int32_t *cu_seqlens, int32_t T, int32_t B,
                                    int32_t max_len, float *pooled_f32, void *unit_bf16, int ld_unit, float *unit_rho_max,
                                    void *last_hidden_bf16, void *stream) {
    return tsim_encoder_forward_ex(e, tok_ids, nullptr, tok_pos, tok_col, cu_seqlens, T, B, max_len, pooled_f32, unit_bf16, ld_unit,
                                   unit_rho_max, last_hidden_bf16, nullptr, stream);
}

extern "C" int tsim_encoder_forward_ex(tsim_encoder *e, const int32_t *tok_ids, const int32_t *tok_type, const int32_t *tok_pos,
                                       const int32_t *tok_col, const int32_t *cu_seqlens, int32_t T, int32_t B,
                                       int32_t max_len, float *pooled_f32, void *unit_bf16, int ld_unit, float *unit_rho_max,
                                       void *last_hidden_bf16, float *logits_f32, void *stream) {
    TSIM_REQUIRE(e && cu_seqlens && (T == 0 || (tok_ids && tok_pos)), "encoder_forward: null pointer");   // T = 0: only empty sequences
    TSIM_REQUIRE(!tok_type || e->n_types > 0, "encoder_forward: tok_type given but no token-type table was set "
                 "(tsim_encoder_set_token_types)");
    TSIM_REQUIRE(!logits_f32 || e->n_labels > 0, "encoder_forward: logits requested but no classification head was set "
                 "(tsim_encoder_set_cls_head)");
    TSIM_REQUIRE(T >= 0 && B >= 0 && T <= e->cfg.max_tokens && B <= e->cfg.max_seqs,
                 "encoder_forward: T=%d B=%d exceed capacity (%d tokens, %d sequences)", T, B, e->cfg.max_tokens, e->cfg.max_seqs);
    // position rows: BERT uses 0 .. len-1, MPNet and RoBERTa pad_id+1 .. pad_id+len (create_position_ids_from_input_ids)
    const int pos_span = max_len + (e->cfg.arch != TSIM_ARCH_BERT ? e->cfg.pad_id + 1 : 0);
    TSIM_REQUIRE(max_len >= 0 && pos_span <= e->cfg.max_pos,
                 "encoder_forward: sequences of %d tokens need position rows up to %d, the table has %d", max_len, pos_span - 1,
                 e->cfg.max_pos);
    TSIM_REQUIRE(!unit_bf16 || ld_unit >= e->cfg.hidden, "encoder_forward: ld_unit < hidden");
    TSIM_REQUIRE(!unit_bf16 || e->cfg.hidden <= 768, "encoder_forward: unit rows need a width <= 768 (got %d)", e->cfg.hidden);
    if (B == 0) return TSIM_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const tsim_encoder_config &c = e->cfg;
    const int H = c.hidden;
    int rc;
    if (T > 0) {
        if ((rc = embed_rows(e, tok_ids, tok_type, tok_pos, tok_col, T, max_len, st))) return rc;
        const int qblocks = (max_len + 31) / 32 > 0 ? (max_len + 31) / 32 : 1;
        const Forward f = {e, cu_seqlens, c.arch == TSIM_ARCH_MPNET ? (tok_col ? tok_col : tok_pos) : nullptr, T, B, H, c.ffn, chain_blocks(e->plan, c.ffn, T),
                           c.ln_eps, dim3((unsigned)(((B + 7) / 8) * 8), (unsigned)((c.heads + 3) / 4), (unsigned)qblocks), st};
        for (int l = 0; l < c.num_layers; ++l) {
            switch (e->plan.family) {
                case TSIM_FAMILY_PP_MX: rc = f.layer_mx(l); break;
                case TSIM_FAMILY_PP: rc = f.layer_pp(l); break;
                case TSIM_FAMILY_H64: rc = f.layer_h64(l); break;
                default: rc = f.layer_384(l);
            }
            if (rc) return rc;
        }
        if (last_hidden_bf16)
            TSIM_HIP_CHECK(hipMemcpyAsync(last_hidden_bf16, e->x0, (size_t)T * H * 2, hipMemcpyDeviceToDevice, st));
    }
    if (pooled_f32 || unit_bf16) {
        if (H % 8 != 0 || H > 1024 || (unit_bf16 && ld_unit % 8 != 0))
            return fail(TSIM_EUNSUPPORTED, "encoder: pooling needs a hidden size that is a multiple of 8, at most 1024 (got %d)", H);
        if (((uintptr_t)pooled_f32 | (uintptr_t)unit_bf16) & 15)
            return fail(TSIM_EINVAL, "encoder: pooled / unit outputs must be 16-byte aligned");
        if ((rc = pool_rows(e, cu_seqlens, B, TSIM_POOL_MEAN, false, pooled_f32, (unit_t *)unit_bf16, ld_unit, unit_rho_max, st))) return rc;
    }
    if (logits_f32) return cls_head(e, cu_seqlens, B, logits_f32, st);
    return TSIM_OK;
}

// Sentence-embedding head: CLS / max / mean / mean-sqrt-len pooling, Dense, Normalize
// (/root/reference/src/modules/modules.py:154-195 and the sentence-transformers modules.json chain; include/tsim.h)
extern "C" int tsim_encoder_forward_head(tsim_encoder *e, const int32_t *tok_ids, const int32_t *tok_type, const int32_t *tok_pos,
                                         const int32_t *tok_col, const int32_t *cu_seqlens, int32_t T, int32_t B, int32_t max_len,
                                         const tsim_sentence_head *head, float *emb_f32, void *unit_f16, int ld_unit,
                                         float *unit_rho_max, void *last_hidden_bf16, void *stream) {
    if (!head)
        return tsim_encoder_forward_ex(e, tok_ids, tok_type, tok_pos, tok_col, cu_seqlens, T, B, max_len, emb_f32, unit_f16, ld_unit,
                                       unit_rho_max, last_hidden_bf16, nullptr, stream);
    TSIM_REQUIRE(e, "encoder_forward_head: null encoder");
    const int H = e->cfg.hidden, mode = head->pool_mode, d_out = head->d_out;
    TSIM_REQUIRE(mode >= TSIM_POOL_MEAN && mode <= TSIM_POOL_MEAN_SQRT_LEN, "encoder_forward_head: unknown pool_mode %d", mode);
    TSIM_REQUIRE(head->normalize == 0 || head->normalize == 1, "encoder_forward_head: normalize=%d is not 0 / 1", head->normalize);
    TSIM_REQUIRE(d_out >= 0, "encoder_forward_head: d_out=%d < 0", d_out);
    if (d_out) {
        TSIM_REQUIRE(head->dense_w, "encoder_forward_head: d_out=%d without dense_w", d_out);
        if (int rc = dense_check(H, d_out, head->dense_act, head->dense_w)) return rc;
    } else {
        TSIM_REQUIRE(!head->dense_w && !head->dense_b, "encoder_forward_head: dense weights given with d_out = 0");
    }
    const int width = d_out ? d_out : H;
    TSIM_REQUIRE(!unit_f16 || width <= 768, "encoder_forward_head: unit rows need a final width <= 768 (got %d)", width);
    TSIM_REQUIRE(!unit_f16 || (ld_unit >= width && ld_unit % 8 == 0), "encoder_forward_head: ld_unit=%d (final width %d)", ld_unit,
                 width);
    TSIM_REQUIRE(H % 8 == 0 && H <= 1024, "encoder_forward_head: pooling needs hidden %% 8 == 0 and <= 1024 (got %d)", H);
    TSIM_REQUIRE((((uintptr_t)emb_f32 | (uintptr_t)unit_f16) & 15) == 0, "encoder_forward_head: outputs must be 16-byte aligned");
    // the layers (validates the rest; writes neither pooled nor unit rows)
    if (int rc = tsim_encoder_forward_ex(e, tok_ids, tok_type, tok_pos, tok_col, cu_seqlens, T, B, max_len, nullptr, nullptr, 0,
                                         nullptr, last_hidden_bf16, nullptr, stream))
        return rc;
    if (B == 0 || (!emb_f32 && !unit_f16)) return TSIM_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    // without a Dense the pooling kernel writes the final rows (Normalize and unit rows fused); with one it writes the pre-Dense
    // rows into scratch: qkv (dead after the last layer, [Tp, 3H] bf16 = 1.5 Tp rows of H floats) or head_x
    float *px = d_out ? (e->head_x ? e->head_x : reinterpret_cast<float *>(e->qkv)) : emb_f32;
    unit_t *pu = d_out ? nullptr : static_cast<unit_t *>(unit_f16);
    const bool norm = !d_out && head->normalize;
    if (int rc = pool_rows(e, cu_seqlens, B, mode, norm, px, pu, ld_unit, unit_rho_max, st)) return rc;
    if (d_out)
        return dense_rows_launch(px, B, H, head->dense_w, head->dense_b, d_out, head->dense_act, head->normalize, emb_f32,
                                 static_cast<unit_t *>(unit_f16), ld_unit, unit_f16 ? unit_rho_max : nullptr, st);
    return TSIM_OK;
}

// sentence-transformers Dense / Normalize (and BertPoolingStrategy's tanh(Linear(.)), modules.py:184-195) on float32 rows
extern "C" int tsim_dense_rows(const float *x, int64_t B, int d_in, const float *w, const float *b, int d_out, int act, int normalize,
                               float *out, void *stream) {
    TSIM_REQUIRE(x && out, "dense_rows: null pointer");
    TSIM_REQUIRE(B >= 0 && B <= INT32_MAX - DN_ROWS, "dense_rows: bad row count %lld", (long long)B);
    TSIM_REQUIRE(normalize == 0 || normalize == 1, "dense_rows: normalize=%d is not 0 / 1", normalize);
    if (int rc = dense_check(d_in, d_out, act, w)) return rc;
    TSIM_REQUIRE((((uintptr_t)x | (uintptr_t)out) & 15) == 0, "dense_rows: x and out must be 16-byte aligned");
    return dense_rows_launch(x, (int)B, d_in, w, b, d_out, act, normalize, out, nullptr, 0, nullptr, reinterpret_cast<hipStream_t>(stream));
}

#include "span_pool.h"   // word-in-context embeddings: span_pool_kernel and tsim_encoder_forward_spans, behind the forward above
