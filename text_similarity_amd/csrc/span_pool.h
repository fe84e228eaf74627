// Word-in-context embeddings (tsim_encoder_forward_spans): the mean of the final hidden states over a LIST of token
// positions, one list ("span") per target word.  Included by encoder.hip behind the forward it reuses unchanged.
//
// The reference does this on the host, per word: `torch.mean(embedded_1[i][w1_c1], dim=0)`
// (/root/reference/src/models/word_encoder.py:85-92, GWSCModel; /root/reference/src/modules/modules.py:68-74,
// WordPoolingStrategy), with the positions that /root/reference/src/dataset/dataset.py:461-480 (find_tokens_positions) aligned
// to WordPiece tokens.
//
// span_pool_kernel: one wave per span, four spans per workgroup, no LDS.  A lane owns 16-byte pieces of the row (features
// 8c .. 8c+7 for c = lane, lane + 64: the lane layout of pool_packed_kernel), so one listed token costs one 16-byte load per
// lane and piece; eight tokens' loads are issued together, the adds stay in list order.  The arithmetic is fixed so that a host
// replay is bit-exact: bf16 -> float32 (exact), float32 adds in list order starting from +0 (a slot past the end of the list
// adds +0, which cannot change a sum that started from +0: such a sum is never -0), ONE float32 division by the count.  A list
// may repeat a position (it counts as often as it is listed), skip positions, or be longer than a wave; an empty list gives a
// zero row (torch.mean of nothing is NaN).
// Nothing faults on a bad table: a sequence index outside [0, B), a position outside [0, len), or list offsets outside
// [0, n_tok] / out of order are clamped into range, computed anyway, and raise TSIM_ENC_ERR_SPAN; a position listed for an
// EMPTY sequence has no row to clamp to and adds zeros.
// HBM: sum of list lengths x H x 2 B in (rows mostly still in L2 / Infinity Cache behind the last layer), S x H x 4 B out.
// Unit rows are not restated here: tsim_l2norm_rows runs on the float32 means, so they are its bits by construction.
#pragma once

namespace tsim {

template <int NP>   // NP: 16-byte pieces per lane = ceil(H / 512)
__global__ __launch_bounds__(256) void span_pool_kernel(const bf16_t *__restrict__ x, const int32_t *__restrict__ cu, int B,
                                                        int H, const int32_t *__restrict__ span_seq,
                                                        const int32_t *__restrict__ span_cu,
                                                        const int32_t *__restrict__ span_tok, int S, int n_tok,
                                                        float *__restrict__ out, int *__restrict__ err_flags) {
    const int lane = threadIdx.x & 63;
    const int s = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));   // wave-uniform: scalar loads below
    if (s >= S) return;
    int bad = 0;
    int b = span_seq[s];
    if (b < 0 || b >= B) { bad = TSIM_ENC_ERR_SPAN; b = b < 0 ? 0 : B - 1; }
    const int t0 = cu[b], len = cu[b + 1] - t0;
    int k0 = span_cu[s], k1 = span_cu[s + 1];
    if (k0 < 0 || k0 > n_tok) { bad = TSIM_ENC_ERR_SPAN; k0 = k0 < 0 ? 0 : n_tok; }
    if (k1 < k0 || k1 > n_tok) { bad = TSIM_ENC_ERR_SPAN; k1 = k1 < k0 ? k0 : n_tok; }
    float acc[NP][8];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[p][e] = 0.f;
    for (int k = k0; k < k1; k += 8) {
        // the rows of eight list entries; an entry past the end repeats the last one (no branch around a load) and adds zeros
        int64_t row[8];
        bool live[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const bool in = k + u < k1;
            int pos = span_tok[in ? k + u : k1 - 1];
            if (pos < 0 || pos >= len) { if (in) bad = TSIM_ENC_ERR_SPAN; pos = pos < 0 ? 0 : len - 1; }
            live[u] = in && len > 0;
            row[u] = (int64_t)(t0 + (len > 0 ? pos : 0)) * H;
        }
        if (len <= 0) continue;   // (wave-uniform) an empty sequence has no row to read
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int f0 = (lane + 64 * p) * 8;
            if (f0 >= H) continue;
            uint4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const uint4 *>(x + row[u] + f0);
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                if (!live[u]) v[u] = make_uint4(0u, 0u, 0u, 0u);
                const uint32_t wv[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc[p][2 * q] += __uint_as_float(wv[q] << 16);
                    acc[p][2 * q + 1] += __uint_as_float(wv[q] & 0xffff0000u);
                }
            }
        }
    }
    const float den = k1 > k0 ? (float)(k1 - k0) : 1.f;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const int f0 = (lane + 64 * p) * 8;
        if (f0 >= H) continue;
        float *o = out + (int64_t)s * H + f0;
        *reinterpret_cast<float4 *>(o) = make_float4(acc[p][0] / den, acc[p][1] / den, acc[p][2] / den, acc[p][3] / den);
        *reinterpret_cast<float4 *>(o + 4) = make_float4(acc[p][4] / den, acc[p][5] / den, acc[p][6] / den, acc[p][7] / den);
    }
    if (bad && lane == 0) atomicOr(err_flags, bad);
}

}  // namespace tsim

// WordEncoderModel.encode (/root/reference/src/models/word_encoder.py:46-50), GWSCModel's `torch.mean(embedded_1[i][w1_c1], dim=0)`
// per target word (:85-92) and WordPoolingStrategy.forward (/root/reference/src/modules/modules.py:68-74) on the device: the
// packed forward, unchanged, then one launch that pools the listed positions out of the final hidden states it leaves in x0.
extern "C" int tsim_encoder_forward_spans(tsim_encoder *e, const int32_t *tok_ids, const int32_t *tok_type, const int32_t *tok_pos,
                                          const int32_t *tok_col, const int32_t *cu_seqlens, int32_t T, int32_t B, int32_t max_len,
                                          float *pooled_f32, void *unit_f16, int ld_unit, float *unit_rho_max,
                                          void *last_hidden_bf16, float *logits_f32, const int32_t *span_seq,
                                          const int32_t *span_cu, const int32_t *span_tok, int32_t S, int32_t n_span_tok,
                                          float *span_out_f32, void *span_unit_f16, int ld_span_unit, float *span_rho_max,
                                          void *stream) {
    using namespace tsim;
    TSIM_REQUIRE(S >= 0 && n_span_tok >= 0, "encoder_forward_spans: S=%d n_span_tok=%d", S, n_span_tok);
    if (S > 0) {   // everything that can be refused is refused before the forward is enqueued
        TSIM_REQUIRE(e, "encoder_forward_spans: null encoder");
        const int H = e->cfg.hidden;
        TSIM_REQUIRE(span_seq && span_cu && (n_span_tok == 0 || span_tok), "encoder_forward_spans: null span table");
        TSIM_REQUIRE(span_out_f32 || span_unit_f16, "encoder_forward_spans: S=%d spans but neither span output", S);
        TSIM_REQUIRE(B > 0, "encoder_forward_spans: S=%d spans need at least one sequence", S);
        TSIM_REQUIRE(H % 8 == 0 && H <= 1024, "encoder_forward_spans: pooling needs hidden %% 8 == 0 and <= 1024 (got %d)", H);
        TSIM_REQUIRE(!span_unit_f16 || H <= 768, "encoder_forward_spans: unit rows need a width <= 768 (got %d)", H);
        TSIM_REQUIRE(!span_unit_f16 || (ld_span_unit >= H && ld_span_unit % 8 == 0), "encoder_forward_spans: ld_span_unit=%d (width %d)",
                     ld_span_unit, H);
        TSIM_REQUIRE((((uintptr_t)span_out_f32 | (uintptr_t)span_unit_f16) & 15) == 0,
                     "encoder_forward_spans: span outputs must be 16-byte aligned");
        // unit rows without float32 rows: the means live in qkv (dead after the last layer, [Tp, 3H] bf16)
        TSIM_REQUIRE(span_out_f32 || (size_t)S * 4 <= (size_t)e->Tp * 6,
                     "encoder_forward_spans: %d unit rows without span_out_f32 exceed the encoder scratch (%d rows)", S, e->Tp / 2 * 3);
    }
    if (int rc = tsim_encoder_forward_ex(e, tok_ids, tok_type, tok_pos, tok_col, cu_seqlens, T, B, max_len, pooled_f32, unit_f16,
                                         ld_unit, unit_rho_max, last_hidden_bf16, logits_f32, stream))
        return rc;
    if (S == 0) return TSIM_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int H = e->cfg.hidden;
    float *means = span_out_f32 ? span_out_f32 : reinterpret_cast<float *>(e->qkv);
    const unsigned g = ((unsigned)S + 3u) / 4u;
#define SPAN(NP) hipLaunchKernelGGL(span_pool_kernel<NP>, dim3(g), dim3(256), 0, st, e->x0, cu_seqlens, B, H, span_seq, span_cu, span_tok, S, n_span_tok, means, e->err_flags)
    if (H <= 512) SPAN(1); else SPAN(2);
#undef SPAN
    TSIM_HIP_CHECK(hipGetLastError());
    if (span_unit_f16)   // the row routine itself: unit rows and rho word are tsim_l2norm_rows(means) by construction
        return tsim_l2norm_rows(means, TSIM_F32, S, H, H, span_unit_f16, ld_span_unit, 1e-8f, span_rho_max, stream);
    return TSIM_OK;
}
