// The encoder's kernel routes, decided once (host only, no launch; included by encoder.hip at the head of its host side).
// encoder_plan: configuration -> family, kernel form of each projection, weight images and scratch buffers, or the
// refusal.  ln384_segments: (T, K) -> the row segments of a hidden-384 LayerNorm GEMM.  tsim_encoder_create validates and
// builds through the plan, the forward executes it, tsim_encoder_route_host shows it; tests/test_encoder_route_cpu.py holds
// DESIGN.md's table "Encoder routes by configuration" as data.
#pragma once
#include "common.h"
#include "gemm_pp.h"

namespace tsim {

// Two thresholds of the T routes are shapes of the ln_tail / ln_split kernels (encoder.hip, which launches them with these):
constexpr int LT_PF = 12;            // ln_tail: k-steps in flight (4 loads each: vmcnt <= 63 allows 16; K / 16 must be a multiple)
constexpr int LS_MAX_BLOCKS = 256;   // ln_tail's limit of 8 192 rows: the capacity of ln_split's image buffer (tsim_encoder_create)

typedef tsim_encoder_route EncoderPlan;   // its T-independent fields: family, form[], images, buffers (the rest stays zero)

static int encoder_plan(const tsim_encoder_config &c, EncoderPlan *p) {
    const int H = c.hidden, F = c.ffn;
    TSIM_REQUIRE(H == 64 || H == 384 || H == 768 || H == 1024, "encoder_create: hidden=%d unsupported (64, 384, 768, 1024)", H);
    TSIM_REQUIRE(c.heads > 0 && H % c.heads == 0, "encoder_create: heads=%d does not divide hidden=%d", c.heads, H);
    const int dh = H / c.heads;
    TSIM_REQUIRE(dh == 16 || dh == 32 || dh == 64, "encoder_create: head_dim=%d unsupported (16, 32, 64)", dh);
    TSIM_REQUIRE(F > 0 && F % 64 == 0 && c.num_layers > 0 && c.max_tokens > 0 && c.max_seqs > 0, "encoder_create: bad ffn/layers/capacity");
    // FFN2 runs with K = ffn: the hidden-384 LayerNorm GEMM of large batches (ln_rows_gemm) needs three 32-wide k-tiles, the
    // ping-pong GEMM of hidden 768 / 1024 two 64-wide ones, and hidden 1024 has no other FFN2 kernel
    if (H != 64 && F < 128)
        return fail(TSIM_EUNSUPPORTED, "encoder_create: ffn=%d unsupported at hidden=%d (a multiple of 64, at least 128)", F, H);
    TSIM_REQUIRE(c.arch == TSIM_ARCH_BERT || c.arch == TSIM_ARCH_MPNET || c.arch == TSIM_ARCH_ROBERTA, "encoder_create: unknown arch");
    const bool mx = c.weight_dtype == TSIM_W_MXFP8;
    TSIM_REQUIRE(c.weight_dtype == TSIM_W_BF16 || mx, "encoder_create: unknown weight_dtype %d", c.weight_dtype);
    if (mx && !(gemm_pp_mx_supported(H, H) && gemm_pp_mx_supported(3 * H, H) && gemm_pp_mx_supported(F, H) && gemm_pp_mx_supported(H, F)))
        return fail(TSIM_EUNSUPPORTED, "encoder_create: MXFP8 projections need hidden and ffn to be multiples of 256 (got %d, %d)", H, F);
    *p = EncoderPlan();
    auto forms = [&](int family, int qkv, int o, int ffn1, int ffn2) {
        p->family = family;
        p->form[TSIM_ROUTE_QKV] = qkv, p->form[TSIM_ROUTE_O] = o, p->form[TSIM_ROUTE_FFN1] = ffn1, p->form[TSIM_ROUTE_FFN2] = ffn2;
    };
    const int tile = F % 128 == 0 ? TSIM_FORM_BF16_128x128 : TSIM_FORM_BF16_128x64;   // FFN1 on gemm_bf16's plain tiles
    if (mx) {
        forms(TSIM_FAMILY_PP_MX, TSIM_FORM_PP_MX, TSIM_FORM_PP_MX_RES_LN, TSIM_FORM_PP_MX, TSIM_FORM_PP_MX_RES_LN);
        p->images = TSIM_IMG_MXFP8, p->buffers = TSIM_BUF_YBUF | TSIM_BUF_MX_ACT;
    } else if (H == 64) {
        forms(TSIM_FAMILY_H64, TSIM_FORM_BF16_128x64, TSIM_FORM_BF16_RES_LN, tile, TSIM_FORM_BF16_RES_LN);
    } else if (H == 384) {
        // gemm_xres2 (96-feature items, a bias image of 2048 floats) produces the block-packed qkv / h1 layout (packed_off) and
        // must then run both projections; MPNet's attention reads row-major qkv.  Row-major, it takes the FFN1 widths that are
        // multiples of XR_BN.
        const bool x2 = F % XR_BN == 0 && F <= 2048, pk = x2 && c.arch != TSIM_ARCH_MPNET;
        if (pk) forms(TSIM_FAMILY_H384_PACKED, TSIM_FORM_XRES2_PACKED, TSIM_FORM_LN384, TSIM_FORM_XRES2_PACKED, TSIM_FORM_LN384);
        else forms(TSIM_FAMILY_H384_ROWMAJOR, TSIM_FORM_XRES2, TSIM_FORM_LN384, x2 ? TSIM_FORM_XRES2 : tile, TSIM_FORM_LN384);
        p->images = TSIM_IMG_LN_KTILE | TSIM_IMG_LN_FRAG, p->buffers = TSIM_BUF_LNIMG;
    } else {
        // H = 768 / 1024 on gemm_pp (N % 128 == 0, K % 64 == 0, K >= 128: F >= 128 serves FFN2).  FFN1 needs F % 128 == 0, and
        // only then are the tile-major copies of the QKV and O matrices built.
        const bool pp1 = gemm_pp_supported(F, H);
        const int ffn1 = !pp1 ? TSIM_FORM_BF16_128x64 : gemm_pp_tile_width(F) == 256 ? TSIM_FORM_PP_256 : TSIM_FORM_PP_128;
        if (pp1) forms(TSIM_FAMILY_PP, TSIM_FORM_PP_256_PACKED_W, TSIM_FORM_PP_RES_LN_PACKED_W, ffn1, TSIM_FORM_PP_RES_LN);
        else forms(TSIM_FAMILY_PP, TSIM_FORM_PP_256, TSIM_FORM_PP_RES_LN, ffn1, TSIM_FORM_PP_RES_LN);
        p->images = pp1 ? TSIM_IMG_PP_QKV_O : 0, p->buffers = TSIM_BUF_YBUF;
    }
    return TSIM_OK;
}

// Whole 256-token blocks of an M-row hidden-384 LayerNorm GEMM that go to ln_rows_gemm (or ln_rows_xres2): whole rounds of 256
// blocks, and a last round that is at least half full
static int ln_rows_blocks(int M) {
    const int t256 = M / 256;
    return (t256 % 256) >= 128 ? t256 : (t256 / 256) * 256;
}

// Chained launches (ln_rows_xres2): wherever the LayerNorm GEMM has whole 256-token blocks for ln_rows_gemm, those blocks'
// workgroups run the next projection too — O-projection -> FFN1, FFN2 -> the next layer's QKV.  Only whole rounds of 256 blocks
// are chained: the stand-alone projection always runs on 256 persistent workgroups, and a chained launch of 128 .. 255 (or 384)
// blocks would run it on a half-empty round.
// Packed family with F <= 1536 (ln_rows_xres2's bias image holds 1536 floats) only.
static int chain_blocks(const EncoderPlan &p, int F, int T) {
    return p.family == TSIM_FAMILY_H384_PACKED && F <= 1536 && ln_rows_blocks(T) % 256 == 0 ? ln_rows_blocks(T) : 0;
}

// The hidden-384 LayerNorm GEMM (TSIM_FORM_LN384) of T rows with contraction length K, as row segments in order (starts are
// multiples of 32: a row block starts at the same element in the row-major and block-packed layouts).  All forms give a row the
// same bits (bit-wise large-vs-small-batch tests).  chained: the ln_rows blocks belong to a ln_rows_xres2 launch.  Returns the count.
static int ln384_segments(int T, int K, bool chained, tsim_route_segment *seg) {
    int n = 0, r0 = 0;
    auto add = [&](int form, int rows) {
        seg[n++] = {form, r0, rows};
        r0 += rows;
    };
    // 256-token tiles, one 32-token row block per wave (ln_rows_gemm_kernel), for whole rounds of 256 tiles and for a last round
    // that is at least half full; everything else — and every small batch — goes through the forms below
    if (ln_rows_blocks(T) > 0) add(chained ? TSIM_SEG_LN_ROWS_CHAINED : TSIM_SEG_LN_ROWS, ln_rows_blocks(T) * 256);
    const bool after_rows = n > 0;   // the rest is the remainder of a ln_rows launch: a true tail
    const int M = T - r0;
    if (M <= 0) return n;
    // few rows (a remainder, or a small batch): one round of 32-row workgroups that stream W straight into registers (ln_tail),
    // or of 32-row x feature-slice workgroups (ln_split) where blocks x slices still fit one round of the chip's 256 CUs
    if (M <= LS_MAX_BLOCKS * 32 && K % (16 * LT_PF) == 0) {
        const int nb = (M + 31) / 32;
        add(nb <= 64 ? TSIM_SEG_LN_SPLIT4 : nb <= 128 ? TSIM_SEG_LN_SPLIT2 : TSIM_SEG_LN_TAIL, M);
        return n;
    }
    // 128-token tiles, one workgroup per CU: mt tiles take ceil(mt/256) rounds and a nearly empty last round costs a full
    // one.  A small remainder is launched separately with 64-token tiles (2x more, 2x shorter workgroups).
    // (64-token tiles throughout measured slower: 64 x 384 x 32-k with two workgroups per CU 2.96 ms per forward, 64 x 384
    // x 64-k 3.08, against 2.74: the W tile is re-staged for half as many tokens)
    const int mt = (M + 127) / 128, full = (mt / 256) * 256, rem = mt - full;
    if (rem > 0 && rem <= 96 && (full > 0 || after_rows)) {
        if (full > 0) add(TSIM_SEG_BF16_128x384, full * 128);
        add(TSIM_SEG_BF16_64x384, T - r0);
    } else add(TSIM_SEG_BF16_128x384, M);
    return n;
}

}  // namespace tsim
