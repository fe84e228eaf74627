"""The encoder's kernel routes, read through tsim_encoder_route_host (host only: no GPU, nothing is created).

``ROUTES`` is DESIGN.md's table "Encoder routes by configuration" as data: for every case of ``encoder_cases.CASES``,
``arch_cases`` and ``config_cases.CASES`` the family, the kernel form of QKV / O + LayerNorm / FFN1 / FFN2 + LayerNorm, the weight
images and scratch buffers, and the chained blocks of a 65 536-token forward.  ``config_cases.REFUSED`` is refused as
tsim_encoder_create refuses it.

The T routes of the hidden-384 LayerNorm GEMM: ``SEGMENTS`` holds the boundaries written out by hand, ``segments_before`` is
the five-way router that ``gemm_res_ln``'s hidden-384 case was before the plan existed, restated line for line from that code
(ln_rows_blocks, then ln_tail_gemm's choice of S, then the 128 / 64-token tiles), and every (T, K) of the lists below must give
what it gives.  The sweep at the end is the proof that no accepted configuration is left without a kernel at forward time, and
that every form the plan can name is reached by some configuration (a form nothing reaches would be a dead launch site).
"""
import itertools

import pytest

import arch_cases
import config_cases
import encoder_cases
from text_similarity_amd import _lib as L
from text_similarity_amd.native_encoder import encoder_route
from text_similarity_amd.presets import EncoderConfig

H64 = (L.FAMILY_H64, L.FORM_BF16_128x64, L.FORM_BF16_RES_LN, None, L.FORM_BF16_RES_LN, 0, 0)
H384 = (None, None, L.FORM_LN384, None, L.FORM_LN384, L.IMG_LN_KTILE | L.IMG_LN_FRAG, L.BUF_LNIMG)
PP_PACKED = (L.FAMILY_PP, L.FORM_PP_256_PACKED_W, L.FORM_PP_RES_LN_PACKED_W, None, L.FORM_PP_RES_LN, L.IMG_PP_QKV_O, L.BUF_YBUF)
PP_ROWMAJOR = (L.FAMILY_PP, L.FORM_PP_256, L.FORM_PP_RES_LN, None, L.FORM_PP_RES_LN, 0, L.BUF_YBUF)
MX = (L.FAMILY_PP_MX, L.FORM_PP_MX, L.FORM_PP_MX_RES_LN, L.FORM_PP_MX, L.FORM_PP_MX_RES_LN, L.IMG_MXFP8, L.BUF_YBUF | L.BUF_MX_ACT)


def _row(base, ffn1, family=None, qkv=None, chain=0):
    r = list(base)
    r[3] = ffn1 if r[3] is None else r[3]
    r[0] = family if r[0] is None else r[0]
    r[1] = qkv if r[1] is None else r[1]
    return tuple(r) + (chain,)


def _packed(chain):
    return _row(H384, L.FORM_XRES2_PACKED, L.FAMILY_H384_PACKED, L.FORM_XRES2_PACKED, chain)


def _rowmajor(ffn1):
    return _row(H384, ffn1, L.FAMILY_H384_ROWMAJOR, L.FORM_XRES2)


# case -> (family, QKV, O + LN, FFN1, FFN2 + LN, images, buffers, chain_blocks at T = 65 536)
ROUTES = {
    # encoder_cases
    "tiny-bert": _row(H64, L.FORM_BF16_128x128),
    "tiny-mpnet": _row(H64, L.FORM_BF16_128x128),
    "bert-384": _packed(256),
    "mpnet-384": _rowmajor(L.FORM_XRES2),
    "bert-768": _row(PP_PACKED, L.FORM_PP_256),
    "mpnet-768": _row(PP_PACKED, L.FORM_PP_256),
    "bert-768-mxfp8": _row(MX, None),
    "mpnet-768-mxfp8": _row(MX, None),
    # arch_cases
    "distilbert": _row(H64, L.FORM_BF16_128x128),
    "roberta": _row(H64, L.FORM_BF16_128x128),
    "xlm-roberta": _row(H64, L.FORM_BF16_128x128),
    "camembert": _row(H64, L.FORM_BF16_128x128),
    "bert-1024": _row(PP_PACKED, L.FORM_PP_256),
    "bert-1024-mxfp8": _row(MX, None),
    # config_cases
    "bert-64-h2-f64": _row(H64, L.FORM_BF16_128x64),
    "mpnet-64-h1-f320": _row(H64, L.FORM_BF16_128x64),
    "bert-384-h6-f768": _packed(256),
    "bert-384-h24-f1920": _packed(0),                       # F > 1536: chain off
    "bert-384-f1024": _rowmajor(L.FORM_BF16_128x128),
    "bert-384-f2112": _rowmajor(L.FORM_BF16_128x64),        # F % 192 = 0 above 2048, F % 128 = 64
    "mpnet-384-h6-f2048": _rowmajor(L.FORM_BF16_128x128),
    "bert-768-h24-f1920": _row(PP_PACKED, L.FORM_PP_128),
    "bert-768-h48-f1984": _row(PP_ROWMAJOR, L.FORM_BF16_128x64),
    "bert-768-h24-f2048-mxfp8": _row(MX, None),
    "bert-1024-h32-f2816": _row(PP_PACKED, L.FORM_PP_256),
}

ALL_CASES = {**encoder_cases.CASES, **{k: (cfg, "bf16") for k, (cfg, _) in arch_cases.ARCHS.items()}, **arch_cases.CASES_1024,
             **config_cases.CASES}


def test_the_table_names_every_case():
    assert set(ROUTES) == set(ALL_CASES)


@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_case_routes(name):
    cfg, dtype = ALL_CASES[name]
    family, qkv, o, ffn1, ffn2, images, buffers, chain = ROUTES[name]
    for layer in range(cfg.num_layers):
        r = encoder_route(cfg, 65536, layer, dtype)
        assert (r.family, r.form, r.images, r.buffers, r.chain_blocks) == (family, [qkv, o, ffn1, ffn2], images, buffers, chain)
        assert r.qkv_chained == (chain > 0 and layer > 0)
        last = layer + 1 == cfg.num_layers
        if o == L.FORM_LN384:   # 65 536 rows: one round of 256 blocks, nothing behind them
            assert r.segments[0] == [(L.SEG_LN_ROWS_CHAINED if chain else L.SEG_LN_ROWS, 0, 65536)]
            assert r.segments[1] == [(L.SEG_LN_ROWS_CHAINED if chain and not last else L.SEG_LN_ROWS, 0, 65536)]
        else:
            assert r.segments == ([], [])
    assert encoder_route(cfg, 4096, 1, dtype).chain_blocks == 0 and not encoder_route(cfg, 4096, 1, dtype).qkv_chained


@pytest.mark.parametrize("name", sorted(config_cases.REFUSED))
def test_refused_as_create_refuses(name):
    cfg, dtype, text = config_cases.REFUSED[name]
    with pytest.raises(ValueError, match=r"\(code 4\): " + text):   # TSIM_EUNSUPPORTED
        encoder_route(cfg, 256, 0, dtype)


def test_bad_arguments():
    cfg = encoder_cases.CASES["bert-384"][0]
    for T, layer in ((-1, 0), (256, -1), (256, cfg.num_layers)):
        with pytest.raises(ValueError, match=r"\(code 1\): encoder_route_host"):
            encoder_route(cfg, T, layer)
    assert encoder_route(cfg, 0).segments == ([], [])


# ---- the T routes of the hidden-384 LayerNorm GEMM -------------------------------------------------------------------------
ROWS, CHAINED, TAIL, SPLIT2, SPLIT4, T128, T64 = (L.SEG_LN_ROWS, L.SEG_LN_ROWS_CHAINED, L.SEG_LN_TAIL, L.SEG_LN_SPLIT2,
                                                  L.SEG_LN_SPLIT4, L.SEG_BF16_128x384, L.SEG_BF16_64x384)
T_LIST = (1, 31, 32, 33, 2048, 2049, 4096, 4097, 8192, 8193, 32767, 32768, 65535, 65536, 65536 + 8192, 65536 + 8193, 65536 + 24577)
K_LIST = (384, 768, 1024, 1536, 1920, 2112)
K_TAIL = (384, 768, 1536, 1920, 2112)   # multiples of 16 x 12: ln_tail / ln_split take them; 1024 is not one

# T -> (segments for K in K_TAIL, segments for K = 1024), ln_rows unchained.  By hand from the code before the plan:
#   ln_rows_blocks(T): t = T // 256; t if t % 256 >= 128 else t // 256 * 256
#   the rows M behind them: M <= 8192 and K % 192 == 0 -> nb = ceil(M / 32): S = 4 up to 64 blocks, 2 up to 128, else ln_tail
#   else mt = ceil(M / 128), full = mt // 256 * 256, rem = mt - full: 0 < rem <= 96 behind ln_rows (or full) -> the 64-row tile
SEGMENTS = {
    2048: ([(SPLIT4, 0, 2048)], [(T128, 0, 2048)]),                      # 64 row blocks
    2049: ([(SPLIT2, 0, 2049)], [(T128, 0, 2049)]),                      # 65
    4096: ([(SPLIT2, 0, 4096)], [(T128, 0, 4096)]),                      # 128
    4097: ([(TAIL, 0, 4097)], [(T128, 0, 4097)]),                        # 129
    8192: ([(TAIL, 0, 8192)], [(T128, 0, 8192)]),                        # 256 = LS_MAX_BLOCKS
    8193: ([(T128, 0, 8193)], [(T128, 0, 8193)]),                        # past ln_tail; no ln_rows in front: no 64-row tile
    32767: ([(T128, 0, 32767)], [(T128, 0, 32767)]),                     # 127 blocks of 256: under half a round; 256 tiles of 128
    32768: ([(ROWS, 0, 32768)], [(ROWS, 0, 32768)]),                     # 128 blocks: half a round
    65535: ([(ROWS, 0, 65280), (SPLIT4, 65280, 255)], [(ROWS, 0, 65280), (T64, 65280, 255)]),   # 255 blocks + 255 rows
    65536: ([(ROWS, 0, 65536)], [(ROWS, 0, 65536)]),                     # one whole round
    65536 + 8192: ([(ROWS, 0, 65536), (TAIL, 65536, 8192)], [(ROWS, 0, 65536), (T64, 65536, 8192)]),     # 32 more blocks: not half a round
    65536 + 8193: ([(ROWS, 0, 65536), (T64, 65536, 8193)], [(ROWS, 0, 65536), (T64, 65536, 8193)]),      # 65 tiles of 128 <= 96
    65536 + 24577: ([(ROWS, 0, 65536), (T128, 65536, 24577)], [(ROWS, 0, 65536), (T128, 65536, 24577)]),  # 193 tiles > 96
}


def _bert384(F, layers=2):
    return EncoderConfig("bert", layers, 384, 12, F, 1000, 260, 1e-12)


def _mpnet384(F):
    return EncoderConfig("mpnet", 2, 384, 12, F, 1000, 262, 1e-5, type_vocab=0, pad_id=1)


def segments_before(T, K, chained):
    """gemm_res_ln's ``case 384`` (with the fragment image, which every hidden-384 encoder has) as it stood, as segments."""
    segs, r0, M, after_rows = [], 0, T, False
    t256 = M // 256
    use = t256 if t256 % 256 >= 128 else t256 // 256 * 256          # ln_rows_blocks
    if use > 0:
        segs.append((CHAINED if chained else ROWS, 0, use * 256))   # tail_only: the caller's ln_rows_xres2 runs these rows
        r0, M, after_rows = use * 256, M - use * 256, True
        if M == 0:
            return segs
    if M <= 256 * 32 and K % (16 * 12) == 0:                        # ln_tail_gemm: S by the row blocks
        nb = (M + 31) // 32
        return segs + [(SPLIT4 if nb <= 64 else SPLIT2 if nb <= 128 else TAIL, r0, M)]
    mt = (M + 127) // 128
    full = mt // 256 * 256
    rem = mt - full
    if 0 < rem <= 96 and (full > 0 or after_rows):
        if full > 0:
            segs.append((T128, r0, full * 128))
        return segs + [(T64, r0 + full * 128, M - full * 128)]
    return segs + [(T128, r0, M)]


def _check_partition(segs, T):
    at = 0
    for form, row0, rows in segs:
        assert row0 == at and row0 % 32 == 0 and rows > 0 and form in (ROWS, CHAINED, TAIL, SPLIT2, SPLIT4, T128, T64)
        at += rows
    assert at == T


@pytest.mark.parametrize("K", K_LIST)
def test_ln384_segments_at_the_boundaries(K):
    """O runs with K = 384 and FFN2 with K = ffn: an MPNet configuration (never chained) of ffn = K shows both."""
    for T in T_LIST:
        o, got = encoder_route(_mpnet384(K), T).segments
        _check_partition(got, T)
        assert got == segments_before(T, K, False), (T, K)
        if T in SEGMENTS:
            assert got == SEGMENTS[T][0 if K in K_TAIL else 1], (T, K)
        assert o == segments_before(T, 384, False)


@pytest.mark.parametrize("F", (768, 1536, 1920))
def test_ln384_chained_segments(F):
    """The chain rule: packed family, F <= 1536, whole rounds of 256 blocks; for FFN2 also a next layer."""
    cfg = _bert384(F, layers=3)
    for T in T_LIST:
        rounds = T // 65536 if (T // 256) % 256 < 128 else 0
        chain = 256 * rounds if F <= 1536 else 0
        for layer in range(3):
            r = encoder_route(cfg, T, layer)
            assert r.chain_blocks == chain and r.qkv_chained == (chain > 0 and layer > 0)
            assert r.segments[0] == segments_before(T, 384, chain > 0), (T, layer)
            assert r.segments[1] == segments_before(T, F, chain > 0 and layer < 2), (T, layer)
            if T in SEGMENTS and chain:
                want = [(CHAINED,) + s[1:] if s[0] == ROWS else s for s in SEGMENTS[T][0]]
                assert r.segments[0] == want and r.segments[1] == (want if layer < 2 else SEGMENTS[T][0])
    assert encoder_route(_mpnet384(1536), 65536, 1).chain_blocks == 0      # MPNet: row-major, never chained


def test_totality_sweep():
    """Every (H, heads, F, arch, dtype) is refused by the plan or has a known form for all four projections and, for hidden 384,
    segments that partition [0, T) at every T of the list; and every form and family the header names is reached."""
    archs = (("bert", 0, 0), ("mpnet", 1, 0), ("bert", 1, 2))   # (arch, pad_id, pos_offset): BERT, MPNet, RoBERTa
    seen_forms, seen_segs, seen_families, accepted, refused = set(), set(), set(), 0, 0
    forms = set(range(L.FORM_BF16_128x64, L.FORM_PP_MX_RES_LN + 1))
    for H, dh, F, (arch, pad, off), dtype in itertools.product((64, 384, 768, 1024), (16, 32, 64), range(64, 4224 + 1, 64), archs,
                                                               ("bf16", "mxfp8")):
        cfg = EncoderConfig(arch, 2, H, H // dh, F, 1000, 300, 1e-12, pad_id=pad, pos_offset=off)
        want_refused = (F == 64 and H > 64) or (dtype == "mxfp8" and (H % 256 != 0 or F % 256 != 0))   # include/tsim.h
        try:
            r = encoder_route(cfg, 1, 0, dtype)
        except ValueError as e:
            assert "(code 4)" in str(e) and want_refused, (H, dh, F, arch, dtype, e)
            refused += 1
            continue
        assert not want_refused, (H, dh, F, arch, dtype)
        accepted += 1
        assert set(r.form) <= forms and 0 not in r.form, (H, dh, F, arch, dtype, r)
        seen_forms.update(r.form)
        seen_families.add(r.family)
        ln384 = [i for i in (1, 3) if r.form[i] == L.FORM_LN384]
        assert ln384 == ([1, 3] if H == 384 else [])
        for T in T_LIST if ln384 and dh == 32 else ():   # (the segments do not depend on the head count)
            for layer in (0, 1):
                rt = encoder_route(cfg, T, layer, dtype)
                assert rt.form == r.form
                for segs in rt.segments:
                    _check_partition(segs, T)
                    seen_segs.update(s[0] for s in segs)
    assert accepted > 0 and refused > 0
    assert seen_forms == forms and seen_families == set(range(5))
    assert seen_segs == {ROWS, CHAINED, TAIL, SPLIT2, SPLIT4, T128, T64}
