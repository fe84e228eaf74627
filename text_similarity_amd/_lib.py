"""ctypes binding of libtsim.so (include/tsim.h).  The library is the product: nothing here falls back
to torch or to the CPU oracle — if the shared object is missing or a call fails, the caller gets an
exception."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TSIM_LIB") or os.path.join(_HERE, "libtsim.so")   # TSIM_LIB: a variant build (build.py TSIM_BUILD_TAG)

TSIM_F32, TSIM_BF16 = 0, 1
TSIM_I32, TSIM_I64 = 2, 3        # index dtypes of the candidate lists (tsim_*_list_topk)
LIST_ST_ROW, LIST_ST_LIMS = 1, 2  # include/tsim.h TSIM_LIST_ST_*
IVF_ST_LIST, IVF_ST_OFF = 1, 2    # include/tsim.h TSIM_IVF_ST_*
COMMUNITY_ST_ROW, COMMUNITY_ST_LIMS = 1, 2   # include/tsim.h TSIM_COMMUNITY_ST_*
IVF_SEG = 512                     # include/tsim.h TSIM_IVF_SEG
IVFPQ_SEG = 4096                  # include/tsim.h TSIM_IVFPQ_SEG
GRAPH_ST_ROW, GRAPH_ST_ITERS = 1, 2   # include/tsim.h TSIM_GRAPH_ST_*
GRAPH_MAX_TABLE_BYTES = 131072    # include/tsim.h TSIM_GRAPH_MAX_TABLE_BYTES
GRAPH_STATIC_LDS_BYTES = 18432    # include/tsim.h TSIM_GRAPH_STATIC_LDS_BYTES
GRAPH_MAX_COARSE_LISTS = 4096     # include/tsim.h TSIM_GRAPH_MAX_COARSE_LISTS
GRAPH_INSERT_ST_ROW = 1           # include/tsim_graph_insert.h TSIM_GRAPH_INSERT_ST_ROW
GRAPH_LINK_POOL = 256             # include/tsim_graph_insert.h TSIM_GRAPH_LINK_POOL
GRAPH_LINK_ST_CUT, GRAPH_LINK_ST_ROW, GRAPH_LINK_ST_LIMS = 1, 2, 4   # include/tsim_graph_insert.h TSIM_GRAPH_LINK_ST_*
ARCH_BERT, ARCH_MPNET, ARCH_ROBERTA = 0, 1, 2
W_BF16, W_MXFP8 = 0, 1
POOL_MEAN, POOL_CLS, POOL_MAX, POOL_MEAN_SQRT_LEN = 0, 1, 2, 3
ACT_IDENTITY, ACT_TANH, ACT_RELU = 0, 1, 2
SPACE_COSINE, SPACE_DOT, SPACE_L2 = 0, 1, 2
ENC_ERR_SPAN = 16                # include/tsim.h TSIM_ENC_ERR_SPAN
RANGE_SLOT_CAP = 2048            # include/tsim.h TSIM_RANGE_SLOT_CAP
RANGE_MERGE_MAX_LISTS = 64       # include/tsim.h TSIM_RANGE_MERGE_MAX_LISTS
# tsim_encoder_route_host (include/tsim.h TSIM_FAMILY_*, TSIM_FORM_*, TSIM_SEG_*, TSIM_IMG_*, TSIM_BUF_*)
FAMILY_H64, FAMILY_H384_PACKED, FAMILY_H384_ROWMAJOR, FAMILY_PP, FAMILY_PP_MX = range(5)
(FORM_BF16_128x64, FORM_BF16_128x128, FORM_XRES2, FORM_XRES2_PACKED, FORM_PP_256_PACKED_W, FORM_PP_256, FORM_PP_128, FORM_PP_MX,
 FORM_BF16_RES_LN, FORM_LN384, FORM_PP_RES_LN_PACKED_W, FORM_PP_RES_LN, FORM_PP_MX_RES_LN) = range(1, 14)
SEG_LN_ROWS, SEG_LN_ROWS_CHAINED, SEG_LN_TAIL, SEG_LN_SPLIT2, SEG_LN_SPLIT4, SEG_BF16_128x384, SEG_BF16_64x384 = range(1, 8)
IMG_PP_QKV_O, IMG_LN_KTILE, IMG_LN_FRAG, IMG_MXFP8 = 1, 2, 4, 8
BUF_YBUF, BUF_LNIMG, BUF_MX_ACT = 1, 2, 4
ROUTE_MAX_SEGS = 4


class TsimError(RuntimeError):
    pass


class EncoderConfigC(C.Structure):
    _fields_ = [("arch", C.c_int32), ("num_layers", C.c_int32), ("hidden", C.c_int32), ("heads", C.c_int32),
                ("ffn", C.c_int32), ("vocab", C.c_int32), ("max_pos", C.c_int32), ("pad_id", C.c_int32),
                ("rel_buckets", C.c_int32), ("ln_eps", C.c_float), ("max_tokens", C.c_int32),
                ("max_seqs", C.c_int32), ("weight_dtype", C.c_int32)]


class RouteSegmentC(C.Structure):
    _fields_ = [("form", C.c_int32), ("row0", C.c_int32), ("rows", C.c_int32)]


class EncoderRouteC(C.Structure):
    _fields_ = [("family", C.c_int32), ("form", C.c_int32 * 4), ("images", C.c_int32), ("buffers", C.c_int32),
                ("chain_blocks", C.c_int32), ("qkv_chained", C.c_int32), ("n_seg", C.c_int32 * 2),
                ("seg", RouteSegmentC * ROUTE_MAX_SEGS * 2)]


_FP = C.POINTER(C.c_float)


class LayerWeightsC(C.Structure):
    _fields_ = [(n, _FP) for n in ("wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo", "ln1_g", "ln1_b",
                                   "w1", "b1", "w2", "b2", "ln2_g", "ln2_b")]


class EncoderWeightsC(C.Structure):
    _fields_ = [("word_emb", _FP), ("pos_emb", _FP), ("type_emb", _FP), ("emb_ln_g", _FP), ("emb_ln_b", _FP),
                ("rel_bias", _FP), ("layers", C.POINTER(LayerWeightsC))]


class SentenceHeadC(C.Structure):
    _fields_ = [("pool_mode", C.c_int32), ("d_out", C.c_int32), ("dense_w", C.c_void_p), ("dense_b", C.c_void_p),
                ("dense_act", C.c_int32), ("normalize", C.c_int32)]


_lib = None

_SIGS = {
    "tsim_version": (C.c_int, []),
    "tsim_last_error": (C.c_char_p, []),
    "tsim_pad_dim": (C.c_int, [C.c_int]),
    "tsim_l2norm_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_int,
                                   C.c_float, C.c_void_p, C.c_void_p]),
    "tsim_cosine_topk_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "tsim_cosine_topk_plan": (C.c_int, [C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    "tsim_cosine_topk_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                      C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_size_t, C.c_void_p]),
    "tsim_max_norm_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "tsim_dot_scaled_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p, C.c_void_p]),
    "tsim_dot_scale": (C.c_double, [C.c_float]),
    "tsim_dot_topk_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                   C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                   C.c_void_p, C.c_size_t, C.c_void_p]),
    "tsim_l2_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                               C.c_void_p]),
    "tsim_l2_query_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int,
                                     C.c_void_p]),
    "tsim_l2_guard_host": (C.c_int, [C.c_float, C.c_float, C.c_double, C.c_double, C.c_float, C.POINTER(C.c_double)]),
    "tsim_l2_topk_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                  C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                  C.c_void_p, C.c_size_t, C.c_void_p]),
    "tsim_l2_topk_large": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "tsim_topk_large_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "tsim_cosine_topk_large": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_size_t, C.c_void_p]),
    "tsim_dot_topk_large": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "tsim_range_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "tsim_cosine_range_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.c_int64, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                         C.c_void_p]),
    "tsim_dot_range_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_size_t, C.c_void_p]),
    "tsim_range_fill": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_float,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "tsim_cosine_range_scan_tau": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                             C.c_void_p]),
    "tsim_dot_range_scan_tau": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_size_t, C.c_void_p]),
    "tsim_range_fill_tau": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "tsim_range_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "tsim_l2_range_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_size_t, C.c_void_p]),
    "tsim_l2_range_scan_tau": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.c_void_p]),
    "tsim_range_merge_asc": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "tsim_list_topk_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    **{name: (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_int64,
                        C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t,
                        C.c_void_p])
       for name in ("tsim_cosine_list_topk", "tsim_dot_list_topk", "tsim_l2_list_topk")},
    "tsim_list_topk_f16": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                                     C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_void_p, C.c_size_t, C.c_void_p]),
    "tsim_code_bytes": (C.c_int, [C.c_int]),
    "tsim_pack_sign_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "tsim_hamming_topk_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "tsim_hamming_topk": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "tsim_sign_rescore_topk": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                                         C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "tsim_int8_bytes": (C.c_int, [C.c_int]),
    "tsim_quantize_int8_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "tsim_int8_ip_topk_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int]),
    "tsim_int8_ip_topk": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "tsim_int8_rescore_topk": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                                         C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "tsim_pq_code_bytes": (C.c_int, [C.c_int]),
    "tsim_pq_encode_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_int64,
                                      C.c_void_p]),
    "tsim_pq_tables": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    "tsim_pq_adc_topk_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64, C.c_int, C.c_int]),
    "tsim_pq_adc_topk": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "tsim_ivf_scan_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int64, C.c_int]),
    "tsim_ivf_scan_topk": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                                     C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "tsim_ivfpq_tables_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int]),
    "tsim_ivfpq_tables": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int,
                                    C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                    C.c_void_p]),
    "tsim_ivfpq_scan_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int64, C.c_int]),
    "tsim_ivfpq_scan_topk": (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int,
                                       C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_void_p,
                                       C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "tsim_graph_search_lds_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "tsim_graph_search": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                                    C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                    C.c_int64, C.c_void_p, C.c_void_p]),
    "tsim_graph_search_seeded": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int,
                                           C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int,
                                           C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                           C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsim_graph_prune": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsim_community_select_workspace_bytes": (C.c_size_t, [C.c_int64, C.c_int64]),
    "tsim_community_select_rounds": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int64, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "tsim_community_select_finish": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "tsim_mst_prim_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "tsim_mst_prim": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_size_t, C.c_void_p]),
    "tsim_hdbscan_tree_labels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "tsim_cosine_topk": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "tsim_time_next_topk": (None, [C.c_void_p, C.c_void_p]),
    "tsim_topk_merge": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "tsim_topk_merge_strided": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsim_wordpiece_create": (C.c_int, [C.c_char_p, C.c_void_p, C.c_int32, C.c_char_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.c_int32, C.c_int32, C.c_int32, C.c_char_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]),
    "tsim_wordpiece_destroy": (None, [C.c_void_p]),
    "tsim_wordpiece_encode": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                        C.c_void_p, C.c_void_p]),
    "tsim_cos_sim": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "tsim_mean_pool": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p,
                                 C.c_void_p]),
    "tsim_pool": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "tsim_dense_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p]),
    "tsim_quantize_mxfp8": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsim_gemm_mxfp8": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                  C.c_int, C.c_void_p]),
    "tsim_encoder_create": (C.c_int, [C.POINTER(EncoderConfigC), C.POINTER(EncoderWeightsC),
                                      C.POINTER(C.c_void_p)]),
    "tsim_encoder_destroy": (None, [C.c_void_p]),
    "tsim_encoder_error_flags": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "tsim_chain_items_host": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int]),
    "tsim_encoder_route_host": (C.c_int, [C.POINTER(EncoderConfigC), C.c_int32, C.c_int32, C.POINTER(EncoderRouteC)]),
    "tsim_encoder_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "tsim_encoder_set_token_types": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "tsim_encoder_set_cls_head": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]),
    "tsim_encoder_set_cls_head_act": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "tsim_encoder_forward_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                          C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "tsim_encoder_forward_head": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                            C.c_int32, C.c_int32, C.POINTER(SentenceHeadC), C.c_void_p, C.c_void_p, C.c_int,
                                            C.c_void_p, C.c_void_p, C.c_void_p]),
    "tsim_encoder_forward_spans": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                             C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
}

DECLARED_SYMBOLS = tuple(_SIGS)

# The entries of include/tsim_graph_insert.h: exported by the same library and bound like the others, in a table of their own
# until they move into include/tsim.h and the table above.
_GRAPH_INSERT_SIGS = {
    "tsim_graph_insert_prune": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "tsim_graph_link_reverse": (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                          C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}
GRAPH_INSERT_SYMBOLS = tuple(_GRAPH_INSERT_SIGS)


def lib() -> C.CDLL:
    """Load libtsim.so once.  Raises TsimError (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TsimError(f"{LIB_PATH} not found: build it with `python -m text_similarity_amd.build` "
                            "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in {**_SIGS, **_GRAPH_INSERT_SIGS}.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                def fn(*a, _n=name, **kw):
                    raise TsimError(f"libtsim.so does not export {_n}: rebuild with python -m text_similarity_amd.build")
                setattr(L, name, fn)
                continue
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().tsim_last_error().decode(errors="replace")
        exc = ValueError if rc in (1, 4) else TsimError
        raise exc(f"{what or 'tsim'} failed (code {rc}): {msg}")
