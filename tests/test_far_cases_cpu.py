"""The proof that tests/test_far_rows_gpu.py and tests/test_large_corpus_gpu.py can fail, on the CPU, without a wrong kernel ever
running on a GPU (the approach of tests/test_encoder_power_cpu.py).

1. The layouts of tests/far_cases.py keep their promises: which byte and element offsets the row starts cross, the row that
   straddles 2^32 bytes, rows on both sides of every boundary, the sizes.
2. For each layout, corpus and width, each modelled truncation (byte offset mod 2^32; element index mod 2^31 and mod 2^32; the
   int32 sign wrap of the element index and of the byte offset, an offset outside the buffer reading as the fill; a 64-bit row
   base that takes the offset inside the row without the carry) changes what is read, and the oracle's top-10 lists on what was
   read differ from the true ones for at least one query.  As measured: the whole-row defects change 6 to 8 of the 8 queries
   (2 to 4 for the element index mod 2^32 on the float32 rows, of which only the last 27 lie beyond 2^32 elements), the lost
   carry (one or two rows read wrongly) 1 or 2.  Both layouts reach every boundary the models wrap at, so every model applies to
   both.
3. The planted-margin condition of the large corpus: in every space the worst planted row beats the best row of the 4 096-row
   block, for every query, by a margin; the planted scores of a query are distinct."""
import numpy as np
import pytest

import far_cases as fc

K = 10


def test_layout_conditions():
    B, F = fc.LAYOUT_B, fc.LAYOUT_F
    assert B.itemsize == 1 and B.stride % 16 == 0 and F.itemsize == 4 and F.stride % 4 == 0
    assert 4.3e9 < B.nbytes < 4.8e9 and 17.2e9 < F.nbytes < 17.4e9
    assert F.nbytes + fc.N * 4 * max(fc.DIMS) < 20e9            # a far buffer and a compact copy
    for lay, widths in ((B, (32, 48, 256, 304)), (F, (4 * 256, 4 * 300))):
        for wb in widths:
            a = lay.start(lay.i0)
            assert a < 1 << 32 < a + wb, f"row {lay.i0} of layout {lay.name} must straddle 2^32 bytes at {wb} bytes a row"
            assert lay.start(lay.rows - 1) + wb <= lay.nbytes
        for b in lay.boundaries:
            below = [r for r in range(lay.rows) if lay.start(r) + max(widths) <= b]
            above = [r for r in range(lay.rows) if lay.start(r) >= b]
            assert len(below) >= 2 and len(above) >= 2, f"layout {lay.name}: no rows on both sides of byte {b}"
            sent = lay.sentinels()
            assert any(r in sent for r in below) and any(r in sent for r in above)
    assert B.boundaries == (1 << 31, 1 << 32) and F.boundaries == (1 << 31, 1 << 32, 1 << 33, 1 << 34)
    assert F.start(F.rows - 1) // 4 > 1 << 32 and F.start(F.i0) == (1 << 32) - 448 and B.start(B.i0) == (1 << 32) - 16
    # the far queries: rows 1, 2 and 4 start beyond 2^31, 2^32 and 2^33 bytes, row 7 straddles 2^32 elements
    S = fc.QUERY_STRIDE_F
    assert S % 4 == 0 and 1 << 31 < 4 * S < 1 << 32 < 8 * S < 1 << 33 < 16 * S and 7 * S < 1 << 32 < 7 * S + min(fc.DIMS)
    assert (7 * fc.QUERY_STRIDE_F + max(fc.DIMS)) * 4 <= F.nbytes


def test_sentinels_sit_in_a_top10_list():
    """every row beside a boundary is in the true top-10 of its query in every space, so misreading it alone shows"""
    for lay in ("F",):          # (Layout B carries code rows only: the code tests below see its straddling row on its own)
        for kind in fc.KINDS:
            for d in fc.DIMS:
                for space in ("cosine", "dot", "l2"):
                    idx = fc.oracle_topk(lay, kind, d, space)[1][:, :K]
                    for t, r in enumerate(fc.LAYOUTS[lay].sentinels()):
                        assert r in idx[1 + t % (fc.Q - 1)], f"layout {lay} {kind} d={d} {space}: row {r} is not in a top-{K} list"


def _differ(a, b):
    """queries whose (values, indices) lists differ"""
    return int(((a[0] != b[0]) | (a[1] != b[1])).any(1).sum())


@pytest.mark.parametrize("model", fc.MODELS)
@pytest.mark.parametrize("d", fc.DIMS)
@pytest.mark.parametrize("kind", fc.KINDS)
def test_float_rows_every_truncation_changes_a_topk_list(kind, d, model):
    q, c = fc.rows("F", kind, d)
    read = fc.misread(fc.LAYOUT_F, c, model)
    bad = fc.rows_misread(c, read)
    print(f"F {kind} d={d} {model}: {bad.size} rows read wrongly, first {bad[:3].tolist()}")
    assert bad.size > 0
    for space in ("cosine", "dot", "l2"):
        s = fc.exact("F", kind, d, space).copy()
        s[:, bad] = fc.scores(space, q, read[bad])
        n = _differ(fc.topk(space, s, K), fc.topk(space, fc.exact("F", kind, d, space), K))
        print(f"   {space}: top-{K} lists of {n} of {fc.Q} queries differ")
        assert n >= 1, f"F {kind} d={d} {space}: the oracle does not see {model} ({n} queries affected)"


@pytest.mark.parametrize("model", fc.MODELS)
@pytest.mark.parametrize("family", ["hamming", "int8", "pq"])
@pytest.mark.parametrize("d", fc.DIMS)
@pytest.mark.parametrize("kind", fc.KINDS)
def test_code_rows_every_truncation_changes_a_topk_list(kind, d, family, model):
    c_codes = fc.codes(kind, d, family)[1]
    read = fc.misread(fc.LAYOUT_B, c_codes, model)
    bad = fc.rows_misread(c_codes, read)
    assert bad.size > 0
    n = _differ(fc.code_topk(kind, d, family, read, K), fc.code_topk(kind, d, family, c_codes, K))
    print(f"B {kind} d={d} {family} {model}: {bad.size} rows read wrongly, top-{K} lists of {n} of {fc.Q} queries differ")
    assert n >= 1, f"B {kind} d={d} {family}: the oracle does not see {model} ({n} queries affected)"


def test_far_queries_every_truncation_changes_what_is_read():
    """the eight far query rows: every model reads at least one of them wrongly (a wrong query changes its whole list)"""
    lay = fc.Layout("Fq", 4, fc.QUERY_STRIDE_F, 7, (1 << 31, 1 << 32, 1 << 33, 1 << 34), rows=fc.Q)
    for d in fc.DIMS:
        q = fc.rows("F", "gauss", d)[0]
        for model in fc.MODELS:
            bad = fc.rows_misread(q, fc.misread(lay, q, model))
            print(f"far queries d={d} {model}: rows {bad.tolist()} read wrongly")
            assert bad.size >= 1


@pytest.mark.parametrize("space", ["cosine", "dot", "l2"])
def test_large_corpus_planted_margin(space):
    """Every planted row beats every block row for every query by a margin; l2 on the first 767 columns (the widest rows the
    Euclidean search takes).  A background of 700 copies of each block row is then irrelevant to rank and to ties among the first
    128 places."""
    q, block, pos, planted = fc.large_inputs()
    w = 767 if space == "l2" else fc.LARGE_D
    sb, sp = fc.scores(space, q[:, :w], block[:, :w]), fc.scores(space, q[:, :w], planted[:, :w])
    if space == "l2":
        sb, sp = -sb, -sp
    best_block, worst_planted = sb.max(1), sp.min(1)
    cb, cp = fc.scores("cosine", q, block), fc.scores("cosine", q, planted)
    print(f"{space}: best block score {best_block.max():.4f}, worst planted score {worst_planted.min():.4f}; "
          f"cosine: block <= {cb.max():.4f}, planted {cp.min():.4f} .. {cp.max():.4f}")
    scale = {"cosine": 1.0, "dot": float(fc.LARGE_D), "l2": 2.0 * fc.LARGE_D}[space]
    assert (worst_planted - best_block >= fc.LARGE_MARGIN * scale).all()
    assert cb.max() < 0.25 and cp.min() > 0.45 and cp.max() < 0.97
    for j in range(fc.Q):
        assert np.unique(sp[j]).size == fc.LARGE_PLANTS, "the planted scores of a query must be distinct"
    # positions: the five spots
    assert {0, 1, fc.LARGE_HALF_ROW - 1, fc.LARGE_HALF_ROW, fc.LARGE_HALF_ROW + 1, fc.LARGE_F32_ROW - 1, fc.LARGE_F32_ROW,
            fc.LARGE_F32_ROW + 1, fc.LARGE_N - 2, fc.LARGE_N - 1} <= set(pos.tolist())
    assert fc.LARGE_HALF_ROW * 2 * fc.LARGE_D < 1 << 32 < (fc.LARGE_HALF_ROW + 1) * 2 * fc.LARGE_D
    assert fc.LARGE_F32_ROW * 4 * fc.LARGE_D < 1 << 32 < (fc.LARGE_F32_ROW + 1) * 4 * fc.LARGE_D
    assert fc.LARGE_N * 2 * fc.LARGE_D > (1 << 32) + (100 << 20) and np.array_equal(fc.large_row(pos), planted)
