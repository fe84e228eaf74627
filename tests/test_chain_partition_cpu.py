"""The item assignment of the chained LayerNorm-GEMM + projection launch (ln_rows_xres2), through the library's host entry
tsim_chain_items_host, which evaluates the kernel's own chain_part / chain_item: workgroup b of G (one per whole 256-token
block) takes the N / 96 items of its own block, then the share [R b / G, R (b + 1) / G) of the R = remainder_blocks x N / 96 items behind the whole
blocks.  Every item must be assigned exactly once, and no workgroup may get more than ceil(total / G) + 1 items."""
import ctypes as C
import os

import pytest

from text_similarity_amd import _lib

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "tsim.h")
# (blocks, remainder_blocks, N / 96, G)
CASES = [(128, 0, 16, 128), (128, 1, 12, 128), (256, 7, 16, 256), (256, 7, 12, 256), (384, 1, 16, 384), (256, 127, 16, 256),
         (512, 3, 16, 512), (512, 127, 12, 512)]      # two whole rounds: the launcher chains multiples of 256 blocks


def _lib_or_skip():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtsim.so is not built")
    return _lib.lib()


def _items(L, blocks, rem, ntiles, G, b):
    n = L.tsim_chain_items_host(blocks, rem, ntiles, G, b, None, 0)
    assert n >= 0
    buf = (C.c_int32 * max(n, 1))()
    assert L.tsim_chain_items_host(blocks, rem, ntiles, G, b, buf, n) == n
    return list(buf[:n])


def test_header_declares_the_entry():
    assert "tsim_chain_items_host(" in open(HDR).read()
    assert "tsim_chain_items_host" in _lib.DECLARED_SYMBOLS


@pytest.mark.parametrize("blocks,rem,ntiles,G", CASES)
def test_every_item_once_and_balanced(blocks, rem, ntiles, G):
    L = _lib_or_skip()
    total = (blocks + rem) * ntiles
    seen = []
    most = 0
    for b in range(G):
        it = _items(L, blocks, rem, ntiles, G, b)
        most = max(most, len(it))
        # own items first: all tiles of block b, in order; then a contiguous run of remainder items
        own = [x for x in it if x < blocks * ntiles]
        assert it[:len(own)] == own
        assert own == [b * ntiles + j for j in range(ntiles)]
        tail = it[len(own):]
        assert tail == list(range(tail[0], tail[0] + len(tail))) if tail else True
        seen += it
    assert sorted(seen) == list(range(total))
    assert most <= -(-total // G) + 1, (most, total, G)


def test_bad_arguments_are_refused():
    L = _lib_or_skip()
    buf = (C.c_int32 * 4)()
    assert L.tsim_chain_items_host(128, 0, 0, 128, 0, buf, 4) < 0        # no feature tiles
    assert L.tsim_chain_items_host(128, 0, 16, 128, 128, buf, 4) < 0     # b outside [0, G)
    assert L.tsim_chain_items_host(128, 0, 16, 0, 0, buf, 4) < 0
    assert L.tsim_chain_items_host(128, -1, 16, 128, 0, buf, 4) < 0
    assert L.tsim_chain_items_host(256, 1, 16, 128, 0, buf, 4) < 0       # one workgroup per whole block: blocks == G
    assert L.tsim_chain_items_host(128, 1, 16, 128, 0, None, 4) < 0      # a capacity without a buffer
