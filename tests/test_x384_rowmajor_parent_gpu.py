"""The row-major form of the K = 384 projection, gemm_xres2_kernel<EPI, false, false> (QKV and FFN1 of an MPNet-style hidden-384
model, whose residual stream stays row-major), against the bits of the parent commit: tests/golden/x384_rowmajor_parent.json,
written by `tools/hash_forward.py x384-rowmajor` there.  The packed instantiations are pinned the same way by
tests/test_residual_packed_gpu.py.  Token counts: residual_cases.X384_TOKENS (every state of the item loop)."""
import json
import os

import pytest

import residual_cases as rc

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "x384_rowmajor_parent.json")


@pytest.fixture(scope="module")
def parent_digests():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def forwards():
    """{T: digests}: one encoder, every token count encoded once."""
    flat, cu = rc.sentences()
    enc = rc.x384_encoder()
    return {T: rc.digests(*rc.encode(enc, *rc.cut(flat, cu, T))) for T in rc.X384_TOKENS}


@pytest.mark.parametrize("T", rc.X384_TOKENS)
def test_bits_of_the_parent(forwards, parent_digests, T):
    want = parent_digests[rc.x384_case_id(T)]
    assert forwards[T]["hidden"] == want["hidden"], f"T={T}: hidden rows differ from the parent's"
    assert forwards[T]["pooled"] == want["pooled"], f"T={T}: pooled rows differ from the parent's"
