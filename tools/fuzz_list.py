#!/usr/bin/env python3
"""Randomised parity sweep of the exact search within candidate lists (ops.cosine_list_topk / dot_list_topk / l2_list_topk)
against the oracle of tests/list_cases.py: scores (float32 bits), indices and status words must be identical.  Every case
draws a space, a width, Q, N, k, the form of the lists (shared / CSR / 2-D, int32 / int64), their lengths (around k, the
wave, the LDS block and TSIM_LIST_SLICE), and sprinkles padding, repeats and rows beyond the corpus into them.
Half of the cases keep the corpus as FLOAT16 rows (ops.f16_list_topk; a row stride of d + 1 or d, rows of subnormal halves among
the kinds): the result must equal the oracle on the widened rows AND the float32 op on them, bit for bit.
Usage: python tools/fuzz_list.py [cases] [seed]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
from list_cases import csr, header_define, list_topk_ref, same_bits
from text_similarity_amd import ops

S = header_define("TSIM_LIST_SLICE")
FN = {"cosine": ops.cosine_list_topk, "dot": ops.dot_list_topk, "l2": ops.l2_list_topk}
cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
bad = 0
t0 = time.time()
for case in range(cases):
    d = int(rng.choice([1, 63, 64, 65, 128, 300, 384, 385, 767, 768]))
    space = str(rng.choice(["cosine", "dot", "l2"] if d <= ops.L2_MAX_DIM else ["cosine", "dot"]))
    Q = int(rng.choice([1, 3, 17, 70]))
    N = int(rng.choice([1, 7, 300, 5000, 20000]))
    k = int(rng.choice([1, 10, 64, 65, 100, 1024]))
    form = str(rng.choice(["shared", "csr", "2d"]))
    dt = np.int32 if rng.random() < 0.5 else np.int64
    uniq = bool(rng.random() < 0.5)
    half = bool(rng.random() < 0.5)
    kind = str(rng.choice(["normal", "dups", "zeros"] + (["subnormal"] if half else [])))
    c = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    if kind == "subnormal":      # multiples of 2^-24 below the smallest normal half, and queries of that size
        c = (rng.integers(-1023, 1024, size=(N, d)) * 2.0 ** -24).astype(np.float32)
        q *= np.float32(2.0 ** -14)
    if kind == "dups":
        c[rng.choice(N, min(N, 300), replace=False)] = q[0]
    elif kind == "zeros":
        c[rng.choice(N, max(1, N // 10), replace=False)] = 0.0
        q[0] = 0.0

    def one_list():
        L = int(rng.choice([0, 1, k - 1, k, k + 1, 63, 64, 65, 1023, 1024, 1025, S - 1, S, S + 1, 2 * S + 1]))
        rows = rng.permutation(N)[:L] if rng.random() < 0.7 else rng.integers(0, N, L)          # distinct, or with repeats
        junk = rng.choice([-1, -5, N, N + 3, 2 ** 31 - 1], int(rng.choice([0, 0, 3]))).astype(np.int64)
        rows = np.concatenate([rows, junk])
        return rng.permutation(rows)

    if form == "shared":
        lists = [one_list()] * Q
        cand, lims = lists[0], None
    elif form == "csr":
        lists = [one_list() for _ in range(Q)]
        cand, lims = csr(lists)
    else:
        lists = [one_list() for _ in range(Q)]
        m = max(1, max(len(x) for x in lists))
        cand = np.full((Q, m), -1, dtype=np.int64)
        for j, x in enumerate(lists):
            cand[j, :len(x)] = x
        lims = None
    if half:
        c = c.astype(np.float16).astype(np.float32)      # the widened rows: what the oracle and the float32 op see
    rs, ri, rst = list_topk_ref(space, q, c, lists, k, idx_offset=11, unique=not uniq)
    qf, cf = torch.from_numpy(q).cuda(), torch.from_numpy(c).cuda()
    args = (torch.from_numpy(cand.astype(dt)).cuda(), None if lims is None else torch.from_numpy(lims).cuda())
    kw = dict(k=k, idx_offset=11, return_status=True, assume_unique=uniq)
    s, i, st = FN[space](qf, cf, *args, **kw)
    torch.cuda.synchronize()
    s, i, st = s.cpu().numpy(), i.cpu().numpy(), st.cpu().numpy()
    ok = same_bits(s, rs) and np.array_equal(i, ri) and np.array_equal(st, rst)
    if half:
        ld = d + int(rng.integers(0, 2))
        buf = torch.full((N, ld), float("nan"), dtype=torch.float16, device="cuda")
        buf[:, :d] = cf.half()
        hs, hi, hst = ops.f16_list_topk(space, qf, buf[:, :d], *args, **kw)
        torch.cuda.synchronize()
        ok = ok and same_bits(hs.cpu().numpy(), rs) and np.array_equal(hi.cpu().numpy(), ri) and np.array_equal(hst.cpu().numpy(), rst)
    bad += not ok
    print(f"case {case:3d} {space:6s} d={d:3d} Q={Q:3d} N={N:6d} k={k:4d} {form:6s} {np.dtype(dt).name:5s} unique={not uniq!s:5s} {kind:9s} {'f16' if half else 'f32'} "
          f"entries={sum(len(x) for x in lists) if form != 'shared' else len(cand):7d} {'ok' if ok else 'MISMATCH'}  ({time.time() - t0:.0f} s)",
          flush=True)
print(f"fuzz_list: {cases - bad}/{cases} cases exact")
sys.exit(1 if bad else 0)
