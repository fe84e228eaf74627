#!/usr/bin/env python3
"""Randomised parity sweep of the inverted-list scan (ops.ivf_scan_topk) against the oracle of tests/ivf_cases.py: scores
(float32 bits), ids and status words must be identical.  Every case draws a space, a width, Q, nlist, nprobe, k, the list
lengths (around the wave, the LDS block and TSIM_IVF_SEG), a permutation for the ids with tombstones sprinkled in, probes with
padding, repeats and list numbers beyond nlist, a sizing hint that may be far too small, and now and then duplicate rows, zero
rows or list offsets that are out of order.
Usage: python tools/fuzz_ivf.py [cases] [seed]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch
from ivf_cases import ST_OFF, arrival_from_packed, clean_offsets, ivf_ref
from list_cases import header_define, same_bits
from text_similarity_amd import ops

SEG = header_define("TSIM_IVF_SEG")
cases = int(sys.argv[1]) if len(sys.argv) > 1 else 24
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 0)
bad = 0
t0 = time.time()
for case in range(cases):
    d = int(rng.choice([1, 63, 64, 65, 128, 300, 384, 385, 767, 768]))
    space = str(rng.choice(["cosine", "dot", "l2"] if d <= ops.L2_MAX_DIM else ["cosine", "dot"]))
    Q = int(rng.choice([1, 3, 17, 70]))
    nlist = int(rng.choice([1, 2, 7, 40]))
    nprobe = int(rng.choice([1, 2, 5, 12]))
    k = int(rng.choice([1, 10, 64, 65, 100, 1024]))
    kind = str(rng.choice(["normal", "dups", "zeros", "badoff"]))
    lens = rng.choice([0, 1, 63, 64, 65, 300, 1023, 1024, 1025, SEG - 1, SEG, SEG + 1, 2 * SEG + 1], nlist)
    if lens.sum() == 0:
        lens[0] = 5
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    N = int(off[-1])
    packed = rng.standard_normal((N, d)).astype(np.float32)
    q = rng.standard_normal((Q, d)).astype(np.float32)
    if kind == "dups":
        packed[rng.choice(N, min(N, 300), replace=False)] = q[0]
    elif kind == "zeros":
        packed[rng.choice(N, max(1, N // 10), replace=False)] = 0.0
        q[0] = 0.0
    elif kind == "badoff" and nlist > 1:
        j = rng.choice(nlist + 1, 2)
        off[j[0]], off[j[1]] = int(rng.choice([-3, N + 9, off[j[1]]])), off[j[0]]
    ids = rng.permutation(N).astype(np.int32)
    ids[rng.random(N) < 0.1] *= -1          # tombstones (id 0 stays live)
    probes = rng.integers(0, nlist, (Q, nprobe))
    junk = rng.random((Q, nprobe))
    probes[junk < 0.1] = -1
    probes[junk > 0.95] = nlist + int(rng.integers(0, 3))
    hint = None if rng.random() < 0.3 else int(rng.choice([0, 1, SEG, int(lens.max()), 10 ** 7]))
    clean = clean_offsets(off, N)
    rows, ln = arrival_from_packed(packed, clean, ids)
    rs, ri, rst = ivf_ref(space, q, rows, ln, probes, k, idx_offset=11, nlist=nlist)
    changed = [bool(clean[l] != off[l] or clean[l + 1] != off[l + 1]) for l in range(nlist)]
    rst = rst | np.array([ST_OFF if any(changed[l] for l in p if 0 <= l < nlist) else 0 for p in probes], dtype=np.int32)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    s, i, st = ops.ivf_scan_topk(space, dev(q), dev(packed), dev(off), dev(ids), dev(probes.astype(np.int64)), k, idx_offset=11,
                                 return_status=True, max_list_len=hint)
    torch.cuda.synchronize()
    s, i, st = s.cpu().numpy(), i.cpu().numpy(), st.cpu().numpy()
    ok = same_bits(s, rs) and np.array_equal(i, ri) and np.array_equal(st, rst)
    bad += not ok
    print(f"case {case:3d} {space:6s} d={d:3d} Q={Q:3d} nlist={nlist:3d} nprobe={nprobe:3d} k={k:4d} N={N:6d} hint={hint!s:8s} {kind:6s} "
          f"{'ok' if ok else 'MISMATCH'}  ({time.time() - t0:.0f} s)", flush=True)
print(f"fuzz_ivf: {cases - bad}/{cases} cases exact")
sys.exit(1 if bad else 0)
