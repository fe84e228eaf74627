"""The encoder kernels against the float64 probe oracle (oracle/encoder_probe.py) on the cases of tests/encoder_cases.py:
weights under which attention, the relative-position bias, every projection bias and the LayerNorms all move the output,
packed batches at the lengths where kernels go wrong, hidden states checked after EVERY layer (an encoder built from the
first l layers, l = 1..L) in two metrics, per token.

The tolerance is not typed in: TOL = 2 x floor, floor = the error of the probe's bf16 emulation against the exact probe
on the same inputs, computed at test time (encoder_cases.tolerances).  tests/test_encoder_power_cpu.py proves that every
named defect (wrong softmax scale, a swapped or shifted relative bias, a leaked or dropped key, a missing bias, a wrong
position row, the other architecture's LayerNorm eps, ...) lies at >= 4 x TOL, so a kernel with one of them fails here.

Each test is one forward per encoder handle.  Run the file under a time limit of its own, for instance
``timeout -k 10 900 python -m pytest tests/test_encoder_sharp_gpu.py -q -m gpu -s``."""
from dataclasses import replace

import numpy as np
import pytest
import torch

import encoder_cases as ec
from text_similarity_amd import presets
from text_similarity_amd.native_encoder import NativeEncoder

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def compare(label, got, ref, floor, tol, cu=None):
    """Print measured error next to floor and TOL; on a miss name the worst token (sequence, column) and feature."""
    e = ec.errors(got, ref)
    print(f"{label}: " + "  ".join(f"{m} measured {e[m]:.4g} floor {floor[m]:.4g} TOL {tol[m]:.4g}" for m in ec.METRICS))
    assert np.isfinite(got).all(), f"{label}: non-finite output"
    for m in ec.METRICS:
        if e[m] > tol[m]:
            d = np.abs(np.asarray(got, dtype=np.float64) - ref)
            t = int(ec.row_rel(got, ref).argmax()) if m == "row_rel" else int(d.max(1).argmax())
            f = int(d[t].argmax())
            where = f"row {t}"
            if cu is not None:
                s = int(np.searchsorted(cu, t, side="right") - 1)
                where = f"token {t} = sequence {s} (length {int(cu[s + 1] - cu[s])}) column {t - int(cu[s])}"
            raise AssertionError(f"{label}: {m} {e[m]:.4g} > TOL {tol[m]:.4g} (floor {floor[m]:.4g}); worst at {where}, "
                                 f"feature {f}: got {float(got[t, f]):.5g}, reference {float(ref[t, f]):.5g}")


@pytest.mark.parametrize("name", list(ec.CASES))
def test_hidden_states_after_every_layer(name):
    cfg, wdtype = ec.CASES[name]
    ids, cu, notes = ec.case_inputs(name)
    w = ec.sharp_weights(cfg, name)
    exact, floor, tol = ec.tolerances(name)
    fd, cd = torch.from_numpy(ids.copy()).to(DEV), torch.from_numpy(cu.astype(np.int32)).to(DEV)
    empty = np.diff(cu) == 0
    assert empty.any()
    for l in range(1, cfg.num_layers + 1):      # the first boundary that misses is the layer that is wrong
        enc = NativeEncoder(replace(cfg, num_layers=l), w, max_tokens=ids.size, max_seqs=cu.size - 1, weight_dtype=wdtype)
        r = enc.forward_packed(fd, cd, pooled=True, unit=True, hidden=True)
        torch.cuda.synchronize()
        enc.check()
        h = r["hidden"].float().cpu().numpy()
        p = r["pooled"].cpu().numpy()
        assert (p[empty] == 0).all() and (r["unit"].float().cpu().numpy()[empty] == 0).all()
        compare(f"{name} boundary {l}", h, exact[l], floor[l], tol[l], cu)
        if l == cfg.num_layers:
            compare(f"{name} pooled", p, ec.pooled_rows(exact[l], cu), floor["pooled"], tol["pooled"])
        del enc


@pytest.mark.parametrize("n", [2300, 4700])
def test_hidden_384_layernorm_gemm_routes_are_right(n):
    """The hidden-384 layer picks its LayerNorm GEMM route by token count (test_encoder_gpu.py::
    test_large_batch_equals_small_batches_bitwise names them: 2300 sentences = ln_rows_gemm + ln_tail_gemm, 4700 = one
    ln_rows_gemm round + the 64-token remainder launch).  That the routes agree bit for bit is tested there; here 48-sentence
    slices of ONE large call are compared with the probe, under weights with large gammas and residuals and the TOL of the
    bert-384 case."""
    name = "bert-384"
    cfg, wdtype = ec.CASES[name]
    w = ec.sharp_weights(cfg, name)
    _, floor, tol = ec.tolerances(name)
    L = cfg.num_layers
    flat, cu = presets.synthetic_token_batch(n, seed="sharp/route", vocab_size=ec.VOCAB, max_len=64)
    cu = cu.astype(np.int64)
    enc = NativeEncoder(cfg, w, max_tokens=int(cu[-1]), max_seqs=n, weight_dtype=wdtype)
    r = enc.forward_packed(torch.from_numpy(flat).to(DEV), torch.from_numpy(cu.astype(np.int32)).to(DEV), pooled=True, hidden=True)
    torch.cuda.synchronize()
    enc.check()
    h, p = r["hidden"].float().cpu().numpy(), r["pooled"].cpu().numpy()
    assert np.isfinite(h).all() and np.isfinite(p).all()
    for s in sorted({0, 480, 1452, n - 48}):
        a, b = int(cu[s]), int(cu[s + 48])
        c = cu[s:s + 49] - cu[s]
        ref = ec.probe(name, w, ids=flat[a:b], cu=c)[L]
        compare(f"{name} n={n} rows {s}..{s + 47} hidden", h[a:b], ref, floor[L], tol[L], c)
        compare(f"{name} n={n} rows {s}..{s + 47} pooled", p[s:s + 48], ec.pooled_rows(ref, c), floor["pooled"], tol["pooled"])
