"""The two contracts of include/tsim.h applied to the entries of include/tsim_graph_insert.h, in the manner of
tests/test_side_stream_gpu.py (whose Delay and helpers are reused): all work of a call is enqueued on the stream it is given,
and calls on different streams may overlap.  Neither entry takes a workspace, so there is nothing to poison; until the entries
move into tsim.h and the registry of tests/contract_cases.py their cases live here (tests/test_graph_insert_cpu.py checks that
the new header's entries are exactly the ones named below).

  default stream   the operand tensors hold the DECOY data and the case runs on them once; synchronise;
  side stream      a delay of at least 10 ms; copy_ the REAL data into the same tensors; run; clone the outputs.
A launch that left the side stream runs during the delay, on the decoy: the outputs are then not the restatement's.  The link
kernel updates its graph operand in place — the copy_ behind the delay restores it — and also runs on two streams at once over
two graphs, each stream's graph its own restatement's."""
import numpy as np
import pytest
import torch

import contract_cases as cases
import graph_insert_cases as gic
from contract_cases import Case, differs
from test_side_stream_gpu import _delayed_ms, _enqueue, delay  # noqa: F401  (delay: the module's fixture)
from text_similarity_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P_N, P_B, P_K0, P_R = 500, 300, 33, 16
L_N, L_D, L_R, L_T = 700, 24, 8, 300


def _prune_operands(which):
    rng = np.random.default_rng(410 + cases.WHICH.index(which))
    graph = rng.integers(-1, P_N, size=(P_N, P_R)).astype(np.int32)
    near = (rng.integers(0, P_N + P_B, size=(P_B, 1)) + rng.integers(0, 2 * P_K0, size=(P_B, P_K0))) % (P_N + P_B)
    cand = np.where(rng.random((P_B, P_K0)) < 0.9, near, rng.integers(-1, P_N + P_B + 2, size=(P_B, P_K0))).astype(np.int32)
    return {"cand": cand, "g": graph}


def _link_operands(which):
    rng = np.random.default_rng(420 + cases.WHICH.index(which))
    rows = rng.standard_normal((L_N, L_D)).astype(np.float32)
    graph = rng.integers(-1, L_N, size=(L_N, L_R)).astype(np.int32)
    targets = np.sort(rng.choice(L_N, size=L_T, replace=False)).astype(np.int32)
    lims = np.concatenate([[0], np.cumsum(rng.integers(0, 20, size=L_T))]).astype(np.int64)
    lims[-1] = 19 * L_T                                    # (one layout for real, decoy and other: the last list takes the slack)
    ids = rng.integers(0, L_N, size=19 * L_T).astype(np.int32)
    return {"c": rows, "g": graph, "targets": targets, "lims": lims, "ids": ids}


def _link_run(t):
    st = ops.graph_link_reverse("cosine", t["c"], t["g"], t["targets"], t["lims"], t["ids"])
    return t["g"], st


CASES = [
    Case("graph-insert-prune", ("tsim_graph_insert_prune",), _prune_operands,
         lambda t: ops.graph_insert_prune(t["cand"], t["g"], return_detours=True), lambda h: gic.insert_prune(h["cand"], h["g"]),
         decoy_rule="other", decoy_check=differs),
    Case("graph-link-reverse", ("tsim_graph_link_reverse",), _link_operands, _link_run,
         lambda h: gic.link_reverse("cosine", h["c"], h["g"], h["targets"], h["lims"], h["ids"]), decoy_rule="other",
         decoy_check=differs),
]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_all_work_is_enqueued_on_the_given_stream(case, delay, monkeypatch):
    device = torch.device(DEV)
    dev = cases.to_device(case.operands("decoy"), device)
    staged = cases.to_device(case.operands("real"), device)
    case.run(dev)                                          # the decoy's run on the default stream
    torch.cuda.synchronize()
    counts = cases.count_calls(monkeypatch, case.entries)
    want, decoy = case.oracle("real"), case.oracle("decoy")
    case.decoy_check(want, decoy)
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        ev, out = _enqueue(case, dev, staged, delay)
        busy = not side.query()
    side.synchronize()
    ms = _delayed_ms(ev)
    assert busy, f"the side stream was idle when run returned (delay {ms:.1f} ms): the op waited for the device"
    case.check(cases.outputs(out), want, "real")
    assert all(n == 1 for n in counts.values()), counts


def test_link_reverse_on_two_streams_at_once_over_two_graphs(delay):
    case = CASES[1]
    device = torch.device(DEV)
    stage = {w: cases.to_device(case.operands(w), device) for w in ("real", "other")}
    devs = [cases.to_device(case.operands("decoy"), device) for _ in range(2)]
    case.run(devs[0])
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device), torch.cuda.Stream(device)]
    got = []
    for s, d, w in zip(streams, devs, ("real", "other")):  # issue order: stream 1, then stream 2
        with torch.cuda.stream(s):
            got.append(_enqueue(case, d, stage[w], delay))
    for s in streams:
        s.synchronize()
    for (ev, out), w in zip(got, ("real", "other")):
        _delayed_ms(ev)
        case.check(cases.outputs(out), case.oracle(w), w)
    assert not all(cases.same(a, b) for a, b in zip(case.oracle("real"), case.oracle("other")))
