"""All work of a call is enqueued on the stream it is given (include/tsim.h, "Every launch and async copy goes to `stream`").

Every other GPU test runs on the default stream, which would hide a launch that forgets its stream argument, a memset on the
null stream, a torch helper inside a composite op that escapes the current stream, or state shared between two streams.  Here
every case of tests/contract_cases.py runs on a side stream behind a delay:

  default stream   the operand tensors are filled with the DECOY data and the case is run on them once (this also loads the
                   kernels, and leaves the decoy's state in the default stream's workspace); synchronise;
  side stream      a delay of at least 10 ms; copy_ the REAL data into the same operand tensors; run; clone the outputs.

A launch that left the side stream runs during the delay: it reads decoy operands, or buffers nobody has produced yet, or writes
after the clone — the outputs are then not the oracle's.  The delay is measured with events around it in every test: below
10 ms the test errors, it never passes.  Where the Python op reads nothing back mid-call (host_sync False) the side stream
must still be busy when run returns.

Two streams at once (the cases that take a workspace): the real operands on one stream and the other operands on a second,
each behind its own delay; each stream's outputs are its own oracle's and ops._workspaces holds two distinct buffers.  The
encoder runs the same way on two handles, one a stream."""
import numpy as np
import pytest
import torch

import contract_cases as cases
from text_similarity_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIN_DELAY_MS, TARGET_DELAY_MS = 10.0, 25.0


class Delay:
    """Something that keeps a stream busy for TARGET_DELAY_MS: torch.cuda._sleep calibrated with events, or, where that is missing
    or does not delay, a chain of large matmuls."""

    def __init__(self, dev):
        self.dev, self.how, self.cycles, self.reps, self.cycles_per_ms = dev, None, 0, 0, None
        probe = 20_000_000
        ms = self._timed(lambda: torch.cuda._sleep(probe)) if hasattr(torch.cuda, "_sleep") else 0.0
        if ms >= 1.0:
            self.how, self.cycles_per_ms = "_sleep", probe / ms
            self.cycles = int(self.cycles_per_ms * TARGET_DELAY_MS)
        else:
            self.how = "matmul"
            self.a = torch.randn((4096, 4096), dtype=torch.float32, device=dev)
            self._timed(self._matmuls, 2)
            ms = self._timed(self._matmuls, 8) / 8
            self.reps = max(1, int(np.ceil(TARGET_DELAY_MS / max(ms, 1e-3))))
        print(f"delay: {self.how}, cycles per ms {self.cycles_per_ms}, cycles {self.cycles}, matmuls {self.reps}")

    def _matmuls(self, n):
        for _ in range(n):
            torch.mm(self.a, self.a)

    def _timed(self, fn, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn(*a)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def enqueue(self):
        """On the current stream; returns the two events around the delay."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if self.how == "_sleep":
            torch.cuda._sleep(self.cycles)
        else:
            self._matmuls(self.reps)
        e1.record()
        return e0, e1


@pytest.fixture(scope="module")
def delay():
    return Delay(torch.device(DEV))


def _delayed_ms(events):
    ms = events[0].elapsed_time(events[1])
    if ms < MIN_DELAY_MS:
        raise RuntimeError(f"the delay lasted {ms:.2f} ms < {MIN_DELAY_MS} ms: the run proves nothing")
    return ms


def _enqueue(case, dev, staged, delay):
    """On the current (side) stream: delay, copy the staged data into the operands, run, clone the outputs."""
    ev = delay.enqueue()
    result = case.run(cases.copy_into(dev, staged))
    result = result if isinstance(result, (tuple, list)) else (result,)
    return ev, tuple(t.clone() for t in result)


@pytest.mark.parametrize("case", cases.CASES, ids=repr)
def test_all_work_is_enqueued_on_the_given_stream(case, delay, monkeypatch):
    device = torch.device(DEV)
    dev = cases.to_device(case.operands("decoy"), device)
    staged = cases.to_device(case.operands("real"), device)
    case.run(dev)                                          # the decoy's run on the default stream
    torch.cuda.synchronize()
    counts = cases.count_calls(monkeypatch, case.entries)
    want = case.oracle("real")
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        ev, out = _enqueue(case, dev, staged, delay)
        busy = not side.query()
        done = torch.cuda.Event()
        done.record()
    side.synchronize()
    assert done.query()
    ms = _delayed_ms(ev)
    if not case.host_sync:
        assert busy, f"the side stream was idle when run returned (delay {ms:.1f} ms): the op waited for the device"
    ops._workspaces.pop((device.index, side.cuda_stream), None)   # (keyed by a pooled stream handle: leave none for a later stream)
    case.check(cases.outputs(out), want, "real")
    missed = [e for e, n in counts.items() if n == 0]
    assert not missed, f"never called: {missed}"


@pytest.mark.parametrize("case", cases.WORKSPACE_CASES, ids=repr)
def test_two_streams_at_once(case, delay):
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
    bufs = [ops._workspaces.get((device.index, s.cuda_stream)) for s in streams]
    assert bufs[0] is not None and bufs[1] is not None and bufs[0] is not bufs[1]
    assert bufs[0].data_ptr() != bufs[1].data_ptr()
    for s in streams:                                      # (the cache is keyed by stream handle: leave none behind for a later stream)
        ops._workspaces.pop((device.index, s.cuda_stream), None)


@pytest.mark.parametrize("case", cases.TWO_HANDLE_CASES, ids=repr)
def test_two_encoder_handles_on_two_streams(case, delay, monkeypatch):
    """Two handles of one preset (separate activation buffers, as tools/concurrency_probe.py makes them), the real tokens on one
    stream and the other tokens on a second, each behind its own delay: each stream's rows are its own oracle's."""
    device = torch.device(DEV)
    stage = {w: cases.to_device(case.operands(w), device) for w in ("real", "other")}
    devs = [cases.to_device(case.operands("decoy"), device) for _ in range(2)]
    for slot in (0, 1):                                    # both handles made and run once on the default stream
        monkeypatch.setattr(cases, "ENC_SLOT", slot)
        case.run(devs[slot])
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device), torch.cuda.Stream(device)]
    got = []
    for slot, (s, w) in enumerate(zip(streams, ("real", "other"))):
        monkeypatch.setattr(cases, "ENC_SLOT", slot)
        with torch.cuda.stream(s):
            got.append(_enqueue(case, devs[slot], stage[w], delay))
            assert not s.query()
    for s in streams:
        s.synchronize()
    for (ev, out), w in zip(got, ("real", "other")):
        _delayed_ms(ev)
        case.check(cases.outputs(out), case.oracle(w), w)


def test_workspace_cache_is_per_stream():
    device = torch.device(DEV)
    s1, s2 = torch.cuda.Stream(device), torch.cuda.Stream(device)
    with torch.cuda.stream(s1):
        a = ops._workspace(device, 1000)
        assert ops._workspace(device, 2000) is a           # the same stream reuses the buffer ...
        b = ops._workspace(device, a.numel() + 1)
        assert b is not a and b.numel() > a.numel()        # ... a larger request replaces it ...
        assert ops._workspace(device, 1000) is b
    with torch.cuda.stream(s2):
        c = ops._workspace(device, 1000)
    assert c is not b and c.data_ptr() != b.data_ptr()     # ... and another stream gets another buffer
    assert ops._workspaces[(device.index, s1.cuda_stream)] is b and ops._workspaces[(device.index, s2.cuda_stream)] is c
    for s in (s1, s2):
        ops._workspaces.pop((device.index, s.cuda_stream), None)
