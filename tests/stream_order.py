"""Helpers of tests/test_stream_gpu.py and tests/test_contexts_gpu.py: one engine call made in
stream order behind a timed gate, so that work the engine does off the caller's stream gives a
wrong answer every time, not only when a race is lost.

A gated call (`gated`):

  warm      the same call with the same sizes on the side stream, then a sync, twice: lazy
            initialisation and scratch growth (and their host syncs) happen in the first; the
            host wall time of the second one's enqueue, the steady state, sizes the gate
  decoys    every device input then holds a decoy: another valid input of the same length (other
            sources, another permutation of the targets, other weights), never out of range, so
            that an early reader computes a wrong row and never faults; the outputs hold the
            canary of tests/test_contract_gpu.py
  gate      on the side stream: a timed device-side delay (torch.cuda._sleep; never a kernel
            that waits for the host), the copies of the true inputs from device staging
            buffers, then the event `opened`
  call      the engine call on the side stream, the outputs set back to the canary in stream
            order, and the call again (it starts from the counters and flags the first one
            leaves, which a reset that ran early on another stream does not cover); `opened`
            must not have fired when the second returns: both returned after enqueueing, and
            whatever they put on another stream or read on the host saw the decoys
  snapshot  on the side stream: the outputs copied to snapshot buffers, the decoys written back
            over the inputs, then shd_route_sync(side)
  compare   by the caller, on the snapshots; shd_route_sync reports a failed entry once

The gate is ten times the warm call's enqueue time, 20 ms at least (host jitter on a shared
machine); the delay primitive is timed with events once per process (`cycles_per_ms`).  A gate
found open on return is tried once more at four times the length; open again fails the test.
"""
from __future__ import annotations

import time

import numpy as np

from tests.test_contract_gpu import Padded

GATE_FLOOR_MS = 20.0
GATE_FACTOR = 10.0

# (label, warm enqueue ms, gate ms used, tries) of every gated call of the process
MEASURED: list = []
_CPM: list = []


def dev():
    import torch
    return torch.device("cuda", 0)


def cycles_per_ms() -> float:
    """torch.cuda._sleep cycles per millisecond, measured with events on a side stream."""
    import torch
    if _CPM:
        return _CPM[0]
    s = torch.cuda.Stream()
    n = 2_000_000
    for _ in range(8):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record(s)
            torch.cuda._sleep(n)
            e1.record(s)
        s.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 10.0:
            _CPM.append(n / ms)
            print(f"stream_order: torch.cuda._sleep {n} cycles = {ms:.2f} ms ({n / ms:.0f} cycles/ms)")
            return _CPM[0]
        n *= 4
    raise AssertionError(f"torch.cuda._sleep({n // 4}) took only {ms} ms: no usable gate")


class In:
    """A device input: `t` is the tensor the engine reads (a decoy between calls), `true` and
    `decoy` device staging copies of the two contents.  `into`: an existing device tensor to
    use as `t` (an output that is also read, e.g. an accumulator or fw_async's matrix)."""

    def __init__(self, true, decoy, into=None):
        import torch
        true, decoy = np.ascontiguousarray(true), np.ascontiguousarray(decoy)
        assert true.shape == decoy.shape and true.dtype == decoy.dtype
        assert true.size == 0 or not np.array_equal(true.view(np.uint8), decoy.view(np.uint8)), "decoy equals the input"
        conv = (lambda a: a.view(np.int64)) if true.dtype == np.uint64 else (lambda a: a)
        self.true = torch.from_numpy(conv(true)).to(dev())
        self.decoy = torch.from_numpy(conv(decoy)).to(dev())
        if into is None:
            self.t = self.decoy.clone()
        else:
            assert into.shape == self.true.shape and into.dtype == self.true.dtype
            self.t = into
            self.t.copy_(self.decoy)


class Out(Padded):
    """An output of tests/test_contract_gpu.py (canary body and guards) with a snapshot buffer."""

    def __init__(self, ns, ld, i32=False, i64=False):
        import torch
        super().__init__(ns, ld, i32=i32)
        self.snap = torch.zeros_like(self.big)
        if i64:
            self.t = self.big[self.off: self.off + ns * ld].view(ns, ld)

    def reset(self):
        self.big.fill_(self.can)

    def snap_bits(self, nt):
        """The nt written columns of the snapshot as integers; nothing else may have changed."""
        b = self.snap.cpu().numpy()
        assert np.all(b[: self.off] == self.can) and np.all(b[self.off + self.ns * self.ld:] == self.can)
        body = b[self.off: self.off + self.ns * self.ld].reshape(self.ns, self.ld)
        assert np.all(body[:, nt:] == self.can)
        return body[:, :nt].copy()

    def f64(self, nt):
        return self.snap_bits(nt).view(np.float64)


class Out16:
    """`count` 16-bit outputs between guards (the u16 payload of shd_route_tri_payload_async)."""
    can = 0x5EAD

    def __init__(self, count):
        import torch
        from tests.test_contract_gpu import GUARD
        self.off, self.count = GUARD, count
        self.big = torch.full((GUARD + count + GUARD,), self.can, dtype=torch.int16, device=dev())
        self.t = self.big[GUARD: GUARD + count]
        self.snap = torch.zeros_like(self.big)

    def reset(self):
        self.big.fill_(self.can)

    def u16(self):
        b = self.snap.cpu().numpy()
        assert np.all(b[: self.off] == self.can) and np.all(b[self.off + self.count:] == self.can)
        return b[self.off: self.off + self.count].view(np.uint16).copy()


def sync_code(route, eng, stream=None):
    try:
        eng.sync(stream)
        return route.OK
    except route.RouteError as e:
        return e.code


def gated(route, eng, ins, outs, call, label, accum=()):
    """One call in stream order (module docstring).  ins: In objects; outs: Out objects, reset to
    the canary before the gated call; accum: In objects whose tensor lies inside an Out (set
    after the reset); call(stream handle) makes the engine call.  Returns shd_route_sync's code;
    the results are in the Outs' snapshots."""
    import torch
    side = torch.cuda.Stream()
    sh = side.cuda_stream
    # warm: the true inputs, the same sizes
    for o in outs:
        o.reset()
    for i in list(ins) + list(accum):
        i.t.copy_(i.true)
    torch.cuda.synchronize()
    call(sh)                                  # (pays the lazy steps and the scratch growth)
    sync_code(route, eng, sh)
    t0 = time.perf_counter()
    call(sh)                                  # the warm call that is timed: the steady state
    enq_ms = (time.perf_counter() - t0) * 1e3
    sync_code(route, eng, sh)
    assert sync_code(route, eng, sh) == route.OK
    gate_ms = max(GATE_FLOOR_MS, GATE_FACTOR * enq_ms)
    cpm = cycles_per_ms()
    for attempt in (1, 2):
        for o in outs:
            o.reset()
        for i in list(ins) + list(accum):
            i.t.copy_(i.decoy)
        torch.cuda.synchronize()
        opened = torch.cuda.Event()
        with torch.cuda.stream(side):
            torch.cuda._sleep(int(gate_ms * cpm))
            for i in list(ins) + list(accum):
                i.t.copy_(i.true, non_blocking=True)
            opened.record(side)
        call(sh)
        # once more behind the same gate, the outputs back to the canary in stream order: the
        # second call starts from the state the first one leaves behind (work-queue counters,
        # flags, parked error words), and a reset that ran early does not cover it
        with torch.cuda.stream(side):
            for o in outs:
                o.reset()
            for i in accum:
                i.t.copy_(i.true, non_blocking=True)
        call(sh)
        shut = not opened.query()
        with torch.cuda.stream(side):
            for o in outs:
                o.snap.copy_(o.big, non_blocking=True)
            for i in ins:
                i.t.copy_(i.decoy, non_blocking=True)
        code = sync_code(route, eng, sh)
        MEASURED.append((label, round(enq_ms, 3), round(gate_ms, 1), attempt))
        print(f"gated {label}: warm enqueue {enq_ms:.3f} ms, gate {gate_ms:.1f} ms, try {attempt}, "
              f"{'shut' if shut else 'OPEN'} on return")
        if shut:
            break
        gate_ms *= 4
    assert shut, f"{label}: the call returned after its {gate_ms / 4:.0f} ms gate had opened, twice"
    assert sync_code(route, eng, sh) == route.OK, "a failed entry is reported once"
    assert sync_code(route, eng) == route.OK
    return code


def rows_differ(a, b):
    """Every row of a differs from the same row of b somewhere (bitwise, NaN = NaN)."""
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    ai = a.view(np.int64 if a.dtype.itemsize == 8 else np.int32).reshape(a.shape[0], -1)
    bi = b.view(np.int64 if b.dtype.itemsize == 8 else np.int32).reshape(b.shape[0], -1)
    return bool(np.all((ai != bi).any(axis=1)))


def decoy_sources(S):
    """The source list rotated by one: position i holds another source (the test asserts it)."""
    S = np.asarray(S, np.int32)
    D = np.roll(S, -1)
    assert np.all(D != S)
    return D


def decoy_targets(T, seed=1):
    """A permutation of the target list that moves every position."""
    T = np.asarray(T, np.int32)
    if len(T) < 2:
        return T.copy()
    k = 1 + np.random.default_rng(seed).integers(0, len(T) - 1)
    D = np.roll(T, int(k))
    return D
