"""Helpers of tests/test_gpu_streams.py: work that keeps one stream busy for a known time, and the one protocol by which a call is run on a
side stream while the default stream is busy.  No tests here.

`Filler` queues bounded, ordinary torch work: `torch.mm(a, a, out=b)` on a private 2048 x 2048 float32 pair, one launch per unit, serial in
stream order.  One unit is timed once per session with events (median of 10 after a warm-up) and printed; `queue(stream, ms)` queues
ceil(ms / unit) units and refuses more than CAP_MS.

`run_on_side(call, warm_call)`:
 1. warm_call() on the default stream + torch.cuda.synchronize(), timed with perf_counter -> t_call.  Same shapes as `call`, other values: it
    builds plans, grows mapped / pinned buffers and lazy weights, so no first-time allocation lands in the measured call.
 2. torch.cuda.synchronize(): the inputs of `call` exist, the device is idle.
 3. The filler goes to the default stream: max(MIN_FILL_MS, R * t_call) ms, at most CAP_MS.
 4. Under a fresh torch.cuda.Stream(), with no wait_stream on the default stream, call() runs; what it returns stays alive.  (The stream is
    picked while the device is still idle, before step 3, among the fresh ones that do not share the default stream's HARDWARE queue:
    runs_beside_default.  One in four does, and waits for the filler whatever the call does.)
 5. side.synchronize(), and at once busy = not default_stream.query().
 6. Still under the side stream the results are copied to the host.
 7. Only then torch.cuda.synchronize() and the reference: the same call() on the default stream.
The side run comes before the reference run and the warm-up used other values, so no freed allocator block can already hold the right bytes.
`busy` shows that the filler outlasted the call and that the call neither waited for the default stream nor synchronised the device.
"""
import math
import time

import numpy as np
import torch

R = 12                  # filler length over t_call: 2 x the largest (side run with the filler queued) / t_call measured, 5.8
                        # (test_gpu_streams.py's docstring has the measurements)
MIN_FILL_MS = 50.0


class Filler:
    SIDE = 2048
    CAP_MS = 1000.0

    def __init__(self, unit_ms=None, device="cuda:0"):
        """`unit_ms`: the time of one unit when it is known (the host test injects it); None: measured on first use."""
        self.unit_ms = unit_ms
        self.device = device
        self._a = self._b = None

    def units(self, ms):
        if not 0 < ms <= self.CAP_MS:
            raise ValueError(f"filler of {ms} ms: expected 0 < ms <= {self.CAP_MS}")
        if self.unit_ms is None:
            self.measure()
        return max(1, math.ceil(ms / self.unit_ms))

    def _launch(self, n):
        if self._a is None:
            # every entry 1 / SIDE: a @ a is a again, so the chain neither overflows nor meets denormals
            self._a = torch.full((self.SIDE, self.SIDE), 1.0 / self.SIDE, device=self.device, dtype=torch.float32)
            self._b = torch.empty_like(self._a)
        for _ in range(n):
            torch.mm(self._a, self._a, out=self._b)

    def measure(self):
        self._launch(5)
        torch.cuda.synchronize()
        times = []
        for _ in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            self._launch(20)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / 20)
        self.unit_ms = float(np.median(times))
        print(f"stream_probe: one filler unit = {self.unit_ms:.4f} ms")
        return self.unit_ms

    def queue(self, stream, ms):
        """Queue ceil(ms / unit) units on `stream`; returns that count."""
        n = self.units(ms)
        with torch.cuda.stream(stream):
            self._launch(n)
        return n


_FILLER = None
TIMES = []              # (t_call ms, filler ms, time of the side run with the filler queued ms, busy) of every run_on_side


def filler():
    global _FILLER
    if _FILLER is None:
        _FILLER = Filler()
        _FILLER.measure()
    return _FILLER


_BESIDE = {}            # stream handle -> does the stream run beside a busy default stream?
PROBE_MS = 6.0


def runs_beside_default(stream):
    """The runtime maps streams onto a few hardware queues (four by default), and a stream that shares the default stream's queue starts
    its work only when the packets the default stream queued before it have been dispatched: it waits for the filler in hardware, whatever
    the call under test does.  Measured once per stream handle on an idle device (torch hands its pool of streams out again and again): one
    small kernel behind PROBE_MS of filler is done within half that time, or the stream shares the queue."""
    key = stream.cuda_stream
    if key not in _BESIDE:
        f = filler()
        x = torch.ones(1024, device=f.device)
        torch.cuda.synchronize()
        f.queue(torch.cuda.default_stream(), PROBE_MS)
        t0 = time.perf_counter()
        with torch.cuda.stream(stream):
            x.mul_(2.0)
            stream.synchronize()
        _BESIDE[key] = (time.perf_counter() - t0) * 1e3 < PROBE_MS / 2
        torch.cuda.synchronize()
    return _BESIDE[key]


def fresh_side_stream():
    """A fresh torch.cuda.Stream() that does not share the default stream's hardware queue (at most 64 are tried)."""
    for _ in range(64):
        stream = torch.cuda.Stream()
        if runs_beside_default(stream):
            return stream
    raise RuntimeError("no stream runs beside the default stream: every hardware queue is shared with it")


def to_host(x):
    """Tensors -> host tensors (a copy on the current stream), containers walked, everything else as it is."""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: to_host(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [to_host(v) for v in x]
    return x


def same(a, b):
    """Byte for byte: dtype, shape and bytes of tensors and arrays (NaN payloads included), == on everything else."""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        return (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape
                and a.contiguous().view(-1).view(torch.uint8).numpy().tobytes() == b.contiguous().view(-1).view(torch.uint8).numpy().tobytes())
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape
                and a.tobytes() == b.tobytes())
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and isinstance(b, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return a == b


def run_on_side(call, warm_call=None, t_call_ms=None, r=R):
    """-> (side results, reference results, busy), results on the host.  `warm_call` None: no warm-up, t_call_ms is given by hand."""
    f = filler()
    if warm_call is not None:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        warm_call()
        torch.cuda.synchronize()
        t_call_ms = (time.perf_counter() - t0) * 1e3
    side = fresh_side_stream()               # (chosen while the device is idle; nothing runs on it before the filler is queued)
    torch.cuda.synchronize()
    fill_ms = min(max(MIN_FILL_MS, r * t_call_ms), Filler.CAP_MS)
    f.queue(torch.cuda.default_stream(), fill_ms)
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        out = call()
        side.synchronize()
        busy = not torch.cuda.default_stream().query()
        t_side = (time.perf_counter() - t0) * 1e3
        got = to_host(out)
    torch.cuda.synchronize()
    ref = to_host(call())
    torch.cuda.synchronize()
    TIMES.append((t_call_ms, fill_ms, t_side, busy))
    return got, ref, busy
