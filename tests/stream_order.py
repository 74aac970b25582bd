"""A caller's own stream as a hostile environment (a helper module next to guarded_alloc.py, imported by
test_gpu_guard_bands.py and test_gpu_stream_order.py only).

Every function of include/gsr.h takes the stream first and every Python wrapper hands in torch's current stream.  What
breaks that contract is silent on the default stream: a helper launch on stream 0, a memset or a readback that waits for
the wrong stream, a device-wide synchronisation in the glue, a missing event between the caller's stream and one of the
product's own.  `SideStream` makes each of them visible while a cell `fn(put)` runs:

  the default stream is blocked   Entry records an event on the default stream, enqueues one long `torch.cuda._sleep` on it
      and records `default_done` behind the sleep; the cell then runs under `torch.cuda.stream(S)` for a fresh non-blocking
      stream S.  `finish` brings the outputs to the host with copies on S, synchronises S ONLY and reads
      `default_done.query()`: the run is `conclusive` only if the default stream was still asleep when the outputs had
      reached the host.  Work the product put on the default stream has then not run (its results are missing: a mismatch
      against the unpatched run), and a wait for the default stream or the device has outlasted the sleep (not conclusive:
      a failure, not a skip).
  the inputs arrive late   `place(t)` allocates on S, fills the tensor with a decoy, enqueues a short sleep on S and only
      then copies the true value in, all from pinned memory without a host wait.  A kernel on any stream that is not
      ordered behind S reads the decoy.  Decoys stay inside the operation's valid domain (`decoy`): a floating tensor of two
      rows or more is its true rows rolled by one along dim 0; integer and bool tensors, scalars and single rows are the
      true value.  An early kernel then computes a valid, different result; nothing here can provoke a fault.

The platform's part, measured on the MI355X: a process opens 4 hardware queues, torch hands out its 32 pooled streams in
turn, and every fourth of them shares a hardware queue with the default stream -- work on such a stream waits for the
default stream's sleep (probed over 40 fresh streams: 32 ran underneath a 30 ms sleep, handles 6, 10, 14, ... of each 32 did
not).  `SideStream` therefore probes a fresh stream with a 1 ms sleep before it uses it and takes the next one where the
two serialise (`_vetted_stream`, verdict remembered per handle); eight in a row that serialise is an error.  The probe is
the precondition of test_gpu_stream_order.py in small.

Sizes.  `torch.cuda._sleep` spins for a number of cycles of the device's wall clock, calibrated once per process with two
events around a sleep: 2.40e6 cycles per millisecond on the MI355X (2.39e6 and 2.41e6 over 2 ms and 21 ms).  The sleep of
a cell is SLEEP_MULTIPLE = 4 times the wall time of the cell's first run under `three_runs` (which is under
GuardedAllocator and loads the code objects, so it is the cell's slowest), at least SLEEP_FLOOR_MS = 200 ms, at most
SLEEP_CAP_MS = 3000 ms.  `place` sleeps PLACE_SLEEP_MS = 1 ms on S: a kernel launch takes about 10 us, and the sleeps of
successive inputs add up on S while the host runs ahead (measured: an unordered kernel and an unordered copy, launched
right after `place` returned, both read the decoy).  On the MI355X the 56 cells of test_gpu_guard_bands.py take 0.3 to 16 ms
in their first run (165 to 738 ms in the four that load a code object), so 52 of them sleep the floor; their outputs are on
the host 1.1 to 41.5 ms after entry, about 1 ms per late input, and the sleep is 5.3 times that where the margin is
smallest (required: 2).  The cell times and windows are in that file's docstring; every run prints its own (`report`).

What it cannot see: a stray stream that happens to share a hardware queue with S runs in S's order and reads true values
(one stream in four); a stray wait shorter than the margin.  The warm-up leaves the right results in the blocks the timed
run gets back from the caching allocator: `run_cell` therefore takes an allocator context that fills the cell's buffers
anew (guarded_alloc.GuardedAllocator), without which a kernel that never ran can go unnoticed.
"""
import contextlib
import time

import numpy as np
import torch

SLEEP_MULTIPLE = 4.0
SLEEP_FLOOR_MS = 200.0
SLEEP_CAP_MS = 3000.0
PLACE_SLEEP_MS = 1.0
PROBE_SLEEP_MS = 1.0

_cycles_per_ms = {}
_concurrent = {}  # (device index, stream handle) -> ran underneath a sleep of the default stream


def cycles_per_ms(device=None):
    """`torch.cuda._sleep` cycles per millisecond on `device`, measured once per process (the larger of two runs of 1e7
    cycles: a run that had to wait for something reads low)."""
    dev = _device(device)
    if dev.index not in _cycles_per_ms:
        best = 0.0
        with torch.cuda.device(dev), torch.cuda.stream(torch.cuda.default_stream(dev)):
            torch.cuda._sleep(100000)  # (loads the kernel)
            for _ in range(2):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                torch.cuda._sleep(10000000)
                b.record()
                b.synchronize()
                best = max(best, 10000000 / a.elapsed_time(b))
        _cycles_per_ms[dev.index] = best
    return _cycles_per_ms[dev.index]


def sleep_ms_for(cell_seconds):
    """The default stream's sleep for a cell whose first run took `cell_seconds`."""
    return min(SLEEP_CAP_MS, max(SLEEP_FLOOR_MS, SLEEP_MULTIPLE * 1e3 * cell_seconds))


def _device(device=None):
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def decoy(t):
    """What an input holds before its true value arrives (module docstring): same dtype, shape and device, inside the
    domain of whatever reads it."""
    t = t.detach()
    if t.dim() == 0 or t.shape[0] < 2 or not t.dtype.is_floating_point:
        return t.clone()
    return torch.roll(t, 1, 0)


def _runs_underneath(stream, dev, blocked=None):
    """True if a tiny operation on `stream` completes while `blocked` (default: the default stream) sleeps for
    PROBE_SLEEP_MS."""
    torch.cuda.synchronize(dev)
    blocked = torch.cuda.default_stream(dev) if blocked is None else blocked
    with torch.cuda.stream(blocked):
        torch.cuda._sleep(int(PROBE_SLEEP_MS * cycles_per_ms(dev)))
    done = torch.cuda.Event()
    done.record(blocked)
    with torch.cuda.stream(stream):
        torch.ones(8, device=dev).mul_(2.0)
    stream.synchronize()
    underneath = not done.query()
    torch.cuda.synchronize(dev)
    return underneath


def _vetted_stream(dev):
    cycles_per_ms(dev)
    for _ in range(8):
        s = torch.cuda.Stream(dev)
        key = (dev.index, s.cuda_stream)
        if key not in _concurrent:
            _concurrent[key] = _runs_underneath(s, dev)
        if _concurrent[key]:
            return s
    raise RuntimeError("eight fresh streams in a row serialise with the default stream: the blocked-default half of SideStream "
                       "cannot be run on this platform")


class SideStream:
    """Context manager; see the module docstring.  `sleep_cycles`: the default stream's sleep.  The stream exists from
    construction, so that a cell can be warmed up on it (`warm_up`) before the window opens."""

    def __init__(self, sleep_cycles, device=None):
        self.device = _device(device)
        self.sleep_cycles = int(sleep_cycles)
        self.place_cycles = int(PLACE_SLEEP_MS * cycles_per_ms(self.device))
        self.stream = _vetted_stream(self.device)
        self.default_done = self.conclusive = self.window_ms = self.sleep_ms = None
        self.placed = 0
        self.decoy_placed = None
        self._late = True
        self._ctx = None

    def warm_up(self, fn, to_host):
        """One run of the cell on the stream, inputs through `place` without its sleeps, outputs brought to the host: the
        caching allocator's pool of this stream and the pinned host blocks then hold everything the timed run asks for."""
        self._late = False
        try:
            with torch.cuda.stream(self.stream):
                det, grads = fn(self.place)
                to_host(det), to_host(grads)
                self.stream.synchronize()
        finally:
            self._late = True
            self.placed = 0

    def __enter__(self):
        if self._ctx is not None:
            raise RuntimeError("SideStream is already active")
        dev = self.device
        torch.cuda.synchronize(dev)
        default = torch.cuda.default_stream(dev)
        self._started = torch.cuda.Event(enable_timing=True)
        self.default_done = torch.cuda.Event(enable_timing=True)
        self._started.record(default)
        with torch.cuda.stream(default):
            torch.cuda._sleep(self.sleep_cycles)
        self.default_done.record(default)
        self._t0 = time.perf_counter()
        self._ctx = torch.cuda.stream(self.stream)
        self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        ctx, self._ctx = self._ctx, None
        try:
            ctx.__exit__(*exc)
        finally:
            torch.cuda.synchronize(self.device)
        return False

    def place(self, tensor):
        """A copy of `tensor` on the device, allocated on the stream, that holds `decoy(tensor)` until a sleep of
        PLACE_SLEEP_MS on the stream has passed.  The host does not wait.  requires_grad is carried over (a leaf)."""
        t = tensor.detach()
        if t.numel() == 0:
            out = t.to(self.device).clone()
        else:
            with torch.cuda.stream(self.stream):
                true = t.contiguous().pin_memory().to(self.device, non_blocking=True)
                out = decoy(true)
                self.decoy_placed = torch.cuda.Event()  # (of the latest input: what test_gpu_stream_order.py orders its reader by)
                self.decoy_placed.record(self.stream)
                if self._late:
                    torch.cuda._sleep(self.place_cycles)
                out.copy_(true)
            self.placed += 1
        return out.requires_grad_(True) if tensor.requires_grad else out

    def finish(self, det, grads, to_host):
        """-> (to_host(det), to_host(grads)), copied on the stream; sets `conclusive`, `window_ms` (entry to outputs on the
        host) and `sleep_ms` (the default stream's sleep as its two events timed it)."""
        out = (to_host(det), to_host(grads))
        self.stream.synchronize()
        self.conclusive = not self.default_done.query()
        self.window_ms = (time.perf_counter() - self._t0) * 1e3
        torch.cuda.synchronize(self.device)
        self.sleep_ms = self._started.elapsed_time(self.default_done)
        return out


def host(d):
    """{name: tensor | number} -> {name: numpy array | number}; the copies run on the current stream."""
    out = {}
    for k, v in (d or {}).items():
        if isinstance(v, torch.Tensor):
            v = v.detach().cpu().contiguous()
            out[k] = v.view(torch.uint8).numpy() if v.dtype == torch.bool else v.numpy()
        else:
            out[k] = v
    return out


def same_bits(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return (isinstance(a, np.ndarray) and isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype
                and a.tobytes() == b.tobytes())
    return type(a) is type(b) and a == b


def run_cell(fn, sleep_ms, reset=None, to_host=host, allocator=contextlib.nullcontext):
    """One warm-up and one run of the cell `fn(put) -> (deterministic outputs, gradients | None)` under SideStream
    -> ((outputs, gradients) on the host, the SideStream).  `reset()`: called in front of either.  `allocator()`: a
    context either runs under -- guarded_alloc.GuardedAllocator with a finite pattern, so that the buffers the cell
    allocates are filled anew on its stream: the warm-up leaves the RIGHT results in the blocks the run gets back from the
    caching allocator, and a kernel that has not run when the outputs are read would otherwise go unnoticed."""
    side = SideStream(int(sleep_ms * cycles_per_ms()))
    if reset is not None:
        reset()
    with allocator():
        side.warm_up(fn, to_host)
    if reset is not None:
        reset()
    with allocator(), side:
        det, grads = fn(side.place)
        out = side.finish(det, grads, to_host)
    return out, side


def verdict(det, plain, side):
    """"mismatch: <name>" where a deterministic output of the stream run is not bit-identical to the unpatched run's,
    "not conclusive" where the outputs reached the host only after the default stream's sleep, else "clean"."""
    if det.keys() != plain.keys():
        return "mismatch: the outputs' names"
    for name in plain:
        if not same_bits(det[name], plain[name]):
            return f"mismatch: {name}"
    return "clean" if side.conclusive else "not conclusive"


def report(side):
    return (f"side stream {side.stream.cuda_stream:#x}: {side.placed} late inputs, outputs on the host after {side.window_ms:.1f} ms "
            f"of a {side.sleep_ms:.0f} ms sleep of the default stream ({side.sleep_ms / max(side.window_ms, 1e-3):.1f}x to spare), "
            + ("conclusive" if side.conclusive else "NOT conclusive"))
