"""A bounded delay on a stream, and a section runner that keeps the device behind the host (test infrastructure).

The suite's kernels finish in microseconds, so an ordering mechanism of the library -- an event wait, a copy on the right stream, a
synchronize() -- is executed by every GPU test and verified by none: the work it orders has long finished.  The helpers here put the
device behind on purpose, for a bounded time, so that a call issued now runs later and a missing wait shows as wrong values.

  gate(stream, ms)        enqueue a delay of about `ms` milliseconds on `stream` (torch.cuda._sleep, cycles calibrated once per process;
                          a chain of torch.mm where _sleep is missing) and return an event recorded directly behind it.  ms > MAX_MS is
                          refused; nothing here waits for a flag the host sets, so a test that dies leaves nothing spinning.
  behind(stream, ms)      a Section: sync the device, launch the gate, then hand every input its real values BEHIND the gate (late()).
  Section.still_gated()   the premise of an asynchronous section, a condition and not a measurement: true after the last call returned =
                          the calls were queued while the device was behind AND none of them waited on the host.

A Section has two modes, so that ONE body of code produces the quiet reference and the gated run:
  "quiet"   every input is ready before the first call and step() synchronises after every call (the twin, and the warm-up);
  "gated"   inputs start as poison (NaN / 0xA5), get their values behind the gate, step() does nothing, finish() synchronises once.
Outputs are pre-filled with a sentinel in both.  The pure logic (arithmetic, refusal, poison / sentinel makers) needs no GPU and is what
tests/test_async_gate_cpu.py covers.
"""
import numpy as np

MAX_MS = 250.0
START_MS = 50.0
CAL_CYCLES = 5_000_000       # one _sleep of this many cycles is timed between two events on an idle stream
POISON_BYTE = 0xA5
SENTINEL_F32 = -12345.0      # no engine output takes this value on the test inputs
SENTINEL_BYTE = 0x5A

_CAL = {}                    # "cycles_per_ms", "realised_ms" (of the calibration sleep), "unit" ("cycles" / "mm")


def cycles_per_ms(cycles, elapsed_ms):
    """calibration arithmetic: units of delay per millisecond from one timed delay"""
    if not (cycles > 0 and elapsed_ms > 0.0):
        raise ValueError("calibration needs a positive count and a positive time")
    return cycles / elapsed_ms


def units_for(ms, per_ms):
    """units of delay for `ms` milliseconds; refuses delays above MAX_MS (and non-positive ones)"""
    if not (0.0 < ms <= MAX_MS):
        raise ValueError("gate: a delay of %r ms is refused (0 < ms <= %g)" % (ms, MAX_MS))
    return max(1, int(round(ms * per_ms)))


def poison_like(a):
    """numpy array shaped and typed like `a`: NaN for floats, bytes 0xA5 for everything else"""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        return np.full(a.shape, np.nan, a.dtype)
    return np.frombuffer(bytes([POISON_BYTE]) * a.nbytes, a.dtype).reshape(a.shape).copy()


def sentinel(shape, dtype):
    """numpy array of the sentinel an output holds before its call: -12345 for floats, bytes 0x5A for everything else"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return np.full(shape, SENTINEL_F32, dtype)
    n = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    return np.frombuffer(bytes([SENTINEL_BYTE]) * n, dtype).reshape(shape).copy()


# ---------------------------------------------------------------- the device part (torch imported on use)
def _delay(stream, units):
    import torch
    with torch.cuda.stream(stream):
        if _CAL["unit"] == "cycles":
            torch.cuda._sleep(int(units))
        else:
            a = _CAL["mm"]
            for _ in range(int(units)):
                torch.mm(a, a, out=_CAL["mm_out"])


def calibrate(device="cuda:0"):
    """once per process: time one delay of a fixed count between two events on an idle stream; prints what it found"""
    if "cycles_per_ms" in _CAL:
        return _CAL
    import torch
    if hasattr(torch.cuda, "_sleep"):
        _CAL["unit"], count = "cycles", CAL_CYCLES
    else:
        _CAL["unit"], count = "mm", 64
        _CAL["mm"] = torch.ones((1024, 1024), device=device)
        _CAL["mm_out"] = torch.empty((1024, 1024), device=device)
    s = torch.cuda.Stream(device)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    _delay(s, count if _CAL["unit"] == "mm" else 1000)   # first use: code objects loaded, clocks up
    torch.cuda.synchronize(device)
    with torch.cuda.stream(s):
        e0.record(s)
    _delay(s, count)
    with torch.cuda.stream(s):
        e1.record(s)
    e1.synchronize()
    ms = e0.elapsed_time(e1)
    _CAL["cycles_per_ms"] = cycles_per_ms(count, ms)
    _CAL["realised_ms"] = ms
    print("async_gate: %s per ms = %.1f (one delay of %d took %.2f ms)" % (_CAL["unit"], _CAL["cycles_per_ms"], count, ms))
    return _CAL


def gate(stream, ms):
    """enqueue a delay of about `ms` milliseconds on `stream`; returns a torch event recorded directly behind it"""
    import torch
    units = units_for(ms, calibrate(stream.device)["cycles_per_ms"])
    _delay(stream, units)
    ev = torch.cuda.Event()
    with torch.cuda.stream(stream):
        ev.record(stream)
    return ev


class Section:
    """one gated (or quiet) section on `stream`: declare inputs and outputs, start(), issue calls, finish()"""

    def __init__(self, stream, ms=START_MS, mode="gated", name=""):
        if mode not in ("gated", "quiet"):
            raise ValueError(mode)
        units_for(ms, 1.0)   # the refusal, before anything is queued
        self.stream, self.ms, self.mode, self.name = stream, ms, mode, name
        self._late, self._event, self.started = [], None, False

    @property
    def gated(self):
        return self.mode == "gated"

    # -- declared before start()
    def inp(self, array):
        """device tensor for a numpy input: its values when quiet; poison now and the values behind the gate when gated"""
        import torch
        assert not self.started, "inputs are declared before the gate"
        a = np.ascontiguousarray(array)
        with torch.cuda.stream(self.stream):
            real = torch.from_numpy(a).to(self.stream.device)
            if not self.gated:
                return real
            dst = torch.from_numpy(poison_like(a)).to(self.stream.device)
        self._late.append((dst, real))
        return dst

    def out(self, shape, dtype=np.float32):
        """device tensor pre-filled with the sentinel"""
        import torch
        assert not self.started, "outputs are allocated before the gate"
        with torch.cuda.stream(self.stream):
            return torch.from_numpy(sentinel(tuple(shape), dtype)).to(self.stream.device)

    # -- the section
    def start(self, sync=True):
        """sync=False: a second section started next to one that is already gated (its device sync would wait that gate out)"""
        import torch
        if sync:
            torch.cuda.synchronize(self.stream.device)
        self.started = True
        if self.gated:
            self._event = gate(self.stream, self.ms)
            for dst, src in self._late:
                self.late(dst, src)
        return self

    def late(self, dst, src):
        """dst.copy_(src) on the section's stream: behind the gate"""
        import torch
        with torch.cuda.stream(self.stream):
            dst.copy_(src, non_blocking=True)

    def regate(self, stream=None, ms=None):
        """a further gate, on `stream` (default: the section's): the premise then refers to it"""
        self._event = gate(stream or self.stream, self.ms if ms is None else ms)

    def still_gated(self):
        return self._event is not None and not self._event.query()

    def premise(self, what=""):
        """asserted by sections made only of calls that must not wait; never skipped: a delay that was too short fails here"""
        if self.gated:
            assert self.still_gated(), ("section %r %s: the gate of %g ms had passed when the last call returned -- a call waited on the "
                                        "host, or issuing took longer than the delay" % (self.name, what, self.ms))

    def step(self):
        """after every call: the quiet twin synchronises, the gated run goes on"""
        if not self.gated:
            self.stream.synchronize()

    def finish(self):
        self.stream.synchronize()


def behind(stream, ms=START_MS, name=""):
    """a gated Section on `stream` (call start() once inputs and outputs are declared)"""
    return Section(stream, ms, "gated", name)
