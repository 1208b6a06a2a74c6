"""WHEN an entry point reads and writes: the stream harness of tests/test_gpu_stream_*.py.

The parity tests hold VALUES, tests/arena.py holds WHERE; both run every call on the default stream and synchronise the device
afterwards, so a launcher that drops its `stream` argument, puts one of two launches on stream 0, waits, or reads a host
argument after it has returned passes them all.  include/sdfgrid.h promises "Calls only enqueue work; the caller synchronises
the stream" and host arguments that are "free again when the call returns".  Two forms hold an entry to that:

Gate.run(case) -- a bounded sleep in front of the call on the caller's stream s (torch.cuda._sleep, T_MS long), then, with
nothing synchronised in between: the real inputs copied into the (so far poisoned) input views, the outputs overwritten with
the canary, the call under test, and a copy of the whole arena (the snapshot: a consumer on the caller's stream).  The moment
the call returns the host reads the clock and scribbles over every host argument the test owns.  Five assertions, each with an
exception class of its own:
  NotOrdered      ordered behind earlier work: the snapshot equals the expected result (Arena.check: bit for bit, Approx for
                  the shaded colour).  A launch on another stream ran during the sleep: it read poison, or what it stored was
                  overwritten by the late canary.
  NotVisible      visible to later work: the same snapshot, taken without a sync.  Reported when the snapshot is wrong and the
                  arena after a device-wide sync is right: the work was ordered behind s but s was not made to wait for it.
  HostArgsLate    host arguments consumed: the snapshot is wrong with the scribble and right in a second run without it.
  Waited          did not wait: host time from just before the sleep was enqueued to the return of the call is below T / 4.
  NotContained    the arena's own check after the run: guards intact, inputs unchanged, outputs as in the snapshot.
The gate also holds ITSELF to two things, or it would be blind: the sleep really lasted T / 2 or longer (event timing), and s is
a stream beside which stream 0 runs -- fresh_stream() draws streams until a launch on stream 0 completes while the drawn one
sleeps (GateBlind when none does).  The runtime maps its streams round-robin onto a few hardware queues (GPU_MAX_HW_QUEUES of
them), and streams that share a queue run in launch order: some fresh streams share stream 0's queue, and a stray stream-0
launch behind such a stream would be ordered by accident.

Capture.run(case) -- the timing-free form of "only enqueues": the call captured on s into a torch.cuda.CUDAGraph, the host
arguments scribbled, the outputs poisoned, replayed, compared; where a case names a second data set, the device inputs are
overwritten in place and a second replay must give the second result (the graph reads device memory at replay, not a copy made
at call time).  A synchronisation, an allocation or a stream-0 launch inside the call makes the capture fail cleanly.

Gate.run_synchronous(case) -- for the three extractors, which are documented to synchronise `stream`: right with the late
inputs, s.query() true on return, host time at least T.  sleep_ms() is "about T" (the calibration's error), so the sleep in
front of these calls is asked to last 1.05 T and the bound asserted is T itself; the event-timed length of the sleep is held
as well (the call cannot have returned before the sleep in front of it ended).

T_MS: measured, not chosen.  The host time of step 3 (sleep enqueue .. return of the call) of all 123 cases of the four test
files was measured on one MI355X; the slowest was ENQUEUE_MS_SLOWEST = 0.17 ms (a one-camera march over the interleaved
volume; the 70-camera march took 0.09 ms), so T = max(50 ms, 100 x 0.17 ms) = 50 ms.  tools/stream_gate_enqueue.py runs
the files and prints the figures again (ENQUEUE_LOG below is what it reads).  sleep_ms() converts through a cycles-per-millisecond factor measured once per session (two
torch.cuda._sleep lengths timed with events, the slope); an unusable slope skips, it is not guessed."""
import ctypes as C
import functools
import time

import numpy as np
import pytest
import torch

import arena as A

ENQUEUE_MS_SLOWEST = 0.17  # measured; see the docstring
T_MS = max(50.0, 100.0 * ENQUEUE_MS_SLOWEST)
ENQUEUE_LOG = {}           # case name -> the largest host time of step 3 seen in this session, ms: tools/stream_gate_enqueue.py prints it


class GateError(AssertionError):
    pass


class NotOrdered(GateError):
    pass


class NotVisible(GateError):
    pass


class HostArgsLate(GateError):
    pass


class Waited(GateError):
    pass


class NotContained(GateError):
    pass


class GateBlind(GateError):
    pass


class DidNotSynchronise(GateError):
    pass


class SleepUnusable(Exception):
    pass


# ---- the sleep ----------------------------------------------------------------------------------------------------------------
def _timed_sleep(cycles):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.cuda._sleep(int(cycles))
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


@functools.lru_cache(maxsize=None)
def cycles_per_ms():
    """The argument of torch.cuda._sleep that spins for one millisecond: the slope between two lengths, so that the launch's own
    cost drops out.  SleepUnusable when the two timings do not rise with the length."""
    _timed_sleep(1000)
    n = 1 << 18
    while _timed_sleep(n) < 4.0:      # grow until the spin, not the launch, is what is timed (bounded: 2^34 cycles)
        n *= 4
        if n > 1 << 34:
            raise SleepUnusable(f"torch.cuda._sleep({n}) returns in under 4 ms: no usable spin")
    a = min(_timed_sleep(n) for _ in range(3))
    b = min(_timed_sleep(2 * n) for _ in range(3))
    slope = (b - a) / n               # ms per cycle
    if not (a > 0.0 and b > a and slope > 0.0 and 1.5 <= b / a <= 2.5):
        raise SleepUnusable(f"torch.cuda._sleep: {n} cycles took {a:.3f} ms and {2 * n} cycles {b:.3f} ms: no usable slope")
    return 1.0 / slope


def sleep_ms(ms):
    """A spin of about `ms` milliseconds on the current stream.  It ends by itself: no host memory, no wait-value."""
    torch.cuda._sleep(int(ms * cycles_per_ms()))


@pytest.fixture(scope="session")
def gate(pkg):
    try:
        cycles_per_ms()
    except SleepUnusable as e:
        pytest.skip(str(e))
    return Gate(T_MS)


@pytest.fixture(scope="session")
def capture(pkg):
    return Capture()


# ---- a case -------------------------------------------------------------------------------------------------------------------
def scribble(obj):
    """Every 32-bit word of a ctypes object or a numpy array alternately a NaN and 0xFFFFFFFF (trailing bytes 0xFF)."""
    if isinstance(obj, np.ndarray):
        raw = obj.reshape(-1).view(np.uint8)
    else:
        raw = np.ctypeslib.as_array((C.c_uint8 * C.sizeof(obj)).from_address(C.addressof(obj)))
    raw[:] = 0xFF
    words = raw[:raw.size // 4 * 4].view(np.uint32)
    words[0::2] = A.NAN_BITS


class Case:
    """One call under test.
      inputs   {name: (host array, align[, misalign])}  device inputs, left alone by the call
      inouts   {name: (host array, align[, misalign])}  updated in place
      outputs  {name: (shape, dtype, align[, misalign])}
      expected {name: ndarray | arena.Untouched | arena.Approx}, one per inout and output, never taken from the library
      host     () -> {name: ctypes object | numpy array}: FRESH host arguments for one call; the gate scribbles over each the
               moment the call returns
      call     (t, h) -> None: the call, over the arena's tensors t[name] and the host arguments h[name], on the current stream
      second   None | ({name: host array} for some inputs / inouts, expected): another data set of the same shapes for
               Capture's second replay
      poison_around, options   arena.Arena's poison_around; {option: value} of pkg.options around the call"""

    def __init__(self, name, call, expected, inputs=None, inouts=None, outputs=None, host=None, second=None, poison_around="all",
                 options=None):
        self.name, self.call, self.expected = name, call, expected
        self.inputs, self.inouts, self.outputs = dict(inputs or {}), dict(inouts or {}), dict(outputs or {})
        self.host = host or (lambda: {})
        self.second, self.poison_around, self.options = second, poison_around, dict(options or {})

    def carve(self, kind):
        """(arena, {name: tensor}) with the real inputs uploaded and the guards holding `kind`."""
        arrays = [a[0] for a in self.inputs.values()] + [a[0] for a in self.inouts.values()] + [(o[0], o[1]) for o in self.outputs.values()]
        band = A.band_for(*arrays)
        ar = A.Arena(A.arena_bytes(band, *arrays), band=band, poison_around=self.poison_around)
        t = {}
        for name, (a, align, *mis) in self.inputs.items():
            t[name] = ar.input(a, align=align, misalign=mis[0] if mis else 0, name=name)
        for name, (a, align, *mis) in self.inouts.items():
            t[name] = ar.inout(a, align=align, misalign=mis[0] if mis else 0, name=name)
        for name, (shape, dtype, align, *mis) in self.outputs.items():
            t[name] = ar.output(shape, dtype, align=align, misalign=mis[0] if mis else 0, name=name)
        ar.repoison(kind)
        return ar, t

    def run_call(self, pkg, t, h):
        if self.options:
            with pkg.options(self.options):
                self.call(t, h)
        else:
            self.call(t, h)


def _problem(ar, expected, raw=None):
    try:
        return None, ar.check(expected, raw=raw)
    except A.ArenaError as e:
        return str(e), None


def runs_beside_stream_0(s, ms=2.0):
    """True when a launch on stream 0 completes while `s` sleeps: the two are on different hardware queues.  (The runtime maps its
    streams onto a few hardware queues, GPU_MAX_HW_QUEUES of them; streams that share one run in the order of their launches.)"""
    done, probe = torch.cuda.Event(enable_timing=True), torch.zeros(64, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        sleep_ms(ms)
        done.record()
    probe.add_(1)
    torch.cuda.current_stream().synchronize()
    beside = not done.query()
    s.synchronize()
    return beside


def fresh_stream(tries=16):
    """A fresh torch.cuda.Stream() (non-blocking: work on stream 0 does not order with it) that runs beside stream 0."""
    tried = []
    for _ in range(tries):
        s = torch.cuda.Stream()
        if runs_beside_stream_0(s):
            return s
        tried.append(s)   # (kept alive so that the pool hands out another one)
    raise GateBlind(f"none of {tries} fresh streams runs beside stream 0: a stray stream-0 launch would be ordered by accident")


class Gate:
    def __init__(self, t_ms):
        self.t_ms = float(t_ms)

    def _once(self, pkg, case, kind, do_scribble, sleep_scale=1.0):
        T = self.t_ms
        s = fresh_stream()
        ar, t = case.carve(kind)
        # 1. warm up: first-use costs (code object, a program's device copy, the camera ring, the side streams) are not timed
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            case.run_call(pkg, t, case.host())
        s.synchronize()
        # 2. set-up on the default stream: the real inputs aside, poison in their place, the outputs back to the canary
        ar.reset()
        written = list(case.inputs) + list(case.inouts)
        staging = {name: ar.bytes_of(name).clone() for name in written}
        for name in written:
            ar.bytes_of(name).copy_(ar.poison_of(name, kind))
        late_poison = {name: ar.poison_of(name, "canary") for name in case.outputs}
        snapshot = torch.empty_like(ar.raw)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        h = case.host()
        torch.cuda.synchronize()
        s.wait_stream(torch.cuda.current_stream())
        # 3. on s, nothing synchronised in between
        t_start = time.perf_counter()
        with torch.cuda.stream(s):
            e0.record()
            sleep_ms(T * sleep_scale)
            e1.record()
            for name in written:
                ar.bytes_of(name).copy_(staging[name])           # the late inputs
            for name in case.outputs:
                ar.bytes_of(name).copy_(late_poison[name])       # the late output poison
            case.run_call(pkg, t, h)
            # 4. the host, as soon as the call returns
            t_return = time.perf_counter()
            done_on_return = s.query()
            if do_scribble:
                for obj in h.values():
                    scribble(obj)
            snapshot.copy_(ar.raw)                               # a consumer on the caller's stream
        # 5.
        s.synchronize()
        slept = e0.elapsed_time(e1)
        torch.cuda.synchronize()
        host_ms = (t_return - t_start) * 1e3
        assert slept >= T / 2, f"the gate's own sleep lasted {slept:.1f} ms of the {T:.0f} asked for: nothing is shown by this run"
        snap_problem, snap = _problem(ar, case.expected, raw=snapshot)
        live_problem, live = _problem(ar, case.expected)
        return dict(host_ms=host_ms, done_on_return=done_on_return, snap_problem=snap_problem,
                    live_problem=live_problem, snap=snap, live=live, slept=slept)

    def run(self, pkg, case, kinds=("nan", "canary")):
        """The five assertions for `case`, once per poison kind; the snapshots of the kinds must agree bit for bit."""
        T, first = self.t_ms, None
        for kind in kinds:
            r = self._once(pkg, case, kind, True)
            tag = f"{case.name}, poison {kind!r}"
            ENQUEUE_LOG[case.name] = max(ENQUEUE_LOG.get(case.name, 0.0), r["host_ms"])
            if r["host_ms"] >= T / 4:
                raise Waited(f"{tag}: did not wait: the call returned {r['host_ms']:.2f} ms after the sleep of {T:.0f} ms was enqueued "
                             f"(limit {T / 4:.1f} ms; a call that synchronises its stream cannot return before {T:.0f})")
            if r["snap_problem"] is not None and r["live_problem"] is None:
                raise NotVisible(f"{tag}: visible to later work: a copy taken on the caller's stream right after the call does not hold "
                                 f"the result, the arena after a device-wide sync does:\n{r['snap_problem']}")
            if r["snap_problem"] is not None:
                again = self._once(pkg, case, kind, False)
                if again["snap_problem"] is None:
                    raise HostArgsLate(f"{tag}: host arguments consumed: wrong once the host arguments are overwritten on return, right when "
                                       f"they are kept:\n{r['snap_problem']}")
                raise NotOrdered(f"{tag}: ordered behind earlier work: the inputs arrive, and the outputs are poisoned, behind a sleep on "
                                 f"the caller's stream just before the call:\n{r['snap_problem']}")
            if r["live_problem"] is not None:
                raise NotContained(f"{tag}: contained: right in the copy taken on the stream, wrong after the sync:\n{r['live_problem']}")
            for name in r["snap"]:
                if not (r["snap"][name] == r["live"][name]).all():
                    raise NotContained(f"{tag}: view {name!r} changed after the copy taken on the caller's stream")
            if first is None:
                first = r["snap"]
            for name, got in r["snap"].items():
                e = case.expected[name]
                same = first[name] == got
                if getattr(e, "undefined", None) is not None:
                    same = same | np.repeat(e.undefined.reshape(-1), ar_itemsize(e))
                if not same.all():
                    raise NotOrdered(f"{case.name}: view {name!r} differs between poison {kinds[0]!r} and {kind!r}")

    def run_synchronous(self, pkg, case, kinds=("nan", "canary")):
        """An entry documented to synchronise `stream`: right with the late inputs, the stream idle on return, the host held for
        at least T."""
        T = self.t_ms
        for kind in kinds:
            r = self._once(pkg, case, kind, True, sleep_scale=1.05)   # so that "about 1.05 T" is at least T
            tag = f"{case.name}, poison {kind!r}"
            if r["snap_problem"] is not None:
                raise NotOrdered(f"{tag}: ordered behind earlier work:\n{r['snap_problem']}")
            if r["live_problem"] is not None:
                raise NotContained(f"{tag}: contained:\n{r['live_problem']}")
            if not r["done_on_return"]:
                raise DidNotSynchronise(f"{tag}: documented to synchronise the stream, yet the stream still had work when it returned")
            if r["host_ms"] < r["slept"]:
                raise DidNotSynchronise(f"{tag}: returned after {r['host_ms']:.2f} ms, before the {r['slept']:.1f} ms sleep in front of it ended")
            assert r["slept"] >= T, f"the gate's own sleep lasted {r['slept']:.1f} ms, below T = {T:.0f} ms"
            if r["host_ms"] < T:
                raise DidNotSynchronise(f"{tag}: returned after {r['host_ms']:.2f} ms, below T = {T:.0f} ms")


def ar_itemsize(e):
    return e.values.dtype.itemsize


class Capture:
    def run(self, pkg, case, kind="canary"):
        s = torch.cuda.Stream()
        ar, t = case.carve(kind)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            case.run_call(pkg, t, case.host())                   # warm up
        s.synchronize()
        h = case.host()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            case.run_call(pkg, t, h)
        for obj in h.values():                                   # "free again when the call returns"
            scribble(obj)
        data_sets = [({}, case.expected)] + ([case.second] if case.second is not None else [])
        for k, (over, expected) in enumerate(data_sets):
            ar.reset()                                           # outputs poisoned, inputs and inouts re-uploaded
            for name, a in over.items():                         # ... and the second data set in place, same addresses
                v = ar.view(name)
                a = np.ascontiguousarray(a)
                assert a.shape == v.shape and a.dtype.itemsize == v.dtype.itemsize
                v.initial = a.copy()
                ar.reset([name])
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            try:
                ar.check(expected)
            except A.ArenaError as e:
                raise NotOrdered(f"{case.name}: replay {k} of the captured call:\n{e}") from None
