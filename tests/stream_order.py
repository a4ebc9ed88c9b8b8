"""What the stream-order tests (tests/test_stream_order_gpu.py) share.  Not a test module.

The library promises stream order: every call of a context is asynchronous on the context's stream and ordered on it.  On the null stream that
cannot be seen, because the null stream waits for every blocking stream and the suites issue everything on it.  Here a chain runs on a side
stream that the null stream does not wait for (torch.cuda.Stream() is non-blocking), behind a delay kernel, and the device inputs hold a DECOY
until that delay has passed:

    the device inputs hold the decoy (and a stateful context has been driven to completion on it); the device is waited for, here and nowhere else
    on the side stream:  delay | copies of the TRUE inputs | the calls under test, a clone behind every output | copies of the decoy
    side.synchronize(), and nothing wider; outputs and clones must be the reference of the true inputs, bit for bit

A step of the library on a stream that does not wait for the side stream runs while the delay holds the true inputs back: it reads the decoy, or
the decoy's state.  A step that is not finished when the side stream is finished is read too early (the output), or is overtaken by the copies of
the decoy (a read deferred past the end of the call).  The clones say whether the output was complete in stream order behind its call.

The conditions that make this a detector are asserted, not assumed: the references of the decoy and of the true inputs differ in every frame of
every compared output (`differ_in_every_frame`, on the CPU, when a case is built); the delay lasts at least MIN_DELAY_MS (`Delay`, two events);
and a chain without a host wait inside the library has been issued completely before the first delay can have passed (`Chain`, host clock).
"""
import time

import numpy as np

MIN_DELAY_MS = 50.0      # a starting value against ~0.1 ms of issue time per call; what matters is the assertion issue time < measured delay


def raw(a):
    """an array's bytes: words whatever their signedness, floats by their bit patterns"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape + (a.dtype.itemsize,)) if a.ndim else a.reshape(1).view(np.uint8)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize and np.array_equal(raw(got), raw(want))


def differ_in_every_frame(true, decoy, what, whole=()):
    """true, decoy: name -> reference output [F, ...] (names in `whole`: one value for the batch).  Every frame of every output differs."""
    assert set(true) == set(decoy), what
    for k in true:
        a, b = np.ascontiguousarray(true[k]), np.ascontiguousarray(decoy[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        if k in whole:
            assert not np.array_equal(raw(a), raw(b)), "%s: output %s of the decoy is the true one" % (what, k)
            continue
        F = a.shape[0]
        eq = (raw(a).reshape(F, -1) == raw(b).reshape(F, -1)).all(axis=1)
        assert not eq.any(), "%s: output %s of the decoy equals the true one in frames %s" % (what, k, np.flatnonzero(eq)[:8])


class Delay:
    """the delay kernel (torch.cuda._sleep), calibrated once: `cycles` that last `ms` >= MIN_DELAY_MS, measured with two events"""

    def __init__(self, torch):
        self.torch = torch
        torch.cuda._sleep(1000)                       # the kernel's first launch is not part of a measurement
        cycles, ms = 1 << 22, 0.0
        for _ in range(16):
            ms = self._measure(cycles)
            if ms >= 1.2 * MIN_DELAY_MS:
                break
            cycles = int(cycles * max(1.5, 1.5 * MIN_DELAY_MS / max(ms, 1e-3)))
        self.cycles, self.ms = cycles, min(ms, self._measure(cycles))
        print("stream order: delay kernel of %d cycles lasts %.1f ms" % (self.cycles, self.ms))
        assert self.ms >= MIN_DELAY_MS, (self.cycles, self.ms)

    def _measure(self, cycles):
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def queue(self):
        """one delay on torch's current stream"""
        self.torch.cuda._sleep(self.cycles)


class Chain:
    """One chain on `side`.  Before the `with`: input() for every device input, and the context driven on the decoy where it keeps state.

        with Chain(...) as ch:
            ch.stage()                  # a delay; the first one is followed by the copies of the true inputs
            ...calls under test, ch.keep(name, output) right behind the call that writes it; ch.stage() again in front of a later stage...
        ch.check(name, reference of the true inputs)

    host_waits: the library waits on the host inside the chain (an early-exit run, a workspace that grows), so the host does not get ahead of
    the delays and the issue-time condition is not asserted; every stage has its own delay for that case.
    behind: this chain is opened inside the block of the chain `behind`, on another stream, and the delay in front of it may be that chain's: nothing
    is waited for when it begins.  The outer chain calls issued() before it opens the inner one, whose end waits.
    control: the detector's own test.  off_side() returns to the null stream, the calls that follow are issued there on a context left on
    the null stream, and the end also waits for the null stream; check() is then given the DECOY's reference."""

    def __init__(self, torch, delay, side, what, host_waits=False, control=False, behind=None):
        self.torch, self.delay, self.side, self.what, self.host_waits, self.control, self.behind = torch, delay, side, what, host_waits, control, behind
        self.inputs, self.out, self.host = [], {}, {}
        self.stages, self.filled, self.issue_ms, self._ctx = 0, False, None, None

    def input(self, true, decoy):
        """a device tensor that holds the decoy now and the true input behind the first delay"""
        true, decoy = np.ascontiguousarray(true), np.ascontiguousarray(decoy)
        assert true.shape == decoy.shape and true.dtype == decoy.dtype and not np.array_equal(raw(true), raw(decoy)), self.what
        as_dev = lambda a: self.torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        t = as_dev(decoy)
        self.inputs.append((t, as_dev(true), as_dev(decoy)))
        return t

    def __enter__(self):
        if self.behind is None:
            self.torch.cuda.synchronize()             # the set-up is done; nothing below waits for the device as a whole
        self._t0 = time.perf_counter()
        self._ctx = self.torch.cuda.stream(self.side)
        self._ctx.__enter__()
        return self

    def stage(self):
        self.delay.queue()
        if not self.filled:
            for t, true, _ in self.inputs:
                t.copy_(true)
            self.filled = True
        self.stages += 1

    def off_side(self):
        assert self.control
        self._ctx.__exit__(None, None, None)
        self._ctx = None

    def keep(self, name, t, in_place=False):
        """an output and its clone, queued right behind the call that writes it; in_place: the output is an input tensor, which the end of the chain
        overwrites with the decoy, so its clone alone is kept"""
        assert name not in self.out, name
        self.out[name] = (None if in_place else t, t.clone())
        return t

    def issued(self):
        """the last call of this chain has returned (where that is not the end of its block)"""
        self.issue_ms = (time.perf_counter() - self._t0) * 1e3

    def __exit__(self, et, ev, tb):
        torch = self.torch
        if self.issue_ms is None:
            self.issued()                                           # from entering the block to the return of the last call
        if self.control:
            torch.cuda.current_stream().synchronize()               # the null stream: the calls of a control are there
        if self._ctx is None:
            self._ctx = torch.cuda.stream(self.side)
            self._ctx.__enter__()
        for t, _, decoy in self.inputs:
            t.copy_(decoy)
        self.side.synchronize()                                     # this stream and nothing wider
        if et is None:
            for name, (t, c) in self.out.items():                   # the copies to the host are on this stream as well
                if t is not None:
                    self.host[name] = t.cpu().numpy()
                self.host[name + " (clone)"] = c.cpu().numpy()
        self._ctx.__exit__(None, None, None)
        if et is not None:
            return False
        delays = self.stages + (self.behind.stages if self.behind is not None else 0)
        assert delays >= 1 and (self.filled or not self.inputs), self.what
        print("stream order: %s: issued in %.2f ms behind %d delay(s) of %.1f ms%s" %
              (self.what, self.issue_ms, delays, self.delay.ms, " (host waits inside)" if self.host_waits else ""))
        if not self.host_waits:
            assert self.issue_ms < self.delay.ms, "%s: issuing took %.2f ms, the delay lasts %.1f ms" % (self.what, self.issue_ms, self.delay.ms)
        return False

    def names(self):
        return {k[:-len(" (clone)")] for k in self.host if k.endswith(" (clone)")} | {k for k in self.host if not k.endswith(" (clone)")}

    def check(self, name, want):
        """output `name` and its clone are `want`, bit for bit"""
        assert name + " (clone)" in self.host, (self.what, name)
        want = np.ascontiguousarray(want)
        for k in (name, name + " (clone)"):
            if k not in self.host:
                continue
            got = self.host[k]
            assert got.shape == want.shape, (self.what, k, got.shape, want.shape)
            if not same_bits(got, want):
                rows = max(got.shape[0], 1) if got.ndim else 1
                bad = np.flatnonzero((raw(got).reshape(rows, -1) != raw(want).reshape(rows, -1)).any(axis=1))
                raise AssertionError("%s: %s differs from the reference in %d of %d rows, first %s" % (self.what, k, len(bad), rows, bad[:8].tolist()))

    def check_all(self, want):
        assert set(want) == self.names(), (self.what, sorted(want), sorted(self.names()))
        for name, w in want.items():
            self.check(name, w)
