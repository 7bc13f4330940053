"""Runs a sequence of library calls "gated" on a non-default stream, for test_gpu_streams.py.  Not a test module:
pytest does not collect it.

include/schwz_hip.h promises that every device entry point is asynchronous on the stream it is handed.  On the legacy
default stream that promise cannot fail: the default stream serialises with itself.  Here every call of a case is
handed a stream S of its own (torch creates its streams non-blocking: S does not synchronise with the default
stream), and S is held shut while the calls are issued:

  1. every device buffer the calls read is allocated full of NaN (index lists: full of INDEX_POISON), every buffer
     they write full of NaN (integers: INT_POISON), on the default stream, and the device is synchronised;
  2. on S: a delay of DELAY_MS, the copies of the true inputs into those buffers, an event `gate`;
  3. the calls, with stream = S;  for a call that reads nothing back on the host the gate must still be shut when the
     call returns ("gate already open: the case did not discriminate" otherwise -- never a skip);
  4. on S: clones of the results;  S.synchronize(), and nothing wider.

A launch, memset or copy of the library that goes to another stream than S runs while the gate is shut: it reads
poison, or its result is overwritten by the copies of step 2, and the result differs from the reference.  The reference
is the same sequence on the default stream, ungated, with fresh objects from the same host arrays in the same
process; the comparison is bit for bit (the library has no floating-point atomics and folds every reduction in a fixed
order).

The default stream must be able to run while S is held shut, or a misdirected launch would simply queue behind the
delay and go unseen.  Where a process has fewer hardware queues than streams, a stream can share its hardware queue
with the default stream, and then exactly that happens: stream_beside_default() probes every candidate (a short
delay on it, a small kernel on the default stream, which must finish first) and the rig takes only streams that pass.
streams_beside_each_other() does the same between the streams of a case that runs several at once.

INDEX_POISON is 0, a valid index: a misdirected launch must read poisoned VALUES (from[0] is NaN), it must not be
turned into an access out of bounds.  That a misdirected launch is caught is itself tested
(test_rig_detects_a_launch_on_the_wrong_stream), which is also the only way to assert that S is non-blocking.

The tensors of a run are allocated on the default stream and held by the Run until it is dropped: the caching
allocator never hands one of them to another stream's work in between."""
import time

import numpy as np

# The delay that holds S shut, in milliseconds: ten times the longest host-side duration of a single call of
# test_gpu_streams.py on the default stream, measured on the MI355X (profiles/r17_stream_contract.txt): 7.3 ms, a GMRES(4)
# solve to a tolerance, which waits for its state once per cycle.  Of the calls that must return while the gate is
# shut the longest took 4.1 ms (the first Csr.spmv of the process, which loads the code object); the first level-plan
# triangular solve and the first CG solve that captures and instantiates a graph stayed below 1.5 ms.
MEASURED_MS = 7.3
DELAY_MS = 10 * MEASURED_MS

INDEX_POISON = 0
INT_POISON = -0x5A5A5A5B
GATE_OPEN = "gate already open: the case did not discriminate"

CALL_LOG = []        # (label, host milliseconds) of every call of an ungated run: what DELAY_MS is derived from

_rate = {}           # the delay's unit per millisecond, measured once per process


def _calibrate(torch):
    """Cycles of torch.cuda._sleep per millisecond (or, without it, 2048^3 fp64 matmuls per millisecond)."""
    if "rate" in _rate:
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        cycles = 20000000
        e0.record()
        torch.cuda._sleep(cycles)
        e1.record()
        torch.cuda.synchronize()
        _rate["rate"] = cycles / max(e0.elapsed_time(e1), 1e-3)
    else:
        a = torch.ones((2048, 2048), dtype=torch.float64, device="cuda")
        _rate["a"] = a
        torch.mm(a, a)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(8):
            torch.mm(a, a)
        e1.record()
        torch.cuda.synchronize()
        _rate["rate"] = 8 / max(e0.elapsed_time(e1), 1e-3)


def delay(torch, ms=None):
    """Occupies the current stream for `ms` milliseconds (DELAY_MS).  No kernel waits for the host."""
    ms = DELAY_MS if ms is None else ms
    _calibrate(torch)
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(ms * _rate["rate"]))
    else:
        for _ in range(int(ms * _rate["rate"]) + 1):
            torch.mm(_rate["a"], _rate["a"])


_beside = {}         # (busy stream handle, other stream handle; 0: the default stream) -> whether `other` runs meanwhile


def _runs_beside(torch, busy, other=None):
    """Whether a kernel on `other` (None: the default stream) finishes while a 5 ms delay still occupies `busy`."""
    key = (busy.cuda_stream, other.cuda_stream if other is not None else 0)
    if key not in _beside:
        _calibrate(torch)
        torch.cuda.synchronize()
        gate, done = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(busy):
            delay(torch, 5.0)
            gate.record(busy)
        with (torch.cuda.stream(other) if other is not None else _Null()):
            torch.zeros(1, device="cuda")            # a kernel on the other stream
            done.record()
        done.synchronize()
        _beside[key] = not gate.query()
        busy.synchronize()
    return _beside[key]


def stream_beside_default(torch, tries=16):
    """A non-blocking stream on which a delay does not hold up the default stream (see the module docstring)."""
    for _ in range(tries):
        S = torch.cuda.Stream()
        if _runs_beside(torch, S):
            return S
    raise AssertionError("no stream found beside which the default stream runs (%d candidates)" % tries)


def streams_beside_each_other(torch, count, tries=24):
    """`count` distinct streams, each beside the default stream, and every one running while any other is busy: work
    on them really overlaps.  A process has a few hardware queues only (four here, one of them the default stream's),
    so count <= 3 is what can be had."""
    found = []
    for _ in range(tries):
        S = torch.cuda.Stream()
        if any(S.cuda_stream == t.cuda_stream for t in found) or not _runs_beside(torch, S):
            continue
        if all(_runs_beside(torch, S, t) and _runs_beside(torch, t, S) for t in found):
            found.append(S)
            if len(found) == count:
                return found
    raise AssertionError("only %d of %d streams found that run beside each other (%d candidates)" % (len(found), count, tries))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.int64, 4: np.int32}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def _np_to_torch(torch, dtype):
    return {np.dtype(np.float64): torch.float64, np.dtype(np.float32): torch.float32, np.dtype(np.int32): torch.int32,
            np.dtype(np.int64): torch.int64}[np.dtype(dtype)]


class Run:
    """One run of a case: gated on a stream of its own, or (gated=False) the reference on the default stream.

        d_b = r.input(b); d_x = r.input(x0)       buffers, before arm()
        r.arm()                                    the delay, the copies of the true values, the gate
        r.call(cg.solve, d_b.data_ptr(), d_x.data_ptr(), 0.0, 40, stream=r.handle, want_stats=False)
        r.snap(d_x)                                a clone, on the run's stream
        x, = r.finish()                            synchronises the run's stream; numpy arrays of the snaps

    r.call(..., reads_back=True) for a call that synchronises by contract: the gate is not looked at."""

    def __init__(self, torch, gated, stream=None):
        self.torch, self.gated = torch, gated
        self.stream = (stream or stream_beside_default(torch)) if gated else None
        self.handle = self.stream.cuda_stream if gated else 0
        self.gate = torch.cuda.Event() if gated else None
        self.pending, self.keep, self.snaps = [], [], []
        self.armed = False

    def _poison(self, shape, dtype, index=False):
        torch = self.torch
        if dtype.is_floating_point:
            return torch.full(shape, float("nan"), dtype=dtype, device="cuda")
        return torch.full(shape, INDEX_POISON if index else INT_POISON, dtype=dtype, device="cuda")

    def input(self, a, index=False):
        """A device buffer that will hold `a` (a numpy array, or a device tensor) once the gate has passed."""
        torch = self.torch
        true = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).cuda()
        assert not self.armed
        if not self.gated:
            buf = true.clone()
        else:
            buf = self._poison(tuple(true.shape), true.dtype, index)
            self.pending.append((buf, true))
        self.keep += [buf, true]
        return buf

    def fill(self, buf, a):
        """The same for a buffer the library owns (a torch view of it, or any tensor): poison now, `a` at the gate."""
        torch = self.torch
        true = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).cuda()
        assert not self.armed
        if not self.gated:
            buf.copy_(true)
        else:
            buf.copy_(self._poison(tuple(true.shape), true.dtype))
            self.pending.append((buf, true))
        self.keep += [buf, true]

    def output(self, n, dtype=np.float64):
        """A poisoned buffer for results.  Once the run is armed it is made on the run's own stream: a fill on the
        default stream could land after the stream's work has written the buffer."""
        with (self.on_stream() if self.armed else _Null()):
            buf = self._poison((max(int(n), 1),), _np_to_torch(self.torch, dtype))
        self.keep.append(buf)
        return buf

    def hold(self, obj):
        """Library objects of the run live as long as it does: destroying one frees device memory, and a free
        synchronises the device."""
        self.keep.append(obj)
        return obj

    def arm(self, sync=True):
        """sync=False: for the second and later runs of a case that gates several streams at once (the device was
        synchronised by the first run's arm(), after the buffers of all of them were made)."""
        torch = self.torch
        assert not self.armed
        self.armed = True
        if sync:
            torch.cuda.synchronize()    # the poison, the uploads and whatever the creation calls queued: all done
        if not self.gated:
            return
        with torch.cuda.stream(self.stream):
            delay(torch)
            for buf, true in self.pending:
                buf.copy_(true)
            self.gate.record(self.stream)

    def check_shut(self, what=""):
        if self.gated:
            assert not self.gate.query(), "%s (%s)" % (GATE_OPEN, what)

    def call(self, fn, *args, reads_back=False, label=None, **kw):
        assert self.armed
        t0 = time.perf_counter()
        out = fn(*args, **kw)
        ms = (time.perf_counter() - t0) * 1e3
        name = label or getattr(fn, "__qualname__", repr(fn))
        if not self.gated:
            CALL_LOG.append((name, ms))
        elif not reads_back:
            self.check_shut("%s returned after %.2f ms of host time, the delay is %.0f ms" % (name, ms, DELAY_MS))
        return out

    def on_stream(self):
        """Context for torch work that belongs to the sequence (the exchange through torch copies)."""
        return self.torch.cuda.stream(self.stream) if self.gated else _Null()

    def snap(self, t):
        with self.on_stream():
            self.snaps.append(t.clone())

    def finish(self):
        if self.gated:
            self.stream.synchronize()
        else:
            self.torch.cuda.synchronize()
        return [s.cpu().numpy() for s in self.snaps]


class _Null:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def _flat(v, out):
    if callable(v):                     # a host value to be read after the run has finished (last_stats)
        v = v()
    if isinstance(v, (tuple, list)):
        for u in v:
            _flat(u, out)
    elif isinstance(v, dict):
        for k in sorted(v):
            _flat(v[k], out)
    elif v is not None:
        out.append(v)
    return out


def assert_same(ref, got, tag):
    """Snaps and host values of two runs, bit for bit."""
    (snaps_r, host_r), (snaps_g, host_g) = ref, got
    assert len(snaps_r) == len(snaps_g), tag
    for k, (a, b) in enumerate(zip(snaps_r, snaps_g)):
        if not same(a, b):
            diff = np.nonzero(bits(a).ravel() != bits(b).ravel())[0] if a.shape == b.shape else []
            raise AssertionError("%s: result %d on the stream differs from the default-stream run in %d of %d entries "
                                 "(first at %s: %r against %r)" %
                                 (tag, k, len(diff), a.size, diff[:1], b.ravel()[diff[:1]], a.ravel()[diff[:1]]))
    hr, hg = _flat(host_r, []), _flat(host_g, [])
    assert len(hr) == len(hg), tag
    for k, (a, b) in enumerate(zip(hr, hg)):
        a, b = np.asarray(a), np.asarray(b)
        assert same(a, b), "%s: host value %d: %r on the stream, %r on the default stream" % (tag, k, b, a)


def both(torch, body, tag):
    """body(run) -> host values: once on the default stream, once gated; compared bit for bit.  Returns the
    reference run's (snaps, host values)."""
    r = Run(torch, False)
    host = body(r)
    ref = (r.finish(), _flat(host, []))
    g = Run(torch, True)
    host_g = body(g)
    got = (g.finish(), _flat(host_g, []))
    assert_same(ref, got, tag)
    del r, g
    return ref
