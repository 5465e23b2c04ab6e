"""A recording proxy of lives_amd.ops that holds every entry point to the stream contract of include/lives_gpu.h, for tests/test_stream_order.py.

The other suites call on the current (null) stream and download behind a device-wide synchronize, so a launch on the wrong stream, a table copied on the null
stream or a scratch stage enqueued somewhere else passes them by construction.  StreamProxy(ops, side) stands where a runner expects `gpu` and turns each
entry-point call into

  1. a warm-up: the same call with `side` current and idle (host time t_warm), side.synchronize(), every recorded tensor put back.  First-use table builds and the
     growth of per-stream scratch are over after it
  2. every recorded tensor W saved (P) and overwritten with its complement; device-wide synchronize
  3. on `side`: busy work of a known length, the event busy_done, then W.copy_(P) for every recorded tensor (device to device, stream ordered)
  4. the call, with `side` current
  5. busy_done.query() the moment the call returns: it must still be pending (the call did not wait for its stream)
  6. side.synchronize() -- this stream only

Whatever part of the call did not go to `side` runs at once (the null stream and any stream of the library are idle, torch's streams do not block on the null
stream): it reads complemented inputs, or writes a destination that step 3 overwrites afterwards.  Either way the caller's comparison with the oracle fails.
That holds only where `side` does not share a hardware queue with the default stream: side_stream() finds such a stream by measurement.

Recording (Recorder) needs no device and no stream: it is the part test_stream_order checks on the CPU.
"""
import contextlib
import inspect
import re
import time

import torch

# functions of lives_amd.ops that do no device work: forwarded untouched, but the tensors they are given are recorded (the track and source builders are where the
# frames of a tick reach the front end)
HOST_HELPERS = {"chain_params", "yuv_source", "yuv422_source", "yuv_layer_source", "chain_sink", "fx_luts", "dissolve_mask", "resize_plan", "pixbuf_plan", "comp_geometry",
                "tuning", "init", "stream_ptr", "dptr", "lut_ptr", "ptr_array"}
STATEFUL = ("Blurzoom", "RgbDelay")
MIN_BUSY_MS, BUSY_FACTOR, MAX_BUSY_MS = 20.0, 20.0, 500.0


def is_host_helper(name):
    return name in HOST_HELPERS or name.endswith("_tracks") or name.startswith("_")


def stream_entry_points(header_text):
    """the names of the prototypes of include/lives_gpu.h that take a `void *stream`, in the header's order"""
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = []
    for name, params in re.findall(r"\b(lgpu_\w+)\s*\(([^()]*)\)\s*;", text):
        if re.search(r"\bvoid\s*\*\s*stream\b", params):
            out.append(name)
    return out


# ---------------------------------------------------------------------------------------------- recording
def tensors_in(obj, out):
    """every torch.Tensor inside obj (lists, tuples and dicts, nested), appended to out"""
    if isinstance(obj, torch.Tensor):
        out.append(obj)
    elif isinstance(obj, (list, tuple)):
        for x in obj:
            tensors_in(x, out)
    elif isinstance(obj, dict):
        for x in obj.values():
            tensors_in(x, out)
    return out


class Recorder:
    """the tensors that reached the front end, each once (the same view handed over twice -- an in-place call -- is one entry)"""

    def __init__(self):
        self.tensors, self.keys = [], set()

    def add(self, *objs):
        for t in tensors_in(objs, []):
            key = (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t.dtype)
            if key not in self.keys:
                self.keys.add(key)
                self.tensors.append(t)


def complement(p):
    """the bytes of a contiguous tensor, every bit flipped, in p's dtype"""
    return p.view(torch.uint8).bitwise_not().view(p.dtype)


def saved(t):
    return t.detach().clone(memory_format=torch.contiguous_format)


# ---------------------------------------------------------------------------------------------- busy work
class Busy:
    """work for one stream that leaves the rest of the device free and lasts a known time.  torch.cuda._sleep where it really spins on the device for a time
    proportional to its argument (measured with events, once per session); otherwise a train of fills of a 256 MiB buffer"""

    def __init__(self):
        self.kind, self.per_ms, self.big = None, None, None

    @staticmethod
    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def calibrate(self):
        if self.kind:
            return self
        sleep = getattr(torch.cuda, "_sleep", None)
        if sleep is not None:
            sleep(1000)                                       # the kernel's first launch loads its code
            c1, c2 = 4_000_000, 40_000_000
            t1, t2 = self.timed(lambda: sleep(c1)), self.timed(lambda: sleep(c2))
            if t2 - t1 > 1.0 and 5.0 < t2 / max(t1, 1e-6) < 20.0:          # on the device, and proportional
                self.kind, self.per_ms = "sleep cycles", (c2 - c1) / (t2 - t1)
        if not self.kind:
            self.big = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
            self.big.fill_(0)
            n = 64
            t = self.timed(lambda: [self.big.fill_(i & 1) for i in range(n)])
            self.kind, self.per_ms = "256 MiB fills", n / t
        print("stream-order: busy work calibrated: %.0f %s per ms" % (self.per_ms, self.kind))
        return self

    def enqueue(self, ms):
        """on the current stream"""
        n = max(1, int(ms * self.per_ms + 0.5))
        if self.kind == "sleep cycles":
            torch.cuda._sleep(n)
        else:
            for i in range(n):
                self.big.fill_(i & 1)


BUSY = Busy()


def overtakes(stream, busy=None):
    """whether work given to the default stream runs while `stream` is busy.  The runtime spreads its streams over a few hardware queues (four here), and two streams
    that share one run in submission order: a stray launch on the default stream would then queue behind the busy work and the re-initialised inputs, and the byte
    check would have no teeth.  Measured, not assumed: a fill and a copy on the default stream must complete while 5 ms of busy work on `stream` are pending"""
    busy = (busy or BUSY).calibrate()
    a, b = torch.zeros(4096, dtype=torch.uint8, device="cuda"), torch.zeros(4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    with torch.cuda.stream(stream):
        busy.enqueue(5.0)
        done.record()
    a.fill_(1)
    b.copy_(a)
    torch.cuda.default_stream().synchronize()
    free = not done.query()
    stream.synchronize()
    return free


_SIDE = []


def side_stream(tries=16):
    """a torch stream that the default stream overtakes (see overtakes()); found once per session"""
    if not _SIDE:
        for i in range(tries):
            s = torch.cuda.Stream()
            free = overtakes(s)
            print("stream-order: candidate side stream %d (%#x): the default stream %s" % (i, s.cuda_stream, "overtakes it" if free else "queues behind it"))
            if free:
                _SIDE.append(s)
                break
        else:
            raise AssertionError("none of %d streams is free of the default stream's hardware queue: the byte check cannot be made" % tries)
    return _SIDE[0]


class Call:
    """what one judged call did: host times in ms, the busy period asked for and measured, and whether busy_done had fired when the call returned"""

    def __init__(self, name, t_warm, t_call, busy_ms, waited):
        self.name, self.t_warm, self.t_call, self.busy_ms, self.waited, self.busy_real, self.judged = name, t_warm, t_call, busy_ms, waited, None, True

    def __str__(self):
        return "%s: warm-up %.3f ms, call %.3f ms on the host, busy period %.1f ms asked, %s ms measured, %s" % (
            self.name, self.t_warm, self.t_call, self.busy_ms, "%.1f" % self.busy_real if self.busy_real is not None else "?",
            "busy_done had FIRED when the call returned" if self.waited else "returned while its stream was busy")


# ---------------------------------------------------------------------------------------------- the proxy
class _Stateful:
    """a Blurzoom / RgbDelay whose process() goes through the proxy"""

    def __init__(self, proxy, kind, real):
        self._proxy, self._kind, self._real = proxy, kind, real

    def process(self, *args, **kwargs):
        return self._proxy._entry("%s.process" % self._kind, self._real.process, args, kwargs)

    def __getattr__(self, name):
        return getattr(self._real, name)


class _Lib:
    """lives_amd.lib as the runners reach it through gpu.lib: call(name, ..., None) of a stream-taking entry point gets the current stream in place of the null
    stream and is judged like any other call (its frames are raw pointers there: the caller records the tensors with proxy.record())"""

    def __init__(self, proxy, real):
        self._proxy, self._real = proxy, real

    def call(self, name, *args):
        if name in self._proxy.stream_names and args and args[-1] is None:
            ops = self._proxy._ops
            return self._proxy._entry(name, lambda *a: self._real.call(name, *(a[:-1] + (ops.stream_ptr(),))), args, {})
        return self._real.call(name, *args)

    def __getattr__(self, name):
        return getattr(self._real, name)


class StreamProxy:
    """see the module's docstring.  expect_wait(name, index) -> bool says which judged calls are allowed -- and then required -- to wait for their stream (index
    counts the judged calls of this proxy from 0); everything else must return while busy_done is pending.  Violations are collected and raised by finish(), so
    that the caller's comparison with the oracle runs first.  stream_names: the entry points lib.call() reroutes (stream_entry_points of the header)"""

    def __init__(self, ops, side, expect_wait=None, stream_names=(), busy=None):
        self._ops, self.side, self._expect_wait, self.stream_names = ops, side, expect_wait or (lambda name, index: False), frozenset(stream_names)
        self._busy = busy or BUSY
        self.rec, self.calls, self.problems, self._queue = Recorder(), [], [], None

    # -- forwarding
    def __getattr__(self, name):
        attr = getattr(self._ops, name)
        if name == "lib":
            return _Lib(self, attr)
        if name in STATEFUL:
            return lambda *a, **k: _Stateful(self, name, attr(*a, **k))
        if not inspect.isfunction(attr):
            return attr
        if is_host_helper(name):
            def helper(*args, **kwargs):
                self.rec.add(args, kwargs)
                return attr(*args, **kwargs)
            return helper
        return lambda *args, **kwargs: self._entry(name, attr, args, kwargs)

    def record(self, *objs):
        self.rec.add(*objs)

    # -- steps 1 to 6
    def _warm(self, run):
        tensors = list(self.rec.tensors)
        snap = [saved(t) for t in tensors]
        torch.cuda.synchronize()
        try:
            with torch.cuda.stream(self.side):
                t0 = time.perf_counter()
                run()
                t_warm = (time.perf_counter() - t0) * 1e3
            self.side.synchronize()
        finally:
            for t, s in zip(tensors, snap):
                t.copy_(s)
            torch.cuda.synchronize()
        return t_warm, tensors, snap

    def _judge(self, calls, warm):
        """calls: [(name, fn, args, kwargs)], all behind ONE busy period with no host synchronisation between them; warm: what the warm-up runs"""
        self._busy.calibrate()
        t_warm, tensors, snap = self._warm(warm)
        if BUSY_FACTOR * t_warm > MAX_BUSY_MS:              # a cold first call (code loading, table builds): judge the steady state, as the contract is about it
            t_warm, tensors, snap = self._warm(warm)
        busy_ms = max(MIN_BUSY_MS, BUSY_FACTOR * t_warm)
        names = "+".join(c[0] for c in calls)
        assert busy_ms <= MAX_BUSY_MS, "%s: too slow to judge (warm-up %.2f ms on the host would need a busy period of %.0f ms)" % (names, t_warm, busy_ms)
        for t, s in zip(tensors, snap):
            t.copy_(complement(s))
        torch.cuda.synchronize()
        start, busy_done = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        done, rets = [], []
        with torch.cuda.stream(self.side):
            start.record()
            self._busy.enqueue(busy_ms)
            busy_done.record()
            for t, s in zip(tensors, snap):
                t.copy_(s, non_blocking=True)
            for name, fn, args, kwargs in calls:
                t0 = time.perf_counter()
                rets.append(fn(*args, **kwargs))
                t_call = (time.perf_counter() - t0) * 1e3
                done.append(Call(name, t_warm, t_call, busy_ms, busy_done.query()))
        self.side.synchronize()
        real = start.elapsed_time(busy_done)
        over = False                                        # behind a call that waited the busy period is over: the calls after it cannot be judged
        for c in done:
            c.busy_real = real
            index = len(self.calls)
            self.calls.append(c)
            c.judged = not over
            if over:
                continue
            over = c.waited
            if c.waited != bool(self._expect_wait(c.name, index)):
                self.problems.append(("%s waited for its stream" if c.waited else "%s is listed as a call that waits, and did not") % c.name + " -- " + str(c))
        if real < 0.5 * busy_ms:
            self.problems.append("%s: the busy period lasted %.2f ms where %.1f ms were asked for; its calls were not judged" % (names, real, busy_ms))
        return rets

    def _entry(self, name, fn, args, kwargs):
        self.rec.add(args, kwargs)
        if self._queue is not None:
            self._queue.append((name, fn, args, kwargs))
            return None
        return self._judge([(name, fn, args, kwargs)], lambda: fn(*args, **kwargs))[0]

    @contextlib.contextmanager
    def batch(self, warm=None):
        """the entry-point calls made inside are queued and, on leaving, made back to back behind ONE busy period (steps 2 and 3 once, the calls, step 6).  They return
        None inside the block, and the host arrays they were given must stay as they are until it ends.  warm: what the warm-up runs in place of the queued calls
        themselves -- for a stateful handle, the same frames through a handle of its own"""
        assert self._queue is None
        self._queue = []
        try:
            yield self
            queue = self._queue
        finally:
            self._queue = None
        if queue:
            self._judge(queue, warm or (lambda: [fn(*a, **k) for _, fn, a, k in queue]))

    def finish(self):
        """the non-blocking verdict over every judged call"""
        assert not self.problems, "; ".join(self.problems)
        return self.calls
