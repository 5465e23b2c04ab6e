"""A proxy of lives_amd.ops that captures every entry-point call into a HIP graph and judges the REPLAY, for tests/test_graph_replay.py.

DESIGN.md section 2: "steady-state launches neither allocate nor synchronise and capture into HIP graphs"; tools/bench_ops.py publishes graph-replay figures and falls back
to the eager one, silently, where a capture fails.  GraphProxy(ops, side) has the interface of tests/stream_order.py:StreamProxy (it IS one: forwarding, lib.call
rerouting, record(), batch(warm=), the Blurzoom / RgbDelay wrappers, side, _ops and finish() are inherited), so every case written against that proxy runs through this one
unchanged.  One entry-point call -- or one batch, which becomes ONE graph -- goes through

  1. warm-up      the call, eagerly, with `side` current; side.synchronize(); every recorded tensor put back.  Table builds and per-stream scratch are created here, on
                  the stream that is captured afterwards (a batch with warm= runs that callable instead)
  2. probe        lgpu_debug_fail_alloc(1) and the same call again, eagerly: LGPU_E_NOMEM says that a warm call still reaches lgpu_malloc / lgpu_malloc_ordered.  Such a
                  call is reported and NOT captured (nothing provokes a capture error on purpose).  Stateful handles are exempt: the probe would advance them
  3. capture      with torch.cuda.graph(g, stream=side): the call(s) -- library calls only, torch's default capture error mode
  4. nothing ran  torch.cuda.synchronize(); every recorded tensor still equals its snapshot, byte for byte (a stage enqueued on some other stream has run by now)
  5. scramble     every writeable numpy array reachable through the arguments is complemented in place until the last replay is over: a graph that reads the caller's
                  host memory at replay shows as a mismatch (kernel arguments are copied at capture time).  Device tensors are never scrambled: some hold parameter
                  blocks and pointer arrays, and nothing may replay on garbage geometry
  6. replay       on `side`: the snapshots back (stream ordered), g.replay() -- twice for calls that are not on a handle, so that state on the device that only
                  host-ordered work outside the graph resets (tickets, histogram slices, flags) shows in the second result -- then side.synchronize().  A handle's host-side
                  rotation and counters were consumed at capture time: one replay of the captured sequence is the sequence
  7. release      the graph is dropped before the proxy returns: it holds pointers into per-stream scratch that a later, larger call on `side` may free

The caller's own comparison with the oracle judges what the last replay wrote.  Violations are collected and raised by finish().  A capture that raises ends the
captures of this proxy and of everything that shares its `gate`; a HIP fault ends the session (pytest.exit): nothing more is started on the device.

The recording and scrambling halves need no device: tests/test_graph_replay.py checks them on the CPU.
"""
import numpy as np
import torch

from tests import stream_order as so

NOMEM = "(-5)"          # LGPU_E_NOMEM in lives_amd.lib.LgpuError's text


# ---------------------------------------------------------------------------------------------- host arrays
def arrays_in(obj, out):
    """every numpy array inside obj (lists, tuples and dicts, nested), appended to out"""
    if isinstance(obj, np.ndarray):
        out.append(obj)
    elif isinstance(obj, (list, tuple)):
        for x in obj:
            arrays_in(x, out)
    elif isinstance(obj, dict):
        for x in obj.values():
            arrays_in(x, out)
    return out


class Scramble:
    """the writeable numpy arrays inside objs, complemented in place between __enter__ and __exit__ (each stretch of memory once: an array handed over twice, or a view
    of one already taken, is left to the first).  Read-only arrays are left alone"""

    def __init__(self, *objs):
        self.arrays = []
        for a in arrays_in(objs, []):
            if a.flags.writeable and a.size and a.dtype != object and not any(np.shares_memory(a, b) for b in self.arrays):
                self.arrays.append(a)

    @staticmethod
    def flip(a):
        b = a.view(np.uint8) if a.flags.c_contiguous and a.ndim else None
        if b is not None:
            np.bitwise_not(b, out=b)
        else:                                                  # a strided view: element by element through a contiguous copy
            c = np.ascontiguousarray(a)
            a[...] = np.bitwise_not(c.view(np.uint8)).view(a.dtype).reshape(a.shape)

    def __enter__(self):
        for a in self.arrays:
            self.flip(a)
        return self

    def __exit__(self, *exc):
        for a in self.arrays:
            self.flip(a)
        return False


def same_bytes(t, snap):
    return torch.equal(so.saved(t).reshape(-1).view(torch.uint8), snap.reshape(-1).view(torch.uint8))


def is_stateful(name):
    return any(name == "%s.process" % kind for kind in so.STATEFUL)


class CaptureFailed(AssertionError):
    pass


def device_is_alive(what, stream=None):
    """synchronise the device (or `stream` alone).  A HIP fault shows at the next synchronisation: nothing more is started on the device then"""
    try:
        if stream is None:
            torch.cuda.synchronize()
        else:
            stream.synchronize()
    except Exception as e:
        import pytest
        pytest.exit("%s: the device reported %s: %s -- nothing further is started on it" % (what, type(e).__name__, e), returncode=3)


def capture(side, run, what):
    """run() captured on `side` into a graph of its own (torch's default capture error mode): (graph, what run() returned).  A capture that raises is ended by torch;
    the device is synchronised and CaptureFailed carries both texts"""
    g = torch.cuda.CUDAGraph()
    try:
        with torch.cuda.graph(g, stream=side):
            rets = run()
    except Exception as e:
        del g
        device_is_alive("the capture of %s" % what)
        raise CaptureFailed("%s: %s" % (type(e).__name__, " / ".join(str(x) for x in (e, e.__context__) if x is not None))) from e
    return g, rets


class Gate:
    """shared by the proxies of one test: after a capture that raised, none of them captures again"""

    def __init__(self):
        self.failed = None


# ---------------------------------------------------------------------------------------------- the proxy
class GraphProxy(so.StreamProxy):
    """see the module's docstring.  capture=False stops after the probe and makes the call eagerly (the probe's own test); replays: how often a graph without a handle
    in it is replayed (the teeth tests show with 1 that it is the SECOND result that differs); arm: lgpu_debug_fail_alloc, or None where `ops` is no lives_amd.ops"""

    def __init__(self, ops, side, stream_names=(), gate=None, capture=True, replays=2, arm="auto"):
        so.StreamProxy.__init__(self, ops, side, stream_names=stream_names)
        self.gate, self.capture, self.replays = gate or Gate(), capture, replays
        if arm == "auto":
            real = getattr(ops, "lib", None)
            arm = real.load().lgpu_debug_fail_alloc if real is not None and hasattr(real, "load") else None
        self._arm = arm
        self.hosts = []          # host arrays the caller named with record_host(): scrambled during every replay, like the arrays among a call's arguments
        self.graphs, self.captured, self.flagged, self.eager = 0, [], [], []          # graphs made; names of the calls inside them; calls the probe flagged; calls made eagerly

    def record_host(self, *arrays):
        """numpy arrays that reach an entry point as raw addresses (lib.call): they carry no array for the scramble to find"""
        self.hosts += arrays_in(arrays, [])

    def _last_error(self):
        real = getattr(self._ops, "lib", None)
        try:
            msg = real.load().lgpu_last_error()
            return msg.decode() if msg else ""
        except Exception:
            return ""

    def _restore(self, tensors, snap):
        for t, s in zip(tensors, snap):
            t.copy_(s)
        device_is_alive("putting the recorded tensors back")

    def _eagerly(self, run, tensors, snap, restore):
        try:
            with torch.cuda.stream(self.side):
                ret = run()
            device_is_alive("an eager call on the side stream", self.side)
        finally:
            if restore:
                self._restore(tensors, snap)
        return ret

    def _judge(self, calls, warm):
        names = "+".join(c[0] for c in calls)
        handle = any(is_stateful(c[0]) for c in calls)
        run = lambda: [fn(*a, **k) for _, fn, a, k in calls]
        tensors = list(self.rec.tensors)
        snap = [so.saved(t) for t in tensors]
        torch.cuda.synchronize()
        # 1. warm-up
        self._eagerly(warm, tensors, snap, restore=True)
        # 2. the allocator probe
        flagged = False
        if self._arm is not None and not handle:
            self._arm(1)
            try:
                self._eagerly(warm, tensors, snap, restore=False)
            except Exception as e:
                if NOMEM not in str(e):
                    raise
                flagged = True
                self.flagged.append(names)
                self.problems.append("%s reaches lgpu_malloc / lgpu_malloc_ordered once warm (%s): it was not captured" % (names, e))
            finally:
                self._arm(0)
                self._restore(tensors, snap)
        if not self.capture or flagged or self.gate.failed:
            self.eager.append(names)
            return self._eagerly(run, tensors, snap, restore=False)
        # 3. capture
        try:
            g, rets = capture(self.side, run, names)
        except CaptureFailed as e:
            self.gate.failed = names
            self.problems.append("the capture of %s raised %s; lgpu_last_error: %r -- no further capture in this test" % (names, e, self._last_error()))
            self.eager.append(names)
            self._restore(tensors, snap)
            return self._eagerly(run, tensors, snap, restore=False)
        self.graphs += 1
        self.captured += [c[0] for c in calls]
        try:
            # 4. nothing ran
            device_is_alive("after the capture of %s" % names)
            ran = [i for i, (t, s) in enumerate(zip(tensors, snap)) if not same_bytes(t, s)]
            if ran:
                self.problems.append("%s: %d of %d recorded tensors changed during the capture (the first: number %d, shape %s): a part of the call ran outside the captured stream" % (
                    names, len(ran), len(tensors), ran[0], tuple(tensors[ran[0]].shape)))
                self._restore(tensors, snap)
            # 5. the host's arrays are somebody else's by now, 6. replay
            with Scramble([(a, k) for _, _, a, k in calls], self.hosts):
                with torch.cuda.stream(self.side):
                    for _ in range(1 if handle else self.replays):
                        for t, s in zip(tensors, snap):
                            t.copy_(s, non_blocking=True)
                        g.replay()
                device_is_alive("the replay of %s" % names, self.side)
        finally:
            del g          # 7.
        return rets

    def finish(self):
        assert not self.problems, "; ".join(self.problems)
        return self.captured
