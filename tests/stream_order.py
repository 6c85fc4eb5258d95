"""The instrument of tests/test_gpu_stream_order.py: bounded delays on both streams of a call, and a library handle that checks the
ordering between them at every ABI call.  A helper module: no test, no fixture.

A wrapper works on two streams.  Torch queues on its current stream `t`; the context queues on a stream of its own (obia_create) or
on the one it was given (obia_create_on_stream), `s`.  Nothing orders the two but explicit waits, and on the suite's small inputs a
missing wait is invisible: torch's kernels have finished before ctypes has marshalled the next call.  Here the races are made to
lose, deterministically and without a fault:

  Delay         a busy kernel of a calibrated, bounded length (torch.cuda._sleep: it counts cycles and ends, no flag to wait for),
                never longer than MAX_MS; a chain of matmuls of the same length where _sleep is missing.
  late(x)       a tensor that holds poison until a Delay on `t` has passed and the values have been copied in: a wrapper that
                reaches the library without waiting for `t` reads the poison.
  Instrumented  a proxy of the ctypes handle obia_amd._lib.load() returns, installed as obia_amd._lib._lib inside a `with` block.
                At entry to every call that takes a context or a session it records whether `t` is idle, then puts a Delay on `s`
                in front of the call's kernels; after the return it records whether `s` is still busy, puts a Delay on `t` in front
                of whatever torch work the wrapper queues next, and appends a Record to its log.  It raises nothing: the tests judge
                the log, so one run shows every violation.  After a refused call (a negative status) it waits for the delay it put
                on `s` itself, so that nothing of its own is left there.

What "idle" means.  The Delay the proxy itself queued on `t` after a call is not torch work of the wrapper: a wrapper that calls
two entry points back to back has nothing to wait for.  So the proxy watches torch's dispatcher (a TorchDispatchMode, or `note()`
from a fake) and records idle_t = t.query() or nothing was dispatched since the previous instrumented return (since the block
was entered, for the first call: what was queued before the block is the caller's to have waited for).  An operator that
only allocates (empty*), only makes a view of its input, or touches no CUDA tensor queues nothing and does not count; everything
else does, the in-place ones included.  A Delay is not queued on `t` while the previous one is still running: delays do not add up.
"""
import time

MAX_MS = 100.0            # no delay is longer
MIN_MS = 5.0              # the shortest the GPU suite uses (the rule of its section "Sizing the delay")

# Calls that are left alone, each with its reason.  Everything else the library exports takes a context or a tiler session as its
# first argument and queues, waits for, or frees work on the context's stream.
BOOKKEEPING = {name: "host only: reads or sets a field of the context or session, touches no stream" for name in (
    "obia_workspace_bytes", "obia_set_profiling", "obia_last_timing", "obia_crowns_last_work", "obia_seedtab_last_work", "obia_test_cc_report",
    "obia_tiler_next_id", "obia_tiler_set_seeding")}
BOOKKEEPING["obia_test_visited_nonzero"] = "the workspace suite's instrument: waits for both streams itself, reads only"
CONTEXT_FREE = {name: "takes no context" for name in (
    "obia_abi_version", "obia_last_error", "obia_create", "obia_create_on_stream", "obia_slic_default_params", "obia_rasterize_info",
    "obia_test_sweep_plan", "obia_test_launch_grid", "obia_test_launch_grid_names", "obia_test_seam_sort_limit")}
NO_DELAY_BEFORE = ("obia_synchronize",)      # logged like the rest: it is the wait itself


class Record(tuple):
    """(entry point, idle_t, pending_s, perf_counter at entry, at return, what the call returned)"""
    __slots__ = ()
    name, idle_t, pending_s, t_in, t_out, result = (property(lambda self, i=i: self[i]) for i in range(6))

    @property
    def refused(self):
        """the call returned an OBIA_E_* status: it read and wrote nothing on the device, or failed and says so (a pointer, None of a
        void function and OBIA_OK are not refusals)"""
        return isinstance(self.result, int) and self.result < 0


def largest_gap(log):
    """seconds between a return and the next entry, the largest: the host time a wrapper spends between two ABI calls"""
    return max((b.t_in - a.t_out for a, b in zip(log, log[1:])), default=0.0)


def delay_ms_for(gap_s):
    """4 x the largest gap (host jitter on a shared machine doubles a sub-millisecond gap easily), at least MIN_MS; the caller checks
    the cap"""
    return max(MIN_MS, 4.0 * gap_s * 1e3)


# ---- delays ------------------------------------------------------------------------------------------------------------------------
class Delay:
    """Delay(ms)(stream): queues a busy kernel of about `ms` milliseconds on `stream`.  Calibrated once per process."""
    per_ms = None         # cycles of _sleep, or links of the matmul chain, per millisecond
    how = None            # "_sleep" or "matmul"
    _mat = None

    def __init__(self, ms):
        if not 0.0 <= ms <= MAX_MS:
            raise ValueError(f"a delay of {ms} ms: the cap is {MAX_MS} ms")
        self.ms = float(ms)

    @classmethod
    def _timed(cls, torch, queue):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        queue()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    @classmethod
    def calibrate(cls):
        """time one call with a pair of events and scale; a second, ten times longer call when the first took under a millisecond"""
        import torch
        if cls.per_ms is not None:
            return cls.per_ms
        sleep = getattr(torch.cuda, "_sleep", None)
        if sleep is not None:
            sleep(1000)                                                    # (loads the kernel)
            torch.cuda.synchronize()
            for cycles in (1_000_000, 10_000_000):
                ms = cls._timed(torch, lambda: sleep(cycles))
                if ms >= 1.0:
                    break
            if 0.05 <= ms <= MAX_MS:
                cls.per_ms, cls.how = cycles / ms, "_sleep"
                return cls.per_ms
        # _sleep is missing or does not take time: a fixed chain of matmuls, one link timed the same way
        cls._mat = torch.ones((1024, 1024), dtype=torch.float32, device="cuda")
        torch.mm(cls._mat, cls._mat)
        torch.cuda.synchronize()
        ms = cls._timed(torch, lambda: [torch.mm(cls._mat, cls._mat) for _ in range(16)]) / 16
        cls.per_ms, cls.how = 1.0 / max(ms, 1e-3), "matmul"       # (links per millisecond)
        return cls.per_ms

    def __call__(self, stream):
        import torch
        n = int(self.ms * self.calibrate())
        if n <= 0:
            return
        with torch.cuda.stream(stream):
            if self.how == "_sleep":
                torch.cuda._sleep(n)
            else:
                for _ in range(n):
                    torch.mm(self._mat, self._mat)


def late(x, t, delay):
    """A tensor like `x` that holds poison (NaN for floats, 0x5A bytes otherwise) until `delay` has passed on `t` and the values of
    `x` have been copied in behind it."""
    import torch
    with torch.cuda.stream(t):
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
        if x.dtype.is_floating_point:
            out.fill_(float("nan"))
        else:
            out.view(-1).view(torch.uint8).fill_(0x5A)
        t.synchronize()                                                    # the poison is there before anybody can look
        delay(t)
        if x.dtype.is_floating_point:
            out.copy_(x)
        else:
            out.view(-1).view(torch.uint8).copy_(x.contiguous().view(-1).view(torch.uint8))  # (bytes: every integer width, uint16 included)
    out._late_source = x                                                   # (alive until the copy has run)
    return out


# ---- which torch operators queue work ------------------------------------------------------------------------------------------------
_ALLOCATES = ("empty", "empty_like", "empty_strided", "new_empty", "new_empty_strided", "empty_permuted")


def queues_work(func, args, kwargs, out, cuda_only=True):
    """Does this dispatched operator put work on the current stream?  Not when it touches no CUDA tensor, only allocates, or returns
    views of its inputs; every other operator does (a wrong "yes" can only make the check stricter)."""
    import torch
    from torch.utils._pytree import tree_leaves
    ins = [v for v in tree_leaves((args, kwargs)) if isinstance(v, torch.Tensor)]
    outs = [v for v in tree_leaves(out) if isinstance(v, torch.Tensor)]
    if cuda_only and not any(v.is_cuda for v in ins + outs):
        return False
    schema = func._schema
    if schema.name.split("::")[-1] in _ALLOCATES:
        return False
    if schema.is_mutable:
        return True
    held = {v.untyped_storage().data_ptr() for v in ins}
    return not (outs and all(v.untyped_storage().data_ptr() in held for v in outs))


def fresh_bytes(args, kwargs, out):
    """bytes of every CUDA allocation among the outputs of a dispatched operator (storages no input holds)"""
    import torch
    from torch.utils._pytree import tree_leaves
    held = {v.untyped_storage().data_ptr() for v in tree_leaves((args, kwargs)) if isinstance(v, torch.Tensor)}
    return {v.untyped_storage().nbytes() for v in tree_leaves(out)
            if isinstance(v, torch.Tensor) and v.is_cuda and v.untyped_storage().data_ptr() not in held}


def _watch(proxy):
    from torch.utils._python_dispatch import TorchDispatchMode

    class Watch(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            fresh = fresh_bytes(args, kwargs, out)
            if fresh:
                proxy.sizes.update(fresh)
            if not proxy._work and queues_work(func, args, kwargs, out):
                proxy.note()
            return out
    return Watch()


# ---- the proxy -----------------------------------------------------------------------------------------------------------------------
class _Call:
    """one exported function: the call instrumented, every other attribute (argtypes, restype, ...) the real function's"""

    def __init__(self, proxy, name, fn):
        object.__setattr__(self, "_p", (proxy, name, fn))

    def __call__(self, *args, **kwargs):
        proxy, name, fn = self._p
        return proxy._call(name, fn, args, kwargs)

    def __getattr__(self, attr):
        return getattr(self._p[2], attr)

    def __setattr__(self, attr, value):
        setattr(self._p[2], attr, value)


class Instrumented:
    """with Instrumented(lib, t, s, delay) as ins: ... ; ins.log.  `s`: the torch-visible stream the context runs on, or None (only
    the `t` side is instrumented); `delay`: a callable that queues a delay on the stream it is given, or None (logging only);
    `delay_s`: another one for `s` (default: `delay`);
    `holder`: the module whose `_lib` is replaced (obia_amd._lib); `watch`: follow torch's dispatcher (False: the caller calls
    note()).  `sizes`: the bytes of every CUDA allocation torch made inside the block, for the stale-block guard of the GPU suite."""

    def __init__(self, lib, t, s=None, delay=None, holder=None, watch=True, clock=time.perf_counter, delay_s=None):
        d = self.__dict__
        d.update(_real=lib, _t=t, _s=s, _delay=delay, _delay_s=delay_s or delay, _holder=holder, _watch=watch, _clock=clock, _calls={}, _work=False, _mode=None,
                 _own=None, log=[], sizes=set())

    # -- installation
    def __enter__(self):
        if self._holder is None:
            from obia_amd import _lib
            self.__dict__["_holder"] = _lib
        self.__dict__["_saved"] = self._holder._lib
        self._holder._lib = self
        if self._watch:
            try:
                self.__dict__["_mode"] = _watch(self)
                self._mode.__enter__()
            except BaseException:
                self._holder._lib = self._saved
                raise
        return self

    def __exit__(self, *exc):
        try:
            if self._mode is not None:
                self._mode.__exit__(*exc)
        finally:
            self._holder._lib = self._saved
        return False

    # -- pass-through
    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name.startswith("_") or not callable(fn) or name in BOOKKEEPING or name in CONTEXT_FREE:
            return fn
        if name not in self._calls:
            self._calls[name] = _Call(self, name, fn)
        return self._calls[name]

    def __setattr__(self, name, value):
        setattr(self._real, name, value)

    def note(self):
        """torch work has been queued on `t` since the last instrumented return"""
        self.__dict__["_work"] = True

    # -- the instrumented call
    def _call(self, name, fn, args, kwargs):
        d = self.__dict__
        idle_t = bool(self._t.query()) or not self._work
        if self._s is not None and self._delay_s is not None and name not in NO_DELAY_BEFORE:
            self._delay_s(self._s)
        t_in = self._clock()
        result = "raised"
        try:
            result = fn(*args, **kwargs)
            return result
        finally:
            t_out = self._clock()
            pending_s = None if self._s is None else not self._s.query()
            if pending_s and self._delay is not None and isinstance(result, int) and result < 0:
                self._s.synchronize()                                      # a refused call queued nothing: what runs on s is the proxy's own delay
            if self._delay is not None and (self._own is None or self._own.query()):
                self._delay(self._t)
                d["_own"] = self._record_own()
            d["_work"] = False
            self.log.append(Record((name, idle_t, pending_s, t_in, t_out, result)))

    def _record_own(self):
        """an event behind the delay just queued on `t` (a fake stream without record_event: the stream itself)"""
        rec = getattr(self._t, "record_event", None)
        return rec() if rec is not None else self._t
