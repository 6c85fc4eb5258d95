"""tests/stream_order.py without a GPU: a fake library of plain Python callables and fake streams whose query() the test controls."""
import pytest

from tests import stream_order as SO


class FakeStream:
    def __init__(self, busy=False):
        self.busy, self.waits = busy, 0

    def query(self):
        return not self.busy

    def synchronize(self):
        self.busy, self.waits = False, self.waits + 1


class FakeFn:
    """a ctypes function as far as the proxy can tell: callable, with argtypes and restype"""

    def __init__(self, body):
        self.body, self.argtypes, self.restype, self.calls = body, ["handle"], int, []

    def __call__(self, *args, **kwargs):
        self.calls.append((args, kwargs))
        return self.body(*args, **kwargs)


class FakeLib:
    def __init__(self):
        self.obia_label_edges_u8_dev = FakeFn(lambda h, *a, **k: ("edges", h, a, k))
        self.obia_image_stretch_u8_dev = FakeFn(lambda h, *a: 0)
        self.obia_synchronize = FakeFn(lambda h: 0)
        self.obia_workspace_bytes = FakeFn(lambda h: 4096)
        self.obia_tiler_next_id = FakeFn(lambda h: 7)
        self.obia_abi_version = FakeFn(lambda: 2)
        self.obia_create = FakeFn(lambda dev: "ctx")
        self.obia_boom_dev = FakeFn(self._boom)
        self.some_value = 11

    @staticmethod
    def _boom(h):
        raise RuntimeError("boom")


class Delays:
    """a delay that marks the stream it is queued on as busy, and says where it was queued"""

    def __init__(self):
        self.on = []

    def __call__(self, stream):
        self.on.append(stream)
        stream.busy = True


def proxy(lib, t, s=None, delay=None):
    return SO.Instrumented(lib, t, s, delay, watch=False)


def test_the_handle_is_restored_on_exit_and_on_exception():
    from obia_amd import _lib
    before, lib = _lib._lib, FakeLib()
    with proxy(lib, FakeStream()) as ins:
        assert _lib._lib is ins and _lib.load() is ins
    assert _lib._lib is before
    with pytest.raises(RuntimeError, match="boom"):
        with proxy(lib, FakeStream()) as ins:
            assert _lib.load() is ins
            ins.obia_boom_dev("h")
    assert _lib._lib is before
    assert [(r.name, r.result, r.refused) for r in ins.log] == [("obia_boom_dev", "raised", False)]   # a call that raised is logged too
    with pytest.raises(KeyError):
        with proxy(lib, FakeStream()):
            raise KeyError("outside a call")
    assert _lib._lib is before


def test_arguments_and_results_pass_through_untouched():
    lib, marker = FakeLib(), object()
    with proxy(lib, FakeStream(), FakeStream(), Delays()) as ins:
        assert ins.obia_label_edges_u8_dev("h", 1, marker, key=marker) == ("edges", "h", (1, marker), {"key": marker})
        assert lib.obia_label_edges_u8_dev.calls == [(("h", 1, marker), {"key": marker})]
        fn = ins.obia_label_edges_u8_dev
        assert fn.argtypes == ["handle"] and fn.restype is int              # attributes are the real function's
        fn.argtypes = ["other"]
        assert lib.obia_label_edges_u8_dev.argtypes == ["other"]
        assert ins.some_value == 11
        ins.some_value = 12
        assert lib.some_value == 12
        with pytest.raises(AttributeError):
            ins.obia_not_exported
        assert ins.obia_label_edges_u8_dev is fn                            # one wrapper per name


def test_bookkeeping_and_context_free_calls_are_left_alone():
    lib, delays = FakeLib(), Delays()
    t, s = FakeStream(), FakeStream()
    with proxy(lib, t, s, delays) as ins:
        for name in ("obia_workspace_bytes", "obia_tiler_next_id", "obia_abi_version", "obia_create"):
            assert getattr(ins, name) is getattr(lib, name), name
        assert ins.obia_workspace_bytes("h") == 4096 and ins.obia_abi_version() == 2 and ins.obia_create(0) == "ctx"
    assert ins.log == [] and delays.on == [] and not t.busy and not s.busy
    for name in ("obia_workspace_bytes", "obia_set_profiling", "obia_last_timing", "obia_crowns_last_work", "obia_seedtab_last_work",
                 "obia_test_cc_report", "obia_test_visited_nonzero"):
        assert name in SO.BOOKKEEPING and len(SO.BOOKKEEPING[name]) > 20
    assert not set(SO.BOOKKEEPING) & set(SO.CONTEXT_FREE)


def test_a_call_entered_with_torch_busy_is_logged_idle_false():
    lib, t = FakeLib(), FakeStream(busy=True)
    with proxy(lib, t) as ins:
        ins.obia_label_edges_u8_dev("h")                                     # busy, but nothing was dispatched inside the block
        ins.note()
        ins.obia_label_edges_u8_dev("h")                                     # busy with work queued inside the block
        t.busy = False
        ins.obia_label_edges_u8_dev("h")
        t.busy = True
        ins.obia_label_edges_u8_dev("h")                                     # busy, but nothing was dispatched since the last return
        ins.note()
        ins.obia_label_edges_u8_dev("h")                                     # busy with work the wrapper queued and did not wait for
    assert [r.idle_t for r in ins.log] == [True, False, True, True, False]
    assert all(r.pending_s is None for r in ins.log)                        # no visible context stream: that side is not judged
    assert all(r.t_out >= r.t_in for r in ins.log) and [r.t_in for r in ins.log] == sorted(r.t_in for r in ins.log)


def test_a_call_that_returns_with_the_context_stream_busy_is_logged_pending():
    lib, t, s = FakeLib(), FakeStream(), FakeStream()

    def synchronous(h):
        s.busy = False                                                     # waits for the stream, the delay in front included
        return 0
    lib.obia_label_edges_u8_dev = FakeFn(synchronous)
    delays = Delays()
    with proxy(lib, t, s, delays) as ins:
        ins.obia_image_stretch_u8_dev("h")                                   # queues and returns
        assert delays.on == [s, t]                                           # in front of the call on s, behind it on t
        ins.obia_label_edges_u8_dev("h")
        assert delays.on == [s, t, s]                                        # (t's first delay still runs: no second one on top)
        ins.obia_synchronize("h")
        assert delays.on == [s, t, s]                                        # no delay in front of the wait itself
        t.busy = False
        ins.obia_image_stretch_u8_dev("h")
        assert delays.on == [s, t, s, s, t]
    assert [(r.name, r.pending_s) for r in ins.log] == [("obia_image_stretch_u8_dev", True), ("obia_label_edges_u8_dev", False),
                                                        ("obia_synchronize", False), ("obia_image_stretch_u8_dev", True)]
    assert all(r.idle_t for r in ins.log)                                  # the proxy's own delay on t is not the wrapper's work


def test_a_refused_call_is_told_from_a_served_one():
    lib = FakeLib()
    lib.obia_image_stretch_u8_dev = FakeFn(lambda h, *a: -1)                 # OBIA_E_INVALID
    lib.obia_tiler_create = FakeFn(lambda h: 140737488355328)                # a pointer
    lib.obia_destroy = FakeFn(lambda h: None)                                # void
    with proxy(lib, FakeStream()) as ins:
        ins.obia_image_stretch_u8_dev("h"), ins.obia_synchronize("h"), ins.obia_tiler_create("h"), ins.obia_destroy("h")
    assert [(r.result, r.refused) for r in ins.log] == [(-1, True), (0, False), (140737488355328, False), (None, False)]
    # with delays: the one in front of a refused call is waited for (it was logged as pending first), a served call's is not
    s, delays = FakeStream(), Delays()
    with proxy(lib, FakeStream(), s, delays) as ins:
        ins.obia_image_stretch_u8_dev("h")
        assert s.waits == 1 and not s.busy
        ins.obia_label_edges_u8_dev("h")
        assert s.waits == 1 and s.busy
    assert [r.pending_s for r in ins.log] == [True, True]


def test_logging_only_queues_nothing():
    lib, t, s = FakeLib(), FakeStream(), FakeStream()
    with proxy(lib, t, s, None) as ins:
        ins.obia_image_stretch_u8_dev("h")
        ins.obia_label_edges_u8_dev("h")
    assert not t.busy and not s.busy and [r.pending_s for r in ins.log] == [False, False]


def test_gap_and_delay_rule():
    R = SO.Record
    log = [R(("a", True, None, 0.0, 1.0, 0)), R(("b", True, None, 1.002, 2.0, 0)), R(("c", True, None, 2.0005, 3.0, 0))]
    assert abs(SO.largest_gap(log) - 0.002) < 1e-12 and SO.largest_gap(log[:1]) == 0.0 and SO.largest_gap([]) == 0.0
    assert abs(SO.delay_ms_for(0.002) - 8.0) < 1e-9 and SO.delay_ms_for(0.0001) == SO.MIN_MS == 5.0
    assert SO.delay_ms_for(0.030) > SO.MAX_MS == 100.0                       # the caller must split such a case
    with pytest.raises(ValueError):
        SO.Delay(100.1)
    with pytest.raises(ValueError):
        SO.Delay(-1.0)


def test_which_torch_operators_count_as_work():
    torch = pytest.importorskip("torch")
    from torch.utils._python_dispatch import TorchDispatchMode
    seen = {}

    class Watch(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            out = func(*args, **(kwargs or {}))
            seen[func._schema.name.split("::")[-1]] = (SO.queues_work(func, args, kwargs, out, cuda_only=False),
                                                       SO.queues_work(func, args, kwargs, out))
            return out
    with Watch():
        a = torch.empty(4, 3)
        a.fill_(1.0)
        a.view(12), a[1:], a.t(), a.reshape(3, 4)
        a.to(torch.float64), a.t().contiguous(), a.sum(), a + a
        a.copy_(a)
    for name in ("empty", "view", "slice", "t"):
        assert seen[name] == (False, False), name
    for name in ("fill_", "_to_copy", "clone", "sum", "add", "copy_"):
        assert seen[name] == (True, False), name                           # work -- but not on a CUDA tensor, so it is not counted


def test_the_tables_of_the_gpu_suite_hold_together():
    """the asynchronous table against the headers, the exceptions of the completeness test against what obia_amd/_lib.py binds"""
    pytest.importorskip("torch")
    from tests import test_gpu_stream_order as T
    from tests import workspace_history as WH
    T.test_the_asynchronous_table_is_the_headers()
    bound = set(WH.bound_entry_points())
    assert T.ASYNC <= bound and set(T.NOT_OBSERVED) <= bound and not T.ASYNC & set(T.NOT_OBSERVED)
    assert T.IDLE_EXEMPT == {}
    assert all(not name.startswith("guards:") for name in T.CASES) and len(T.NEW) >= 37
    assert set(T.REUSED) == {name for name in T.WHT.OPS if not name.startswith("guards:")}
