"""The entry point of include/obia_shapes.h through guarded outputs (tests/guarded.py, both poisons) with the labels off a 16-byte
boundary (tests/offset_views.py): the tables bit for bit, no stray write, no element left unwritten, the input unchanged, two runs
equal; what is refused writes nothing and leaves the context as it was; the call on a context whose workspace was filled by
obia_test_poison_workspace_dev equals the same call on a fresh context; and the wrapper under tests/stream_order.py: an input
produced late on torch's stream is waited for, and the context's stream is idle when the wrapper returns.  obia_amd._lib._SHAPE_ENTRIES
is no *_SIGNATURES or *_BINDINGS table, so the decision tables of tests/workspace_history.py and tests/test_gpu_stream_order.py do not
list it: these are the equivalent checks.  Every entry point of the table is exercised here."""
import ctypes
import functools

import numpy as np
import pytest

from tests import shapes_restatement as S
from tests import stream_order as SO
from tests.guarded import POISONS, guarded, snapshot, unchanged
from tests.offset_views import offset_view, residue

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EXERCISED = ("obia_shape_sums_dev",)
I32, I64 = np.int32, np.int64
TH, TW = 16, 32
H, W, START, N = 2 * TH + 3, 2 * TW + 5, 1, 12


@functools.lru_cache(maxsize=None)
def case():
    rs = np.random.RandomState(29)
    labels = np.kron(rs.randint(-1, N + 2, (-(-H // 3), -(-W // 4))), np.ones((3, 4), int))[:H, :W].astype(I32)
    labels[labels == 5] = 4                                                    # label 5 occurs nowhere: a row of zeros that must be written
    sums, box = S.tables(labels, START, N)
    assert (sums[:, 0] > 0).sum() == N - 1 and not sums[4].any() and (labels < START).any() and (labels >= START + N).any()
    return dict(labels=labels, sums=sums, box=box)


def dev_off(a, k):
    t = offset_view(torch.as_tensor(np.ascontiguousarray(a)).cuda(), k)
    torch.cuda.synchronize()
    return t


def run_all(ctx, k, poison):
    """the entry point on guarded outputs, the labels k elements off a boundary; returns (outputs, inputs)"""
    from obia_amd import _lib
    lib = _lib.load()
    r = case()
    ins = {"labels": dev_off(r["labels"], k)}
    o = {"sums": guarded((N, 7), I64, poison, "cuda", k), "box": guarded((N, 4), I32, poison, "cuda", k)}
    rc = lib.obia_shape_sums_dev(ctx.handle, ins["labels"].data_ptr(), H, W, START, N, o["sums"].ptr, o["box"].ptr)
    assert rc == 0, (rc, _lib.last_error())
    torch.cuda.synchronize()
    return o, ins


def judge_all(o):
    r = case()
    got = {name: g.host() for name, g in o.items()}
    for name, g in o.items():
        assert S.same_bits(got[name], r[name]), name
        assert g.findings(name=name) == []                                   # no stray write, every element written
    return got


def test_every_entry_point_of_the_table_is_exercised():
    from obia_amd import _lib
    assert set(EXERCISED) == set(_lib._SHAPE_ENTRIES)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("poison", POISONS, ids=[f"{p:02X}" for p in POISONS])
def test_buffers_off_the_boundary_and_guarded_outputs(k, poison):
    """the labels and the box 4, 8 and 12 bytes past a 16-byte boundary, the sums 8 bytes (k odd)"""
    from obia_amd import _lib
    ctx = _lib.default_context(0)
    runs = []
    for _ in range(2):
        o, ins = run_all(ctx, k, poison)
        assert residue(ins["labels"]) == 4 * k and o["box"].ptr % 16 == 4 * k and o["sums"].ptr % 16 == (8 * k) % 16
        snap = snapshot(ins["labels"])
        got = judge_all(o)
        assert unchanged(ins["labels"], snap) and np.array_equal(ins["labels"].cpu().numpy(), case()["labels"])
        runs.append({name: a.tobytes() for name, a in got.items()})
    assert runs[0] == runs[1]


@pytest.mark.parametrize("poison", POISONS, ids=[f"{p:02X}" for p in POISONS])
def test_refusals_write_nothing_and_leave_the_context_intact(poison):
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.Context(0)
    try:
        r, k = case(), 1
        ins = dev_off(r["labels"], k)
        snap = snapshot(ins)
        L = ins.data_ptr()
        g = {"s": guarded((N, 7), I64, poison, "cuda", k), "b": guarded((N, 4), I32, poison, "cuda", k)}
        s, b = g["s"].ptr, g["b"].ptr
        held = ctx.workspace_bytes()

        def sh(l_=L, H_=H, W_=W, st=START, n_=N, s_=s, b_=b):
            return lib.obia_shape_sums_dev(ctx.handle, l_, H_, W_, st, n_, s_, b_)

        invalid = [sh(l_=None), sh(l_=L + 2), sh(s_=None), sh(b_=None), sh(s_=s + 4), sh(b_=b + 2), sh(H_=0), sh(W_=-3), sh(H_=-1, W_=-1), sh(n_=-1),
                   sh(n_=2 ** 31 - 2), sh(s_=L), sh(b_=L), sh(s_=b), sh(n_=0, l_=None)]
        assert invalid == [_lib.E_INVALID] * len(invalid), invalid
        assert "null, misaligned or overlapping" in _lib.last_error()
        unsupported = [sh(H_=65536, W_=32768), sh(H_=46341, W_=46341), sh(H_=1, W_=2 ** 21), sh(H_=2 ** 21, W_=1), sh(H_=1024, W_=2 ** 21 - 1)]
        assert unsupported == [_lib.E_UNSUPPORTED] * len(unsupported), unsupported
        torch.cuda.synchronize()
        assert all(v.untouched() and v.stray().size == 0 for v in g.values()) and unchanged(ins, snap)
        # a call that has nothing to do is valid and writes nothing
        assert sh(n_=0) == 0 and sh(n_=0, s_=None, b_=None) == 0
        torch.cuda.synchronize()
        assert all(v.untouched() and v.stray().size == 0 for v in g.values()) and ctx.workspace_bytes() == held
        # and the context serves the next call as a fresh one would
        assert sh() == 0
        torch.cuda.synchronize()
        assert S.same_bits(g["s"].host(), r["sums"]) and S.same_bits(g["b"].host(), r["box"])
        assert g["s"].findings(name="sums") == [] and g["b"].findings(name="box") == [] and ctx.workspace_bytes() == held
    finally:
        ctx.close()


@pytest.mark.parametrize("byte", [0x01, 0xFF])
def test_a_used_context_gives_what_a_fresh_one_gives(byte):
    """the entry point on a fresh context against the same call on a context whose workspace, one block of 64 MiB, holds `byte` in
    every byte: equal bit for bit, twice, and the context holds what it held -- the call takes nothing from the workspace"""
    from obia_amd import _lib
    lib = _lib.load()
    fresh, used = _lib.Context(0), _lib.Context(0)
    try:
        want = {name: a.tobytes() for name, a in judge_all(run_all(fresh, 1, POISONS[0])[0]).items()}
        held, nz = ctypes.c_int64(-1), ctypes.c_int64(-1)
        torch.cuda.synchronize()
        _lib.check(lib.obia_test_poison_workspace_dev(used.handle, 64 << 20, byte, ctypes.byref(held), ctypes.byref(nz)))
        assert held.value >= 64 << 20 and used.workspace_bytes() == held.value
        for _ in range(2):
            assert {name: a.tobytes() for name, a in judge_all(run_all(used, 1, POISONS[0])[0]).items()} == want
            assert used.workspace_bytes() == held.value
    finally:
        fresh.close()
        used.close()


# ------------------------------------------------------------------------------------------------------------------ stream order
DELAY_MS = 20.0      # the wrapper makes one ABI call, so there is no host gap to scale by: four times tests/stream_order.py's MIN_MS


@pytest.mark.parametrize("arrangement", ["A", "B", "C"])
def test_stream_order_of_the_wrapper(arrangement):
    """A: torch on a fresh stream t, the context on a stream of its own, the labels late on t (they hold 0x5A bytes until a delay has
    passed): at the ABI entry t is idle and the result is right.  B: the context on a second torch stream s with a delay in front of
    the call's kernels: the call returns with s idle (the header: "the call returns with its work done").  C: the context on t."""
    from obia_amd import _lib, segment_shapes
    real, r = _lib.load(), case()
    t = torch.cuda.Stream()
    s = torch.cuda.Stream() if arrangement == "B" else None
    delay = None if arrangement == "C" else SO.Delay(DELAY_MS)
    with torch.cuda.stream(t):
        ctx = _lib.Context(0, stream={"A": None, "B": s and s.cuda_stream, "C": t.cuda_stream}[arrangement])
        try:
            with SO.Instrumented(real, t, s, delay) as ins:
                lab = torch.as_tensor(r["labels"]).cuda()
                if delay is not None:
                    lab = SO.late(lab, t, delay)
                table = segment_shapes(lab, START, n_labels=N, ctx=ctx)
                s_idle = s is None or s.query()
                got = (table.sums.cpu().numpy(), table.box.cpu().numpy(), table.orientation.cpu().numpy())
        finally:
            t.synchronize()
            if s is not None:
                s.synchronize()
            ctx.close()
    log = [rec for rec in ins.log if rec.name in EXERCISED]
    assert len(log) == 1 and [rec.name for rec in ins.log] == list(EXERCISED), [rec.name for rec in ins.log]
    assert log[0].idle_t and not log[0].refused, "entered with torch's stream busy"
    assert s_idle and not log[0].pending_s, "the context's stream was still busy when the call returned"
    assert S.same_bits(got[0], r["sums"]) and S.same_bits(got[1], r["box"])
    want = S.derived(r["sums"], r["box"])["orientation"]
    assert np.array_equal(np.isnan(got[2]), np.isnan(want)) and np.nanmax(np.abs(got[2] - want)) <= 8 * 2.22e-16   # ORIENTATION_BOUND of tests/test_gpu_shapes.py
