"""The entry point of include/obia_shapes.h through guarded outputs (tests/guarded.py, both poisons) with the labels off a 16-byte
boundary (tests/offset_views.py): the tables bit for bit, no stray write, no element left unwritten, the input unchanged, two runs
equal; what is refused writes nothing and leaves the context as it was.  Every entry point of the table is exercised here.  (The
call on a poisoned workspace is the case `body:shapes` of tests/test_gpu_workspace_history.py, which runs run_all and judge_all below;
the wrapper's stream order is the case `shapes:segment_shapes` of tests/test_gpu_stream_order.py.)"""
import functools

import numpy as np
import pytest

from tests import shapes_restatement as S
from tests.guarded import POISONS, guarded, snapshot, unchanged
from tests.offset_views import offset_view, residue
from tests.refusal_text import refused_saying

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
        # ... in full: a null output, an output one byte on, an output where the labels start
        refused_saying("shapes: sums: bad arguments (null, misaligned or overlapping buffers)", sh, dict(s_=None), dict(b_=None), dict(s_=s + 1),
                       dict(b_=b + 1), dict(b_=L), dict(s_=b))
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
