"""The wave and workgroup primitives of obia_amd/csrc/wave_ops.hpp, driven one at a time through obia_test_wave_ops_dev
(include/obia_testing.h) at every (primitive, workgroup size) pair the library's kernels instantiate, against numpy.cumsum / sum.

Sizes: 0, 1, around one wave (63, 64, 65), around one workgroup (nt - 1, nt, nt + 1: at nt + 1 a thread of the one-workgroup scan owns
two elements while the trailing threads own none), 2 nt + 3, and 3 nt (every chunk full).  For the per-workgroup primitives the last
workgroup is partial at every size that is no multiple of nt.  Outputs lie between poisoned guards (tests/guarded.py): nothing next to
them is written, no element is left out.  Everything is an integer: array_equal, no tolerance."""
import numpy as np
import pytest

from tests.guarded import guarded

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SCAN_IN_PLACE, SCAN_I32, SCAN_I64, BLOCK_SCAN, BLOCK_SUM, BLOCK_FLAG_RANK, BLOCK_SCAN_TWICE = range(7)
# include/obia_testing.h: exactly these are served
PAIRS = [(SCAN_IN_PLACE, 1024), (SCAN_I32, 1024), (SCAN_I64, 256), (SCAN_I64, 1024), (BLOCK_SCAN, 256), (BLOCK_SCAN, 1024),
         (BLOCK_SUM, 256), (BLOCK_SUM, 1024), (BLOCK_FLAG_RANK, 256), (BLOCK_SCAN_TWICE, 256), (BLOCK_SCAN_TWICE, 1024)]
POISON = 0xA5


def sizes(nt):
    return [0, 1, 63, 64, 65, nt - 1, nt, nt + 1, 2 * nt + 3, 3 * nt]


def wave_ops(op, nt, values, ctx=None):
    """obia_test_wave_ops_dev on `values` (int32): (out, totals) as int64 arrays, after the guards of both were checked"""
    from obia_amd import _device, _lib
    values = np.ascontiguousarray(values, np.int32)
    n = len(values)
    x = torch.as_tensor(values).cuda() if n else torch.zeros(0, dtype=torch.int32, device="cuda")
    out = guarded((n,), np.int64, POISON, "cuda")
    totals = guarded((1 if op <= SCAN_I64 else -(-n // nt),), np.int64, POISON, "cuda")
    lib, c = _device.begin(0, ctx)
    _lib.check(lib.obia_test_wave_ops_dev(c.handle, op, nt, x.data_ptr(), n, out.ptr, totals.ptr))
    assert out.findings(name="out") + totals.findings(name="totals") == []
    return out.host(), totals.host()


def exclusive(v):
    v = np.asarray(v, np.int64)
    return np.cumsum(v) - v


def expected(op, nt, values):
    """(out, totals) by numpy"""
    v = np.asarray(values, np.int64)
    if op <= SCAN_I64:
        return exclusive(v), np.array([v.sum()], np.int64)
    if op == BLOCK_FLAG_RANK:
        v = (v != 0).astype(np.int64)
    if op == BLOCK_SCAN_TWICE:
        v = v + 1
    blocks = [v[b:b + nt] for b in range(0, len(v), nt)]
    each = [np.full(len(b), b.sum()) if op == BLOCK_SUM else exclusive(b) for b in blocks]
    return (np.concatenate(each) if each else np.zeros(0, np.int64)).astype(np.int64), np.array([b.sum() for b in blocks], np.int64)


def value_sets(op, n):
    sets = {"random 0..7": np.random.RandomState(1234 + n).randint(0, 8, n), "zeros": np.zeros(n, np.int64)}
    if op == BLOCK_FLAG_RANK:
        last = np.zeros(n, np.int64)
        if n >= 64:
            last[n // 64 * 64 - 1] = 1                                         # lane 63 of the last whole wave, nothing else
        sets.update({"all set": np.ones(n, np.int64), "lane 63 of the last wave": last})
    return sets


@pytest.mark.parametrize("op,nt", PAIRS)
def test_primitive_equals_numpy(op, nt):
    for n in sizes(nt):
        for what, values in value_sets(op, n).items():
            got, want = wave_ops(op, nt, values), expected(op, nt, values)
            assert np.array_equal(got[0], want[0]), f"op {op}, nt {nt}, n {n}, {what}: out"
            assert np.array_equal(got[1], want[1]), f"op {op}, nt {nt}, n {n}, {what}: totals"


@pytest.mark.parametrize("nt", [256, 1024])
def test_int64_scan_passes_2_31(nt):
    values = np.full(5, 1 << 30, np.int64)
    out, totals = wave_ops(SCAN_I64, nt, values)
    assert np.array_equal(out, exclusive(values)) and totals.tolist() == [5 << 30] and totals[0] > 1 << 31


def test_in_place_equals_out_of_place():
    for n in sizes(1024):
        values = np.random.RandomState(99 + n).randint(0, 8, n)
        a, b = wave_ops(SCAN_IN_PLACE, 1024, values), wave_ops(SCAN_I32, 1024, values)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), n


def test_only_the_library_s_pairs_are_served():
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.default_context(0)
    x = torch.zeros(8, dtype=torch.int32, device="cuda")
    out, totals = torch.zeros(8, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def call(op, nt, x_ptr=x.data_ptr(), n=8, out_ptr=out.data_ptr(), totals_ptr=totals.data_ptr(), handle=ctx.handle):
        return lib.obia_test_wave_ops_dev(handle, op, nt, x_ptr, n, out_ptr, totals_ptr)
    served = set(PAIRS)
    for op in range(-1, 9):
        for nt in (0, 64, 128, 256, 512, 1024, 2048):
            assert (call(op, nt) == _lib.OBIA_OK) == ((op, nt) in served), (op, nt)
    assert call(BLOCK_SUM, 256, handle=None) == _lib.E_INVALID
    assert call(BLOCK_SUM, 256, x_ptr=None) == _lib.E_INVALID
    assert call(BLOCK_SUM, 256, out_ptr=None) == _lib.E_INVALID
    assert call(BLOCK_SUM, 256, totals_ptr=None) == _lib.E_INVALID
    assert call(BLOCK_SUM, 256, totals_ptr=out.data_ptr()) == _lib.E_INVALID
    assert call(BLOCK_SUM, 256, out_ptr=out.data_ptr() + 4) == _lib.E_INVALID
    assert call(BLOCK_SUM, 256, n=-1) == _lib.E_INVALID
    totals.fill_(7)
    torch.cuda.synchronize()
    assert call(SCAN_I64, 256, x_ptr=None, n=0, out_ptr=None) == _lib.OBIA_OK and int(totals.cpu()[0]) == 0
