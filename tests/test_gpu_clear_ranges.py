"""clear_ranges_kernel (obia_amd/csrc/context.cpp), the one launch that stands for a tile batch's neighbouring fills, driven through
its test entry obia_test_clear_ranges_dev (include/obia_testing.h).  Every range lies in one byte arena that is filled with a guard
pattern first; after the call every byte inside a range must hold the range's value and every other byte of the arena the pattern
it had: nothing left unwritten, nothing written outside -- at every start offset from a 16-byte boundary (the kernel stores 16 bytes
at a time and single bytes in front of and behind them), at lengths below, at and above one store, above one workgroup's share, and
with ranges that touch each other."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LENGTHS = [0, 1, 15, 16, 17, 4097, (1 << 20) + 3]
OFFSETS = [0, 1, 4, 15]
VALUES = [0x00, 0x01, 0xff]


def guard_pattern(n):
    """no byte equals 0x00, 0x01 or 0xff: an unwritten byte inside a range cannot pass for a written one"""
    return torch.as_tensor((np.arange(n, dtype=np.int64) * 7 % 250 + 2).astype(np.uint8)).cuda()


def run(ranges, arena_bytes):
    """ranges: (start, length, value) in an arena whose base is 256-byte aligned.  Returns the arena before and after, on the host."""
    from obia_amd import _lib
    raw = guard_pattern(arena_bytes + 256)
    skew = (-raw.data_ptr()) % 256
    arena = raw[skew:skew + arena_bytes]
    assert arena.data_ptr() % 256 == 0
    before = arena.cpu().numpy().copy()
    n = len(ranges)
    ptrs = (ctypes.c_void_p * max(n, 1))(*[arena.data_ptr() + s for s, _, _ in ranges])
    lens = (ctypes.c_int64 * max(n, 1))(*[ln for _, ln, _ in ranges])
    vals = (ctypes.c_int32 * max(n, 1))(*[v for _, _, v in ranges])
    ctx = _lib.Context(0)
    _lib.check(_lib.load().obia_test_clear_ranges_dev(ctx.handle, ptrs, lens, vals, n))
    fills = ctx.timing()["fills"]
    torch.cuda.synchronize()
    return before, arena.cpu().numpy(), fills


def verify(ranges, before, after, what):
    want = before.copy()
    for s, ln, v in ranges:
        want[s:s + ln] = v
    bad = np.nonzero(after != want)[0]
    inside = np.zeros(len(before), bool)
    for s, ln, _ in ranges:
        inside[s:s + ln] = True
    print(f"{what}: {len(ranges)} ranges, {int(inside.sum())} bytes inside, {len(bad)} bytes wrong"
          + (f" (first at {bad[0]}: {after[bad[0]]:#x}, wanted {want[bad[0]]:#x}, {'inside' if inside[bad[0]] else 'a guard byte'})" if len(bad) else ""))
    assert not len(bad), f"{what}: {len(bad)} bytes wrong, the first at {bad[0]} ({'inside a range' if inside[bad[0]] else 'a guard byte'})"


def lay_out(specs, gap=48):
    """(offset from a 16-byte boundary, length, value) -> (start, length, value), `gap` guard bytes or more between two ranges"""
    ranges, pos = [], 64
    for off, ln, v in specs:
        start = (pos + 15) // 16 * 16 + off
        ranges.append((start, ln, v))
        pos = start + ln + gap
    return ranges, pos + 64


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("value", VALUES)
def test_two_ranges_every_length_pair(offset, value):
    """every length beside every other length, both at the same offset from a boundary, in sets of two (a set of two is the smallest
    the kernel runs for; the grid is sized by the longer range)"""
    other = {0x00: 0xff, 0x01: 0x00, 0xff: 0x01}[value]
    for a in LENGTHS:
        b = LENGTHS[(LENGTHS.index(a) + 3) % len(LENGTHS)]
        ranges, size = lay_out([(offset, a, value), (offset, b, other)])
        before, after, fills = run(ranges, size)
        verify(ranges, before, after, f"offset {offset}, lengths {a} + {b}, values {value:#x} / {other:#x}")
        assert fills == (1 if a and b else (1 if a or b else 0))


@pytest.mark.parametrize("offset", OFFSETS)
def test_one_range_is_a_plain_fill(offset):
    for ln in LENGTHS:
        ranges, size = lay_out([(offset, ln, 0xff)])
        before, after, fills = run(ranges, size)
        verify(ranges, before, after, f"one range, offset {offset}, length {ln}")
        assert fills == (1 if ln else 0)


def test_sixteen_ranges_all_lengths_offsets_and_values():
    """one launch: all seven lengths, all four offsets and all three values, the longest range in the middle"""
    specs = [(OFFSETS[i % 4], LENGTHS[(i * 3) % 7], VALUES[i % 3]) for i in range(16)]
    assert {ln for _, ln, _ in specs} == set(LENGTHS)
    ranges, size = lay_out(specs)
    before, after, fills = run(ranges, size)
    verify(ranges, before, after, "sixteen ranges")
    assert fills == 1, "sixteen ranges are one launch"


def test_aligned_set_takes_the_vector_only_kernel():
    """every range starts and ends on a 16-byte boundary: the variant without byte stores"""
    specs = [(0, 16, 0x00), (0, 4096, 0xff), (0, (1 << 20) + 16, 0x01), (0, 0, 0xff), (0, 32, 0x00)]
    ranges, size = lay_out(specs)
    before, after, fills = run(ranges, size)
    verify(ranges, before, after, "aligned set")
    assert fills == 1


def test_adjacent_ranges():
    """ranges that touch: the last byte of one is the neighbour of the first byte of the next, at odd boundaries, with different
    values -- a store that ran one byte over would show in the neighbour"""
    ranges, pos = [], 64 + 5
    for i, ln in enumerate([1, 15, 16, 17, 4097, 1, (1 << 20) + 3, 15, 16, 0, 17, 33]):
        ranges.append((pos, ln, VALUES[i % 3]))
        pos += ln
    before, after, fills = run(ranges, pos + 64)
    verify(ranges, before, after, "adjacent ranges")
    assert fills == 1


def test_seventeen_ranges_are_two_launches():
    specs = [(OFFSETS[i % 4], 40 + i, VALUES[i % 3]) for i in range(17)]
    ranges, size = lay_out(specs)
    before, after, fills = run(ranges, size)
    verify(ranges, before, after, "seventeen ranges")
    assert fills == 2


def test_refusals():
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.Context(0)
    buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    one_ptr, one_len, one_val = (ctypes.c_void_p * 1)(buf.data_ptr()), (ctypes.c_int64 * 1)(-1), (ctypes.c_int32 * 1)(0)
    assert lib.obia_test_clear_ranges_dev(ctx.handle, one_ptr, one_len, one_val, 1) == _lib.E_INVALID
    assert lib.obia_test_clear_ranges_dev(ctx.handle, None, one_len, one_val, 1) == _lib.E_INVALID
    assert lib.obia_test_clear_ranges_dev(None, one_ptr, one_len, one_val, 1) == _lib.E_INVALID
    assert lib.obia_test_clear_ranges_dev(ctx.handle, (ctypes.c_void_p * 1)(None), (ctypes.c_int64 * 1)(8), one_val, 1) == _lib.E_INVALID
    assert lib.obia_test_clear_ranges_dev(ctx.handle, one_ptr, one_len, one_val, 0) == _lib.OBIA_OK
    assert int(buf.sum()) == 0
