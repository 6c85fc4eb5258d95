"""The grids of the clamped launches without a GPU (obia_amd/csrc/launch_grids.hpp through obia_test_launch_grid,
include/obia_testing.h; DESIGN.md, "Launch clamps").

A clamped launch lets its workgroups walk what is left in a stride loop, and the second trip of that loop runs only above the clamp.
Here: every named launch takes one trip at its threshold and two one work item above it; no grid leaves the device's limits
(grid.x <= 2^31 - 1, grid.y <= 65535) at any size up to the entry point's maxima; every launch site's function is in the table of
names; and every shape of tests/test_gpu_launch_clamps.py crosses the clamp it says it crosses."""
import itertools
import os
import re

import numpy as np
import pytest

from obia_amd import _lib
from tests import launch_grids as LG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "obia_amd", "csrc")

# launches none of whose axes is clamped: the grid grows with the input, the kernel's own loop bounds the work of a workgroup
UNCLAMPED = {"image_clahe_hist"}
SWEEP = (1, 2, 7, 255, 256, 257, 4096, 65535, 65536, 65537, (1 << 20) + 1, 1 << 24, (1 << 31) - 2, (1 << 31) - 1)
SMALL = (1, 3, 129)                       # the sizes held fixed while one is searched


def test_the_names_are_the_functions_the_launch_sites_call():
    names = LG.names()
    assert len(names) >= 40 and all(len(sizes) in (1, 2, 4) for sizes in names.values())
    used = set()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".cpp", ".hpp")) and f != "launch_grids.hpp":
            used |= set(re.findall(r"\bgrids::([a-z][a-z0-9_]*)\s*\(", open(os.path.join(CSRC, f)).read()))
    helpers = {"table", "image_clahe_hist_rows"}
    assert used - helpers <= set(names), f"launch sites call grid functions the table does not name: {sorted(used - helpers - set(names))}"
    # ... and no launch keeps a clamp of its own inside a dim3(...): the literals live in launch_grids.hpp
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(".hip"):
            for line in open(os.path.join(CSRC, f)):
                for inner in dim3_arguments(line.split("//")[0]):
                    assert not re.search(r"std::min|\b(2048|4096|8192|16384|65535|65536|262144)\b", inner), f"{f}: {line.strip()}"


def dim3_arguments(code):
    """the text inside every dim3( ... ) of a line of code"""
    out, at = [], 0
    while True:
        at = code.find("dim3(", at)
        if at < 0:
            return out
        depth, j = 1, at + 5
        while j < len(code) and depth:
            depth += {"(": 1, ")": -1}.get(code[j], 0)
            j += 1
        out.append(code[at + 5:j - 1])
        at = j


@pytest.mark.parametrize("name", sorted(LG.names()))
def test_one_trip_at_the_threshold_two_above(name):
    n = len(LG.names()[name])
    found = 0
    for fixed in SMALL:
        for vary in range(n):
            base = tuple(fixed for _ in range(n))
            if name == "tiles":
                base = (fixed, fixed, 64, 16)
                if vary >= 2:
                    continue
            for axis in ("x", "y"):
                at = LG.crossing(name, base, vary, axis)
                if at is None:
                    continue
                found += 1
                above, below = list(base), list(base)
                above[vary], below[vary] = at, at - 1
                assert at >= 2, (name, base, vary, axis)
                assert LG.trips(name, tuple(above), axis) == 2, (name, above, LG.grid(name, *above))
                assert LG.trips(name, tuple(below), axis) == 1, (name, below, LG.grid(name, *below))
    assert (found == 0) == (name in UNCLAMPED), f"{name}: {found} thresholds found"


@pytest.mark.parametrize("name", sorted(LG.names()))
def test_no_grid_leaves_the_device_limits(name):
    n = len(LG.names()[name])
    sweep = SWEEP if n <= 2 else SWEEP[::2] + (SWEEP[-1],)
    for sizes in itertools.product(*[[v for v in sweep if v <= LG.size_max(s)] for s in LG.names()[name]]):
        gx, gy, tx, ty = LG.grid(name, *sizes)
        assert 1 <= gx <= 2 ** 31 - 1 and 1 <= gy <= 65535 and tx >= 1 and ty >= 1, (name, sizes, (gx, gy, tx, ty))


def test_trips_never_decrease_with_a_size():
    """what `crossing` bisects on"""
    for name, sizes in LG.names().items():
        n = len(sizes)
        for vary in range(n if name != "tiles" else 2):
            last = (0, 0)
            for v in SWEEP:
                s = [5] * n if name != "tiles" else [5, 5, 64, 16]
                if v > LG.size_max(sizes[vary]):
                    break
                s[vary] = v
                g = LG.grid(name, *s)
                assert g[2] >= last[0] and g[3] >= last[1], (name, s, g, last)
                last = (g[2], g[3])


def test_bad_requests_are_refused():
    lib = _lib.load()
    out = np.zeros(4, np.int64)
    one = np.array([5], np.int64)
    assert lib.obia_test_launch_grid(b"no_such_launch", one.ctypes.data, 1, out.ctypes.data) == _lib.E_INVALID
    assert "no_such_launch" in _lib.last_error()
    assert lib.obia_test_launch_grid(b"flat", one.ctypes.data, 2, out.ctypes.data) == _lib.E_INVALID
    assert lib.obia_test_launch_grid(b"flat", np.array([0], np.int64).ctypes.data, 1, out.ctypes.data) == _lib.E_INVALID
    assert lib.obia_test_launch_grid(b"flat", np.array([1 << 31], np.int64).ctypes.data, 1, out.ctypes.data) == _lib.E_INVALID
    assert lib.obia_test_launch_grid(None, one.ctypes.data, 1, out.ctypes.data) == _lib.E_INVALID
    assert lib.obia_test_launch_grid_names(None, 0) == _lib.E_INVALID
    assert (out == 0).all()


@pytest.mark.parametrize("case", sorted(LG.cases()))
def test_every_gpu_case_crosses_its_clamp(case):
    LG.check(LG.cases()[case])


def test_a_unit_is_the_last_size_of_one_workgroup():
    """the column tile of the rasteriser's large shapes and the side of a pair tile of the seed merge, as the wide-shape and pair tests
    take them: one workgroup up to the unit, two from one more -- and the trips follow the units"""
    for name, sizes, vary, axis in (("rast_large", (1, 1), 1, "y"), ("seeds_pairs", (1,), 0, "x")):
        u = LG.unit(name, sizes, vary, axis)
        at, above = list(sizes), list(sizes)
        at[vary], above[vary] = u, u + 1
        k = LG.AXIS[axis] - 2
        assert u >= 32 and LG.grid(name, *at)[k] == 1 and LG.grid(name, *above)[k] >= 2, (name, u)     # (65 seeds: three pair tiles)
    T = LG.unit("rast_large", (1, 1), 1, "y")
    assert T % 32 == 0                                           # a tile is whole 32-bit words of the bit plane
    cap = LG.grid("rast_large", 1, LG.SIZE_MAX)[1]
    assert LG.crossing("rast_large", (1, 1), 1, "y") == cap * T + 1
    P = LG.unit("seeds_pairs", (1,), 0, "x")
    cap = LG.grid("seeds_pairs", LG.SIZE_MAX)[0]
    nt = -(-LG.crossing("seeds_pairs", (1,), 0, "x") // P)
    assert nt * (nt + 1) // 2 > cap >= (nt - 1) * nt // 2       # the first seed count whose tile pairs outnumber the workgroups


def test_the_two_grids_that_had_no_clamp_have_one():
    """quickshift's density / parent pass and the CLAHE interpolation put a row count into grid.y: clamped like their neighbours"""
    for name, W in (("quickshift_density", 1), ("image_clahe_interp", 8)):
        for H in ((1 << 24) + 1, (1 << 31) - 1):
            gx, gy, tx, ty = LG.grid(name, H, W)
            assert gy == 65535 and ty >= 2, (name, H, (gx, gy, tx, ty))
