"""The grids of the clamped launches as the library states them (test helper, not a conftest): obia_test_launch_grid
(include/obia_testing.h; obia_amd/csrc/launch_grids.hpp) needs no GPU, so a test can ask whether its shape reaches the second trip of
a stride loop -- and tests/test_launch_grids_cpu.py asks it of every shape tests/test_gpu_launch_clamps.py uses.

`CASES` are those shapes.  None of them is a literal threshold: `crossing()` searches the library's own answer for the smallest size
with two trips, so a retuned clamp moves the shapes with it."""
import ctypes
import functools

import numpy as np

SIZE_MAX = 2 ** 31 - 1                    # the entry point's documented maximum of every size
NP_MAX = 65535                            # ... but of `np`, the problems of one batch
AXIS = {"x": 2, "y": 3}                   # index of an axis' trips in {grid.x, grid.y, trips.x, trips.y}


@functools.lru_cache(maxsize=None)
def names():
    """{name: (size name, ...)} of every launch the library names"""
    from obia_amd import _lib
    text = ctypes.create_string_buffer(1 << 14)
    assert _lib.load().obia_test_launch_grid_names(text, len(text)) == _lib.OBIA_OK, _lib.last_error()
    out = {}
    for line in text.value.decode().splitlines():
        w = line.split()
        out[w[0]] = tuple(w[1:])
    return out


@functools.lru_cache(maxsize=None)
def grid(name, *sizes):
    """(grid.x, grid.y, trips.x, trips.y) of the launch `name` at `sizes`"""
    from obia_amd import _lib
    s = np.array(sizes, np.int64)
    out = np.zeros(4, np.int64)
    rc = _lib.load().obia_test_launch_grid(name.encode(), s.ctypes.data, len(s), out.ctypes.data)
    assert rc == _lib.OBIA_OK, (name, sizes, _lib.last_error())
    return tuple(int(v) for v in out)


def size_max(size_name):
    return NP_MAX if size_name == "np" else SIZE_MAX


def trips(name, sizes, axis):
    return grid(name, *sizes)[AXIS[axis]]


@functools.lru_cache(maxsize=None)
def crossing(name, sizes, vary, axis):
    """the smallest value of sizes[vary] (the others as given) at which `axis` takes two trips, or None when no size up to SIZE_MAX
    does (65535 for `np`).  Trips do not decrease with a size: bisection."""
    def t(v):
        s = list(sizes)
        s[vary] = v
        return trips(name, tuple(s), axis)
    top = size_max(names()[name][vary])
    if t(top) < 2:
        return None
    lo, hi = 1, top                  # t(hi) >= 2; t(lo - 1) < 2 by convention
    while lo < hi:
        mid = (lo + hi) // 2
        if t(mid) >= 2:
            hi = mid
        else:
            lo = mid + 1
    return lo


@functools.lru_cache(maxsize=None)
def unit(name, sizes, vary, axis):
    """the largest value of sizes[vary] (the others as given) that `axis` still gives ONE workgroup: what a workgroup takes per trip
    on that axis -- the column tile of `rast_large`, the side of a pair tile of `seeds_pairs`.  Workgroups do not decrease with a
    size: bisection."""
    def g(v):
        s = list(sizes)
        s[vary] = v
        return grid(name, *s)[AXIS[axis] - 2]
    lo, hi = 1, size_max(names()[name][vary])                  # g(lo) == 1, g(hi) >= 2
    assert g(lo) == 1 and g(hi) >= 2, (name, sizes, vary, axis)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if g(mid) >= 2:
            hi = mid
        else:
            lo = mid
    return lo


def not_multiple(n, m):
    """n, or the next size that is no multiple of m (the byte-chunking kernels: a head or tail of its own)"""
    return n if m == 1 or n % m else n + 1


class Case:
    """One shape of tests/test_gpu_launch_clamps.py: the launch it is about, the sizes it gives that launch, the axis whose second
    trip it is there for, and -- for a case that shows the threshold -- the index of the size of which one fewer takes one trip."""

    def __init__(self, launch, sizes, axis, threshold=None):
        self.launch, self.sizes, self.axis, self.threshold = launch, tuple(int(s) for s in sizes), axis, threshold


def _rows(launch, W):
    return Case(launch, (crossing(launch, (1, W), 0, "y"), W), "y", threshold=0)


def _flat(launch, extra=(), chunk=1):
    n = crossing(launch, (1,) + tuple(extra), 0, "x")
    m = not_multiple(n, chunk)
    return Case(launch, (m,) + tuple(extra), "x", threshold=0 if m == n else None)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    # rows past grid.y: tall, narrow rasters
    c["boundaries_rows"] = c["mark_rows"] = _rows("image_rows", 5)
    c["cost_combine_rows"] = _rows("cost_rows", 5)
    c["cost_sobel_rows"] = _rows("cost_sobel", 3)
    c["cost_entropy_rows"] = _rows("cost_entropy", 3)
    c["seeds_flag_rows"] = _rows("seeds_flag", 3)
    c["clahe_rows"] = _rows("image_clahe_interp", 8)                      # 8: the narrowest raster CLAHE takes
    c["quickshift_rows"] = _rows("quickshift_density", 1)
    c["label_edges_rows"] = Case("label_edges", (crossing("label_edges", (1,), 0, "x"),), "x", threshold=0)
    # columns past grid.x
    c["boundaries_cols"] = c["mark_cols"] = Case("image_rows", (3, crossing("image_rows", (3, 1), 1, "x")), "x", threshold=1)
    c["cost_edge_count_cols"] = Case("cost_edge_count", (300, crossing("cost_edge_count", (300, 1), 1, "x")), "x", threshold=1)
    # flat arrays past 8192 workgroups (or the launch's own clamp); byte-chunking kernels get a length that is no multiple of 4 / 12
    c["stretch"] = _flat("image_stretch", chunk=4)
    c["lut_rep1"] = _flat("image_lut", (1,), chunk=4)
    c["lut_rep3"] = _flat("image_lut", (3,), chunk=4)
    c["gray_hist"] = _flat("image_gray_hist", chunk=4)
    c["compose"] = Case("training_compose", (1399 * -(-crossing("training_compose", (1,), 0, "x") // 1399),), "x")     # 1399 rows
    c["minmax_scale"] = _flat("training_minmax_scale", chunk=4)
    c["sharpness_minmax"] = Case("sharpness_minmax", (727 * -(-crossing("sharpness_minmax", (1,), 0, "x") // 727),), "x")   # 727 columns
    c["flat_plane"] = Case("flat", (1025 * 2049,), "x")                     # a 1025 x 2049 plane: the sharpness copies, the point rasters
    c["flat"] = _flat("flat")                                               # boxes fill / winner / dissolve, crowns init / finish, points rasters / finish
    c["scale_transform"] = Case("scale_transform", (crossing("scale_transform", (1, 129), 0, "x"), 129), "x", threshold=0)
    c["boxes_iou_a"] = Case("boxes_iou", (crossing("boxes_iou", (1, 3), 0, "y"), 3), "y", threshold=0)
    c["boxes_iou_b"] = Case("boxes_iou", (2, crossing("boxes_iou", (2, 1), 1, "x")), "x", threshold=1)
    c["points_segments"] = Case("points_segments", (crossing("points_segments", (1,), 0, "x") + 257,), "x")
    # the seed merge: pair tiles past grid.x; the rasteriser's large shapes: vertices of one shape, column tiles of one band
    c["seeds_pairs"] = Case("seeds_pairs", (crossing("seeds_pairs", (1,), 0, "x") + 37,), "x")
    c["rast_band_bin"] = Case("rast_band_bin", (1, crossing("rast_band_bin", (1, 1), 1, "y") + 300), "y")
    c["rast_large"] = Case("rast_large", (2, crossing("rast_large", (2, 1), 1, "y") + 40), "y")       # two bands: 9 rows
    # masked SLIC on one tall window (rows of four per workgroup and trip), the seam import of the sharded driver
    c["slic_mask_pack"] = Case("slic_mask_pack", (crossing("slic_mask_pack", (1, 1), 0, "x") + 150, 1), "x")
    c["tiler_seam"] = Case("tiler_seam", (crossing("tiler_seam", (1,), 0, "x") + 257,), "x")          # tests/test_gpu_seam_import.py
    return c


def check(case):
    """the case's shape takes at least two trips on its axis; one fewer of its threshold size takes exactly one"""
    assert trips(case.launch, case.sizes, case.axis) >= 2, (case.launch, case.sizes, grid(case.launch, *case.sizes))
    if case.threshold is not None:
        s = list(case.sizes)
        s[case.threshold] -= 1
        assert trips(case.launch, tuple(s), case.axis) == 1, (case.launch, s, grid(case.launch, *s))
