"""The segment adjacency graph without a GPU: the restatement (tests/adjacency_restatement.py) against a double loop over pixels, its
components against SciPy, the perimeter against the pixel count; what the header says; what the source file must not do (take workspace, allocate,
use an atomic on anything but an integer, launch a grid of its own); the new row of the launch-grid table; and the refusals of the
Python functions that fire before the library is loaded."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from tests import adjacency_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rasters():
    """30 random rasters of at most 12 x 12: labels in -1 .. 6, start_label 1 or 0, n_labels 5 (so 0 or -1, and 6, are background)"""
    rs = np.random.RandomState(11)
    out = []
    for k in range(30):
        H, W = rs.randint(1, 13), rs.randint(1, 13)
        hi = (3, 7, 7)[k % 3]
        out.append((rs.randint(-1, hi, (H, W)).astype(np.int32), k % 2, 5))
    return out


def partition(labels):
    """the partition a labelling stands for, as a canonical tuple"""
    first = {}
    return tuple(first.setdefault(int(v), i) for i, v in enumerate(labels))


# ---------------------------------------------------------------------------------------------------------------------- the graph
def test_the_restatement_is_the_double_loop_over_pixels():
    for lab, start, N in rasters():
        got, want = R.graph(lab, start, N), R.graph_loop(lab, start, N)
        assert all(R.same_bits(g, w) for g, w in zip(got, want)), (lab.tolist(), start)
        indptr, nb, border = got
        assert indptr[0] == 0 and indptr[-1] == len(nb) and (border > 0).all()
        for i in range(N):                                                    # ascending inside a row: real, then N, then N + 1
            row = nb[indptr[i]:indptr[i + 1]]
            assert (np.diff(row) > 0).all() and (row != i).all() and (row <= N + 1).all()
        # symmetric: border[i -> j] == border[j -> i]
        at = {(int(i), int(j)): int(b) for i, j, b in zip(R.rows_of(indptr), nb, border)}
        assert all(at[(j, i)] == b for (i, j), b in at.items() if j < N)


@pytest.mark.parametrize("tile", [(3, 4), (16, 32), (1, 1)])
def test_the_records_of_the_tiles_add_up_to_the_graph(tile):
    for lab, start, N in rasters():
        total = {}
        for key, edges in R.tile_records(lab, start, N, *tile):
            assert (np.diff(key) > 0).all()                                   # distinct inside a tile
            for k, e in zip(key.tolist(), edges.tolist()):
                total[k] = total.get(k, 0) + e
        indptr, nb, border = R.graph(lab, start, N)
        want = {int(i) * (N + 2) + int(j): int(b) for i, j, b in zip(R.rows_of(indptr), nb, border)}
        assert total == want


def test_the_perimeter_is_four_per_pixel_less_two_per_inner_pair():
    for lab, start, N in rasters():
        indptr, nb, border = R.graph(lab, start, N)
        per = R.row_sum(indptr, border)
        seg = R.segment_index(lab, start, N)
        for i in range(N):
            m = seg == i
            inner = int((m[:, 1:] & m[:, :-1]).sum() + (m[1:] & m[:-1]).sum())
            assert per[i] == 4 * int(m.sum()) - 2 * inner, i


def test_one_label_in_two_places_is_one_row_and_a_known_answer():
    lab = np.array([[1, 2, 1],
                    [0, 2, 3]], np.int32)
    indptr, nb, border = R.graph(lab, 1, 3)
    assert indptr.tolist() == [0, 4, 8, 11]
    # segment 0 (label 1, two pixels apart): 2 edges to label 2, 1 to label 3, 1 to the background pixel, 4 frame edges
    assert nb.tolist() == [1, 2, 3, 4, 0, 2, 3, 4, 0, 1, 4] and border.tolist() == [2, 1, 1, 4, 2, 1, 1, 2, 1, 1, 2]
    assert R.graph(np.zeros((3, 4), np.int32), 1, 0)[0].tolist() == [0]           # n_labels = 0: an empty graph


# ------------------------------------------------------------------------------------------------------------------- components
def scipy_parts(indptr, nb, N, link):
    keep = (np.asarray(link) != 0) & (nb < N)
    A = sp.coo_matrix((np.ones(int(keep.sum())), (R.rows_of(indptr)[keep], nb[keep])), shape=(N, N))
    return connected_components(A, directed=False)[1]


def check_roots(root, parts):
    assert partition(root) == partition(parts)
    for p in np.unique(parts):
        members = np.flatnonzero(parts == p)
        assert (root[members] == members.min()).all()


def test_components_against_scipy():
    rs = np.random.RandomState(5)
    for lab, start, N in rasters():
        indptr, nb, _ = R.graph(lab, start, N)
        for p in (0.0, 0.3, 1.0):
            link = (rs.uniform(size=len(nb)) < p).astype(np.uint8) * 7           # any non-zero byte; one direction is enough
            check_roots(R.components(indptr, nb, N, link), scipy_parts(indptr, nb, N, link))
    # a path, linked from the higher end only
    N = 300
    indptr = np.concatenate([[0], np.cumsum([1] + [2] * (N - 2) + [1])]).astype(np.int64)
    nb = np.array([1] + [v for i in range(1, N - 1) for v in (i - 1, i + 1)] + [N - 2], np.int32)
    link = (nb < R.rows_of(indptr)).astype(np.uint8)
    assert (R.components(indptr, nb, N, link) == 0).all()
    link[R.rows_of(indptr) % 3 == 0] = 0
    check_roots(R.components(indptr, nb, N, link), scipy_parts(indptr, nb, N, link))


def test_the_table_functions_on_a_known_case():
    nan = np.nan
    # rows: 0 -> 1, 2, N; 1 -> 0; 2 -> 0, N + 1; 3 -> nothing
    indptr, nb = np.array([0, 3, 4, 6, 6], np.int64), np.array([1, 2, 4, 0, 0, 5], np.int32)
    border = np.array([2, 6, 1, 2, 6, 9], np.int64)
    v = np.array([[1.0, nan], [3.0, 2.0], [0.0, nan], [7.0, 7.0]])
    d = R.d2(indptr, nb, 4, v[:, :1])
    assert d[[0, 1, 3, 4]].tolist() == [4.0, 1.0, 4.0, 1.0] and np.isnan(d[[2, 5]]).all() and R.same_bits(d[[2, 5]], np.array([R.NAN] * 2))
    assert np.isnan(R.d2(indptr, nb, 4, v)[[0, 1]]).all()                          # a NaN feature propagates
    st = R.neighbor_stats(indptr, nb, border, 4, v)
    assert st["mean"][:, 0].tolist()[:3] == [(2 * 3.0 + 6 * 0.0) / 8, 1.0, 1.0] and np.isnan(st["mean"][3, 0])
    assert st["used"].tolist() == [[2, 1], [1, 0], [1, 0], [0, 0]] and st["min"][0].tolist() == [0.0, 2.0] and st["max"][0].tolist() == [3.0, 2.0]
    assert R.class_border(indptr, nb, border, 4, [0, 1, 1, 5], 2).tolist() == [[0, 8], [2, 0], [6, 0], [0, 0]]
    best, bd = R.best_neighbor(indptr, nb, 4, d)
    assert best.tolist() == [2, 0, 0, -1] and bd[:3].tolist() == [1.0, 4.0, 1.0] and np.isnan(bd[3])
    tie = R.best_neighbor(indptr, nb, 4, np.array([5.0, 5.0, 1.0, nan, 2.0, 0.0]))
    assert tie[0].tolist() == [1, -1, 0, -1]                                       # a tie goes to the first; pseudo entries never win
    assert R.compact_roots([0, 0, 2, 0, 4], 3).tolist() == [3, 3, 4, 3, 5]
    assert R.relabel(np.array([[-2, 0, 1, 2, 3, 4]], np.int32), [7, 8, 7], 1).tolist() == [[-2, 0, 7, 8, 7, 0]]


# ------------------------------------------------------------------------------------------------- the header and the source
def _library():
    pytest.importorskip("torch")
    from obia_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib


def test_the_header_says_there_is_no_overflow_path():
    full = open(os.path.join(ROOT, "include", "obia_adjacency.h")).read()
    assert "NO OVERFLOW PATH AND NO PASS COUNT" in full and "The reference has no counterpart" in full


def test_the_source_takes_no_workspace_and_every_atomic_is_on_an_integer():
    src = open(os.path.join(ROOT, "obia_amd", "csrc", "adjacency.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"arena\.(get|alloc)\b|\bA\.get<|\.arena\b", src)   # every buffer is the caller's
    assert not re.search(r"hipMalloc|hipFree|hipHostMalloc|Staging|upload_async", code)
    # integer atomics only: the LDS table, its list and record counters, the union-find's parents -- all declared as integers
    targets = {"keys": r"unsigned long long keys\[", "cnt": r"\bint cnt\[", "s_n": r"\bint s_n\b", "s_rec": r"\bint s_n, s_rec\b",
               "parent": r"\bint \*parent\b"}
    found = list(re.finditer(r"\batomic([A-Za-z]+)\s*\(\s*&(\w+)", code))
    assert len(found) == len(re.findall(r"\batomic[A-Z]\w*\s*\(", code)) >= 5
    for m in found:
        assert m.group(1) in ("Add", "Min", "CAS") and m.group(2) in targets, m.group(0)
        assert re.search(targets[m.group(2)], code), m.group(2)
    assert not re.search(r"atomic\w*\s*\(\s*[^;]*(float|double)", code) and "unsafeAtomic" not in code
    assert not re.search(r"__hip_atomic_fetch|__atomic_fetch", code)
    # every launch takes its grid from launch_grids.hpp, by name; no dim3 carries a clamp
    sites = re.findall(r"hipLaunchKernelGGL\([^;]*;", code)
    assert len(sites) == 10
    for site in sites:
        assert re.search(r"to_dim3\(grids::(flat|adj_tiles)\(", site) and "dim3(256)" in site, site
    assert not re.search(r"std::min|std::max", code)


def test_the_launch_grid_rows():
    _lib = _library()
    from tests import launch_grids as LG
    names = LG.names()
    assert names["adj_tiles"] == ("H", "W") and names["flat"] == ("n",)
    TH, TW = _lib.ADJ_TILE_H, _lib.ADJ_TILE_W
    assert LG.grid("adj_tiles", TH, TW)[:2] == (1, 1) and LG.grid("adj_tiles", TH + 1, TW + 1)[:2] == (2, 2)
    # both axes are clamped, and both crossings lie within what a thin raster can afford
    h, w = LG.crossing("adj_tiles", (1, 3), 0, "y"), LG.crossing("adj_tiles", (3, 1), 1, "x")
    assert h % TH == 1 and w % TW == 1 and 3 * h <= 2 ** 20 and 3 * w <= 2 ** 20
    assert LG.trips("adj_tiles", (h - 1, 3), "y") == 1 and LG.trips("adj_tiles", (h, 3), "y") == 2
    assert LG.trips("adj_tiles", (3, w - 1), "x") == 1 and LG.trips("adj_tiles", (3, w), "x") == 2


# ------------------------------------------------------------------------------------------------------------------- the wrappers
def test_public_names_and_refusals_before_any_device_use(monkeypatch):
    pytest.importorskip("torch")
    import obia_amd
    from obia_amd import _lib, adjacency as A
    for name in ("SegmentGraph", "segment_graph", "compact_roots", "relabel", "merge_by_threshold", "dissolve_by_class", "merge_similar",
                 "context_columns"):
        assert getattr(obia_amd, name) is getattr(A, name)
    for prop in ("n_neighbors", "perimeter", "border_background", "border_frame", "border_segments", "real", "indptr", "neighbor", "border"):
        assert isinstance(getattr(A.SegmentGraph, prop), property), prop
    for method in ("d2", "weights", "neighbor_stats", "border_to_class", "best_neighbor", "components"):
        assert callable(getattr(A.SegmentGraph, method))

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    lab = np.ones((4, 5), np.int32)
    for bad in (np.ones(5, np.int32), np.ones((0, 5), np.int32), np.ones((2, 2, 2), np.int32)):
        for call in (lambda: A.segment_graph(bad), lambda: A.relabel(bad, [1]), lambda: A.merge_by_threshold(np.ones((1, 1)), bad, 1.0),
                     lambda: A.dissolve_by_class(bad, [0]), lambda: A.merge_similar(np.ones((4, 5, 1)), bad, 1.0)):
            with pytest.raises(ValueError):
                call()
    with pytest.raises(ValueError):
        A.segment_graph(lab, n_labels=-1)
    with pytest.raises(ValueError):
        A.segment_graph(lab, start_label=1.5)
    with pytest.raises(ValueError):
        A.merge_by_threshold(np.ones((1, 1)), lab, -1.0)
    with pytest.raises(ValueError):
        A.merge_by_threshold(np.ones((1, 1)), lab, float("nan"))
    with pytest.raises(ValueError):
        A.merge_similar(np.ones((4, 5, 1)), lab, 1.0, max_rounds=-1)
    with pytest.raises(ValueError):
        A.relabel(lab, np.ones((2, 2), np.int32))
    import torch
    with pytest.raises(ValueError):
        A.segment_graph(torch.ones((4, 5), dtype=torch.int32))                # a CPU tensor is refused: its pointer reaches no kernel
