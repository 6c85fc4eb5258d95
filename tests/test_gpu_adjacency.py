"""The segment adjacency graph on the GPU (include/obia_adjacency.h, obia_amd/csrc/adjacency.hip) against
tests/adjacency_restatement.py, exactly: the two tile passes at the ABI (the records of every tile as a multiset) and the graph the
wrapper builds from them, over the raster shapes around a tile, the table at the most a tile can own, borders that cross tiles, one
label in two places, empty graphs, both clamps of the tile launch and the flat clamp of the table kernels; the table kernels on
hand-built CSRs whose values change their bits under any other order of summation; the components against SciPy; the drivers round
by round; the context columns.  Equality is np.array_equal, or the bits for floats."""
import ctypes
import functools

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from tests import adjacency_restatement as R
from tests import launch_grids as LG
from tests.guarded import POISONS, guarded
from tests.test_gpu_launch_clamps import call, dev, env

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = POISONS[0]
F32, F64, U8, I32, I64 = np.float32, np.float64, np.uint8, np.int32, np.int64
TH, TW = 16, 32                                                 # OBIA_ADJ_TILE_H, OBIA_ADJ_TILE_W (asserted below)


def test_the_tiles_are_the_library_s():
    from obia_amd import _lib
    assert (_lib.ADJ_TILE_H, _lib.ADJ_TILE_W) == (TH, TW)
    assert LG.unit("adj_tiles", (3, 1), 1, "x") == TW and LG.unit("adj_tiles", (1, 3), 0, "y") == TH


# ----------------------------------------------------------------------------------------------------------- the two tile passes
def tile_passes(lab, start, N):
    """obia_adj_tile_count_dev and obia_adj_tile_write_dev on guarded outputs: (count, key, edges) as NumPy"""
    _lib, lib, c = env()
    H, W = lab.shape
    nt = -(-H // TH) * -(-W // TW)
    L = dev(lab)
    count = guarded((nt,), I32, POISON, "cuda", 1)
    call(lib.obia_adj_tile_count_dev, L.data_ptr(), H, W, start, N, count.ptr)
    assert count.findings(name="count") == []
    cnt = count.host().astype(I64)
    offset, total = dev(np.cumsum(cnt) - cnt), int(cnt.sum())
    key, edges = guarded((total,), I64, POISON, "cuda", 1), guarded((total,), I32, POISON, "cuda", 3)
    work = guarded((4,), I32, POISON, "cuda", 1)
    call(lib.obia_adj_tile_write_dev, L.data_ptr(), H, W, start, N, offset.data_ptr(), total, key.ptr, edges.ptr, work.ptr)
    assert key.findings(name="key") == [] and edges.findings(name="edges") == [] and work.stray().size == 0
    return cnt, key.host(), edges.host()


def check_raster(lab, start, N, name=""):
    """the records of every tile are the restatement's multiset; the wrapper's graph is the restatement's; returns the graph"""
    from obia_amd import segment_graph
    lab = np.ascontiguousarray(lab, I32)
    cnt, key, edges = tile_passes(lab, start, N)
    want = R.tile_records(lab, start, N, TH, TW)
    assert cnt.tolist() == [len(k) for k, _ in want], name
    at = 0
    for t, (wk, we) in enumerate(want):
        order = np.argsort(key[at:at + len(wk)], kind="stable")
        assert np.array_equal(key[at:at + len(wk)][order], wk) and np.array_equal(edges[at:at + len(wk)][order], we), (name, t)
        at += len(wk)
    g = segment_graph(lab, start_label=start, n_labels=N)
    indptr, nb, border = R.graph(lab, start, N)
    assert isinstance(g.indptr, np.ndarray) and g.n_labels == N and g.start_label == start
    assert R.same_bits(g.indptr, indptr) and R.same_bits(g.neighbor, nb) and R.same_bits(g.border, border), name
    return g


SHAPES = [(1, 1), (1, 2), (2, 1), (1, TW + 1), (TH + 1, 1), (TH - 1, TW - 1), (TH, TW), (TH + 1, TW + 1), (2 * TH + 3, 3 * TW + 5)]


@pytest.mark.parametrize("start", [1, 0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_raster_shapes_around_a_tile(shape, start):
    """labels in -1 .. 6 with five segments from `start`: with 1, the values 0, -1 and 6 are background; with 0, the values -1, 5, 6"""
    rs = np.random.RandomState(shape[0] * 131 + shape[1])
    for blocky in (False, True):
        lab = rs.randint(-1, 7, shape)
        if blocky:                                                             # runs of equal labels: edges inside a segment
            lab = np.kron(rs.randint(-1, 7, (-(-shape[0] // 3), -(-shape[1] // 4))), np.ones((3, 4), int))[:shape[0], :shape[1]]
        g = check_raster(lab, start, 5, f"{shape} {start} {blocky}")
        per = R.row_sum(R.graph(lab, start, 5)[0], R.graph(lab, start, 5)[2])
        assert np.array_equal(g.perimeter, per) and np.array_equal(g.perimeter, g.border_segments + g.border_background + g.border_frame)
        assert np.array_equal(g.n_neighbors, R.row_sum(g.indptr, g.real))


@pytest.mark.parametrize("shape", [(TH + 1, TW + 1), (2 * TH, 2 * TW)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_table_at_the_most_a_tile_can_own(shape):
    """every pixel its own label, in shuffled order: every owned edge is a pair of its own"""
    n = shape[0] * shape[1]
    lab = (np.random.RandomState(3).permutation(n) + 1).reshape(shape)
    g = check_raster(lab, 1, n, "design maximum")
    cnt, _, _ = tile_passes(np.ascontiguousarray(lab, I32), 1, n)
    full = 2 * 2 * TH * TW + (TH + TW - 1)                                     # the first tile: two real pairs a pixel, the frame's pairs
    assert cnt[0] == full and (g.perimeter == 4).all()


def test_borders_that_cross_tiles():
    H, W = 3 * TH + 1, 2 * TW
    for name, at in (("inside a tile", TW - 5), ("on a tile border", TW)):
        lab = np.where(np.arange(W)[None, :] < at, 1, 2) * np.ones((H, 1), int)
        g = check_raster(lab, 1, 2, name)
        assert g.neighbor.tolist() == [1, 3, 0, 3] and g.border.tolist()[::2] == [H, H]      # one pair, counted in four tile rows
    stair = np.where(np.arange(W)[None, :] < (np.arange(H)[:, None] * W) // H, 1, 2)
    g = check_raster(stair, 1, 2, "staircase")
    assert g.border[0] == g.border[2] > H


def test_one_label_in_two_far_blobs():
    lab = np.full((2 * TH + 4, 3 * TW), 2)
    lab[2:6, 2:7] = 1
    lab[TH + 8:TH + 11, 2 * TW + 3:2 * TW + 9] = 1
    g = check_raster(lab, 1, 2, "blobs")
    assert g.indptr.tolist()[:2] == [0, 1] and g.neighbor[0] == 1 and g.border[0] == 2 * (4 + 5) + 2 * (3 + 6)


def test_empty_graphs():
    from obia_amd import segment_graph
    for lab, N in ((np.arange(12).reshape(3, 4), 0), (np.zeros((TH + 2, TW + 2), int), 4), (np.full((5, 5), -7), None)):
        g = segment_graph(lab.astype(I32), start_label=1, n_labels=N)
        n = 0 if N is None else N
        assert g.n_labels == n and g.nnz == 0 and g.indptr.tolist() == [0] * (n + 1) and g.neighbor.shape == g.border.shape == (0,)
        assert g.perimeter.tolist() == [0] * n and g.n_neighbors.tolist() == [0] * n
        cnt, key, edges = tile_passes(lab.astype(I32), 1, n)
        assert not cnt.any() and key.size == edges.size == 0
        if n:
            st = g.neighbor_stats(np.ones((n, 2)))
            assert np.isnan(st["mean"]).all() and not st["used"].any() and g.best_neighbor(np.zeros(0))[0].tolist() == [-1] * n
            assert g.components(np.zeros(0, U8)).tolist() == list(range(n)) and not g.border_to_class(np.zeros(n, I32), 3).any()


@pytest.mark.parametrize("axis", ["y", "x"])
def test_both_clamps_of_the_tile_launch(axis):
    """thin rasters one tile below the second trip of the stride loop on an axis, and at it"""
    vary = 0 if axis == "y" else 1
    base = (1, 3) if axis == "y" else (3, 1)
    at = LG.crossing("adj_tiles", base, vary, axis)
    case = LG.Case("adj_tiles", tuple(at if k == vary else 3 for k in range(2)), axis, threshold=vary)
    LG.check(case)
    rs = np.random.RandomState(at)
    for size in (at - 1, at):
        shape = tuple(size if k == vary else 3 for k in range(2))
        assert LG.trips("adj_tiles", shape, axis) == (2 if size == at else 1)
        lab = np.kron(rs.randint(0, 40, (-(-shape[0] // 2), -(-shape[1] // 2))), np.ones((2, 2), int))[:shape[0], :shape[1]]
        lab[-1, -1] = 39                                                       # the last pixel: the end of the last trip
        check_raster(lab, 1, 39, f"{axis} {shape}")


def test_wrong_tables_are_refused_and_nothing_is_written_outside():
    _lib, lib, c = env()
    rs = np.random.RandomState(9)
    lab = np.ascontiguousarray(rs.randint(0, 9, (2 * TH + 3, 2 * TW + 1)), I32)
    H, W = lab.shape
    cnt, key, edges = tile_passes(lab, 1, 8)
    offset, total = np.cumsum(cnt) - cnt, int(cnt.sum())
    L = dev(lab)

    def write(off, tot, room):
        k, e = guarded((room,), I64, POISON, "cuda", 1), guarded((room,), I32, POISON, "cuda", 1)
        work = guarded((4,), I32, POISON, "cuda", 0)
        o = dev(np.asarray(off, I64))
        rc = lib.obia_adj_tile_write_dev(c.handle, L.data_ptr(), H, W, 1, 8, o.data_ptr(), tot, k.ptr, e.ptr, work.ptr)
        torch.cuda.synchronize()
        assert k.stray().size == 0 and e.stray().size == 0 and work.stray().size == 0
        return rc, _lib.last_error()
    assert write(offset, total, total)[0] == 0
    shifted = offset.copy()
    shifted[3:] += 1
    for off, tot, room in ((shifted, total + 1, total + 1), (offset, total - 1, total - 1), (offset, total + 1, total + 1),
                           (offset + 1, total + 1, total + 1), (offset[::-1].copy(), total, total), (np.full_like(offset, -5), total, total),
                           (np.full_like(offset, 2 ** 40), total, total), (np.zeros_like(offset), total, total)):
        rc, msg = write(off, tot, room)
        assert rc == _lib.E_INVALID and "not those of the count" in msg, (rc, msg)


def test_two_runs_give_the_same_graph():
    from obia_amd import segment_graph
    rs = np.random.RandomState(21)
    lab = np.kron(rs.randint(1, 400, (70, 90)), np.ones((3, 3), int)).astype(I32)
    a, b = segment_graph(lab), segment_graph(torch.as_tensor(lab).cuda())
    assert isinstance(b.indptr, torch.Tensor) and b.indptr.is_cuda                # a tensor in: tensors out
    for name in ("indptr", "neighbor", "border", "perimeter"):
        assert getattr(a, name).tobytes() == getattr(b, name).cpu().numpy().tobytes(), name
    ta, tb = tile_passes(lab, 1, 399), tile_passes(lab, 1, 399)
    assert np.array_equal(ta[0], tb[0])


# --------------------------------------------------------------------------------------------------- table kernels, hand-built CSRs
@functools.lru_cache(maxsize=None)
def hand_csr():
    """rows of 0, 1, 63, 64, 65 and 300 real neighbours, then short ones; pseudo entries on every third and fourth row (row 0: pseudo
    entries only); borders up to 2^31 - 1"""
    rs = np.random.RandomState(33)
    N = 320
    lengths = [0, 1, 63, 64, 65, 300] + rs.randint(0, 6, N - 6).tolist()
    indptr, nb = [0], []
    for i, n in enumerate(lengths):
        row = np.sort(rs.choice(np.setdiff1d(np.arange(N), [i]), n, replace=False)).tolist()
        row += ([N] if i % 3 == 0 else []) + ([N + 1] if i % 4 == 0 else [])
        nb += row
        indptr.append(len(nb))
    border = rs.randint(1, 1000, len(nb)).astype(I64)
    border[::17] = 2 ** 31 - 1
    return N, np.array(indptr, I64), np.array(nb, I32), border


def hand_values(F, seed):
    """values of which any other order of summation changes the bits (1e16, 1, -1e16 ...), with NaN, both zeros and infinities;
    every neighbour of row 1 is NaN in every feature, every neighbour of row 2 in feature 0"""
    N, indptr, nb, _ = hand_csr()
    rs = np.random.RandomState(seed)
    pool = np.array([1e16, 1.0, -1e16, 3.5, -0.0, 0.0, 1e-3, 7.0, -2.25, np.nan])
    v = rs.choice(pool, (N, F), p=[.15, .18, .15, .1, .05, .05, .1, .1, .1, .02])
    far = np.setdiff1d(np.arange(N), np.r_[5, nb[indptr[5]:indptr[6]]])[:3]      # not beside the long row, whose sums stay finite
    v[far[0]], v[far[1]], v[far[2], ::2] = np.inf, -np.inf, np.inf               # inf - inf and inf + -inf arise in other rows
    v[nb[indptr[1]:indptr[2]]] = np.nan
    real = nb[indptr[2]:indptr[3]]
    v[real[real < N], 0] = np.nan
    return v


def graph_of(csr):
    from obia_amd import SegmentGraph
    N, indptr, nb, border = csr
    return SegmentGraph(indptr, nb, border, N)


@pytest.mark.parametrize("F", [1, 3, 9])
def test_d2_and_neighbor_statistics_on_hand_built_rows(F):
    N, indptr, nb, border = hand_csr()
    g, v = graph_of(hand_csr()), hand_values(F, 50 + F)
    assert R.same_bits(g.d2(v), R.d2(indptr, nb, N, v))
    assert np.array_equal(g.weights(v), np.sqrt(R.d2(indptr, nb, N, v)), equal_nan=True)
    got, want = g.neighbor_stats(v), R.neighbor_stats(indptr, nb, border, N, v)
    assert sorted(got) == sorted(want) == sorted(("mean", "min", "max", "used", "diff"))
    for name in want:
        assert R.same_bits(got[name], want[name]), name
    assert (want["used"][1] == 0).all() and want["used"][2, 0] == 0 and want["used"][0].tolist() == [0] * F     # all NaN; pseudo entries only
    assert np.isnan(want["mean"][1]).all() and (want["used"][5] > 200).all()
    # the order matters: summed backwards, some mean of the long rows has other bits
    if F == 9:
        rnb, rborder = nb.copy(), border.copy()
        rnb[indptr[5]:indptr[6]], rborder[indptr[5]:indptr[6]] = nb[indptr[5]:indptr[6]][::-1], border[indptr[5]:indptr[6]][::-1]
        rev = R.neighbor_stats(indptr, rnb, rborder, N, v)
        assert not R.same_bits(rev["mean"][5], want["mean"][5]) and R.same_bits(rev["mean"][:5], want["mean"][:5])


def test_d2_is_the_same_bits_in_both_directions():
    from obia_amd import segment_graph
    rs = np.random.RandomState(4)
    lab = np.kron(rs.randint(1, 300, (40, 50)), np.ones((5, 6), int)).astype(I32)
    g = segment_graph(lab)
    v = rs.normal(0, 1e3, (g.n_labels, 3)) * rs.choice([1.0, 1e12, 1e-9], (g.n_labels, 3))
    d = g.d2(v)
    assert R.same_bits(d, R.d2(g.indptr, g.neighbor, g.n_labels, v))
    real = g.real
    rows, nb, bits = R.rows_of(g.indptr)[real], g.neighbor.astype(I64)[real], d[real].view(np.uint64)
    there, back = np.argsort(rows * g.n_labels + nb), np.argsort(nb * g.n_labels + rows)      # i -> j beside j -> i
    assert np.array_equal(rows[there], nb[back]) and np.array_equal(bits[there], bits[back])
    assert np.isnan(d[~real]).all() and real.sum() > 1000


def test_best_neighbor_with_ties_nan_rows_and_empty_rows():
    N, indptr, nb, border = hand_csr()
    g = graph_of(hand_csr())
    rs = np.random.RandomState(6)
    d = rs.choice([1.0, 2.0, 0.5, np.nan], len(nb), p=[.4, .3, .1, .2])            # few values: exact ties in every long row
    d[indptr[3]:indptr[4]] = np.nan                                            # a row of NaN only
    d[indptr[4]:indptr[5]] = 4.0                                               # a row that is one tie
    best, bd = g.best_neighbor(d)
    wb, wd = R.best_neighbor(indptr, nb, N, d)
    assert R.same_bits(best, wb) and R.same_bits(bd, wd)
    assert best[0] == -1 and best[3] == -1 and np.isnan(bd[3]) and best[4] == nb[indptr[4]] and bd[4] == 4.0


def test_border_to_class_ignores_classes_outside_the_table():
    N, indptr, nb, border = hand_csr()
    g = graph_of(hand_csr())
    K = 4
    classes = np.random.RandomState(8).randint(-1, K + 1, N).astype(I32)      # -1 and K add nothing
    got, want = g.border_to_class(classes, K), R.class_border(indptr, nb, border, N, classes, K)
    assert R.same_bits(got, want) and want.max() > 2 ** 32 and (want.sum(1) <= R.row_sum(indptr, border * (nb < N))).all()
    assert (want.sum(1) < R.row_sum(indptr, border * (nb < N))).any()


# ------------------------------------------------------------------------------------------------------------------- components
def check_components(g, link, indptr, nb, N):
    root = g.components(link)
    keep = (np.asarray(link) != 0) & (nb < N)
    A = sp.coo_matrix((np.ones(int(keep.sum())), (R.rows_of(indptr)[keep], nb[keep].astype(I64))), shape=(N, N))
    n_parts, parts = connected_components(A, directed=False)
    least = np.full(n_parts, N, I64)
    np.minimum.at(least, parts, np.arange(N))
    assert root.dtype == I32 and np.array_equal(root, least[parts])            # the same partition, every root its smallest member
    return n_parts


def path_csr(N):
    indptr = np.concatenate([[0], np.cumsum(np.r_[1, np.full(N - 2, 2), 1])]).astype(I64)
    nb = np.empty(indptr[-1], I32)
    nb[indptr[1:] - 1] = np.minimum(np.arange(N) + 1, N - 1)                   # the last entry of a row: the right neighbour ...
    nb[indptr[:-1]] = np.maximum(np.arange(N) - 1, 0)                          # ... the first: the left one
    nb[0], nb[-1] = 1, N - 2
    return N, indptr, nb, np.ones(len(nb), I64)


def test_components_of_a_path_of_70000_rows():
    from obia_amd import SegmentGraph
    N, indptr, nb, border = path_csr(70000)
    g = SegmentGraph(indptr, nb, border, N)
    link = np.ones(len(nb), U8)
    assert check_components(g, link, indptr, nb, N) == 1
    rows = R.rows_of(indptr)
    cut = link.copy()
    cut[(np.minimum(rows, nb) % 3 == 0)] = 0                                   # every third link, in both directions
    assert check_components(g, cut, indptr, nb, N) == 1 + -(-(N - 1) // 3)          # {0}, {1, 2, 3}, {4, 5, 6}, ...
    one_way = (nb > rows).astype(U8) * 255                                      # set on i -> i + 1 only: linked all the same
    assert check_components(g, one_way, indptr, nb, N) == 1


def test_components_of_a_raster_graph_with_links_in_one_direction():
    from obia_amd import segment_graph
    rs = np.random.RandomState(12)
    lab = rs.randint(1, 4000, (200, 300)).astype(I32)
    g = segment_graph(lab)
    rows = R.rows_of(g.indptr)
    link = ((rows < g.neighbor) & (rs.uniform(size=g.nnz) < 0.04)).astype(U8)   # pseudo entries too: they link nothing
    n = check_components(g, link, g.indptr, g.neighbor, g.n_labels)
    assert 1 < n < g.n_labels


# ---------------------------------------------------------------------------------------- the flat clamp of the table kernels
def test_table_kernels_past_the_flat_grid():
    """a path of more rows than 8192 workgroups take in one trip, so that every table kernel and the relabelling take the second;
    what a path gives is written down in closed form (F = 1: no order to speak of)"""
    from obia_amd import SegmentGraph, relabel
    (n,) = LG.Case("flat", (LG.crossing("flat", (1,), 0, "x"),), "x", threshold=0).sizes
    LG.check(LG.Case("flat", (n,), "x", threshold=0))
    N, indptr, nb, _ = path_csr(n + 4)
    rs = np.random.RandomState(2)
    border = rs.randint(1, 50, len(nb)).astype(I64)
    v = rs.randint(-1000, 1000, (N, 1)).astype(F64)
    g = SegmentGraph(indptr, nb, border, N)
    rows = R.rows_of(indptr)
    d = (v[rows, 0] - v[nb, 0]) ** 2
    assert R.same_bits(g.d2(v), d)
    # first (left) and last (right) entry of every row; the two ends have one entry, which is both
    first, last = indptr[:-1], indptr[1:] - 1
    two = first != last
    best = np.where(two & (d[last] < d[first]), nb[last], nb[first]).astype(I32)
    gb, gd = g.best_neighbor(d)
    assert R.same_bits(gb, best) and R.same_bits(gd, np.where(two & (d[last] < d[first]), d[last], d[first]))
    w1, w2, v1, v2 = border[first].astype(F64), np.where(two, border[last], 0).astype(F64), v[nb[first], 0], v[nb[last], 0]
    st = g.neighbor_stats(v)
    assert R.same_bits(st["mean"][:, 0], ((0.0 + w1 * v1) + np.where(two, w2 * v2, 0.0)) / ((0.0 + w1) + w2))
    assert R.same_bits(st["min"][:, 0], np.minimum(v1, v2)) and R.same_bits(st["max"][:, 0], np.maximum(v1, v2))
    assert np.array_equal(st["used"][:, 0], 1 + two)
    classes = (np.arange(N) % 3).astype(I32)
    want = np.zeros((N, 3), I64)
    np.add.at(want, (rows, classes[nb]), border)
    assert R.same_bits(g.border_to_class(classes, 3), want)
    link = (np.minimum(rows, nb) % 1000 != 999).astype(U8)
    assert np.array_equal(g.components(link), (np.arange(N) // 1000 * 1000).astype(I32))
    lab = rs.randint(-2, N + 3, (-(-n // 3), 3)).astype(I32)                     # 3 n' >= n pixels
    table = rs.randint(1, 10 ** 6, N).astype(I32)
    assert lab.size >= n and R.same_bits(relabel(lab, table, start_label=1), R.relabel(lab, table, 1))


# ------------------------------------------------------------------------------------------------------------------------ drivers
def blocks(seed=1, contrast=True, gap=False):
    """a 40 x 56 x 3 raster of 8 x 8 blocks, 35 labels from 1: the blocks of the left and of the right half differ by 100 (the
    strong contrast), the blocks of one half by less than 4 per band (the weak one)"""
    rs = np.random.RandomState(seed)
    bi, bj = np.mgrid[0:5, 0:7]
    lab = np.kron(bi * 7 + bj + 1, np.ones((8, 8), int)).astype(I32)
    level = 100.0 * (bj >= 4)[..., None] + (rs.randint(0, 16, (5, 7, 3)) * 0.25 if contrast else rs.randint(0, 2, (5, 7, 3)) * 1.0)
    raw = np.kron(level, np.ones((8, 8, 1))).astype(F32)
    if gap:
        lab[:, 24:32] = 0                                                       # a column of blocks becomes background
    return raw, lab


def zonal_means(raw, labels):
    """this project's zonal_stats, on the device whatever came in: the same means on both sides"""
    from obia_amd import zonal_stats
    t = lambda a, dt: a if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a, dt)).cuda()
    m = zonal_stats(t(raw, F32), t(labels, I32))["mean"]
    return m


def zonal_means_np(raw, labels):
    return zonal_means(raw, labels).cpu().numpy()


def test_single_cuts_dissolve_and_relabel():
    from obia_amd import dissolve_by_class, merge_by_threshold, relabel
    raw, lab = blocks()
    means = zonal_means_np(raw, lab)
    for thr in (0.0, 1.0, 2.5, 50.0, 1000.0):
        got, n = merge_by_threshold(raw, lab, thr)
        want, wn = R.merge_by_threshold(means, lab, thr)
        assert n == wn and R.same_bits(got, want), thr
        got2, n2 = merge_by_threshold(means, lab, thr)                         # a table of values instead of the raster
        assert n2 == wn and R.same_bits(got2, want)
    assert R.merge_by_threshold(means, lab, 50.0)[1] == 2 and R.merge_by_threshold(means, lab, 1000.0)[1] == 1
    classes = np.random.RandomState(5).randint(-1, 3, 35)
    got, n = dissolve_by_class(lab, classes)
    want, wn = R.dissolve_by_class(lab, classes)
    assert n == wn and R.same_bits(got, want) and n < 35
    t = dissolve_by_class(torch.as_tensor(lab).cuda(), torch.as_tensor(classes).cuda())[0]
    assert t.is_cuda and R.same_bits(t.cpu().numpy(), want)
    odd = np.array([[-3, 0, 1, 2, 35, 36, 40]], I32)                            # below start: kept; past the table: start_label - 1
    table = np.arange(100, 135, dtype=I32)
    assert relabel(odd, table).tolist() == [[-3, 0, 100, 101, 134, 0, 0]]
    assert relabel(odd, table[:3], start_label=0).tolist() == [[-3, 100, 101, 102, -1, -1, -1]]


def test_merge_similar_round_by_round():
    from obia_amd import merge_similar
    raw, lab = blocks()
    want, counts, merged = R.merge_similar(raw, lab, 10.0, zonal_means_np, max_rounds=16)
    assert sum(m > 0 for m in merged) >= 2 and counts[-1] == 2                  # at least two rounds merge something; two halves remain
    got, got_counts = merge_similar(raw, lab, 10.0, max_rounds=16, stats=zonal_means)
    assert got_counts == counts and R.same_bits(got, want)
    for rounds in (1, 2, 3):                                                   # ... and every round on its own
        w, c, _ = R.merge_similar(raw, lab, 10.0, zonal_means_np, max_rounds=rounds)
        g, gc = merge_similar(raw, lab, 10.0, max_rounds=rounds, stats=zonal_means)
        assert gc == c == counts[:rounds] and R.same_bits(g, w), rounds
    plain, plain_counts = merge_similar(raw, lab, 10.0, max_rounds=16)                       # without `stats`: zonal_stats' means as well
    assert plain_counts == counts and R.same_bits(plain, want)


def test_boundary_thresholds():
    from obia_amd import merge_by_threshold, merge_similar, segment_graph
    raw, lab = blocks(seed=2, contrast=False)                                   # constant blocks of whole numbers: their means are exact
    means = zonal_means_np(raw, lab)
    assert np.array_equal(means, raw[::8, ::8].reshape(35, 3).astype(F64))
    got, n = merge_by_threshold(raw, lab, 0.0)                                 # threshold 0: only neighbours with identical means
    want, wn = R.merge_by_threshold(means, lab, 0.0)
    assert n == wn and R.same_bits(got, want) and 2 < n < 35
    for new in np.unique(got):
        assert len(np.unique(raw[got == new].reshape(-1, 3), axis=0)) == 1
    sim, counts = merge_similar(raw, lab, 0.0, max_rounds=64, stats=zonal_means)
    wsim, wcounts, _ = R.merge_similar(raw, lab, 0.0, zonal_means_np, max_rounds=64)
    assert counts == wcounts and R.same_bits(sim, wsim)
    # a huge threshold: one segment per connected part of the segment graph
    raw, lab = blocks(gap=True)
    g = segment_graph(lab)
    real = g.real
    A = sp.coo_matrix((np.ones(int(real.sum())), (R.rows_of(g.indptr)[real], g.neighbor[real].astype(I64))), shape=(g.n_labels, g.n_labels))
    n_parts, parts = connected_components(A, directed=False)
    out, counts = merge_similar(raw, lab, 1e30, max_rounds=64, stats=zonal_means)
    assert counts[-1] == len(np.unique(parts[g.perimeter > 0])) == 2 and n_parts == 7 and counts == sorted(counts, reverse=True) and len(counts) < 64
    seg = lab > 0
    first = {}
    assert [first.setdefault(int(a), int(b)) == int(b) for a, b in zip(out[seg], parts[lab[seg] - 1])].count(False) == 0
    assert len(first) == len(set(first.values())) and (out[~seg] == 0).all()


def test_context_columns_of_an_objects_table():
    from obia_amd import context_columns, create_objects, segment_graph
    raw, lab = blocks()
    lab = np.where(lab == 17, 36, lab).astype(I32)                              # label 17 is absent: 36 rows in the graph, 35 in the table
    objects = create_objects(lab, raw, calculate_textural=False, geometry=False)
    g = segment_graph(lab)
    assert g.n_labels == 36 and len(objects) == 35 and g.perimeter[16] == 0
    cols = ["b0_mean", "b2_max"]
    cc = context_columns(objects, g, columns=cols)
    assert list(cc.columns) == ["n_neighbors", "perimeter", "rel_border_background", "rel_border_frame"] + \
        [f"{c}_nb_{s}" for c in cols for s in ("mean", "diff", "min", "max")]
    assert cc.index.equals(objects.index) and len(cc) == 35
    present = g.perimeter > 0
    values = np.full((36, 2), np.nan)
    values[present] = objects[cols].to_numpy(dtype=F64)
    st = g.neighbor_stats(values)
    want = R.neighbor_stats(g.indptr, g.neighbor, g.border, 36, values)
    for k, c in enumerate(cols):
        for s in ("mean", "diff", "min", "max"):
            assert R.same_bits(cc[f"{c}_nb_{s}"].to_numpy(), st[s][present, k]) and R.same_bits(st[s], want[s]), (c, s)
    assert np.array_equal(cc["perimeter"].to_numpy(), g.perimeter[present]) and (cc["perimeter"] == 32).all()
    assert np.array_equal(cc["n_neighbors"].to_numpy(), g.n_neighbors[present]) and cc["n_neighbors"].min() == 2
    assert np.array_equal(cc["rel_border_frame"].to_numpy(), g.border_frame[present] / 32.0) and (cc["rel_border_background"] == 0).all()
    every = context_columns(objects, g)                                        # every numeric column but segment_id
    assert "b1_variance_nb_mean" in every.columns and "segment_id_nb_mean" not in every.columns
