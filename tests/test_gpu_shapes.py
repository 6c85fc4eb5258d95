"""The shape columns on the GPU (include/obia_shapes.h, obia_amd/csrc/shapes.hip, obia_amd/shapes.py) against
tests/shapes_restatement.py.  The integer tables are equal, through the ABI on guarded outputs and through the wrapper: raster shapes
around a tile, the LDS table at the most a tile can hold, one segment over both clamps of the tile launch, a tall raster whose sums
pass 2^32, start_label 0, labels outside the table, a label in two places, N == 0, golden SLIC maps.  On the same inputs the area is
zonal_stats' count and the perimeter segment_graph's; every derived column built from + - x / sqrt is the restatement's bits;
orientation is within ORIENTATION_BOUND of it; merge after a round of mutual best neighbours equals a fresh pass; NumPy and
CUDA-tensor inputs give one result.

ORIENTATION.  torch's device atan2 against NumPy's on these tables, as 0.5 * atan2(2 mu_rc, mu_rr - mu_cc) with the same arguments
bit for bit: the largest absolute difference measured over every case of this file on an MI355X was 2.22e-16 (2^-52: one unit in the
last place of an angle above 1 rad, two of one above 0.5; in 25 of the 63 tables compared every row is equal).  The bound is 8 x that, as in tests/test_shapes_restatement_cpu.py."""
import functools
import os

import numpy as np
import pytest

from tests import launch_grids as LG
from tests import shapes_restatement as S
from tests.guarded import POISONS, guarded
from tests.test_gpu_launch_clamps import call, dev, env

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = POISONS[0]
F32, F64, I32, I64 = np.float32, np.float64, np.int32, np.int64
TH, TW = 16, 32                                                 # OBIA_ADJ_TILE_H, OBIA_ADJ_TILE_W (asserted below)
ORIENTATION_BOUND = 8 * 2.22e-16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXACT = ("centroid", "mu", "eigenvalues", "major_axis_length", "minor_axis_length", "eccentricity", "extent", "compactness", "shape_index",
         "smoothness")
worst = {"orientation": 0.0}


def test_the_tiles_are_the_library_s():
    from obia_amd import _lib
    assert (_lib.ADJ_TILE_H, _lib.ADJ_TILE_W, _lib.SHAPE_SUMS) == (TH, TW, 7) and _lib.SHAPE_TABLE > TH * TW


def abi_tables(lab, start, N, k=1):
    """obia_shape_sums_dev on guarded outputs: (sums, box) as NumPy; no stray write, no element left unwritten"""
    _lib, lib, c = env()
    H, W = lab.shape
    L = dev(lab)
    if N == 0:                                                                 # buffers of no elements may be null
        call(lib.obia_shape_sums_dev, L.data_ptr(), H, W, start, 0, None, None)
        return np.zeros((0, 7), I64), np.zeros((0, 4), I32)
    sums, box = guarded((N, 7), I64, POISON, "cuda", k), guarded((N, 4), I32, POISON, "cuda", k)
    call(lib.obia_shape_sums_dev, L.data_ptr(), H, W, start, N, sums.ptr, box.ptr)
    assert sums.findings(name="sums") == [] and box.findings(name="box") == []
    return sums.host(), box.host()


def check_columns(table, sums, box, name=""):
    """every column of a ShapeTable (NumPy out) against the restatement of the same integer tables"""
    d = S.derived(sums, box)
    assert S.same_bits(table.sums, sums) and S.same_bits(table.box, box), name
    assert np.array_equal(table.present, d["present"]) and table.present.dtype == np.bool_
    for k in S.INT_COLUMNS:
        assert S.same_bits(getattr(table, k), d[k]), (name, k)
    for k in EXACT:
        assert S.same_bits(getattr(table, k), d[k]), (name, k)
    got = table.orientation
    assert got.dtype == F64 and np.array_equal(np.isnan(got), ~d["present"]) and S.same_bits(got[~d["present"]], d["orientation"][~d["present"]])
    if d["present"].any():
        diff = float(np.max(np.abs(got[d["present"]] - d["orientation"][d["present"]])))
        worst["orientation"] = max(worst["orientation"], diff)
        print(f"{name}: orientation differs from NumPy's by at most {diff:.3e} (worst so far {worst['orientation']:.3e})")
        assert diff <= ORIENTATION_BOUND, (name, diff)
    affine = [0.5, 0.0, 0.0, -0.5, 1000.0, 2000.0]
    assert S.same_bits(table.centroid_xy(affine), S.centroid_xy(d["centroid"], affine)), name
    return d


def check_raster(lab, start, N, name="", graph=True):
    """ABI and wrapper against the restatement; the area against zonal_stats, the perimeter against segment_graph"""
    from obia_amd import segment_graph, segment_shapes, zonal_stats
    lab = np.ascontiguousarray(lab, I32)
    want = S.tables(lab, start, N)
    got = abi_tables(lab, start, N)
    assert S.same_bits(got[0], want[0]) and S.same_bits(got[1], want[1]), name
    table = segment_shapes(lab, start_label=start, n_labels=N)
    assert isinstance(table.sums, np.ndarray) and table.n_labels == N and table.start_label == start
    d = check_columns(table, *want, name=name)
    if graph and N:
        zeros = np.zeros(lab.shape + (1,), F32)
        assert np.array_equal(want[0][:, 0], np.asarray(zonal_stats(zeros, lab, start_label=start, n_labels=N)["count"]).astype(I64)), name
        assert np.array_equal(want[0][:, 6], segment_graph(lab, start_label=start, n_labels=N).perimeter), name
    return table, d


SHAPES = [(1, 1), (1, TW + 1), (TH + 1, 1)] + [(h, w) for h in (TH - 1, TH, TH + 1) for w in (TW - 1, TW, TW + 1)] + [(2 * TH + 3, 3 * TW + 5)]


@pytest.mark.parametrize("start", [1, 0])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_raster_shapes_around_a_tile(shape, start):
    """labels in -1 .. 6 with five segments from `start`: with 1, the values 0, -1 and 6 are background; with 0, the values -1, 5, 6
    -- negative labels, labels past the table, and n_labels below the largest label in one"""
    rs = np.random.RandomState(shape[0] * 131 + shape[1])
    for blocky in (False, True):
        lab = rs.randint(-1, 7, shape)
        if blocky:                                                             # runs of equal labels that cross rows and tiles
            lab = np.kron(rs.randint(-1, 7, (-(-shape[0] // 3), -(-shape[1] // 7))), np.ones((3, 7), int))[:shape[0], :shape[1]]
        check_raster(lab, start, 5, f"{shape} {start} {blocky}")


@pytest.mark.parametrize("shape", [(TH, TW), (TH + 1, TW + 1)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_table_at_the_most_a_tile_can_hold(shape):
    """every pixel its own label, in shuffled order: 512 segments in the first tile's table"""
    n = shape[0] * shape[1]
    lab = (np.random.RandomState(3).permutation(n) + 1).reshape(shape)
    table, d = check_raster(lab, 1, n, "design maximum")
    assert (table.area == 1).all() and (table.perimeter == 4).all() and (d["eccentricity"] == 0).all()


@pytest.mark.parametrize("shape", [(2049, 33), (17, 2049)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_segment_over_both_clamps_of_the_tile_launch(shape):
    """the second trip of the workgroups on y (2049 rows) and on x (2049 columns); the flush's translation terms over many tiles"""
    H, W = shape
    assert LG.trips("adj_tiles", shape, "y" if H > W else "x") == 2 and LG.trips("adj_tiles", (H - 1, W - 1), "y" if H > W else "x") == 1
    table, d = check_raster(np.full(shape, 7), 7, 1, f"one segment {shape}")
    assert table.area[0] == H * W and table.perimeter[0] == 2 * (H + W) and table.box.tolist() == [[0, 0, H, W]]
    assert table.sums[0, 3] == (H - 1) * H * (2 * H - 1) // 6 * W and table.sums[0, 5] == (H * (H - 1) // 2) * (W * (W - 1) // 2)
    assert d["extent"][0] == 1.0 and d["smoothness"][0] == 1.0 and d["mu"][0, 2] == 0.0
    lab = np.full(shape, 1)
    lab[H // 2:, W // 2:] = 2                                                  # and two segments whose border crosses tiles
    check_raster(lab, 1, 2, f"two segments {shape}")


def test_a_tall_raster_magnitudes_and_translation_bits():
    """20 000 x 40: the same blob at the top and 19 950 rows lower (sum r^2 past 2^32) inside a third segment; every float column but
    the centroid is the same bits for the two"""
    from tests.test_shapes_restatement_cpu import blob
    m = blob()
    lab = np.full((20000, 40), 3)
    lab[5:5 + m.shape[0], 3:3 + m.shape[1]][m] = 1
    lab[19955:19955 + m.shape[0], 24:24 + m.shape[1]][m] = 2
    table, d = check_raster(lab, 1, 3, "tall")
    assert table.sums[1, 3] > 2 ** 32 and table.sums[2, 3] > 2 ** 45 and table.area[0] == table.area[1] == int(m.sum())
    for k in EXACT[1:] + ("orientation",):
        col = getattr(table, k)
        assert S.same_bits(col[0], col[1]), k
    assert table.box.tolist()[:2] == [[5, 3, 5 + m.shape[0], 3 + m.shape[1]], [19955, 24, 19955 + m.shape[0], 24 + m.shape[1]]]


def test_one_label_in_two_far_blobs_and_an_empty_table():
    lab = np.full((2 * TH + 4, 3 * TW), 2)
    lab[2:6, 2:7] = 1
    lab[TH + 8:TH + 11, 2 * TW + 3:2 * TW + 9] = 1
    table, _ = check_raster(lab, 1, 2, "blobs")
    assert table.area[0] == 20 + 18 and table.perimeter[0] == 2 * (4 + 5) + 2 * (3 + 6) and table.box[0].tolist() == [2, 2, TH + 11, 2 * TW + 9]
    table, _ = check_raster(lab, 1, 4, "rows without pixels")                  # labels 3 and 4 occur nowhere
    assert not table.sums[2:].any() and not table.box[2:].any() and table.present.tolist() == [True, True, False, False]
    for lab0, start in ((np.zeros((5, 40), I32), 1), (np.full((5, 40), -3, I32), 0)):
        table, _ = check_raster(lab0, start, 0, "N == 0")                      # N == 0: null outputs, nothing written
        assert table.sums.shape == (0, 7) and table.box.shape == (0, 4) and table.orientation.shape == (0,)
        from obia_amd import segment_shapes
        assert segment_shapes(lab0, start_label=start).n_labels == 0          # the default n_labels: up to the largest label


@functools.lru_cache(maxsize=None)
def golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z["raw"].astype(F32), z["labels"].astype(I32)


@pytest.mark.parametrize("name", ["c2s_256x256x4_c025", "quickstart_128x128x3", "mask_128x160x4_c025"])
def test_a_golden_slic_map(name):
    """the tables are the restatement's; the columns are scikit-image's within the bounds of tests/test_shapes_restatement_cpu.py
    (the restatement is, there; here the device columns are the restatement's bits)"""
    raw, lab = golden(name)
    N = int(lab.max())
    table, d = check_raster(lab, 1, N, name)
    g = np.load(os.path.join(GOLDEN, "shapes", name + ".npz"))
    idx = g["label"].astype(I64) - 1
    assert np.array_equal(table.area[idx], g["area"]) and np.array_equal(table.box[idx], g["bbox"])
    assert np.array_equal(table.centroid[idx], g["centroid"]) and np.array_equal(table.extent[idx], g["extent"])


def test_numpy_and_cuda_tensors_give_one_result():
    from obia_amd import ShapeTable, segment_shapes
    raw, lab = golden("quickstart_128x128x3")
    a = segment_shapes(lab)
    b = segment_shapes(torch.as_tensor(lab).cuda())
    assert isinstance(a.sums, np.ndarray) and b.sums.is_cuda and b.box.is_cuda and b.orientation.is_cuda and b.present.dtype == torch.bool
    for k in ("sums", "box", "present") + S.INT_COLUMNS + EXACT + ("orientation",):
        assert S.same_bits(getattr(a, k), getattr(b, k).cpu().numpy()), k
    c = ShapeTable(a.sums, a.box, a.n_labels)                                  # a table from its raw parts
    assert S.same_bits(c.mu, a.mu) and isinstance(c.mu, np.ndarray)
    with pytest.raises(ValueError, match="sums must be"):
        ShapeTable(a.sums[:, :6], a.box, a.n_labels)


def test_merge_after_a_round_of_mutual_best_neighbours_is_a_fresh_pass():
    from obia_amd import compact_roots, relabel, segment_graph, segment_shapes, zonal_stats
    raw, lab = golden("quickstart_128x128x3")
    N = int(lab.max())
    g = segment_graph(lab)
    means = zonal_stats(raw, lab, n_labels=N)["mean"]
    best, best_d2 = g.best_neighbor(g.d2(means))
    me = np.arange(N)
    mutual = (best >= 0) & (best[np.maximum(best, 0)] == me)
    root = np.where(mutual, np.minimum(me, best), me).astype(I32)
    assert 10 < int(mutual.sum()) // 2 < N // 2
    table = segment_shapes(lab)
    merged = table.merge(root, g)
    want = S.merge(table.sums, table.box, root, g.indptr, g.neighbor, g.border)
    assert S.same_bits(merged.sums, want[0]) and S.same_bits(merged.box, want[1])
    relab = relabel(lab, compact_roots(root, 1, present=table.present), 1)
    fresh = segment_shapes(relab)
    keep = merged.present
    assert fresh.n_labels == int(keep.sum()) == N - int(mutual.sum()) // 2
    assert S.same_bits(merged.sums[keep], fresh.sums) and S.same_bits(merged.box[keep], fresh.box)
    for k in EXACT + ("orientation",):
        assert S.same_bits(getattr(merged, k)[keep], getattr(fresh, k)), k
    check_columns(merged, *want, name="merged")
    # tensors in, tensors out
    tm = segment_shapes(torch.as_tensor(lab).cuda()).merge(torch.as_tensor(root).cuda(), segment_graph(torch.as_tensor(lab).cuda()))
    assert tm.sums.is_cuda and S.same_bits(tm.sums.cpu().numpy(), want[0]) and S.same_bits(tm.box.cpu().numpy(), want[1])
    with pytest.raises(ValueError, match="root must"):
        table.merge(root[:-1], g)


def test_pair_shapes_and_a_link_rule_with_a_shape_criterion():
    from obia_amd import pair_shapes, segment_graph, segment_shapes, zonal_stats
    raw, lab = golden("mask_128x160x4_c025")                                   # label 0 is background here: pseudo entries N
    N = int(lab.max())
    g, table = segment_graph(lab), segment_shapes(lab)
    pairs = pair_shapes(g, table)
    want = S.pair_shapes(g.indptr, g.neighbor, g.border, table.sums, table.box)
    assert set(pairs) == set(want) == {"area", "perimeter", "box", "compactness", "shape_index", "smoothness"}
    for k in want:
        assert S.same_bits(pairs[k], want[k]), k
    assert (g.neighbor >= N).any() and np.isnan(pairs["compactness"][g.neighbor >= N]).all() and not np.isnan(pairs["compactness"][g.real]).any()
    d2 = g.d2(zonal_stats(raw, lab, n_labels=N)["mean"])
    plain = g.components(d2 <= 300.0 ** 2)
    shaped = g.components((d2 <= 300.0 ** 2) & (pairs["compactness"] >= 0.4))
    n_plain, n_shaped = len(np.unique(plain)), len(np.unique(shaped))
    assert n_plain < n_shaped < N, (n_plain, n_shaped, N)                       # the shape criterion refuses some of the colour's links
    tp = pair_shapes(segment_graph(torch.as_tensor(lab).cuda()), segment_shapes(torch.as_tensor(lab).cuda()))
    assert all(tp[k].is_cuda and S.same_bits(tp[k].cpu().numpy(), want[k]) for k in want)


def test_shape_columns_of_an_objects_table():
    from obia_amd import create_objects, segment_shapes, shape_columns
    from obia_amd.shapes import SHAPE_COLUMNS
    from tests.test_gpu_adjacency import blocks
    raw, lab = blocks()
    lab = np.where(lab == 17, 36, lab).astype(I32)                              # label 17 is absent: 36 rows in the table, 35 objects
    objects = create_objects(lab, raw, calculate_textural=False, geometry=False)
    table = segment_shapes(lab)
    affine = [2.0, 0.0, 0.0, -2.0, 500.0, 900.0]
    sc = shape_columns(objects, table, affine=affine)
    assert list(sc.columns) == list(SHAPE_COLUMNS) + ["centroid_x", "centroid_y"] and sc.index.equals(objects.index) and len(sc) == 35
    assert list(shape_columns(objects, table).columns) == list(SHAPE_COLUMNS)
    p = table.present
    assert p.sum() == 35 and not p[16]
    assert (sc["area"] == 64).all() and (sc["perimeter"] == 32).all() and (sc["shape_index"] == 1.0).all() and (sc["extent"] == 1.0).all()
    for col, want in (("centroid_row", table.centroid[p, 0]), ("centroid_col", table.centroid[p, 1]), ("mu_rr", table.mu[p, 0]),
                      ("mu_rc", table.mu[p, 2]), ("major_axis_length", table.major_axis_length[p]), ("orientation", table.orientation[p]),
                      ("compactness", table.compactness[p]), ("smoothness", table.smoothness[p]), ("centroid_x", table.centroid_xy(affine)[p, 0]),
                      ("centroid_y", table.centroid_xy(affine)[p, 1]), ("eccentricity", table.eccentricity[p])):
        assert S.same_bits(sc[col].to_numpy(), want), col
    assert sc["centroid_x"].iloc[0] == 500.0 + 2.0 * 4.0 and sc["centroid_y"].iloc[0] == 900.0 - 2.0 * 4.0
    with pytest.raises(ValueError, match="rows"):
        shape_columns(objects.iloc[:-1], table)


def test_the_overflow_rule_at_its_threshold_through_the_abi():
    """1 x (2^21 - 1) is served (8 MiB of labels); 1 x 2^21 and its kin are refused before anything is read"""
    _lib, lib, c = env()
    W = 2 ** 21 - 1
    lab = np.zeros((1, W), I32)
    lab[0, W - 5:] = 1
    sums, box = abi_tables(lab, 1, 1)
    assert sums.tolist() == [[5, 0, 5 * W - 15, 0, sum(k * k for k in range(W - 5, W)), 0, 12]] and box.tolist() == [[0, W - 5, 1, W]]
    L = dev(np.zeros((1, 64), I32))
    out, bx = guarded((1, 7), I64, POISON, "cuda", 1), guarded((1, 4), I32, POISON, "cuda", 1)
    for H, Wd in ((1, 2 ** 21), (2 ** 21, 1), (4, 1321123), (1321123, 4), (65536, 32768)):
        assert lib.obia_shape_sums_dev(c.handle, L.data_ptr(), H, Wd, 1, 1, out.ptr, bx.ptr) == _lib.E_UNSUPPORTED, (H, Wd)
        assert ("2^63" if H * Wd < 2 ** 31 else "2^31") in _lib.last_error()
    assert 1321123 ** 3 * 4 >= 2 ** 63 > 1321122 ** 3 * 4
    torch.cuda.synchronize()
    assert out.untouched() and bx.untouched() and out.stray().size == 0 and bx.stray().size == 0
