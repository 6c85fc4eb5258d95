"""The ground filter on the GPU (include/obia_groundfilter.h, obia_amd/csrc/groundfilter.hip) against tests/groundfilter_restatement.py,
bit for bit: the grey filters over every raster shape around the line kernels' tiles, every class of radius and of contents; the cell
minimum for every order and cut; the threshold raster; ground_filter and classify_ground end to end, the chain into
normalize_heights and points_to_rasters on CUDA tensors, the accumulator form; two runs bit for bit; every launch clamp crossed.
Outputs of the direct calls lie between poisoned guards (tests/guarded.py)."""
import ctypes
import functools

import numpy as np
import pytest

from tests import groundfilter_restatement as R
from tests import launch_grids as LG
from tests import pointcloud_restatement as PR
from tests.guarded import POISONS, guarded
from tests.test_gpu_launch_clamps import call, crossed, dev, env, judge

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = POISONS[0]
F32, F64, U8, I32, I64 = np.float32, np.float64, np.uint8, np.int32, np.int64
TILE_X, TILE_Y = 1024, 128                                      # OBIA_MORPH_ROW_TILE, OBIA_MORPH_COL_TILE (asserted below)


def plane(shape, seed, nan=0.3):
    rs = np.random.RandomState(seed)
    Z = rs.normal(0, 10, shape).astype(F32)
    Z[rs.uniform(size=shape) < nan] = np.nan
    return Z


def run_filter(Z, r, op, name="dst"):
    """obia_morph_filter_dev on guarded planes; the result, judged against nothing yet"""
    _lib, lib, c = env()
    H, W = Z.shape
    src = dev(Z)
    tmp, dst = guarded((H, W), F32, POISON, "cuda", 1), guarded((H, W), F32, POISON, "cuda", 3)
    call(lib.obia_morph_filter_dev, src.data_ptr(), H, W, r, op, tmp.ptr, dst.ptr)
    assert tmp.stray().size == 0, name
    return dst


def check_filters(Z, r, name):
    judge(run_filter(Z, r, 0), R.erosion(Z, r), f"{name}: erosion r={r}")
    judge(run_filter(Z, r, 1), R.dilation(Z, r), f"{name}: dilation r={r}")


def sizes(r, tile):
    return [1, 2, r, 2 * r, 2 * r + 1, tile - 1, tile, tile + 1, tile + 2 * r + 1, 2 * tile + 3]


def test_the_tiles_are_the_library_s():
    from obia_amd import _lib
    assert (_lib.MORPH_ROW_TILE, _lib.MORPH_COL_TILE) == (TILE_X, TILE_Y)
    assert LG.unit("morph_rows", (3, 1), 1, "x") == TILE_X and LG.unit("morph_cols", (1, 3), 0, "y") == TILE_Y


# ------------------------------------------------------------------------------------------------------------- filters: raster shapes
@pytest.mark.parametrize("r", [3, 16])
def test_filters_over_the_shapes_around_the_tiles(r):
    """every W and every H of {1, 2, r, 2r, 2r + 1, tile - 1, tile, tile + 1, tile + 2r + 1, 2 tile + 3}, each in two rasters, none of
    them square"""
    Hs, Ws = sizes(r, TILE_Y), sizes(r, TILE_X)
    shapes = set(zip(Hs, Ws[::-1])) | set(zip(Hs, Ws[3:] + Ws[:3]))
    assert {s[0] for s in shapes} == set(Hs) and {s[1] for s in shapes} == set(Ws) and all(h != w for h, w in shapes)
    for k, (H, W) in enumerate(sorted(shapes)):
        check_filters(plane((H, W), 100 * r + k), r, f"{H}x{W}")


def test_a_radius_that_covers_the_raster():
    """r >= H, r >= W, both; the widest window over more than one tile on either axis"""
    for k, (H, W, r) in enumerate(((5, 2 * TILE_X + 3, 127), (2 * TILE_Y + 3, 7, 127), (100, 100, 127), (1, 1, 127), (1, 300, 16), (300, 1, 16),
                                   (TILE_Y + 255, 40, 127), (3, TILE_X + 255, 127), (2, 2, 1), (40, 33, 16))):
        check_filters(plane((H, W), 500 + k), r, f"{H}x{W}")


# -------------------------------------------------------------------------------------------------------------------- filters: radii
@pytest.mark.parametrize("r", [1, 2, 3, 4, 16, 127])
def test_filters_at_every_class_of_radius(r):
    """windows of 3 = 2 + 1, 5 = 4 + 1, 7, 9 = 8 + 1, 33 = 32 + 1 and 255: a power of two plus one, and neither"""
    from obia_amd import grey_dilation, grey_erosion, grey_opening
    Z = plane((300, 1100), r)
    check_filters(Z, r, "300x1100")
    t = torch.as_tensor(Z).cuda()
    o = grey_opening(t, r)
    assert o.is_cuda and o.dtype == torch.float32 and R.same_bits(o.cpu().numpy(), R.opening(Z, r))
    e, d = grey_erosion(Z, r), grey_dilation(Z.astype(F64), r)               # NumPy in, NumPy out; other dtypes are cast
    assert isinstance(e, np.ndarray) and R.same_bits(e, R.erosion(Z, r)) and R.same_bits(d, R.dilation(Z, r))


def test_radius_128_is_refused():
    from obia_amd import _lib, grey_opening
    lib, ctx = _lib.load(), _lib.default_context(0)
    Z = dev(plane((9, 9), 1))
    g = [guarded((9, 9), F32, POISON, "cuda", 1) for _ in range(2)]
    assert lib.obia_morph_filter_dev(ctx.handle, Z.data_ptr(), 9, 9, 128, 0, g[0].ptr, g[1].ptr) == _lib.E_UNSUPPORTED
    assert lib.obia_morph_filter_dev(ctx.handle, Z.data_ptr(), 9, 9, 0, 0, g[0].ptr, g[1].ptr) == _lib.E_INVALID
    assert lib.obia_morph_filter_dev(ctx.handle, Z.data_ptr(), 9, 9, 1, 2, g[0].ptr, g[1].ptr) == _lib.E_INVALID
    assert all(v.untouched() and v.stray().size == 0 for v in g)
    with pytest.raises(NotImplementedError):
        grey_opening(Z, 128)


# ------------------------------------------------------------------------------------------------------------------ filters: contents
def test_filters_on_empties_and_infinities():
    rs = np.random.RandomState(11)
    H, W, r = 150, 1300, 4
    Z = rs.normal(0, 5, (H, W)).astype(F32)
    runs = Z.copy()
    runs[:, 100:140], runs[60:85, :], runs[10, 1020:1030] = np.nan, np.nan, np.nan       # runs longer than the window, across both tiles' seams
    border = Z.copy()
    border[:r + 3], border[-(r + 3):], border[:, :r + 3], border[:, -(r + 3):] = np.nan, np.nan, np.nan, np.nan
    one = np.full((H, W), np.nan, F32)
    one[140, 1025] = -3.5
    inf = plane((H, W), 12, nan=0.5)
    inf[rs.uniform(size=(H, W)) < 0.05] = np.inf                          # data, not empties
    inf[rs.uniform(size=(H, W)) < 0.05] = -np.inf
    inf[20:40, 200:260] = np.inf                                             # a window of nothing but +inf stays +inf in the erosion
    inf[50:70, 200:260] = -np.inf
    inf[80:100, 200:260] = np.nan
    inf[90, 230] = np.inf                                                    # +inf alone among empties: +inf around it, not NaN
    zeros = np.where(rs.uniform(size=(H, W)) < 0.5, F32(-0.0), F32(0.0)).astype(F32)
    for name, P in (("nan runs", runs), ("nan border", border), ("all nan", np.full((H, W), np.nan, F32)), ("one cell", one), ("infinities", inf),
                    ("zeros", zeros)):
        check_filters(P, r, name)
    e = R.erosion(inf, r)
    assert np.isposinf(e[30, 230]) and np.isneginf(e[60, 230]) and np.isposinf(e[90, 230]) and np.isnan(e[85, 212])
    assert not np.signbit(run_filter(zeros, r, 0).host()).any()


# ---------------------------------------------------------------------------------------------------------------------- cell minimum
@functools.lru_cache(maxsize=None)
def cloud():
    """tests/pointcloud_restatement.py's base case (10 007 points, 37 x 53, north-up; points on cell borders and corners, outside, NaN
    and infinite coordinates) with elevations in float64: NaN, both infinities, -0, values beyond the float32 range, ties"""
    c = PR.base_case()
    rs = np.random.RandomState(21)
    z = c["z"].astype(F64) * 3.0 - 20.0 + rs.uniform(0, 1e-9, len(c["z"]))   # float64 values that round to float32
    z[::29], z[1::31], z[2::37], z[3::41], z[4::43] = -0.0, -np.inf, 1e300, -1e300, 0.0
    z[6::53], z[8] = F64(F32(-7.25)), np.inf
    assert np.isnan(z).sum() > 300 and np.isposinf(z).any()
    x, y = c["x"].copy(), c["y"].copy()
    for a in (x, y, z):
        a.setflags(write=False)
    keys = R.cell_keys(x, y, z, c["inv"], PR.H, PR.W)
    return dict(x=x, y=y, z=z, inv=c["inv"], affine=c["affine"], keys=keys, zmin=R.cell_min_finish(keys))


def add_points(keys_g, x, y, z, inv, H, W):
    _lib, lib, c = env()
    n = len(x)
    X, Y, Z = dev(np.array(x)), dev(np.array(y)), dev(np.array(z))
    call(lib.obia_gf_cell_min_dev, X.data_ptr() if n else None, Y.data_ptr() if n else None, Z.data_ptr() if n else None, n, (ctypes.c_double * 6)(*inv),
         H, W, keys_g.ptr)


def zero_state(shape, dtype=I32):
    g = guarded(shape, dtype, POISON, "cuda", 1)
    g.t.zero_()
    torch.cuda.synchronize()
    return g


def finish(keys_g, H, W):
    _lib, lib, c = env()
    out = guarded((H, W), F32, POISON, "cuda", 1)
    call(lib.obia_gf_cell_min_finish_dev, keys_g.ptr, H, W, out.ptr)
    return out


def test_cell_minimum_for_every_order_and_cut():
    c = cloud()
    n, H, W = len(c["x"]), PR.H, PR.W
    assert np.isnan(c["zmin"]).any() and np.isinf(c["zmin"]).any() and R.same_bits(c["zmin"], R.cell_min(c["x"], c["y"], c["z"], c["inv"], H, W))
    p = np.random.RandomState(3).permutation(n)
    for order, cuts in ((np.arange(n), (0, n)), (p, (0, n)), (np.arange(n), (0, 4099, 4099, 9000, n)), (p, (0, 1, 258, n))):
        g = zero_state((H, W))
        for a, b in zip(cuts[:-1], cuts[1:]):                                # (one cut is empty: n = 0 does nothing)
            i = order[a:b]
            add_points(g, c["x"][i], c["y"][i], c["z"][i], c["inv"], H, W)
        assert R.same_bits(g.host().view(np.uint32), c["keys"]) and g.stray().size == 0
        judge(finish(g, H, W), c["zmin"], "zmin")


def test_cell_minimum_of_many_points_in_one_cell_and_of_few():
    rs = np.random.RandomState(4)
    inv = R.invert_affine([1.0, 0.0, 0.0, -1.0, 0.0, 3.0])
    n = 70000
    x, y, z = rs.uniform(1.0, 2.0, n), rs.uniform(1.0, 2.0, n), rs.normal(0, 100, n)
    z[::7] = np.sort(rs.normal(0, 100, len(z[::7])))[::-1]                    # a falling run: every point lowers the minimum
    for m in (n, 0, 1, 257):
        g = zero_state((3, 4))
        add_points(g, x[:m], y[:m], z[:m], inv, 3, 4)
        keys = R.cell_keys(x[:m], y[:m], z[:m], inv, 3, 4)
        assert R.same_bits(g.host().view(np.uint32), keys) and g.stray().size == 0, m
        assert (keys != 0).sum() == (1 if m else 0)
        judge(finish(g, 3, 4), R.cell_min_finish(keys), f"zmin of {m}")


# ------------------------------------------------------------------------------------------------------------------------- threshold
def run_threshold(zmin, radii, dh):
    _lib, lib, c = env()
    H, W = zmin.shape
    K = len(radii)
    src = dev(zmin.copy())
    tmp0, tmp1 = guarded((H, W), F32, POISON, "cuda", 1), guarded((H, W), F32, POISON, "cuda", 2)
    S, T = guarded((H, W), F32, POISON, "cuda", 3), guarded((H, W), F32, POISON, "cuda", 1)
    call(lib.obia_gf_threshold_dev, src.data_ptr(), H, W, (ctypes.c_int32 * K)(*radii), (ctypes.c_double * K)(*dh), K, tmp0.ptr, tmp1.ptr, S.ptr, T.ptr)
    assert tmp0.stray().size == 0 and tmp1.stray().size == 0
    return S, T


@functools.lru_cache(maxsize=None)
def small_zmin():
    """a 150 x 1100 cell minimum with a slope, bumps, objects and holes: more than one tile on either axis"""
    rs = np.random.RandomState(31)
    yy, xx = np.mgrid[0:150, 0:1100]
    Z = (50 + 0.05 * xx + 0.02 * yy + 2 * np.sin(xx / 40.0) * np.cos(yy / 23.0) + rs.normal(0, 0.03, xx.shape)).astype(F32)
    for _ in range(60):
        cy, cx, h, w = rs.randint(0, 150), rs.randint(0, 1100), rs.randint(2, 30), rs.randint(2, 30)
        Z[cy:cy + h, cx:cx + w] += F32(rs.uniform(3, 20))
    Z[rs.uniform(size=Z.shape) < 0.2] = np.nan
    Z[40:60, 500:560] = np.nan
    Z.setflags(write=False)
    return Z


SCHEDULES = {"default": R.schedule(), "linear": R.schedule(0.5, 0.3, 0.1, 1.0, 10.0, False, 2.0), "one step": ([3], [0.25]),
             "sixteen steps": R.schedule(1.0, 0.2, 0.1, 2.0, 33.0, False, 1.0), "a radius over the raster": ([2, 127], [0.15, 2.5])}


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_threshold(name):
    radii, dh = SCHEDULES[name]
    assert len(SCHEDULES["sixteen steps"][0]) == 16
    zmin = small_zmin() if name != "a radius over the raster" else small_zmin()[:100, :120]
    S, T = run_threshold(zmin, radii, dh)
    wS, wT = R.threshold(zmin, radii, dh)
    judge(S, wS, f"{name}: surface")
    judge(T, wT, f"{name}: threshold")


def test_threshold_of_an_empty_and_of_a_sparse_plane():
    Z = np.full((9, 40), np.nan, F32)
    for name, P in (("empty", Z.copy()), ("one cell", Z.copy())):
        if name == "one cell":
            P[4, 3] = 7.0
        S, T = run_threshold(P, [1, 2], [0.5, 1.0])
        wS, wT = R.threshold(P, [1, 2], [0.5, 1.0])
        judge(S, wS, name)
        judge(T, wT, name)
        assert np.isnan(wT).sum() == (360 if name == "empty" else 270)


# ------------------------------------------------------------------------------------------------------------------------ end to end
def test_ground_filter_on_the_scene():
    from obia_amd import ground_filter
    x, y, z, truth = R.scene()
    want = R.scene_result()
    gf = ground_filter({"X": x, "Y": y, "Z": z})
    assert gf.shape == R.SCENE_SHAPE and gf.affine_transformation == R.SCENE_AFFINE and (gf.radii, gf.dh) == tuple(R.schedule())
    assert isinstance(gf.ground, np.ndarray) and gf.ground.dtype == np.bool_ and np.array_equal(gf.ground.astype(U8), want["flags"])
    for name in ("zmin", "surface", "threshold"):
        assert R.same_bits(getattr(gf, name), want[name]), name
    assert gf.counters == dict(zip(R.COUNTERS, (int(v) for v in want["counters"]))) and gf.counters["ground"] > 100000
    # the caller's grid, a structured array, another schedule; points outside, a z that is not finite
    cloud_ = np.zeros(len(x), dtype=[("X", F64), ("Y", F64), ("Z", F64), ("Intensity", np.uint16)])
    cloud_["X"], cloud_["Y"], cloud_["Z"] = x, y, z
    cloud_["Z"][::501] = np.nan
    affine, shape = [2.0, 0.0, 0.0, -2.0, 10.0, 190.0], (85, 97)
    gf = ground_filter(cloud_, slope=0.3, max_window_size=20.0, affine_transformation=affine, shape=shape)
    radii, dh = R.schedule(2.0, 0.3, 0.15, 2.5, 20.0)
    assert gf.cell_size == 2.0 and (gf.radii, gf.dh) == (radii, dh) and len(radii) == 3
    want = R.ground_filter(x, y, cloud_["Z"], affine, shape, radii, dh)
    assert np.array_equal(gf.ground.astype(U8), want["flags"]) and R.same_bits(gf.threshold, want["threshold"])
    assert gf.counters == dict(zip(R.COUNTERS, (int(v) for v in want["counters"]))) and min(gf.counters.values()) > 0


def test_the_accumulator_form_is_the_one_shot_form():
    from obia_amd import GroundFilter, ground_filter
    x, y, z, _ = R.scene()
    n = len(x)
    one = ground_filter({"X": x, "Y": y, "Z": z})
    gf = GroundFilter(one.shape, one.affine_transformation, one.radii, one.dh)
    cuts = (0, 50001, 50001, 120000, n)
    pieces = [{"X": x[a:b], "Y": y[a:b], "Z": z[a:b]} for a, b in zip(cuts[:-1], cuts[1:])]
    for p in pieces[::-1]:
        gf.add(p)
    gf.finish()
    flags = np.concatenate([gf.classify(p) for p in pieces])
    assert np.array_equal(flags, one.ground) and gf.counters == one.counters
    for name in ("zmin", "surface", "threshold"):
        assert R.same_bits(getattr(gf, name), getattr(one, name)), name
    with pytest.raises(RuntimeError):
        gf.add(pieces[0])


def test_the_chain_from_a_raw_cloud_stays_on_the_device(monkeypatch):
    """normalize_heights(classify_ground(raw)) into points_to_rasters on CUDA tensors: no tensor is copied to the host on the way"""
    from obia_amd import classify_ground, normalize_heights, points_to_rasters
    x, y, z, _ = R.scene()
    raw = {"X": torch.as_tensor(x).cuda(), "Y": torch.as_tensor(y).cuda(), "Z": torch.as_tensor(z).cuda(),
           "Intensity": torch.arange(len(x), dtype=torch.int32).cuda().to(torch.uint8)}
    want = R.scene_result()

    def boom(*a, **k):
        raise AssertionError("a tensor was copied to the host")
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "cpu", boom)
        m.setattr(torch.Tensor, "numpy", boom)
        m.setattr(torch.Tensor, "tolist", boom)
        classified = classify_ground(raw)
        cloud_ = normalize_heights(classified, count=3)
        rasters = points_to_rasters(cloud_, R.SCENE_AFFINE, R.SCENE_SHAPE)
    assert set(classified) == {"X", "Y", "Z", "Intensity", "Classification"} and classified["X"] is raw["X"]
    cls = classified["Classification"]
    assert cls.is_cuda and cls.dtype == torch.uint8 and np.array_equal(cls.cpu().numpy(), np.where(want["flags"] == 1, 2, 1).astype(U8))
    assert all(v.is_cuda for v in cloud_.values()) and all(v.is_cuda for v in rasters.values())
    # heights above the ground that was found: a ground point is its own nearest neighbour, height 0; the block stands 8 m over a
    # terrain whose gradient stays below 0.25 m/m (0.08 + 3 / 25 and 0.05 + 3 / 31 along the axes), and none of its points is farther
    # than 10 m + a point spacing from the ground around it: within 8 +- 3 m
    hag = cloud_["HeightAboveGround"].cpu().numpy()
    g = want["flags"] == 1
    assert hag.dtype == F32 and np.abs(hag[g]).max() == 0.0 and np.isfinite(hag).all()
    b = (x > 60) & (x < 85) & (y > 120) & (y < 140)
    assert b.sum() > 1000 and not g[b].any() and np.abs(hag[b] - 8.0).max() < 3.0
    chm = rasters["chm"].cpu().numpy()
    assert np.nanmax(chm) > 15.0 and np.nanmedian(chm) < 1.0
    # other classes, a NumPy cloud: the same flags
    out = classify_ground({"X": x, "Y": y, "Z": z}, ground_class=9, other_class=0)
    assert out["Classification"].dtype == np.uint8 and np.array_equal(out["Classification"], np.where(g, 9, 0))


# ---------------------------------------------------------------------------------------------------------------------- repeatability
def test_two_runs_agree_bit_for_bit():
    from obia_amd import ground_filter
    x, y, z, _ = R.scene()
    p = np.random.RandomState(9).permutation(len(x))
    a = ground_filter({"X": x, "Y": y, "Z": z})
    b = ground_filter({"X": x[p], "Y": y[p], "Z": z[p]})                      # ... and for another order of the points
    c = ground_filter({"X": x, "Y": y, "Z": z})
    for name in ("zmin", "surface", "threshold"):
        assert R.same_bits(getattr(a, name), getattr(c, name)) and R.same_bits(getattr(a, name), getattr(b, name)), name
    assert np.array_equal(a.ground, c.ground) and np.array_equal(a.ground[p], b.ground) and a.counters == b.counters == c.counters
    Z = plane((300, 1100), 77)
    assert run_filter(Z, 16, 0).host().tobytes() == run_filter(Z, 16, 0).host().tobytes()


# ---------------------------------------------------------------------------------------------------------------------- launch clamps
def new_case(name, W):
    """the clamps of the two grids this file's kernels added, found as tests/launch_grids.py finds the others': the smallest H with a
    second trip in y, confirmed through the library"""
    case = LG.Case(name, (LG.crossing(name, (1, W), 0, "y"), W), "y", threshold=0)
    LG.check(case)
    return case.sizes


def test_rows_past_the_grid_of_the_row_pass():
    H, W = new_case("morph_rows", 5)
    Z = plane((H, W), 41)
    Z[-1, -1] = -99.0                                                       # the last cell: the end of the last trip
    check_filters(Z, 2, "morph_rows")


def test_row_tiles_past_the_grid_of_the_column_pass():
    H, W = new_case("morph_cols", 3)
    assert H % TILE_Y == 1
    Z = plane((H, W), 42)
    Z[-1, -1] = -99.0
    check_filters(Z, 1, "morph_cols")
    S, T = run_threshold(Z, [1], [0.5])                                      # the folding column pass takes the second trip too
    wS, wT = R.threshold(Z, [1], [0.5])
    judge(S, wS, "surface")
    judge(T, wT, "threshold")


def test_flat_launches_past_their_grid():
    """cell minimum and classification over more points, the finish over more cells than 8192 workgroups take in one trip"""
    _lib, lib, c = env()
    (n,) = crossed("flat")
    (npx,) = crossed("flat_plane")
    H, W = 1025, 2049
    assert H * W == npx
    rs = np.random.RandomState(43)
    x, y, z = rs.uniform(-3, W + 3, n), rs.uniform(-3, H + 3, n), rs.normal(100, 5, n)
    z[::97] = np.nan
    x[-1], y[-1], z[-1] = W - 0.5, 0.5, -50.0                                # the last point: the end of the last trip, the last cell
    inv = R.invert_affine([1.0, 0.0, 0.0, -1.0, 0.0, float(H)])
    g = zero_state((H, W))
    add_points(g, x, y, z, inv, H, W)
    keys = R.cell_keys(x, y, z, inv, H, W)
    assert R.same_bits(g.host().view(np.uint32), keys) and g.stray().size == 0
    zmin = R.cell_min_finish(keys)
    judge(finish(g, H, W), zmin, "zmin")
    thresh = np.where(np.isnan(zmin), F32(np.nan), zmin + F32(4.0)).astype(F32)
    want, counters = R.classify(x, y, z, inv, thresh)
    flags = guarded((n,), U8, POISON, "cuda", 1)
    cnt = zero_state((4,), I64)
    X, Y, Zd, Td = dev(x), dev(y), dev(z), dev(thresh)
    call(lib.obia_gf_classify_dev, X.data_ptr(), Y.data_ptr(), Zd.data_ptr(), n, (ctypes.c_double * 6)(*inv), Td.data_ptr(), H, W, flags.ptr, cnt.ptr)
    judge(flags, want, "flags")
    assert cnt.host().view(np.uint64).tolist() == counters.tolist() and cnt.stray().size == 0 and min(counters) > 0 and want[-1] == 1
