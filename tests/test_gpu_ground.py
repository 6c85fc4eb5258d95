"""Height above ground on the GPU (obia_amd.pointcloud's GroundIndex and friends, include/obia_ground.h) against the brute-force
restatement (tests/ground_restatement.py), bit for bit: ``hag`` as uint32, ``zg`` as uint64, ``m`` as it is.  The tolerance is derived,
not measured -- every operation of the header is one correctly rounded IEEE operation in a stated order, and the kernel is built with
contraction off.  Every case first asserts, on the restatement's own result, that the classes it exists for are present."""
import ctypes
import functools

import numpy as np
import pytest

from tests import ground_restatement as G
from tests import launch_grids as LG
from tests import pointcloud_restatement as R
from tests.guarded import POISONS, guarded, snapshot, unchanged
from tests.offset_views import offset_view, residue
from tests.refusal_text import refused_saying

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EXERCISED = ("obia_ground_query_dev", "obia_ground_dtm_dev")
U = {1: np.uint8, 4: np.uint32, 8: np.uint64}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(U[a.dtype.itemsize])


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    assert bad.size == 0, (what, bad.size, bad[:5].tolist(), got.reshape(-1)[bad[:5]].tolist(), want.reshape(-1)[bad[:5]].tolist())


def cloud(x, y, z, **extra):
    return dict({"X": x, "Y": y, "Z": z}, **extra)


def index_of(given):
    from obia_amd.pointcloud import GroundIndex
    idx = GroundIndex(cloud(*given))
    kept, dropped = G.keep_ground(*given)
    assert idx.dropped == dropped and idx.n_ground == len(kept[0])
    assert 1 <= idx.shape[0] * idx.shape[1] <= 4 * idx.n_ground + 16 and idx.side > 0.0
    return idx, kept


def compare(idx, kept, x, y, z, count, md, want=None):
    """the three results of one query set against the restatement; returns the restatement's"""
    want = want or G.ground_z(kept, x, y, count, md)
    same(idx.ground_z(x, y, count=count, max_distance=md), want["zg"], "zg")
    same(idx.neighbours(x, y, count=count, max_distance=md), want["m"], "m")
    same(idx.height_above_ground(cloud(x, y, z), count=count, max_distance=md), G.hag(z, want["zg"]), "hag")
    return want


# ---------------------------------------------------------------------------------------------------------------- the base case
@functools.lru_cache(maxsize=None)
def base():
    given = G.base_ground()
    idx, kept = index_of(given)
    x, y, z = G.base_queries(given, idx.side)
    return idx, kept, x, y, z


@functools.lru_cache(maxsize=None)
def base_want(count, md):
    _, kept, x, y, _ = base()
    return G.ground_z(kept, x, y, count, md)


@pytest.mark.parametrize("md", [0.0, 1.5, 0.75])
@pytest.mark.parametrize("count", [1, 2, 3, 8])
def test_base_case(count, md):
    idx, kept, x, y, z = base()
    want = base_want(count, md)
    finite = np.isfinite(x) & np.isfinite(y)
    nearest = np.sqrt(base_want(1, 0.0)["d2"][:, 0])
    assert idx.dropped == 5 and (~finite).sum() == 6
    assert want["tie"].sum() > 0 and (nearest[finite] > idx.side).sum() > 300 and (nearest[finite] > 40 * idx.side).sum() > 100
    assert (want["d2"][:, 0] == 0.0).sum() > 0 and ((np.floor(x / idx.side) * idx.side == x) & finite).sum() > 300
    assert np.isnan(G.hag(z, want["zg"])).mean() < 0.5 and np.isnan(z).sum() > 300
    if md:
        assert (want["m"][finite] == 0).sum() > 300 and ((want["m"] > 0) & (want["m"] < count)).sum() >= (0 if count == 1 else 50)
    compare(idx, kept, x, y, z, count, md, want)


def test_exact_ties_go_to_the_lowest_index():
    rs = np.random.RandomState(11)
    jx, jy = np.meshgrid(np.arange(12.0), np.arange(9.0))
    p = rs.permutation(jx.size)
    given = (jx.reshape(-1)[p], jy.reshape(-1)[p], rs.uniform(100.0, 110.0, jx.size))
    idx, kept = index_of(given)
    hx, hy = np.meshgrid(np.arange(-1.5, 13.0, 0.5), np.arange(-1.5, 10.0, 0.5))       # lattice points, edge midpoints, cell centres, outside
    x, y = hx.reshape(-1), hy.reshape(-1)
    z = rs.uniform(100.0, 130.0, len(x))
    for count in (1, 2, 3, 5):
        want = G.ground_z(kept, x, y, count, 0.0)
        assert want["tie"].sum() > 300 and (want["d2"][:, 0] == 0.0).sum() == 108
        centre = (x == 4.5) & (y == 3.5)                                                  # four at d2 = 0.5: the lowest indices, in order
        four = np.sort(np.flatnonzero((np.abs(kept[0] - 4.5) == 0.5) & (np.abs(kept[1] - 3.5) == 0.5)))
        assert want["idx"][centre][0].tolist()[:min(count, 4)] == four[:min(count, 4)].tolist()
        compare(idx, kept, x, y, z, count, 0.0, want)
    compare(idx, kept, x, y, z, 5, 1.0)                                                   # the cut-off on exact squares: equality is in


def test_two_far_clusters():
    """Three points in one cluster and 200 in another 10^4 point spacings away: the grid's side grows with the extent (the cells are
    O(ng)), so each cluster fills a cell and some thirty empty cells lie between them.  count = 8 beside the small cluster must take
    neighbours from both."""
    rs = np.random.RandomState(12)
    ax, ay = np.array([0.0, 0.7, 0.3]), np.array([0.0, 0.2, 0.9])
    bx, by = 10000.0 + rs.uniform(0.0, 14.0, 200), 2500.0 + rs.uniform(0.0, 14.0, 200)
    given = (np.concatenate([ax, bx]), np.concatenate([ay, by]), np.concatenate([[50.0, 51.0, 52.0], rs.uniform(80.0, 90.0, 200)]))
    idx, kept = index_of(given)
    assert idx.shape[1] > 20 and 10000.0 / idx.side > 20
    x = np.concatenate([rs.uniform(-2.0, 3.0, 40), 5000.0 + rs.uniform(-500.0, 500.0, 40), 10000.0 + rs.uniform(-3.0, 17.0, 40)])
    y = np.concatenate([rs.uniform(-2.0, 3.0, 40), 1250.0 + rs.uniform(-500.0, 500.0, 40), 2500.0 + rs.uniform(-3.0, 17.0, 40)])
    z = rs.uniform(50.0, 120.0, len(x))
    want = G.ground_z(kept, x, y, 8, 0.0)
    both = (want["idx"][:40] < 3).any(1) & (want["idx"][:40] >= 3).any(1)
    assert both.all() and (want["idx"][80:] >= 3).all()
    compare(idx, kept, x, y, z, 8, 0.0, want)
    for count, md in ((1, 0.0), (3, 0.0), (8, 6000.0), (2, 3.0)):
        compare(idx, kept, x, y, z, count, md)


@pytest.mark.parametrize("name", ["one", "two", "one_xy", "along_x", "along_y"])
def test_degenerate_ground_sets(name):
    rs = np.random.RandomState(13)
    t = np.sort(rs.uniform(0.0, 40.0, 57))
    given = {"one": ([12.5], [-3.25], [7.0]),
             "two": ([12.5, 13.0], [-3.25, 4.0], [7.0, 9.0]),
             "one_xy": ([3.0] * 5, [4.0] * 5, [1.0, 2.0, 3.0, 4.0, 5.0]),
             "along_x": (100.0 + t, np.full(57, 8.0), rs.uniform(0.0, 5.0, 57)),
             "along_y": (np.full(57, -8.0), 100.0 + t, rs.uniform(0.0, 5.0, 57))}[name]
    given = tuple(np.asarray(v, np.float64) for v in given)
    idx, kept = index_of(given)
    assert idx.shape[0] * idx.shape[1] <= 4 * len(given[0]) + 16
    if name == "along_x":
        assert idx.shape[0] == 1 and idx.shape[1] > 8
    if name == "along_y":
        assert idx.shape[1] == 1 and idx.shape[0] > 8
    cx, cy = given[0].mean(), given[1].mean()
    x = np.concatenate([given[0], cx + rs.uniform(-60.0, 60.0, 300)])
    y = np.concatenate([given[1], cy + rs.uniform(-60.0, 60.0, 300)])
    z = rs.uniform(0.0, 30.0, len(x))
    want = compare(idx, kept, x, y, z, 8, 0.0)
    assert want["m"].max() == min(8, len(given[0])) and (want["d2"][:, 0] == 0.0).sum() >= len(given[0])
    compare(idx, kept, x, y, z, 1, 0.0)
    compare(idx, kept, x, y, z, 8, 10.0)


def test_a_tall_grid_is_walked_in_linear_time():
    """100 000 collinear ground points along y make a grid of one column and about 50 000 rows.  A query as far to the side as the line
    is long, must walk every ring; queries beyond its ends and beside it walk a few.  A ring of such a grid has two
    pieces inside it -- the edge columns lie outside -- so the walk is about 10^5 pieces of two dependent loads each, some tenths of a
    second at a few microseconds a piece; a walk that also steps through the 2 r - 1 cells of each absent edge takes 5 * 10^9 steps,
    minutes.  The bound of 5 s stands between the two by more than a factor of ten either way."""
    import time
    rs = np.random.RandomState(19)
    ng = 100000
    t = np.sort(rs.uniform(0.0, 20000.0, ng))
    given = (np.full(ng, 500.0), 7000.0 + t, 100.0 + 0.001 * t)
    idx, kept = index_of(given)
    assert idx.shape[1] == 1 and idx.shape[0] > 40000
    L = 20000.0
    x = np.concatenate([500.0 + rs.uniform(L, 2.0 * L, 32) * rs.choice([-1.0, 1.0], 32), 500.0 + rs.uniform(-3.0, 3.0, 32),
                        500.0 + rs.uniform(-50.0, 50.0, 32)])
    y = np.concatenate([7000.0 + rs.uniform(0.0, L, 32), 7000.0 + L + rs.uniform(1.0, 5.0, 16), 7000.0 - rs.uniform(1.0, 5.0, 16),
                        7000.0 + rs.uniform(0.0, L, 32)])
    z = rs.uniform(100.0, 150.0, len(x))
    want = G.ground_z(kept, x, y, 8, 0.0)
    assert (np.sqrt(want["d2"][:32, 0]) > 40000 * idx.side).all()                         # rings to the end of the grid
    same(idx.ground_z(x[:1], y[:1], count=1), G.ground_z(kept, x[:1], y[:1], 1, 0.0)["zg"], "warm-up")
    t0 = time.perf_counter()
    got = idx.ground_z(x, y, count=8)
    seconds = time.perf_counter() - t0
    same(got, want["zg"], "zg")
    assert seconds < 5.0, seconds
    cut = G.ground_z(kept, x, y, 8, 6.0)
    assert (cut["m"][:32] == 0).all() and (cut["m"][32:64] > 0).all() and (cut["m"][64:] == 0).any()      # the cut-off ends a walk early too
    compare(idx, kept, x, y, z, 8, 6.0, cut)


def test_utm_sized_coordinates():
    rs = np.random.RandomState(14)
    gx = 600000.0 + np.round(rs.uniform(0.0, 25.0, 500), 3)
    gy = 4200000.0 + np.round(rs.uniform(0.0, 25.0, 500), 3)
    given = (gx, gy, 1500.0 + rs.uniform(0.0, 3.0, 500))
    idx, kept = index_of(given)
    x = 600000.0 + np.round(rs.uniform(-5.0, 30.0, 1500), 3)
    y = 4200000.0 + np.round(rs.uniform(-5.0, 30.0, 1500), 3)
    pick = rs.randint(0, 500, 300)
    x[::5], y[::5] = gx[pick] + 0.001, gy[pick] - 0.001                                   # a millimetre beside a ground point
    z = 1500.0 + rs.gamma(2.0, 5.0, len(x))
    want = G.ground_z(kept, x, y, 3, 0.0)
    assert (np.sqrt(want["d2"][:, 0]) < 0.002).sum() > 50 and (np.sqrt(want["d2"][:, 0]) > idx.side).sum() > 50
    compare(idx, kept, x, y, z, 3, 0.0, want)
    compare(idx, kept, x, y, z, 8, 2.0)


def test_order_and_cuts():
    idx, kept, x, y, z = base()
    want = base_want(3, 1.5)
    rs = np.random.RandomState(15)
    p = rs.permutation(len(x))
    same(idx.height_above_ground(cloud(x[p], y[p], z[p]), count=3, max_distance=1.5), G.hag(z, want["zg"])[p], "permuted queries")
    cuts = [slice(0, 1234), slice(1234, 1235), slice(1235, None)]
    got = np.concatenate([idx.height_above_ground(cloud(x[c], y[c], z[c]), count=3, max_distance=1.5) for c in cuts])
    same(got, G.hag(z, want["zg"]), "three cuts")
    # a permuted ground set is another ground set: ties go to what stands first now
    g = rs.permutation(len(kept[0]))
    given = tuple(v[g] for v in kept)
    idx2, kept2 = index_of(given)
    q = slice(0, 1500)
    w2 = compare(idx2, kept2, x[q], y[q], z[q], 3, 0.0)
    w1 = G.ground_z(kept, x[q], y[q], 3, 0.0)
    assert w2["tie"].sum() > 0 and (bits(w2["zg"]) != bits(w1["zg"])).sum() > 0           # some tie went the other way


def test_height_above_ground_of_a_classified_cloud():
    from obia_amd.pointcloud import GroundIndex, height_above_ground
    rs = np.random.RandomState(16)
    (gx, gy, gz), _ = G.keep_ground(*G.base_ground(seed=5, n=1200))
    n_veg = 1500
    vx, vy = G.ORIGIN[0] + rs.uniform(0.0, G.EXTENT[0], n_veg), G.ORIGIN[1] + rs.uniform(0.0, G.EXTENT[1], n_veg)
    x, y = np.concatenate([gx, vx]), np.concatenate([gy, vy])
    z = np.concatenate([gz, 300.0 + rs.gamma(2.0, 6.0, n_veg)])
    cls = np.concatenate([np.full(len(gx), 2, np.uint8), rs.choice([1, 3, 4, 5], n_veg).astype(np.uint8)])
    p = rs.permutation(len(x))
    x, y, z, cls = x[p], y[p], z[p], cls[p]
    c = cloud(x, y, z, Classification=cls)
    is_g = cls == 2
    kept = (x[is_g], y[is_g], z[is_g])
    want = G.hag(z, G.ground_z(kept, x, y, 1, 0.0)["zg"])
    # a ground point finds itself at d2 = 0 -- unless a lower-indexed ground point shares its (x, y): the eleven duplicates
    first = {}
    later = np.zeros(is_g.sum(), bool)
    for i, key in enumerate(zip(kept[0].tolist(), kept[1].tolist())):
        later[i] = key in first
        first.setdefault(key, i)
    assert later.sum() == 11 and (want[is_g][~later] == 0.0).all() and (np.abs(want[is_g][later]) == np.float32(1.25)).all()
    got = height_above_ground(c)
    same(got, want, "ground from Classification")
    assert isinstance(got, np.ndarray)
    same(height_above_ground(c, ground=cloud(*kept)), want, "ground as a cloud")
    same(height_above_ground(c, GroundIndex.from_cloud(c, ground_class=2)), want, "ground as an index")
    t = {k: torch.as_tensor(v).cuda() for k, v in c.items()}
    got_t = height_above_ground(t, count=3, max_distance=2.0)
    assert torch.is_tensor(got_t) and got_t.is_cuda
    same(got_t.cpu().numpy(), G.hag(z, G.ground_z(kept, x, y, 3, 2.0)["zg"]), "tensors")
    rec = np.zeros(len(x), dtype=[("X", "f8"), ("Y", "f8"), ("Z", "f8"), ("Classification", "u1"), ("HeightAboveGround", "f4")])
    rec["X"], rec["Y"], rec["Z"], rec["Classification"], rec["HeightAboveGround"] = x, y, z, cls, -7.0
    same(height_above_ground([rec]), want, "a structured array: Z is read, never HeightAboveGround")


@pytest.mark.parametrize("affine", [[1.5, 0.0, 0.0, -1.5, G.ORIGIN[0] - 4.0, G.ORIGIN[1] + 52.0],
                                    [1.5 * np.cos(0.3), -1.5 * np.sin(0.3), -1.5 * np.sin(0.3), -1.5 * np.cos(0.3), G.ORIGIN[0] + 5.0, G.ORIGIN[1] + 60.0]],
                         ids=["north_up", "rotated"])
def test_to_raster_and_height_above_dtm(affine):
    from obia_amd.pointcloud import height_above_dtm
    idx, kept, x, y, z = base()
    shape = (37, 53)
    want = G.to_raster(kept, shape, affine, 3, 4.0)
    assert 50 < np.isnan(want).sum() < want.size // 2                                     # the disc and what lies beyond the ground
    dtm = idx.to_raster(shape, affine, count=3, max_distance=4.0)
    same(dtm, want, "to_raster")
    same(idx.to_raster(shape, affine), G.to_raster(kept, shape, affine), "to_raster, nearest point")
    px = R.pixel_of(x, y, R.invert_affine(affine), *shape)
    assert (px < 0).sum() > 300 and (px >= 0).sum() > 2000
    want_hag = G.hag(z, G.dtm_z(x, y, want, affine))
    assert 0.1 < np.isnan(want_hag).mean() < 0.9
    same(height_above_dtm(cloud(x, y, z), want, affine), want_hag, "height_above_dtm")
    got_t = height_above_dtm({k: torch.as_tensor(v).cuda() for k, v in cloud(x, y, z).items()}, torch.as_tensor(want).cuda(), affine)
    assert torch.is_tensor(got_t)
    same(got_t.cpu().numpy(), want_hag, "height_above_dtm, tensors")
    poles = want.copy()
    poles[3, 4], poles[5, 6] = np.inf, -np.inf                                            # a pixel that is not finite is no ground
    same(height_above_dtm(cloud(x, y, z), poles, affine), G.hag(z, G.dtm_z(x, y, poles, affine)), "infinite pixels")


def test_normalize_heights_feeds_the_rasters():
    from obia_amd.pointcloud import PointRasters, normalize_heights
    idx, kept, x, y, z = base()
    inten = (np.arange(len(x)) % 65536).astype(np.uint16)
    out = normalize_heights(cloud(x, y, z, Intensity=inten), idx, count=3, max_distance=1.5)
    assert sorted(out) == ["HeightAboveGround", "Intensity", "X", "Y"] and out["Intensity"] is not None
    want = G.hag(z, base_want(3, 1.5)["zg"])
    same(out["HeightAboveGround"], want, "normalize_heights")
    assert sorted(normalize_heights(cloud(x, y, z), idx)) == ["HeightAboveGround", "X", "Y"]
    affine, shape = [0.5, 0.0, 0.0, -0.5, G.ORIGIN[0] - 2.0, G.ORIGIN[1] + 50.0], (104, 136)
    a = PointRasters(shape, affine).add(out).result()
    b = PointRasters(shape, affine).add({"X": x, "Y": y, "HeightAboveGround": want}).result()
    assert np.isfinite(a["chm"]).sum() > 1000
    for name in ("chm", "density", "count"):
        same(a[name], b[name], name)
    dtm_affine = [1.5, 0.0, 0.0, -1.5, G.ORIGIN[0] - 4.0, G.ORIGIN[1] + 52.0]
    dtm = G.to_raster(kept, (37, 53), dtm_affine, 1, 0.0)
    via = normalize_heights(cloud(x, y, z), dtm=dtm, affine_transformation=dtm_affine)
    same(via["HeightAboveGround"], G.hag(z, G.dtm_z(x, y, dtm, dtm_affine)), "normalize_heights over a dtm")


def test_second_trip_of_the_stride_loop():
    n = LG.crossing("ground_query", (1,), 0, "x")
    assert LG.trips("ground_query", (n,), "x") == 2 and LG.trips("ground_query", (n - 1,), "x") == 1
    rs = np.random.RandomState(17)
    given = (rs.uniform(0.0, 8.0, 16), rs.uniform(0.0, 8.0, 16), rs.uniform(10.0, 12.0, 16))
    idx, kept = index_of(given)
    x, y = rs.uniform(-2.0, 10.0, n), rs.uniform(-2.0, 10.0, n)
    z = rs.uniform(10.0, 40.0, n)
    x[-1], y[-1] = given[0][7], given[1][7]                                               # the one query of the second trip
    want = compare(idx, kept, x, y, z, 2, 0.0)
    assert want["zg"][-1] == given[2][7]


# ------------------------------------------------------------------------------------------------------------------- the buffers
@functools.lru_cache(maxsize=None)
def small():
    rs = np.random.RandomState(18)
    (gx, gy, gz), _ = G.keep_ground(*G.base_ground(seed=6, n=600))
    idx, kept = index_of((gx, gy, gz))
    x, y, z = G.base_queries((gx, gy, gz), idx.side, seed=8, n=1500)
    affine = [1.5, 0.0, 0.0, -1.5, G.ORIGIN[0] - 4.0, G.ORIGIN[1] + 52.0]
    dtm = G.to_raster(kept, (37, 53), affine, 1, 6.0)
    want = G.ground_z(kept, x, y, 3, 1.5)
    assert want["tie"].sum() > 0 and (want["m"] == 0).sum() > 100 and np.isnan(dtm).any()
    return dict(idx=idx, x=x, y=y, z=z, want=want, hag=G.hag(z, want["zg"]), affine=affine, dtm=dtm, dtm_zg=G.dtm_z(x, y, dtm, affine),
                rs=rs)


def test_every_entry_point_of_the_table_is_exercised():
    from obia_amd import _lib
    assert set(EXERCISED) == set(_lib._GROUND_SIGNATURES)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("poison", POISONS, ids=[f"{p:02X}" for p in POISONS])
def test_buffers_off_the_boundary_and_guarded_outputs(k, poison):
    """every input k elements past a 16-byte boundary (8-byte arrays 8 bytes for odd k, the int32 arrays 4, 8 and 12), every output
    between guards: the results bit for bit, every element written, no guard byte touched, the inputs unchanged, two runs equal; and
    what is refused, or empty, writes nothing"""
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.default_context(0)
    s = small()
    idx, n = s["idx"], len(s["x"])
    dev = lambda a: offset_view(torch.as_tensor(np.ascontiguousarray(a)).cuda(), k)      # noqa: E731
    gx, gy, gz, gi, cs = (offset_view(t.clone(), k) for t in (idx._gx, idx._gy, idx._gz, idx._gidx, idx._cell_start))
    x, y, z, dtm = dev(s["x"]), dev(s["y"]), dev(s["z"]), dev(s["dtm"])
    assert residue(gx) == residue(x) == (8 * k) % 16 and residue(gi) == residue(cs) == residue(dtm) == 4 * k
    ins = [gx, gy, gz, gi, cs, x, y, z, dtm]
    snaps = [snapshot(t) for t in ins]
    inv = (ctypes.c_double * 6)(*R.invert_affine(s["affine"]))
    h = ctx.handle
    ncy, ncx = idx.shape
    cx0, cy0 = idx._cell0
    H, W = s["dtm"].shape

    def query(o, n_=n, count=3, md=1.5, gx_=gx.data_ptr(), gi_=gi.data_ptr(), cs_=cs.data_ptr(), ng=idx.n_ground, ncx_=ncx, ncy_=ncy, side=idx.side,
              x_=x.data_ptr(), z_=z.data_ptr(), zg="zg", hag="hag", m="m", cx0_=cx0):
        p = lambda name: None if name is None else o[name].ptr if isinstance(name, str) else name      # noqa: E731
        return lib.obia_ground_query_dev(h, gx_, gy.data_ptr(), gz.data_ptr(), gi_, ng, cs_, ncx_, ncy_, cx0_, cy0, side, x_, y.data_ptr(), z_, n_,
                                         count, md, p(zg), p(hag), p(m))

    def dtm_call(o, n_=n, x_=x.data_ptr(), inv_=inv, dtm_=dtm.data_ptr(), H_=H, zg="dzg", hag="dhag"):
        p = lambda name: None if name is None else o[name].ptr if isinstance(name, str) else name      # noqa: E731
        return lib.obia_ground_dtm_dev(h, x_, y.data_ptr(), z.data_ptr(), n_, inv_, dtm_, H_, W, p(zg), p(hag))

    def outputs():
        return {name: guarded((n,), dt, poison, "cuda", k) for name, dt in (("zg", np.float64), ("hag", np.float32), ("m", np.uint8),
                                                                            ("dzg", np.float64), ("dhag", np.float32), ("zg2", np.float64))}
    runs = []
    for _ in range(2):
        o = outputs()
        assert o["zg"].ptr % 16 == (8 * k) % 16 and o["hag"].ptr % 16 == 4 * k and o["m"].ptr % 16 == k
        calls = [query(o), dtm_call(o), query(o, z_=None, zg="zg2", hag=None, m=None)]
        assert calls == [0, 0, 0], (calls, _lib.last_error())
        for name, want in (("zg", s["want"]["zg"]), ("hag", s["hag"]), ("m", s["want"]["m"]), ("dzg", s["dtm_zg"]),
                           ("dhag", G.hag(s["z"], s["dtm_zg"])), ("zg2", s["want"]["zg"])):
            same(o[name].host(), want, name)
            assert o[name].findings(name=name) == []
        runs.append({name: g.host().tobytes() for name, g in o.items()})
    assert runs[0] == runs[1]

    # refused or empty: nothing is written
    o = outputs()
    X, GX, GI, CS, Z = x.data_ptr(), gx.data_ptr(), gi.data_ptr(), cs.data_ptr(), z.data_ptr()
    invalid = [query(o, n_=-1), query(o, count=0), query(o, count=9), query(o, md=-1.0), query(o, md=float("nan")), query(o, side=0.0),
               query(o, side=float("nan")), query(o, side=float("inf")), query(o, ng=0), query(o, ncx_=0), query(o, ncy_=0),
               query(o, ncx_=4 * idx.n_ground + 17, ncy_=1), query(o, ncx_=2 ** 40, ncy_=2 ** 40), query(o, cx0_=2 ** 31), query(o, gx_=None),
               query(o, gx_=GX + 4), query(o, gi_=GI + 2), query(o, cs_=CS + 1), query(o, cs_=None), query(o, x_=None), query(o, x_=X + 4),
               query(o, z_=Z + 4), query(o, z_=None), query(o, hag=None), query(o, zg=None), query(o, zg=o["zg"].ptr + 4), query(o, hag=o["hag"].ptr + 2),
               query(o, zg=X), query(o, zg="zg", hag="zg"), query(o, m="hag"),
               dtm_call(o, n_=-1), dtm_call(o, x_=None), dtm_call(o, x_=X + 4), dtm_call(o, inv_=None), dtm_call(o, dtm_=None),
               dtm_call(o, dtm_=dtm.data_ptr() + 2), dtm_call(o, H_=0), dtm_call(o, hag=None), dtm_call(o, zg=o["dzg"].ptr + 4), dtm_call(o, zg=X),
               dtm_call(o, hag=dtm.data_ptr())]
    assert invalid == [_lib.E_INVALID] * len(invalid), invalid
    # ... and says so in full: a null output, an output one byte on, an output where an input starts
    refused_saying("ground: query: bad arguments (null, misaligned or overlapping buffers)", query,
                   dict(o=o, zg=None), dict(o=o, zg=o["zg"].ptr + 1), dict(o=o, hag=o["hag"].ptr + 1), dict(o=o, zg=Z), dict(o=o, m=CS))
    refused_saying("ground: dtm: bad arguments (null, misaligned or overlapping buffers)", dtm_call,
                   dict(o=o, hag=None), dict(o=o, zg=o["dzg"].ptr + 1), dict(o=o, hag=o["dhag"].ptr + 1), dict(o=o, zg=Z), dict(o=o, hag=dtm.data_ptr()))
    unsupported = [query(o, n_=2 ** 31), query(o, ng=2 ** 31), dtm_call(o, n_=2 ** 31)]
    assert unsupported == [_lib.E_UNSUPPORTED] * len(unsupported), unsupported
    empty = [query(o, n_=0), query(o, n_=0, x_=None, z_=None, hag=None), dtm_call(o, n_=0), dtm_call(o, n_=0, x_=None)]
    assert empty == [0] * len(empty), (empty, _lib.last_error())
    assert all(g.untouched() and g.stray().size == 0 for g in o.values())
    assert all(unchanged(t, sn) for t, sn in zip(ins, snaps))
