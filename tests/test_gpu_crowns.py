"""obia_amd.crowns on the GPU against the restatement (tests/crowns_restatement.py): the distance bit for bit, the labels equal.

With T the side of the tile one workgroup relaxes, the shapes are 1 x 1, 1 x (2T + 6), (2T + 6) x 1, T x T, (T + 1) x (2T + 1) and
(3T + 5) x (2T + 3): one pixel, one row and one column across three tiles, exactly one tile, one pixel more than a tile on both axes,
and twelve tiles with ragged edges.  Every case runs at every shape.  The entry point once through guarded outputs (tests/guarded.py,
both poisons) with every buffer off a 16-byte boundary (tests/offset_views.py); one run end to end from a canopy height model."""
import ctypes
import functools
import math

import numpy as np
import pytest

from tests import crowns_restatement as C
from tests.guarded import POISONS, guarded, snapshot, unchanged
from tests.offset_views import offset_view, residue

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from obia_amd._lib import CROWNS_TILE as T  # noqa: E402

SHAPES = ((1, 1), (1, 2 * T + 6), (2 * T + 6, 1), (T, T), (T + 1, 2 * T + 1), (3 * T + 5, 2 * T + 3))
SHAPE_IDS = [f"{h}x{w}" for h, w in SHAPES]
KINDS = ("random8", "random4", "constant", "quant-w0", "quant-w05", "zero", "pixel", "seams", "several", "nan-inf", "pocket", "mask",
         "max-dist")


def random_seeds(rs, H, W, n_ids=None):
    """(0, 0) and about one seed per 150 pixels more, some off the raster; ids 1 .. n_ids drawn with repeats"""
    n = 1 + H * W // 150
    rows = np.concatenate([[0], rs.randint(-1, H + 1, n)]).astype(np.int32)
    cols = np.concatenate([[0], rs.randint(-1, W + 1, n)]).astype(np.int32)
    ids = rs.randint(1, (n_ids or n + 1) + 1, n + 1).astype(np.int32)
    return rows, cols, ids


@functools.lru_cache(maxsize=None)
def case(kind, shape):
    """inputs of one case, and what the restatement makes of them (computed once, shared, never changed)"""
    H, W = shape
    rs = np.random.RandomState(KINDS.index(kind) * 1000 + H * 7 + W)
    cost = rs.rand(H, W).astype(np.float32)
    rows, cols, ids = random_seeds(rs, H, W)
    mask = None
    kw = dict(weight=0.5, pixel_size=1.0, connectivity=8, max_dist=None)
    if kind == "random4":
        kw["connectivity"] = 4
    elif kind == "constant":
        cost[:] = 0.25                                                       # ties everywhere
    elif kind in ("quant-w0", "quant-w05"):
        cost = (rs.randint(0, 3, (H, W)) / 2).astype(np.float32)
        kw["weight"] = 0.0 if kind == "quant-w0" else 0.5
    elif kind == "zero":
        cost[:] = 0
    elif kind == "pixel":
        kw["pixel_size"] = (0.5, 2.0)
        kw["weight"] = 1.75
    elif kind == "seams":                                                    # the four corners and both sides of every tile seam
        edge_r = sorted({0, H - 1} | {r for k in range(1, 4) for r in (k * T - 1, k * T) if r < H})
        edge_c = sorted({0, W - 1} | {c for k in range(1, 4) for c in (k * T - 1, k * T) if c < W})
        rows = np.array([r for r in edge_r for _ in edge_c], np.int32)
        cols = np.array([c for _ in edge_r for c in edge_c], np.int32)
        ids = (1 + rs.permutation(len(rows))).astype(np.int32)
    elif kind == "several":                                                  # three ids for all seeds; two seeds on (0, 0) and on the last pixel
        rows, cols, ids = random_seeds(rs, H, W, n_ids=3)
        rows = np.concatenate([rows, [0, H - 1, H - 1]]).astype(np.int32)
        cols = np.concatenate([cols, [0, W - 1, W - 1]]).astype(np.int32)
        ids = np.concatenate([ids, [ids[0] + 1, 9, 8]]).astype(np.int32)
    elif kind == "nan-inf" and H * W > 1:
        flat = cost.reshape(-1)
        flat[1 + rs.permutation(H * W - 1)[:max(2, H * W // 40)]] = np.nan
        flat[1 + rs.permutation(H * W - 1)[:max(1, H * W // 60)]] = np.inf
        flat[-1] = -np.inf
    elif kind == "pocket" and H * W > 1:                                     # a sealed box about the centre: its inside is unreachable
        mask = np.ones((H, W), np.uint8)
        r0, c0 = H // 2 - 2, W // 2 - 2
        inside = np.zeros((H, W), bool)
        for r in range(max(r0, 0), min(r0 + 5, H)):
            for c in range(max(c0, 0), min(c0 + 5, W)):
                if r in (r0, r0 + 4) or c in (c0, c0 + 4):
                    mask[r, c] = 0
                else:
                    inside[r, c] = True
        keep = np.array([not (0 <= r < H and 0 <= c < W and inside[r, c]) for r, c in zip(rows, cols)])
        rows, cols, ids = rows[keep], cols[keep], ids[keep]
        kw["_inside"] = inside
    elif kind == "mask" and H * W > 1:
        mask = (rs.rand(H, W) < 0.8).astype(np.uint8) * rs.randint(1, 256, (H, W)).astype(np.uint8)   # any non-zero byte is passable
        mask[0, 0] = 1
    elif kind == "max-dist":
        kw["max_dist"] = 6.5
    inside = kw.pop("_inside", None)
    want = C.allocate(cost, rows, cols, ids, mask=mask, **kw)
    for a in (cost, rows, cols, ids, mask) + want:
        if a is not None:
            a.setflags(write=False)
    return dict(cost=cost, rows=rows, cols=cols, ids=ids, mask=mask, kw=kw, want=want, inside=inside)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("kind", KINDS)
def test_allocation_is_the_restatements(kind, shape):
    from obia_amd import cost_allocation
    c = case(kind, shape)
    D, L = cost_allocation(c["cost"], c["rows"], c["cols"], c["ids"], mask=c["mask"], **c["kw"])
    wD, wL = c["want"]
    assert isinstance(D, np.ndarray) and isinstance(L, np.ndarray) and D.dtype == np.float64 and L.dtype == np.int32
    assert same_bits(D, wD), f"dist: {int((D.view(np.uint64) != wD.view(np.uint64)).sum())} of {D.size} differ"
    assert np.array_equal(L, wL), f"labels: {int((L != wL).sum())} of {L.size} differ"
    assert np.array_equal(L == 0, np.isinf(D))
    if c["inside"] is not None:
        assert c["inside"].any() and np.isinf(D[c["inside"]]).all() and (L[c["inside"]] == 0).all()
    if kind == "max-dist" and min(shape) > 1:
        assert np.isinf(D).any() and D[np.isfinite(D)].max() <= 6.5
    if kind == "nan-inf" and shape != (1, 1):
        assert np.isinf(D[~np.isfinite(c["cost"])]).all()


def test_tensors_in_tensors_out():
    from obia_amd import cost_allocation
    c = case("mask", SHAPES[4])
    dev = [torch.as_tensor(np.array(c[k])).cuda() for k in ("cost", "rows", "cols", "ids", "mask")]
    D, L = cost_allocation(dev[0], dev[1], dev[2], dev[3], mask=dev[4], **c["kw"])
    assert D.is_cuda and L.is_cuda and D.dtype == torch.float64 and L.dtype == torch.int32
    assert same_bits(D.cpu().numpy(), c["want"][0]) and np.array_equal(L.cpu().numpy(), c["want"][1])
    D, L = cost_allocation(dev[0], c["rows"], c["cols"], c["ids"], mask=c["mask"] != 0, **c["kw"])   # lists and a bool mask beside a tensor
    assert D.is_cuda and same_bits(D.cpu().numpy(), c["want"][0]) and np.array_equal(L.cpu().numpy(), c["want"][1])


def work_of_last_call():
    from obia_amd import _lib
    w = (ctypes.c_int64 * 4)()
    _lib.check(_lib.load().obia_crowns_last_work(_lib.default_context(0).handle, w))
    return list(w)


def test_a_spiral_wall_needs_many_rounds():
    """the only seed sits at the centre of (2T + 1)^2; the corridor re-enters tiles that had settled, so no tile is done in one round"""
    from obia_amd import cost_allocation
    n = 2 * T + 1
    m = C.spiral_wall(n)
    cost = np.random.RandomState(5).rand(n, n).astype(np.float32)
    for connectivity in (8, 4):
        D, L = cost_allocation(cost, [T], [T], [7], mask=m, connectivity=connectivity)
        wD, wL = C.allocate(cost, [T], [T], [7], mask=m, connectivity=connectivity)
        assert same_bits(D, wD) and np.array_equal(L, wL)
        assert (L[m != 0] == 7).all() and (L[m == 0] == 0).all()
        rounds_d, rounds_l, changed_d, changed_l = work_of_last_call()
        print(f"spiral, {connectivity}-connected: {rounds_d} distance rounds, {rounds_l} label rounds")
        assert rounds_d >= 3 and rounds_l >= 3                               # (about four a ring in practice; the schedule decides)
        assert rounds_d <= n * n + 1 and rounds_l <= n * n + 1
        assert changed_d >= rounds_d - 1 and changed_l >= rounds_l - 1       # every round but the last changed a tile


def test_refusals_on_the_device():
    from obia_amd import cost_allocation
    cost = np.random.RandomState(2).rand(T + 3, T + 5).astype(np.float32)
    bad = cost.copy()
    bad[T + 1, 3] = -1e-3
    with pytest.raises(ValueError, match="negative cost"):
        cost_allocation(bad, [0], [0], [1])
    mask = np.ones(cost.shape, np.uint8)
    mask[T + 1, 3] = 0                                                       # ... unless the mask hides it
    D, L = cost_allocation(bad, [0], [0], [1], mask=mask)
    wD, wL = C.allocate(bad, [0], [0], [1], mask=mask)
    assert same_bits(D, wD) and np.array_equal(L, wL)
    neg0 = cost.copy()
    neg0[2, 2] = -0.0                                                        # not negative
    assert same_bits(cost_allocation(neg0, [0], [0], [1])[0], C.allocate(neg0, [0], [0], [1])[0])
    nan = cost.copy()
    nan[4, 4] = np.nan
    for rows, cols in (([-1], [0]), ([0], [T + 5]), ([4], [4]), ([T + 3, 4], [0, 4])):
        with pytest.raises(ValueError, match="no seed"):
            cost_allocation(nan, rows, cols, [1] * len(rows))
    with pytest.raises(ValueError, match="no seed"):
        cost_allocation(cost, [0], [0], [1], mask=np.zeros(cost.shape, np.uint8))
    for ids in ([0], [-3], [2 ** 31 - 1]):
        with pytest.raises(ValueError, match="seed ids"):
            cost_allocation(cost, [0], [0], ids)
    assert cost_allocation(cost, [0], [0], [2 ** 31 - 2])[1].max() == 2 ** 31 - 2


# ---- buffers ---------------------------------------------------------------------------------------------------------------------
def dev_off(a, k):
    t = offset_view(torch.as_tensor(np.array(a)).cuda(), k)
    assert residue(t) == (k * t.element_size()) % 16
    return t


def judge(g, want, name):
    """the guarded output holds `want` bit for bit, nothing around it changed, nothing in it was left as it was"""
    got = g.host()
    bits = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    assert np.array_equal(got.view(bits), want.view(bits)), f"{name}: {int((got.view(bits) != want.view(bits)).sum())} differ"
    poison = np.frombuffer(bytes([g.poison]) * want.dtype.itemsize, bits)[0]
    assert g.findings(exempt=want.view(bits) == poison, name=name) == []


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("poison", POISONS, ids=[f"{p:02X}" for p in POISONS])
def test_buffers_off_the_boundary_and_guarded_outputs(k, poison):
    """float32 and int32 buffers 4, 8 and 12 bytes past a 16-byte boundary, dist 8 bytes, the mask 1 byte; two runs agree bit for bit"""
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.default_context(0)
    for kind, shape in (("mask", SHAPES[5]), ("pocket", SHAPES[4]), ("max-dist", SHAPES[1]), ("several", SHAPES[2]), ("random4", SHAPES[0])):
        c = case(kind, shape)
        H, W = shape
        kw = c["kw"]
        sy, sx = (kw["pixel_size"],) * 2 if np.ndim(kw["pixel_size"]) == 0 else kw["pixel_size"]
        cost, ids = dev_off(c["cost"], k), dev_off(c["ids"], k)
        rc = dev_off(np.stack([c["rows"], c["cols"]], 1), k)
        mask = dev_off(c["mask"], 1) if c["mask"] is not None else None
        assert residue(cost) == 4 * k and (mask is None or residue(mask) == 1)
        ins = [t for t in (cost, ids, rc, mask) if t is not None]
        snaps = [snapshot(t) for t in ins]
        outs = []
        for _ in range(2):
            gd = guarded((H, W), np.float64, poison, "cuda", 1)
            gl = guarded((H, W), np.int32, poison, "cuda", k)
            assert gd.ptr % 16 == 8 and gl.ptr % 16 == 4 * k
            rounds = (ctypes.c_int32 * 2)(-1, -1)
            torch.cuda.synchronize()
            rcode = lib.obia_crowns_allocate_dev(ctx.handle, cost.data_ptr(), mask.data_ptr() if mask is not None else None, H, W, rc.data_ptr(),
                                                 ids.data_ptr(), len(c["ids"]), kw["weight"], sx, sy, math.sqrt(sx * sx + sy * sy),
                                                 kw["connectivity"], -1.0 if kw["max_dist"] is None else kw["max_dist"], gd.ptr, gl.ptr, rounds)
            assert rcode == 0, (rcode, _lib.last_error())
            judge(gd, c["want"][0], f"dist {kind} {shape}")
            judge(gl, c["want"][1], f"labels {kind} {shape}")
            assert 1 <= rounds[0] <= H * W + 1 and 1 <= rounds[1] <= H * W + 1
            outs.append((gd.host(), gl.host()))
        assert same_bits(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
        assert all(unchanged(t, s) for t, s in zip(ins, snaps))
    # refused before anything is launched: nothing is written
    gd = guarded((H, W), np.float64, poison, "cuda", 1)
    gl = guarded((H, W), np.int32, poison, "cuda", k)
    good = dict(cost=cost.data_ptr(), H=H, W=W, rc=rc.data_ptr(), ids=ids.data_ptr(), n=len(c["ids"]), weight=0.5, lh=1.0, lv=1.0, ld=math.sqrt(2.0),
                conn=8, md=-1.0, dist=gd.ptr, labels=gl.ptr)
    for change in (dict(conn=6), dict(weight=-1.0), dict(weight=float("nan")), dict(lh=0.0), dict(ld=float("inf")), dict(md=float("nan")),
                   dict(H=0), dict(n=0), dict(cost=cost.data_ptr() + 2), dict(dist=gd.ptr + 4), dict(labels=gl.ptr + 1), dict(rc=None),
                   dict(ids=ids.data_ptr() + 3), dict(dist=None), dict(dist=gd.ptr + 1), dict(labels=cost.data_ptr()), dict(dist=cost.data_ptr())):
        a = dict(good, **change)
        rcode = lib.obia_crowns_allocate_dev(ctx.handle, a["cost"], None, a["H"], a["W"], a["rc"], a["ids"], a["n"], a["weight"], a["lh"], a["lv"],
                                             a["ld"], a["conn"], a["md"], a["dist"], a["labels"], None)
        assert rcode == _lib.E_INVALID, (change, rcode)
        # a null output, an output one byte on, an output where the cost raster starts: the refusal in full
        if change in (dict(dist=None), dict(dist=gd.ptr + 1), dict(labels=gl.ptr + 1), dict(labels=cost.data_ptr()), dict(dist=cost.data_ptr())):
            assert _lib.last_error() == "crowns: bad arguments (null, misaligned or overlapping buffers)", change
    assert gd.untouched() and gl.untouched()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
AFFINE = [0.5, 0.0, 0.0, -0.5, 1000.0, 5000.0]


@functools.lru_cache(maxsize=None)
def scene():
    """a canopy height model of Gaussian crowns on 96 x 128 at 0.5 m, and a point density that follows it"""
    rs = np.random.RandomState(17)
    H, W = 96, 128
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    chm = np.zeros((H, W))
    for cy in range(9, H, 16):
        for cx in range(9, W, 16):
            y, x, h, s = cy + rs.uniform(-3, 3), cx + rs.uniform(-3, 3), rs.uniform(6, 18), rs.uniform(2.5, 4.5)
            chm = np.maximum(chm, h * np.exp(-((yy - y) ** 2 + (xx - x) ** 2) / (2 * s * s)))
    chm = chm.astype(np.float32)
    return chm, (1.5 * chm).astype(np.float32), (chm > 1.0).astype(np.uint8)


def test_from_a_canopy_height_model_to_crowns(tmp_path, capsys):
    from obia_amd import grow_crowns, make_canonical_seeds, make_chm_seeds, make_density_seeds, polygonize, zonal_stats
    from obia_amd.consumers import invert_affine
    from obia_amd.cost import chm_gradient
    chm, density, canopy = scene()
    s_chm = make_chm_seeds(chm, affine_transformation=AFFINE)
    s_den = make_density_seeds(density, affine_transformation=AFFINE)
    cost = chm_gradient(chm).astype(np.float32)
    gpkg = tmp_path / "canonical.gpkg"
    canon = make_canonical_seeds(s_chm, s_den, cost, out_path=str(gpkg), cost_affine=AFFINE, debug_dist=False)
    clusters = np.unique(canon["cluster"])
    N = len(clusters)
    assert 20 <= N < len(canon["x"])                                         # CHM and density peaks of one crown were merged
    labels, dist = grow_crowns(cost, canon, mask=canopy, cost_affine=AFFINE, return_distance=True)
    assert isinstance(labels, np.ndarray) and labels.dtype == np.int32 and labels.shape == chm.shape
    assert np.unique(labels).tolist() == list(range(N + 1))                  # 0 .. N, every id present
    assert (labels[canopy == 0] == 0).all() and (labels[canopy != 0] > 0).all()
    # the restatement on the same seeds: the pixel that contains (x, y), ids 1 .. N in ascending order of the cluster
    ia, _, _, ie, c0, r0 = invert_affine(AFFINE)
    cols, rows = np.floor(ia * canon["x"] + c0).astype(np.int64), np.floor(ie * canon["y"] + r0).astype(np.int64)
    assert np.array_equal(rows[:len(s_chm["row"])], s_chm["row"]) and np.array_equal(cols[:len(s_chm["col"])], s_chm["col"])
    ids = 1 + np.searchsorted(clusters, canon["cluster"])
    wD, wL = C.allocate(cost, rows, cols, ids, mask=canopy, pixel_size=(0.5, 0.5))
    assert same_bits(dist, wD) and np.array_equal(labels, wL)
    assert np.array_equal(grow_crowns(cost, str(gpkg), mask=canopy, cost_affine=AFFINE), labels)      # the layer it wrote
    # one crown per seed, a bound, tensors
    by_id = grow_crowns(cost, canon, mask=canopy, cost_affine=AFFINE, by="id", connectivity=4, max_dist=3.0)
    w4 = C.allocate(cost, rows, cols, 1 + np.argsort(np.argsort(canon["id"])), mask=canopy, pixel_size=(0.5, 0.5), connectivity=4, max_dist=3.0)
    assert np.array_equal(by_id, w4[1]) and N < by_id.max() <= len(canon["x"]) and (by_id[canopy != 0] == 0).any()
    t = grow_crowns(torch.as_tensor(cost).cuda(), canon, mask=torch.as_tensor(canopy).cuda(), cost_affine=AFFINE)
    assert t.is_cuda and t.dtype == torch.int32 and np.array_equal(t.cpu().numpy(), labels)
    # the consumers take the raster as it is
    st = zonal_stats(chm[:, :, None], labels, n_labels=N)
    assert st["count"].shape == (N,) and (st["count"] > 0).all() and int(st["count"].sum()) == int((labels > 0).sum())
    assert len(polygonize(labels, AFFINE, start_label=1)) == N
