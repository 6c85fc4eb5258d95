"""Crowns from seeds, host side: the restatement (tests/crowns_restatement.py) against SciPy's Dijkstra, bit for bit, and against answers
worked out by hand; the argument checks of obia_amd.crowns that fire before the device is touched."""
import math

import numpy as np
import pytest

from tests import crowns_restatement as C

SQRT2 = math.sqrt(2.0)


# ---- the distance is Dijkstra's, bit for bit -------------------------------------------------------------------------------------
def probe_case(H, W, kind, seed):
    rs = np.random.RandomState(seed)
    cost = rs.rand(H, W).astype(np.float32)
    if kind == "const":
        cost[:] = 0.25
    if kind == "quant":
        cost = (rs.randint(0, 3, (H, W)) / 2).astype(np.float32)
    mask = np.ones((H, W), np.uint8)
    mask[5:30, 20] = 0
    mask[10, 5:20] = 0
    seeds = [(0, 0, 3), (H - 1, W - 1, 1), (H // 2, W // 2, 2), (H // 2, W // 2 + 1, 2), (7, 21, 5)]
    return cost, mask, seeds


def scipy_distance(cost, mask, seeds, weight, pixel_size, connectivity):
    sp = pytest.importorskip("scipy.sparse")
    from scipy.sparse.csgraph import dijkstra
    H, W = cost.shape
    ok = C.passable(cost, mask)
    c = cost.astype(np.float64)
    idx = np.arange(H * W).reshape(H, W)
    rows, cols, vals = [], [], []
    for dy, dx, length in C.steps(pixel_size, connectivity):
        for r in range(max(-dy, 0), H + min(-dy, 0)):
            for q in range(max(-dx, 0), W + min(-dx, 0)):
                if ok[r, q] and ok[r + dy, q + dx]:
                    rows.append(idx[r, q])
                    cols.append(idx[r + dy, q + dx])
                    vals.append(C.edge_weight(length, weight, float(c[r, q]), float(c[r + dy, q + dx])))
    g = sp.csr_matrix((vals, (rows, cols)), shape=(H * W, H * W))
    src = [idx[r, q] for r, q, _ in seeds if ok[r, q]]
    return dijkstra(g, directed=True, indices=src, min_only=True).reshape(H, W)


@pytest.mark.parametrize("H,W,connectivity,kind", [(37, 53, 8, "rand"), (33, 65, 4, "rand"), (40, 40, 8, "const"), (40, 40, 8, "quant")])
def test_the_restatements_distance_is_scipys_dijkstra_bit_for_bit(H, W, connectivity, kind):
    cost, mask, seeds = probe_case(H, W, kind, 3)
    r, q, i = zip(*seeds)
    for weight, px in ((0.5, 1.0), (0.0, 1.0), (1.75, (0.5, 2.0))):
        D, L = C.allocate(cost, r, q, i, mask=mask, weight=weight, pixel_size=px, connectivity=connectivity)
        want = scipy_distance(cost, mask, seeds, weight, px, connectivity)
        assert D.dtype == np.float64 and np.array_equal(D, want)            # +inf included: barriers and what no seed reaches
        assert np.isinf(D[mask == 0]).all() and (L[mask == 0] == 0).all() and (L[mask != 0] > 0).all()
        assert sorted(np.unique(L).tolist()) == [0, 1, 2, 3, 5]
        assert [L[a, b] for a, b, _ in seeds] == [k if mask[a, b] else 0 for a, b, k in seeds]   # (20, 20) of 40 x 40 lies on the wall


# ---- by hand ---------------------------------------------------------------------------------------------------------------------
def test_a_row_of_seven_with_seeds_at_its_ends():
    for weight, c in ((0.5, 0.25), (0.0, 0.7), (2.0, 1.0)):
        cost = np.full((1, 7), c, np.float32)
        D, L = C.allocate(cost, [0, 0], [0, 6], [2, 1], weight=weight)
        step = 1.0 * (1.0 + weight * (0.5 * (float(np.float32(c)) + float(np.float32(c)))))
        want = [0.0]
        for _ in range(3):
            want.append(want[-1] + step)                                     # k steps are k additions: k * step only up to rounding
        assert D[0].tolist() == want + want[2::-1]
        assert np.allclose(D[0, :4], np.arange(4) * (1 + weight * c), rtol=1e-14)
        assert L[0].tolist() == [2, 2, 2, 1, 1, 1, 1]                        # the middle pixel is equally far: the lower id


def test_two_seeds_on_one_pixel_and_one_id_on_two_pixels():
    cost = np.zeros((3, 5), np.float32)
    D, L = C.allocate(cost, [1, 1, 1], [2, 2, 0], [7, 4, 9])
    assert (L[:, 1:] == 4).all() and (L[:, 0] == 9).all() and D[1, 2] == 0 and D[1, 0] == 0
    D, L = C.allocate(cost, [0, 2], [0, 4], [3, 3])
    assert (L == 3).all() and D[0, 0] == 0 and D[2, 4] == 0 and D[1, 2] == 1 + SQRT2


def test_a_wall_with_one_gap():
    cost = np.zeros((5, 7), np.float32)
    mask = np.ones((5, 7), np.uint8)
    mask[:, 3] = 0
    mask[4, 3] = 1
    D, L = C.allocate(cost, [0], [0], [1], mask=mask, weight=0.0, connectivity=4)
    assert D[0, 4] == 4 + 4 + 4 and D[4, 3] == 7 and D[4, 4] == 8 and np.isinf(D[:4, 3]).all()
    assert (L[mask != 0] == 1).all() and (L[:4, 3] == 0).all()
    D8, _ = C.allocate(cost, [0], [0], [1], mask=mask, weight=0.0, connectivity=8)
    assert math.isclose(D8[4, 3], 1 + 3 * SQRT2, rel_tol=1e-14)              # one step down, three diagonal ones
    assert math.isclose(D8[0, 4], 4 + 4 * SQRT2, rel_tol=1e-14)              # ... and up again: one diagonal step, three straight ones
    sealed = mask.copy()
    sealed[4, 3] = 0
    D, L = C.allocate(cost, [0], [0], [1], mask=sealed)
    assert np.isinf(D[:, 3:]).all() and (L[:, 3:] == 0).all() and np.isfinite(D[:, :3]).all()


def test_weight_zero_is_the_chamfer_distance_with_steps_1_and_sqrt2():
    cost = np.random.RandomState(1).rand(9, 11).astype(np.float32)
    D, _ = C.allocate(cost, [4], [5], [1], weight=0.0)
    yy, xx = np.mgrid[0:9, 0:11]
    dy, dx = abs(yy - 4), abs(xx - 5)
    assert np.allclose(D, np.minimum(dy, dx) * SQRT2 + abs(dy - dx), rtol=1e-14, atol=0)
    assert D[4, 9] == 4.0 and D[0, 5] == 4.0 and D[3, 4] == SQRT2
    D4, _ = C.allocate(cost, [4], [5], [1], weight=0.0, connectivity=4, pixel_size=(0.5, 2.0))
    assert np.array_equal(D4, dy * 0.5 + dx * 2.0)


def test_max_dist_cuts_at_the_first_value_above_it():
    cost = np.zeros((1, 9), np.float32)
    for max_dist, kept in ((3.0, 4), (2.999, 3), (0.0, 1), (100.0, 9)):
        D, L = C.allocate(cost, [0], [0], [5], weight=0.0, max_dist=max_dist)
        assert D[0, :kept].tolist() == list(range(kept)) and np.isinf(D[0, kept:]).all()
        assert (L[0, :kept] == 5).all() and (L[0, kept:] == 0).all()


def test_barriers_negative_costs_and_seeds_that_do_not_count():
    cost = np.zeros((4, 4), np.float32)
    cost[1, 1], cost[2, 2] = np.nan, np.inf
    D, L = C.allocate(cost, [1, 0, -1, 9], [1, 0, 0, 0], [1, 2, 3, 4])
    assert np.isinf(D[1, 1]) and np.isinf(D[2, 2]) and L[1, 1] == 0 and L[2, 2] == 0 and (L[np.isfinite(D)] == 2).all()
    with pytest.raises(ValueError, match="no seed"):
        C.allocate(cost, [1, 4], [1, 0], [1, 2])
    cost[0, 3] = -1.0
    with pytest.raises(ValueError, match="negative cost"):
        C.allocate(cost, [0], [0], [1])
    mask = np.ones((4, 4), np.uint8)
    mask[0, 3] = 0                                                           # a negative cost the mask hides is not looked at
    assert C.allocate(cost, [0], [0], [1], mask=mask)[1][0, 3] == 0


def test_the_spiral_is_one_corridor():
    T = 32
    m = C.spiral_wall(2 * T + 1)
    D, L = C.allocate(np.zeros(m.shape, np.float32), [T], [T], [1], mask=m, weight=0.0)
    n = int(m.sum())
    assert np.isfinite(D[m != 0]).all() and (L[m != 0] == 1).all()
    assert D.max(where=np.isfinite(D), initial=0) > n - 2 * (2 * T + 1)      # no shortcut: about one step per corridor pixel
    assert n > 2000


# ---- argument checks: no device work ---------------------------------------------------------------------------------------------
def test_refusals_before_the_device_is_touched():
    torch = pytest.importorskip("torch")
    from obia_amd import crowns as cr
    cost = np.zeros((6, 7), np.float32)
    seeds = ([1], [2], [1])
    for kw, match in ((dict(weight=-0.1), "weight"), (dict(weight=float("nan")), "weight"), (dict(weight=float("inf")), "weight"),
                      (dict(weight="1"), "weight"), (dict(connectivity=6), "connectivity must be 4 or 8"),
                      (dict(connectivity=None), "connectivity"), (dict(max_dist=-1.0), "max_dist"), (dict(max_dist=float("nan")), "max_dist"),
                      (dict(pixel_size=0.0), "pixel_size"), (dict(pixel_size=(1.0, -2.0)), "pixel_size"), (dict(pixel_size=(1, 2, 3)), "pixel_size"),
                      (dict(pixel_size=float("inf")), "pixel_size"), (dict(mask=np.ones((6, 8), np.uint8)), "the mask is")):
        with pytest.raises(ValueError, match=match):
            cr.cost_allocation(cost, *seeds, **kw)
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        cr.cost_allocation(np.zeros((6, 7, 2), np.float32), *seeds)
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        cr.cost_allocation(np.zeros((0, 7), np.float32), *seeds)
    with pytest.raises(ValueError, match="one length"):
        cr.cost_allocation(cost, [1, 2], [2], [1])
    with pytest.raises(ValueError, match="one length"):
        cr.cost_allocation(cost, [[1]], [[2]], [[1]])
    with pytest.raises(ValueError, match="no seeds"):
        cr.cost_allocation(cost, [], [], [])
    for args in ((torch.zeros(6, 7), *seeds), (cost, torch.tensor([1]), [2], [1]), (cost, [1], [2], torch.tensor([1], dtype=torch.int32))):
        with pytest.raises(ValueError, match="must live on the GPU"):
            cr.cost_allocation(*args)
    with pytest.raises(ValueError, match="must live on the GPU"):
        cr.cost_allocation(cost, *seeds, mask=torch.ones(6, 7, dtype=torch.uint8))


def test_grow_crowns_refusals_before_the_device_is_touched():
    torch = pytest.importorskip("torch")
    from obia_amd import crowns as cr
    cost = np.zeros((6, 7), np.float32)
    table = {"id": np.arange(2), "cluster": np.array([0, 0], np.int32), "x": np.array([1.5, 2.5]), "y": np.array([1.5, 2.5])}
    for affine in ([0.5, 0.1, 0, -0.5, 0, 0], [0.5, 0, -0.2, -0.5, 0, 0]):
        with pytest.raises(ValueError, match="unrotated"):
            cr.grow_crowns(cost, table, cost_affine=affine)
    with pytest.raises(ValueError, match="singular"):
        cr.grow_crowns(cost, table, cost_affine=[0.0, 0, 0, -0.5, 0, 0])
    with pytest.raises(ValueError, match='"cluster" or "id"'):
        cr.grow_crowns(cost, table, by="origin")
    no_cluster = {k: v for k, v in table.items() if k != "cluster"}
    with pytest.raises(ValueError, match="x, y and cluster"):
        cr.grow_crowns(cost, no_cluster)
    with pytest.raises(ValueError, match="x, y and id"):
        cr.grow_crowns(cost, {"x": table["x"], "y": table["y"], "cluster": table["cluster"]}, by="id")
    with pytest.raises(ValueError, match="x, y and cluster"):
        cr.grow_crowns(cost, [1, 2, 3])
    with pytest.raises(ValueError, match=r"\(H, W\)"):
        cr.grow_crowns(np.zeros((6, 7, 1), np.float32), table)
    for kw, match in ((dict(weight=-1), "weight"), (dict(connectivity=5), "connectivity"), (dict(max_dist=-2), "max_dist")):
        with pytest.raises(ValueError, match=match):
            cr.grow_crowns(cost, table, **kw)
    with pytest.raises(ValueError, match="must live on the GPU"):
        cr.grow_crowns(torch.zeros(6, 7), table)
    with pytest.raises(ValueError, match="must live on the GPU"):
        cr.grow_crowns(cost, dict(table, x=torch.tensor([1.5, 2.5], dtype=torch.float64)))


def test_the_package_exports_the_module():
    pytest.importorskip("torch")
    import obia_amd
    assert obia_amd.cost_allocation is obia_amd.crowns.cost_allocation and obia_amd.grow_crowns is obia_amd.crowns.grow_crowns
