"""The spatial-only pre-pass sweeps of maskSLIC exist twice: `slic_spatial_kernel` (slic_spatial.hip: winners decided by runs on
pixel rows, the reference's float expression only at segment ends, around predicted crossings and wherever the proven margin does
not hold) and `slic_prepass_kernel` (every pixel visits its candidates; OBIA_PREPASS_VISITS=1).  The pre-pass produces centroids
only, so the labels before connectivity (a function of those centroids) and the final labels must be IDENTICAL with either kernel
-- on inputs that sit on the hard cases of the run walk: exact ties (symmetric grids on an all-ones mask, bisectors on pixel centres
and between them), cells that end at window edges (sparse masks), valid pixels no window reaches (the batch repeats), steps from 2
to more than 40 pixels, image edges that are no multiple of 64 or 16, caller-supplied seeds that share a coordinate or lie one ulp
apart, tiles with more candidates than LDS slots, anisotropic spacing.  And a seeded random set against the oracle, bit for bit.
The pre-pass only runs with a mask: every case passes one."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def image(H, W, C, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([300 * np.sin(xx / (5 + 2 * c)) * np.cos(yy / (6 + c)) + 800 + 40 * c + rs.normal(0, 25, (H, W))
                     for c in range(C)], -1).astype(np.float32)


def run_both(img, mask, ctx=None, **kw):
    """(pre, final) labels with the run kernel and with the visit kernel"""
    from obia_amd.segmentation import slic
    dev = torch.as_tensor(img).cuda()
    old = os.environ.pop("OBIA_PREPASS_VISITS", None)
    try:
        new = [slic(dev, mask=mask, _normalize_bands=True, _stage=s, ctx=ctx, **kw).cpu().numpy() for s in ("pre", "full")]
        os.environ["OBIA_PREPASS_VISITS"] = "1"
        ref = [slic(dev, mask=mask, _normalize_bands=True, _stage=s, **kw).cpu().numpy() for s in ("pre", "full")]
    finally:
        os.environ.pop("OBIA_PREPASS_VISITS", None)
        if old is not None:
            os.environ["OBIA_PREPASS_VISITS"] = old
    return new, ref


def assert_same(new, ref, what):
    n_pre, n_fin = int((new[0] != ref[0]).sum()), int((new[1] != ref[1]).sum())
    print(f"{what}: {n_pre} pixels differ before connectivity, {n_fin} after")
    assert n_pre == 0 and n_fin == 0, f"{what}: {n_pre} / {n_fin} pixels differ before / after connectivity"


# all-ones mask: the seed grid is symmetric, every cell boundary of the first sweeps is an exact tie.  Sizes and segment counts so that
# the bisectors fall on pixel centres (odd step) and between pixels (even step), steps from 2 to 46, edges off every multiple of 16.
@pytest.mark.parametrize("H,W,n_seg", [(96, 96, 36), (100, 100, 25), (128, 160, 80), (130, 75, 39), (64, 64, 1024), (72, 88, 1584),
                                       (190, 257, 23), (257, 321, 40), (129, 130, 700), (200, 200, 100), (65, 333, 12), (48, 1000, 300)])
def test_all_ones_mask_symmetric_grid(H, W, n_seg):
    new, ref = run_both(image(H, W, 3, H + W), np.ones((H, W), np.uint8), n_segments=n_seg, compactness=10.0, convert2lab=False)
    assert_same(new, ref, f"all-ones {H}x{W} n_segments {n_seg}")


def sparse_mask(kind, H, W, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "rects":
        m = np.zeros((H, W), bool)
        for _ in range(5):
            y0, x0 = rs.randint(0, H - 8), rs.randint(0, W - 8)
            m[y0:y0 + rs.randint(4, H // 3), x0:x0 + rs.randint(4, W // 3)] = True
        return m
    if kind == "stripes":
        return ((xx + 2 * yy) % 17) < 5
    if kind == "disc":
        return ((yy - H / 2) ** 2 + (xx - W / 2) ** 2 < (0.45 * max(H, W)) ** 2) & ~((abs(yy - H / 3) < H / 10) & (abs(xx - W / 2) < W / 8))
    return rs.rand(H, W) < 0.08   # "dust"


@pytest.mark.parametrize("kind", ["rects", "stripes", "disc", "dust"])
@pytest.mark.parametrize("H,W,n_seg", [(190, 257, 60), (257, 130, 400), (300, 333, 30)])
def test_sparse_masks_cells_end_at_window_edges(kind, H, W, n_seg):
    mask = sparse_mask(kind, H, W, H)
    new, ref = run_both(image(H, W, 4, 7), mask, n_segments=n_seg, compactness=10.0, convert2lab=False)
    assert_same(new, ref, f"{kind} {H}x{W} n_segments {n_seg}")


def test_valid_region_no_window_reaches_repeats_the_batch():
    from obia_amd import _lib
    H, W = 256, 300
    mask = np.zeros((H, W), bool)
    mask[:, :70] = True                       # a block that gets the seeds ...
    mask[10:250:40, 150:152] = True           # ... and islands far from it
    mask[30:250:40, 260:263] = True
    ctx = _lib.Context(0)
    new, ref = run_both(image(H, W, 4, 12), mask, ctx=ctx, n_segments=60, compactness=10.0, convert2lab=False)
    assert ctx.timing()["batch_repeats"] > 0, "the case is meant to take the orphan repeat (obia_last_timing 12)"
    assert_same(new, ref, "orphan islands")


@pytest.mark.parametrize("n_seg", [4, 16, 90, 900, 9000])   # steps of ~100, 50, 21, 6.7 and 2 pixels on 200 x 200
def test_steps_from_two_to_a_hundred_pixels(n_seg):
    H, W = 200, 203
    mask = np.ones((H, W), np.uint8)
    mask[90:110, 40:160] = 0
    new, ref = run_both(image(H, W, 2, n_seg), mask, n_segments=n_seg, compactness=10.0, convert2lab=False)
    assert_same(new, ref, f"n_segments {n_seg}")


def seeded(seeds_yx, step, H=150, W=170):
    from obia_amd.segmentation import slic
    img, mask = image(H, W, 3, 5), np.ones((H, W), np.uint8)
    dev = torch.as_tensor(img).cuda()
    out = {}
    for name, env in (("runs", None), ("visits", "1")):
        os.environ.pop("OBIA_PREPASS_VISITS", None)
        if env:
            os.environ["OBIA_PREPASS_VISITS"] = env
        try:
            out[name] = [slic(dev, mask=mask, seeds=(np.asarray(seeds_yx, np.float64), (1.0, step, step)), compactness=10.0, convert2lab=False,
                              _normalize_bands=True, _stage=s).cpu().numpy() for s in ("pre", "full")]
        finally:
            os.environ.pop("OBIA_PREPASS_VISITS", None)
    return out["runs"], out["visits"]


def test_seeds_sharing_a_coordinate_and_one_ulp_apart():
    g = np.mgrid[12:150:25, 10:170:25].reshape(2, -1).T.astype(np.float64)   # a regular lattice: rows share cy, columns share cx
    new, ref = seeded(g, 25.0)
    assert_same(new, ref, "lattice seeds")
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(1e9)))
    close = np.array([[40.25, 50.5], [40.25, up(50.5)], [up(40.25), 50.5], [100.0, 60.0], [100.0, 120.0], [up(100.0), 90.0],
                      [40.25, 50.5], [75.5, 85.5], [75.5, 85.5], [20.0, 150.0], [130.0, up(20.0)], [130.0, 20.0]])
    new, ref = seeded(close, 30.0)
    assert_same(new, ref, "seeds one ulp apart / identical")


def test_tile_with_more_candidates_than_slots():
    H, W = 140, 150
    mask = np.ones((H, W), np.uint8)
    mask[:, 70:74] = 0
    new, ref = run_both(image(H, W, 3, 3), mask, n_segments=H * W // 4, compactness=10.0, convert2lab=False)   # step 2: > 1000 candidates per tile
    assert_same(new, ref, "dense centroids")


@pytest.mark.parametrize("H,W,n_seg", [(100, 100, 127), (300, 340, 1300), (132, 132, 220)])
def test_tiles_with_65_to_96_candidates_use_footprint_lists(H, W, n_seg):
    """steps of 8 - 9 pixels: edge tiles hold more than 64 and at most 96 candidates (a list with per-footprint lists), inner tiles more"""
    new, ref = run_both(image(H, W, 8, 2), np.ones((H, W), np.uint8), n_segments=n_seg, compactness=10.0, convert2lab=False)
    assert_same(new, ref, f"step 8-9, {H}x{W}")


def test_anisotropic_spacing_takes_the_direct_path():
    H, W = 120, 131
    new, ref = run_both(image(H, W, 3, 9), np.ones((H, W), np.uint8), n_segments=50, compactness=10.0, convert2lab=False, spacing=(1.0, 2.0, 1.0))
    assert_same(new, ref, "spacing (2, 1)")


def random_case(seed):
    rs = np.random.RandomState(5000 + seed)
    H = int(rs.choice([33, 64, 65, 100, 129, 190, 257, 300]))
    W = int(rs.choice([31, 64, 80, 127, 130, 200, 321, 400]))
    C = int(rs.choice([1, 3, 4, 8, 9]))
    n_seg = int(max(2, H * W / rs.choice([9, 30, 80, 200, 500, 2000])))
    kind = ["ones", "rects", "stripes", "disc", "dust"][rs.randint(0, 5)]
    mask = np.ones((H, W), bool) if kind == "ones" else sparse_mask(kind, H, W, seed)
    if mask.sum() < 4:
        mask = np.ones((H, W), bool)
    kw = dict(n_segments=n_seg, compactness=float(rs.choice([5.0, 10.0, 20.0])), max_num_iter=int(rs.choice([2, 3, 10])),
              start_label=int(rs.choice([0, 1])), convert2lab=False)
    return image(H, W, C, seed), mask, kw


@pytest.mark.parametrize("seed", range(48))
def test_random_masked_case_vs_oracle_and_visit_kernel(oracle, seed):
    """compactness >= 5: the library is bit-exact against the oracle there (tests/test_gpu_random_parity.py), before and after connectivity"""
    img, mask, kw = random_case(seed)
    okw = dict(n_segments=kw["n_segments"], compactness=kw["compactness"], max_iter=kw["max_num_iter"], start_label=kw["start_label"],
               convert2lab=False, mask=mask.astype(np.uint8))
    try:
        o_fin, o_pre, _ = oracle.slic(oracle.normalize(img), return_all=True, **okw)
    except ValueError:
        from obia_amd.segmentation import slic
        with pytest.raises(ValueError):
            slic(img, mask=mask, _normalize_bands=True, **kw)
        return
    new, ref = run_both(img, mask, **kw)
    assert_same(new, ref, f"seed {seed} runs vs visits")
    assert_same(new, (o_pre, o_fin), f"seed {seed} runs vs oracle ({img.shape}, {kw})")
