"""Quickshift stage by stage against the oracle's float64 restatement (tests/qs_stages.py states the two tiers and the bars):
staged image, densities, parents before the max_dist cut, dist_parent, roots and labels.  Labels must be IDENTICAL wherever
the oracle finds no near-tie that counts in the tier; the generated inputs below are asserted to carry none, except the
deliberate tie cases, which name the flags they provoke."""
import os

import numpy as np
import pytest

from tests import qs_stages as qs

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DENS, DIST, CUT = 1, 2, 4


def textured(H, W, C, seed, lo=0.2, hi=0.8):
    """Smooth bands plus noise, kept inside (0, 1) so no clipping flattens a region (flat regions are where densities tie)."""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.stack([0.5 + 0.5 * np.sin(xx / (5.0 + 2 * c) + c) * np.cos(yy / (7.0 + c)) for c in range(C)], -1)
    img = lo + (hi - lo) * base + 0.03 * rs.normal(size=(H, W, C))
    return np.clip(img, 0.0, 1.0).astype(np.float32)


def make_image(kind, H, W, C, seed):
    if kind == "textured":
        return textured(H, W, C, seed)
    if kind == "constant":
        return np.full((H, W, C), 0.4, np.float32)
    if kind == "levels":          # three distinct values in blocks: many exact distance ties
        yy, xx = np.mgrid[0:H, 0:W]
        v = np.array([0.1, 0.5, 0.9], np.float32)[(yy // 7 + xx // 5) % 3]
        return np.repeat(v[..., None], C, -1).astype(np.float32)
    if kind == "ramp":            # a smooth ramp: long parent chains for the pointer jumping
        xx = np.mgrid[0:H, 0:W][1].astype(np.float64)
        return np.repeat((0.1 + 0.8 * xx / max(W - 1, 1))[..., None], C, -1).astype(np.float32)
    raise ValueError(kind)


def run_case(oracle, img, ks, md, ratio=1.0, sigma=0.0, lab=False, normalize=False, seed=0, expect=0, name="", image=None):
    tier = "B" if (lab or sigma > 0) else "A"
    g = qs.run_gpu(img if image is None else image, ratio=ratio, kernel_size=ks, max_dist=md, sigma=sigma, convert2lab=lab,
                   random_seed=seed, _normalize_bands=normalize)
    ref_img = qs.oracle_image(oracle, img, ratio, sigma, lab, normalize)
    assert np.array_equal(g["noise"], np.random.RandomState(seed).normal(scale=0.00001, size=img.shape[:2]))
    o = oracle.quickshift_stages(ref_img, g["noise"], ks, md, tau=qs.TAU)
    qs.check(g, o, md, tier, expect_flags=expect, staged_ref=ref_img, name=name)
    return g, o


# name: (H, W, C, kernel_size, max_dist, ratio, sigma, lab, kind, expected counting flags)
CASES = {
    # LDS-staged kernel: 1 / 3 / 4 bands, kernel_size <= 5
    "row_1x300": (1, 300, 3, 2.0, 6.0, 1.0, 0, False, "textured", 0),
    "col_257x1": (257, 1, 1, 3.0, 10.0, 1.0, 0, False, "textured", 0),
    "tiny_2x2": (2, 2, 4, 1.0, 10.0, 1.0, 0, False, "textured", 0),
    "below_window_9x13": (9, 13, 3, 5.0, 10.0, 1.0, 0, False, "textured", 0),
    "tile_31x33_ks1.5": (31, 33, 1, 1.5, 8.0, 1.0, 0, False, "textured", 0),
    "tile_32x48_ks2.5": (32, 48, 4, 2.5, 8.0, 1.0, 0, False, "textured", 0),
    "tile_49x47_ks5": (49, 47, 3, 5.0, 10.0, 1.0, 0, False, "textured", 0),          # kw = 15, the widest staged window
    "tile_17x65_ks4.9": (17, 65, 1, 4.9, 10.0, 1.0, 0, False, "textured", 0),
    "ragged_61x77_ks3.3": (61, 77, 3, 3.3, 10.0, 1.0, 0, False, "textured", 0),
    "ratio_0.37": (40, 50, 3, 2.0, 6.0, 0.37, 0, False, "textured", 0),
    "ratio_2.5": (33, 35, 4, 1.7, 9.0, 2.5, 0, False, "textured", 0),
    # global-memory kernel: other band counts or a window wider than the staged one
    "global_c2": (33, 17, 2, 2.0, 8.0, 1.0, 0, False, "textured", 0),
    "global_c5": (47, 50, 5, 1.7, 8.0, 1.0, 0, False, "textured", 0),
    "global_c8": (16, 65, 8, 1.0, 6.0, 1.0, 0, False, "textured", 0),
    "global_c16": (20, 20, 16, 1.2, 6.0, 1.0, 0, False, "textured", 0),
    "global_ks5.01": (40, 41, 3, 5.01, 10.0, 1.0, 0, False, "textured", 0),           # kw = 16
    "global_ks7_c1": (45, 50, 1, 7.0, 12.0, 1.0, 0, False, "textured", 0),
    "global_c4_ks6_below_window": (11, 30, 4, 6.0, 12.0, 1.0, 0, False, "textured", 0),
    # exact ties, broken alike on both sides: purely spatial distances (first in scan order wins), few distinct values
    "constant": (30, 34, 3, 2.0, 10.0, 1.0, 0, False, "constant", 0),
    "levels_c1": (35, 40, 1, 2.0, 10.0, 1.0, 0, False, "levels", 0),
    "levels_c5_global": (24, 30, 5, 1.5, 10.0, 1.0, 0, False, "levels", 0),
    # max_dist edges: exactly the distance of a link (kept: the cut is `>`), everything cut, nothing cut
    "constant_md_1": (30, 34, 3, 2.0, 1.0, 1.0, 0, False, "constant", 0),
    "md_0": (29, 31, 3, 2.0, 0.0, 1.0, 0, False, "textured", 0),
    "md_1e9": (29, 31, 4, 2.0, 1e9, 1.0, 0, False, "textured", 0),
    "ramp_chains": (20, 200, 1, 1.0, 1e9, 1.0, 0, False, "ramp", 0),
    # Tier B: Lab, smoothing, both, a sigma wider than the raster (repeated reflections)
    "lab": (37, 45, 3, 2.0, 8.0, 1.0, 0, True, "textured", 0),
    "lab_global_ks6": (30, 33, 3, 6.0, 12.0, 1.0, 0, True, "textured", 0),
    "sigma_c4": (36, 40, 4, 3.0, 8.0, 0.5, 1.3, False, "textured", 0),
    "lab_sigma": (33, 47, 3, 2.0, 10.0, 0.7, 0.8, True, "textured", 0),
    "sigma_wider_than_raster": (5, 7, 1, 1.0, 6.0, 1.0, 9.0, False, "textured", 0),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_quickshift_stages_fixed(oracle, name):
    H, W, C, ks, md, ratio, sigma, lab, kind, expect = CASES[name]
    img = make_image(kind, H, W, C, seed=len(name))
    g, o = run_case(oracle, img, ks, md, ratio, sigma, lab, seed=7, expect=expect, name=name)
    if kind == "constant":
        assert (o["flags"] & DIST).any()                  # the distance ties this case is about are really there
        assert np.array_equal(g["parent"], o["parent"])   # Tier A: equal everywhere
    if name == "constant_md_1":
        assert (o["flags"] & CUT).any() and (o["dist_parent"] == 1.0).any()
        assert np.array_equal(g["labels"], o["labels"])   # dist_parent is exactly 1.0 on both sides: the link is kept
    if name == "md_0":
        assert g["n_labels"] == H * W
    if name == "md_1e9":
        assert np.array_equal(qs.cut(g["parent"], g["dist_parent"], md), g["parent"])
    if name == "ramp_chains":
        depth = 0
        p = g["parent"].reshape(-1).astype(np.int64)
        cur = np.arange(p.size)
        while not np.array_equal(p[cur], cur):
            cur, depth = p[cur], depth + 1
        assert depth >= 16, f"longest chain {depth}: the case no longer exercises pointer jumping"


def test_quickshift_stages_normalised_bands(oracle):
    """create_segments' path: every band normalised (float32) on the device before the float64 stages."""
    rs = np.random.RandomState(4)
    raw = (textured(43, 52, 4, 9) * 3000.0 + rs.uniform(0, 5, (43, 52, 4)) + 200.0).astype(np.float32)
    run_case(oracle, raw, 2.0, 8.0, ratio=0.9, normalize=True, seed=3, name="normalised")


def test_quickshift_stages_host_vs_device_input(oracle):
    """NumPy in and CUDA tensor in take the same stages; quickshift() itself returns the hook's labels on both."""
    from obia_amd.segmentation import quickshift
    img = textured(45, 38, 3, 5)
    g, _ = run_case(oracle, img, 2.0, 8.0, seed=11, name="host")
    gd, _ = run_case(oracle, img, 2.0, 8.0, seed=11, name="device", image=torch.as_tensor(img).cuda())
    for k in ("image", "noise", "dens", "parent", "dist_parent", "roots", "labels"):
        assert np.array_equal(g[k], gd[k]), k
    lh = quickshift(img, kernel_size=2.0, max_dist=8.0, convert2lab=False, random_seed=11)
    ld = quickshift(torch.as_tensor(img).cuda(), kernel_size=2.0, max_dist=8.0, convert2lab=False, random_seed=11)
    assert np.array_equal(lh, g["labels"]) and np.array_equal(ld.cpu().numpy(), g["labels"])


@pytest.mark.parametrize("lab", [False, True])
def test_quickshift_stages_device_noise(oracle, lab):
    """rng="device": the noise drawn on the GPU is returned and fed to the oracle, which must then agree exactly."""
    from obia_amd.segmentation import quickshift, _quickshift_stages
    img = textured(50, 61, 3, 12)
    t = torch.as_tensor(img).cuda()
    g = qs.run_gpu(t, kernel_size=3.0, max_dist=10.0, convert2lab=lab, rng="device")
    assert 0 < np.abs(g["noise"]).max() < 1e-3 and np.abs(g["noise"]).std() > 5e-6
    ref_img = qs.oracle_image(oracle, img, 1.0, 0.0, lab)
    o = oracle.quickshift_stages(ref_img, g["noise"], 3.0, 10.0, tau=qs.TAU)
    qs.check(g, o, 10.0, "B" if lab else "A", staged_ref=ref_img, name=f"device noise, lab={lab}")
    assert np.array_equal(quickshift(t, kernel_size=3.0, max_dist=10.0, convert2lab=lab, rng="device").cpu().numpy(), g["labels"])
    with pytest.raises(ValueError):
        _quickshift_stages(img[..., :2], convert2lab=True)


@pytest.mark.parametrize("seed", range(int(os.environ.get("OBIA_RANDOM_QS_STAGE_CASES", "24"))))
def test_quickshift_stages_random(oracle, seed):
    rs = np.random.RandomState(61000 + seed)
    H, W = int(rs.choice([1, 2, 15, 16, 17, 31, 32, 33, rs.randint(3, 90)])), int(rs.choice([1, 3, 16, 17, 47, 48, 49, rs.randint(3, 110)]))
    C = int(rs.choice([1, 2, 3, 3, 4, 5, 8]))
    ks = float(rs.choice([1.0, 1.3, 2.0, 2.7, 4.0, 5.0, 5.01, 6.2]))
    md = float(rs.choice([0.0, 2.0, 6.0, 10.0, 30.0]))
    ratio = float(rs.choice([0.3, 1.0, 1.7]))
    lab = C == 3 and rs.rand() < 0.4
    sigma = float(rs.choice([0.0, 0.0, 0.7, 2.2])) if rs.rand() < 0.4 else 0.0
    img = textured(H, W, C, 100 + seed)
    run_case(oracle, img, ks, md, ratio, sigma, lab, seed=seed,
             name=f"seed {seed}: {H}x{W}x{C} ks {ks} md {md} ratio {ratio} sigma {sigma} lab {lab}")


def test_quickshift_stages_above_one_scan_thread(oracle):
    """4 410 000 pixels (not a multiple of the 4096-pixel chunk): qs_scan_kernel gives each of its 1024 threads two chunks.
    The whole raster against the oracle."""
    H = W = 2100
    img = textured(H, W, 3, 77)
    assert H * W > 1024 * 4096 and (H * W) % 4096
    run_case(oracle, img, 1.0, 4.0, seed=5, name="2100x2100x3")
