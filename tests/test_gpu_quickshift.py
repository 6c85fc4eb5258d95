"""GPU parity of quickshift (BASELINE config 5) against the scikit-image 0.18.3 golden vectors and
the oracle.  float64 on both sides; the only difference is exp/pow/cbrt (device libm vs glibc), which can flip a
parent only on near-ties: labels IDENTICAL to the goldens (the stage hook and the oracle's near-tie flags say why wherever
they would not be, tests/qs_stages.py); the earlier bar (ARI >= 0.99, label count within 2 %) is kept beside it."""
import os

import numpy as np
import pytest

from tests import qs_stages as qs
from tests.metrics import adjusted_rand_index

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_quickshift_vs_skimage_goldens(oracle):
    from obia_amd.segmentation import quickshift
    z = np.load(os.path.join(GOLD, "quickshift_small.npz"))
    for i in range(3):
        ks, md = z[f"par{i}"]
        raw = z[f"raw{i}"].astype(np.float32)
        lab = quickshift(raw, ratio=1.0, kernel_size=float(ks), max_dist=float(md), convert2lab=True, random_seed=42,
                         _normalize_bands=True)
        gold = z[f"labels{i}"]
        assert lab.shape == gold.shape and lab.dtype == np.int64
        ari = adjusted_rand_index(lab, gold)
        n_l, n_g = len(np.unique(lab)), len(np.unique(gold))
        assert ari >= 0.99, f"case {i}: ARI {ari} ({(lab != gold).mean():.3%} px differ)"
        assert abs(n_l - n_g) <= max(1, 0.02 * n_g)
        assert lab.min() == 0 and lab.max() == n_l - 1          # consecutive ids by root order
        # stage by stage: the staged image is scikit-image's float64 Lab image (x ratio 1), the labels the golden's exactly
        g = qs.run_gpu(raw, ratio=1.0, kernel_size=float(ks), max_dist=float(md), convert2lab=True, random_seed=42, _normalize_bands=True)
        o = oracle.quickshift_stages(z[f"lab{i}"] * 1.0, g["noise"], float(ks), float(md), tau=qs.TAU)
        assert np.array_equal(o["labels"], gold)
        qs.check(g, o, float(md), "B", staged_ref=z[f"lab{i}"] * 1.0, name=f"quickshift_small {i}")
        assert np.array_equal(g["labels"], gold) and np.array_equal(lab, gold), f"case {i}: {(lab != gold).sum()} px differ"


def test_quickshift_with_sigma_vs_skimage_goldens(oracle):
    """sigma (the Gaussian pre-smoothing of _quickshift.py, float64) against scikit-image's labels (tests/golden/quickshift_sigma.npz)
    and, without the Lab conversion, against the oracle on a random raster."""
    from obia_amd.segmentation import quickshift
    z = np.load(os.path.join(GOLD, "quickshift_sigma.npz"))
    for i in range(3):
        ks, md, sg, ratio, lab_flag = z[f"par{i}"]
        raw = z[f"raw{i}"].astype(np.float32)
        lab = quickshift(raw, ratio=float(ratio), kernel_size=float(ks), max_dist=float(md), sigma=float(sg), convert2lab=bool(lab_flag),
                         random_seed=42, _normalize_bands=True)
        gold = z[f"labels{i}"]
        ari = adjusted_rand_index(lab, gold)
        n_l, n_g = len(np.unique(lab)), len(np.unique(gold))
        assert ari >= 0.99, f"case {i}: ARI {ari} ({(lab != gold).mean():.3%} px differ)"
        assert abs(n_l - n_g) <= max(1, 0.02 * n_g)
        # stage by stage: the staged image is SciPy's smoothed float64 image x ratio, the labels the golden's exactly
        g = qs.run_gpu(raw, ratio=float(ratio), kernel_size=float(ks), max_dist=float(md), sigma=float(sg), convert2lab=bool(lab_flag),
                       random_seed=42, _normalize_bands=True)
        ref_img = z[f"smoothed{i}"] * float(ratio)
        o = oracle.quickshift_stages(ref_img, g["noise"], float(ks), float(md), tau=qs.TAU)
        assert np.array_equal(o["labels"], gold)
        qs.check(g, o, float(md), "B", staged_ref=ref_img, name=f"quickshift_sigma {i}")
        assert np.array_equal(g["labels"], gold) and np.array_equal(lab, gold), f"case {i}: {(lab != gold).sum()} px differ"
    rs = np.random.RandomState(11)
    H, W, C = 75, 93, 4
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.clip(np.stack([((yy // 19 + xx // 23 + c) % 3) / 2.0 for c in range(C)], -1) + 0.08 * rs.normal(size=(H, W, C)), 0, 1).astype(np.float32)
    noise = np.random.RandomState(5).normal(scale=0.00001, size=(H, W))
    ref = oracle.quickshift_core(oracle.quickshift_smooth(img.astype(np.float64), 1.3) * 0.5, noise, 3.0, 8.0)
    out = quickshift(img, ratio=0.5, kernel_size=3.0, max_dist=8.0, sigma=1.3, convert2lab=False, random_seed=5)
    assert adjusted_rand_index(out, ref) >= 0.99 and abs(len(np.unique(out)) - len(np.unique(ref))) <= max(1, 0.02 * len(np.unique(ref)))
    assert np.array_equal(out, ref), f"{(out != ref).sum()} px differ"
    with pytest.raises(ValueError):
        quickshift(img, sigma=-1.0, convert2lab=False)


def test_quickshift_vs_oracle_nolab_and_device_entry(oracle):
    from obia_amd.segmentation import quickshift, create_segments
    rs = np.random.RandomState(3)
    H, W = 70, 90
    img = np.zeros((H, W, 3), np.float32)
    img[:35, :45, 0] = 1; img[35:, :45, 1] = 1; img[35:, 45:, 2] = 1
    img = np.clip(img + 0.05 * rs.normal(size=img.shape), 0, 1).astype(np.float32)
    noise = np.random.RandomState(7).normal(scale=0.00001, size=(H, W))
    ref = oracle.quickshift_core(img.astype(np.float64) * 0.8, noise, 3.0, 8.0)
    lab = quickshift(img, ratio=0.8, kernel_size=3, max_dist=8, convert2lab=False, random_seed=7)
    assert adjusted_rand_index(lab, ref) >= 0.99
    lab_t = quickshift(torch.as_tensor(img).cuda(), ratio=0.8, kernel_size=3, max_dist=8, convert2lab=False, random_seed=7)
    assert np.array_equal(lab_t.cpu().numpy(), lab)
    # create_segments(method="quickshift") normalises every band first, like the reference
    seg = create_segments(img * 1000.0 + 5.0, method="quickshift", ratio=0.8, kernel_size=3, max_dist=8, convert2lab=False,
                          random_seed=7)
    assert seg.shape == (H, W)
    with pytest.raises(ValueError):
        quickshift(np.zeros((8, 8, 4), np.float32), convert2lab=True)


@pytest.mark.parametrize("C,ks,md", [(2, 3.0, 8.0), (5, 2.0, 6.0), (8, 3.0, 10.0), (3, 7.0, 15.0), (1, 6.5, 12.0)])
def test_quickshift_any_band_count_and_kernel_size(oracle, C, ks, md):
    """The reference forwards **kwargs untouched (segment_boundaries.py:48-49): 2, 5 or 8 bands and kernel_size > 5 (a
    window wider than the LDS-staged one) run the same arithmetic on global memory -- compared with the oracle."""
    from obia_amd.segmentation import quickshift
    rs = np.random.RandomState(C * 10 + int(ks))
    H, W = 60, 76
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([((yy // 20 + xx // 25 + c) % 3) / 2.0 for c in range(C)], -1)
    img = np.clip(base + 0.04 * rs.normal(size=base.shape), 0, 1).astype(np.float32)
    noise = np.random.RandomState(11).normal(scale=0.00001, size=(H, W))
    ref = oracle.quickshift_core(img.astype(np.float64), noise, ks, md)
    lab = quickshift(img, ratio=1.0, kernel_size=ks, max_dist=md, convert2lab=False, random_seed=11)
    assert adjusted_rand_index(lab, ref) >= 0.99
    assert lab.min() == 0 and lab.max() == len(np.unique(lab)) - 1
    assert abs(len(np.unique(lab)) - len(np.unique(ref))) <= max(1, 0.02 * len(np.unique(ref)))


def test_config5_full_size_quickshift_properties(oracle):
    """BASELINE configs[4] at full size: 8192 x 8192 x 3, quickshift(kernel_size=5, max_dist=10).  No oracle finishes this whole;
    the stage hook pins the forest exactly (roots are fixed points, every root is its own cut parent, every pixel shares its cut
    parent's root, every link climbs to a strictly higher density, labels are the rank of the root among the roots -- the scan runs
    16 chunks per thread here), and the oracle checks three crops of the hook's staged image and noise.  Earlier
    properties: consecutive ids 0..N-1 in ascending order of each segment's root pixel (np.unique(..., return_inverse)),
    every link of the forest is shorter than max_dist in the 5-D feature space so no segment reaches farther than its
    pixel count allows, a second run is bit-identical, and the count sits in the range the 512-pixel goldens predict."""
    from obia_amd.segmentation import quickshift, _quickshift_stages
    S = 8192
    g = torch.Generator(device="cuda").manual_seed(5)
    yy = torch.arange(S, device="cuda", dtype=torch.float32)[:, None]
    xx = torch.arange(S, device="cuda", dtype=torch.float32)[None, :]
    img = torch.stack([0.5 + 0.4 * torch.sin(xx / (11 + 3 * c)) * torch.cos(yy / (13 + 2 * c))
                       + 0.02 * torch.randn((S, S), device="cuda", generator=g) for c in range(3)], -1).clamp_(0, 1).contiguous()
    lab = quickshift(img, kernel_size=5, max_dist=10, ratio=1.0, rng="device")
    st = _quickshift_stages(img, kernel_size=5, max_dist=10, ratio=1.0, rng="device")
    lab2 = st["labels"]
    assert torch.equal(lab, lab2)
    n = int(lab.max().item()) + 1
    assert int(lab.min().item()) == 0
    sizes = torch.bincount(lab.reshape(-1), minlength=n)
    assert int((sizes == 0).sum().item()) == 0                       # ids 0..N-1 all used
    flat = lab.reshape(-1).to(torch.int64)
    first = torch.full((n,), S * S, dtype=torch.int64, device="cuda").scatter_reduce_(0, flat, torch.arange(S * S, device="cuda"), "amin")
    # a root is its segment's pixel of highest density, not its first pixel, but ids follow the ROOT order; what must hold for
    # any forest: first pixels are distinct and every id has one
    assert int(torch.unique(first).numel()) == n
    assert 1e4 <= n <= 2e6
    # the forest, exactly
    idx = torch.arange(S * S, device="cuda", dtype=torch.int64)
    roots = st["roots"].reshape(-1).to(torch.int64)
    dens = st["dens"].reshape(-1)
    cutp = torch.where(st["dist_parent"].reshape(-1) > 10.0, idx, st["parent"].reshape(-1).to(torch.int64))
    assert torch.equal(roots[roots], roots)
    is_root = roots == idx
    assert torch.equal(cutp[is_root], idx[is_root])
    assert torch.equal(roots[cutp], roots)
    link = cutp != idx
    assert bool((dens[cutp[link]] > dens[link]).all())
    rank = torch.cumsum(is_root.to(torch.int64), 0) - 1
    assert torch.equal(rank[roots], flat) and st["n_labels"] == n == int(is_root.sum().item())
    # three crops against the oracle, on the hook's staged image and noise: densities >= kw from a cut edge, parents >= 2 kw
    kw = 15
    for name, (y0, x0) in {"top-left": (0, 0), "bottom-right": (S - 150, S - 150), "centre": (S // 2 - 75, S // 2 - 75)}.items():
        ys, xs = slice(y0, y0 + 150), slice(x0, x0 + 150)
        crop = st["image"][:, ys, xs].permute(1, 2, 0).contiguous().cpu().numpy()
        o = oracle.quickshift_stages(crop, st["noise"][ys, xs].contiguous().cpu().numpy(), 5.0, 10.0, tau=qs.TAU)

        def inner(m):   # rows / columns at least m from every crop edge that is not an image edge
            r = np.arange(150)
            ok_y = ((r >= m) | (y0 == 0)) & ((r < 150 - m) | (y0 + 150 == S))
            ok_x = ((r >= m) | (x0 == 0)) & ((r < 150 - m) | (x0 + 150 == S))
            return ok_y[:, None] & ok_x[None, :]
        d1, d2 = inner(kw), inner(2 * kw)
        gd = st["dens"][ys, xs].cpu().numpy()
        np.testing.assert_allclose(gd[d1], o["dens"][d1], rtol=qs.DENS_RTOL, atol=0, err_msg=name)
        gp = st["parent"][ys, xs].cpu().numpy().astype(np.int64)
        op = o["parent"]
        op_global = (op // 150 + y0) * S + (op % 150 + x0)
        untied = d2 & ((o["flags"] & 1) == 0)
        assert np.array_equal(gp[untied], op_global[untied]), f"{name}: {(gp[untied] != op_global[untied]).sum()} parents differ"
        same = d2 & (gp == op_global)
        gdp = st["dist_parent"][ys, xs].cpu().numpy()
        assert np.array_equal(gdp[same], o["dist_parent"][same]), name
        assert untied.sum() >= 0.9 * d2.sum()


def test_quickshift_device_noise_matches_the_goldens_away_from_ties():
    """rng="device" draws the tie-breaking noise on the GPU (not NumPy's stream): on natural images densities never tie
    to within 1e-5, so the partition is that of the golden vectors to the same tolerance."""
    from obia_amd.segmentation import quickshift
    z = np.load(os.path.join(GOLD, "quickshift_small.npz"))
    ks, md = z["par0"]
    raw = z["raw0"].astype(np.float32)
    lab = quickshift(torch.as_tensor(raw).cuda(), ratio=1.0, kernel_size=float(ks), max_dist=float(md), convert2lab=True,
                     rng="device", _normalize_bands=True).cpu().numpy()
    assert adjusted_rand_index(lab, z["labels0"]) >= 0.99
    with pytest.raises(ValueError):
        quickshift(raw, rng="device")
