"""GLCM texture (texture_kernel<false / true>, bbox_kernel) against oracle/glcm.py at 1e-9, at the edges of the kernels:
NaN pixels, band subsets, 16 bands, start_label 0 and labels out of range; bounding boxes of 4096 / 4097 pixels (the LDS
path / the dense path); one crop per LDS table size (tbits 8..13) filled by uniform noise; more than 256 dense-path
segments (grid-stride reuse of the scratch); more than 65 536 labels (grid stride of the LDS launch); 64 x 64 blocks
with more than BB_SLOTS = 128 labels (bbox_kernel's global fallback); strips of width / height 1 and 2; grey values that
sit exactly on quantisation levels.  The reference driver finds the boxes with scipy.ndimage.find_objects and caches
glcm_props by quantised crop, so the many-label cases stay fast."""
import numpy as np
import pytest
from scipy.ndimage import find_objects

from oracle.glcm import PROPS, glcm_props, quantise_crop

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def texture_reference(raw, lab, bands=None, start_label=1, n_labels=None):
    C = raw.shape[2]
    bands = list(range(C)) if bands is None else list(bands)
    if n_labels is None:
        n_labels = int(lab.max()) - start_label + 1
    out = {p: np.full((n_labels, len(bands)), np.nan) for p in PROPS}
    rel = lab.astype(np.int64) - start_label + 1
    rel[(rel < 1) | (rel > n_labels)] = 0
    cache = {}
    for i, sl in enumerate(find_objects(rel, max_label=n_labels)):
        if sl is None:
            continue
        inside = rel[sl] == i + 1
        for j, b in enumerate(bands):
            q = quantise_crop(raw[sl + (b,)].astype(np.float32), inside)
            if q is None:
                continue
            key = (q.shape, q.tobytes())
            if key not in cache:
                cache[key] = glcm_props(q)
            for p, v in cache[key].items():
                out[p][i, j] = v
    return out


def check(raw, lab, **kw):
    from obia_amd.statistics import texture_stats
    ref = texture_reference(raw, lab, **kw)
    tx = texture_stats(torch.as_tensor(raw).cuda(), torch.as_tensor(lab).cuda(), **kw)
    for p in PROPS:
        got = tx[p].cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(ref[p])), p
        np.testing.assert_allclose(got, ref[p], rtol=1e-9, atol=1e-12, equal_nan=True, err_msg=p)
    return ref


def blocks(H, W, s, rs=None, jitter=0.0):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    if rs is not None:
        yy = yy + jitter * rs.randn(H, W)
        xx = xx + jitter * rs.randn(H, W)
    return ((yy // s).astype(np.int64) * ((W + s - 1) // s + 2) + (xx // s).astype(np.int64) + 1).astype(np.int32)


def test_nan_subsets_16_bands_start0_out_of_range():
    rs = np.random.RandomState(1)
    H, W, C = 50, 70, 16
    raw = (rs.gamma(2.0, 30.0, (H, W, C)) + 500).astype(np.float32)
    raw[rs.rand(H, W, C) < 0.05] = np.nan
    raw[:, :, 5] = np.nan
    lab = blocks(H, W, 13, rs, 1.0) - 1
    lab[rs.rand(H, W) < 0.05] = -1
    n = int(lab.max()) - 3                                  # the largest labels fall out of range
    check(raw, lab, start_label=0, n_labels=n)
    check(raw, lab + 1, bands=[15, 3, 5, 0], n_labels=n + 7)


def bbox_inputs(h, w):
    """(raw, labels): label 1 fills an h x w box, with a hole row of another label inside it"""
    rs = np.random.RandomState(h * 7 + w)
    raw = rs.uniform(0, 1000, (h + 4, w + 4, 2)).astype(np.float32)
    lab = np.zeros((h + 4, w + 4), np.int32)
    lab[2:2 + h, 2:2 + w] = 1
    lab[2 + h // 2, 2:2 + w] = 2 if h > 2 else 1            # a hole row (another label) inside the box
    lab[0, 0] = 3
    return raw, lab


@pytest.mark.parametrize("hw", [(64, 64), (1, 4096), (4096, 1), (17, 241), (1, 4097), (4097, 1), (65, 63)])
def test_bbox_4096_4097(hw):
    """Bounding boxes of exactly 4096 pixels (LDS path) and 4097 (dense path), as squares and strips."""
    check(*bbox_inputs(*hw))


def test_lds_table_sizes_full_of_noise():
    """Crops of 120, 256, 500, 1024, 2000 and 4080 pixels: tbits 8, 9, 10, 11, 12, 13, each filled by uniform noise."""
    sizes = [(10, 12), (16, 16), (20, 25), (32, 32), (40, 50), (60, 68)]
    rs = np.random.RandomState(3)
    H, W = 64, sum(w for _, w in sizes) + len(sizes)
    raw = rs.uniform(0, 1, (H, W, 3)).astype(np.float32)
    lab = np.zeros((H, W), np.int32)
    x = 0
    for i, (h, w) in enumerate(sizes):
        lab[:h, x:x + w] = i + 1
        x += w + 1
    check(raw, lab)


def test_more_than_256_dense_segments():
    rs = np.random.RandomState(4)
    lab = blocks(15 * 65, 20 * 65, 65)                     # 300 segments of 65 x 65 = 4225 pixels
    raw = rs.uniform(0, 500, lab.shape + (1,)).astype(np.float32)
    raw[rs.rand(*raw.shape) < 0.01] = np.nan
    ref = check(raw, lab)
    assert np.isfinite(ref["contrast"]).sum() >= 300


def test_more_than_65536_labels_and_crowded_blocks():
    """67 200 one-pixel labels (the LDS launch strides its grid) -- 4096 of them per 64 x 64 block, far past BB_SLOTS."""
    rs = np.random.RandomState(5)
    H, W = 280, 240
    lab = (np.arange(H * W).reshape(H, W) + 1).astype(np.int32)
    raw = rs.uniform(0, 100, (H, W, 1)).astype(np.float32)
    raw[rs.rand(H, W, 1) < 0.02] = np.nan
    assert lab.max() > 65536
    from obia_amd.statistics import texture_stats
    tx = texture_stats(torch.as_tensor(raw).cuda(), torch.as_tensor(lab).cuda())
    one = glcm_props(quantise_crop(raw[:1, :1, 0], np.ones((1, 1), bool)))   # every 1 x 1 crop with a valid pixel
    valid = ~np.isnan(raw[:, :, 0].ravel())
    for p in PROPS:
        got = tx[p].cpu().numpy()[:, 0]
        assert np.array_equal(np.isnan(got), ~valid), p
        np.testing.assert_allclose(got[valid], one[p], rtol=1e-9, atol=1e-12, err_msg=p)
    # blocks of 64 x 64 with ~300 labels each and boxes that span several blocks
    lab2 = rs.randint(1, 4000, (200, 200)).astype(np.int32)
    check(rs.uniform(0, 100, (200, 200, 1)).astype(np.float32), lab2)


def thin_strips_inputs():
    rs = np.random.RandomState(6)
    H, W = 40, 60
    raw = rs.uniform(0, 100, (H, W, 2)).astype(np.float32)
    lab = np.zeros((H, W), np.int32)
    lab[:, 0] = 1                                           # w = 1
    lab[:, 2:4] = 2                                         # w = 2
    lab[0, 5:] = 3                                          # h = 1
    lab[2:4, 5:] = 4                                        # h = 2
    lab[5:, 5:] = blocks(H - 5, W - 5, 7) + 4
    return raw, lab


def test_thin_strips():
    check(*thin_strips_inputs())


@pytest.mark.parametrize("den", [1.0, 3.0, 7.0, 100.0, 255.0, 1000.0, 4095.0, 65535.0])
def test_values_on_quantisation_levels(den):
    """lo = 0 (zeros outside the segment) and values k * den / 255: (v - lo) / den * 255 lands on or next to k in float32,
    where dividing after the scaling, or rounding instead of truncating, gives another grey level."""
    rs = np.random.RandomState(int(den))
    H, W = 48, 64
    k = rs.randint(0, 256, (H, W, 2))
    raw = (k * np.float32(den) / np.float32(255)).astype(np.float32)
    raw[..., 1] = (k[..., 1] * (den / 255.0)).astype(np.float32)
    lab = blocks(H, W, 8)
    lab[::5, ::3] = 0                                       # holes: zeros inside the crops
    raw[:, :, 0][lab == lab[0, 0]] = np.float32(den)        # a crop whose max is exactly den
    check(raw, lab)
