"""Image previews on the GPU (obia_amd.image, Segments.to_segmented_image) against the CPU restatement tests/image_restatement.py,
which tests/test_image_cpu.py pins to NumPy, to scikit-image 0.18.3 (goldens) and to answers worked out by hand.  Every comparison
is exact equality of uint8 arrays.  The OpenCV parts are restated from OpenCV's algorithm and are NOT compared with cv2 anywhere."""
import glob
import os

import numpy as np
import pytest

from tests import image_restatement as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "boundaries", "*.npz")))


def same(got, want):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.dtype == np.uint8 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, f"{bad.size} of {want.size} differ, first at {np.unravel_index(bad[0], want.shape)}: " \
                          f"{got.ravel()[bad[0]]} for {want.ravel()[bad[0]]}"


def raster(shape, seed, dtype=np.float32):
    rs = np.random.RandomState(seed)
    return (rs.normal(900, 300, shape).clip(0, 4000)).astype(dtype)


# ---- rescale_to_8bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 3), (7, 13, 3), (64, 257, 3), (4099,)])
@pytest.mark.parametrize("pq", [(2, 98), (0, 100), (25, 25), (50, 50.0001)])
def test_rescale_shapes_and_percentiles(shape, pq):
    from obia_amd.image import rescale_to_8bit
    x = raster(shape, 1)
    same(rescale_to_8bit(x, *pq), R.rescale_to_8bit(x, *pq))


def test_rescale_virtual_index_is_an_integer():
    from obia_amd.image import rescale_to_8bit
    x = raster((101,), 2)                         # (n - 1) * q = 2 and 98 exactly
    same(rescale_to_8bit(x), R.rescale_to_8bit(x))
    x = raster((3, 17, 1), 3)                     # n = 51: (n - 1) * 0.02 = 1, (n - 1) * 0.98 = 49
    same(rescale_to_8bit(x), R.rescale_to_8bit(x))


@pytest.mark.parametrize("dtype", [np.float64, np.uint16, np.uint8, np.int16])
def test_rescale_dtypes(dtype):
    from obia_amd.image import rescale_to_8bit
    x = raster((19, 23, 3), 4).astype(dtype) if dtype != np.uint8 else np.random.RandomState(4).randint(0, 256, (19, 23, 3)).astype(dtype)
    if dtype == np.int16:
        x = (x - 900).astype(dtype)
    same(rescale_to_8bit(x), R.rescale_to_8bit(x))
    same(rescale_to_8bit(x, 10, 60), R.rescale_to_8bit(x, 10, 60))


def test_rescale_constant_nan_and_torch():
    from obia_amd.image import rescale_to_8bit
    const = np.full((9, 11, 3), 412.5, np.float32)
    same(rescale_to_8bit(const), np.zeros(const.shape, np.uint8))
    x = raster((12, 10, 3), 5)
    bad = x.copy()
    bad[3, 4, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        rescale_to_8bit(bad)
    t = torch.as_tensor(x).cuda()
    out = rescale_to_8bit(t)
    assert isinstance(out, torch.Tensor) and out.device == t.device and out.dtype == torch.uint8
    same(out, R.rescale_to_8bit(x))
    assert isinstance(rescale_to_8bit(x), np.ndarray)


# ---- to_image -----------------------------------------------------------------------------------------------------------------
def want_image(raw, bands, p_min, p_max, stretch_type):
    rgb = np.empty(raw.shape[:2] + (3,), np.float32)
    for i, b in enumerate(bands):
        rgb[:, :, i] = raw[:, :, b]
    out = R.rescale_to_8bit(rgb, p_min, p_max)                   # the percentile over the three bands TOGETHER
    if stretch_type == "histogram_equalization":
        out = R.apply_histogram_equalization(out)
    elif stretch_type == "clahe":
        out = R.apply_clahe(out)
    return out


@pytest.mark.parametrize("bands", [(4, 0, 2), [1, 1, 1]])
@pytest.mark.parametrize("stretch_type", [None, "histogram_equalization", "clahe"])
def test_to_image(bands, stretch_type):
    from obia_amd.image import Image, to_image
    raw = np.stack([raster((40, 52), 10 + c) * (1 + 0.3 * c) for c in range(5)], -1).astype(np.float32)
    want = want_image(raw, bands, 2, 98, stretch_type)
    arr = to_image(raw, bands, stretch_type=stretch_type, as_array=True)
    same(arr, want)
    pil = Image(raw).to_image(bands, stretch_type=stretch_type)
    assert pil.mode == "RGB" and pil.size == (52, 40)
    same(np.array(pil), want)
    t = to_image(Image(torch.as_tensor(raw).cuda()), bands, p_min=5, p_max=90, stretch_type=stretch_type, as_array=True)
    assert isinstance(t, torch.Tensor) and t.is_cuda
    same(t, want_image(raw, bands, 5, 90, stretch_type))


# ---- histogram equalisation -------------------------------------------------------------------------------------------------------
def u8(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


@pytest.mark.parametrize("name", ["grey", "rgb", "two_values", "constant", "constant_rgb", "all_values", "row", "flat_large"])
def test_histogram_equalization(name):
    from obia_amd.image import apply_histogram_equalization
    img = {"grey": lambda: u8((33, 47), 1), "rgb": lambda: u8((33, 47, 3), 2),
           "two_values": lambda: np.where(u8((21, 30), 3) < 100, 10, 200).astype(np.uint8),
           "constant": lambda: np.full((13, 9), 93, np.uint8), "constant_rgb": lambda: np.full((13, 9, 3), (10, 200, 77), np.uint8),
           "all_values": lambda: np.arange(256, dtype=np.uint8).reshape(16, 16).repeat(3, 0)[:, ::-1].copy(),
           "row": lambda: u8((1, 5, 3), 4),
           "flat_large": lambda: np.pad(np.full((300, 400), 7, np.uint8), 2, constant_values=250)}[name]()   # many workgroups, one bin
    same(apply_histogram_equalization(img), R.apply_histogram_equalization(img))


# ---- CLAHE -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 8), (16, 24), (37, 41), (40, 41), (41, 40), (9, 9), (8, 9), (512, 520)])
def test_clahe_sizes(shape):
    from obia_amd.image import apply_clahe
    img = u8(shape, shape[0] * 1000 + shape[1])
    same(apply_clahe(img), R.apply_clahe(img))


def tile_residuals(plane):
    """(excess, excess % 256) of the 64 tiles of the padded plane"""
    H, W = plane.shape
    ph, pw, th, tw, clip, _ = R.clahe_geometry(H, W)
    padded = plane[np.ix_([R.reflect101(y, H) for y in range(ph)], [R.reflect101(x, W) for x in range(pw)])]
    out = []
    for ty in range(8):
        for tx in range(8):
            h = np.bincount(padded[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256)
            e = int(np.maximum(h - clip, 0).sum())
            out.append((e, e % 256))
    return out


def test_clahe_content():
    from obia_amd.image import apply_clahe
    noise = u8((37, 41), 6)
    same(apply_clahe(noise), R.apply_clahe(noise))
    const = np.full((48, 344), 200, np.uint8)                    # tiles of 6 x 43 = 258, clip 2: the maximal excess 256, residual 0
    assert set(tile_residuals(const)) == {(256, 0)}
    same(apply_clahe(const), R.apply_clahe(const))
    step1 = np.full((128, 128), 50, np.uint8)                    # tiles of 256, clip 2: excess 254 = residual > 128, so step = 1
    assert set(tile_residuals(step1)) == {(254, 254)}
    same(apply_clahe(step1), R.apply_clahe(step1))
    patch = u8((96, 104), 7)
    patch[20:70, 30:90] = 140                                    # a constant patch in noise: residuals with step > 1 among the tiles
    assert any(1 < 256 // r for e, r in tile_residuals(patch) if r)
    same(apply_clahe(patch), R.apply_clahe(patch))
    rgb = np.stack([u8((37, 41), 8), patch[:37, :41], np.full((37, 41), 3, np.uint8)], -1)     # three channels, different content
    same(apply_clahe(rgb), R.apply_clahe(rgb))
    t = torch.as_tensor(rgb).cuda()
    out = apply_clahe(t)
    assert isinstance(out, torch.Tensor) and out.is_cuda
    same(out, R.apply_clahe(rgb))
    with pytest.raises(ValueError, match="8 x 8"):
        apply_clahe(u8((7, 20), 9))


# ---- boundaries -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[:-4] for p in GOLDENS])
def test_boundaries_and_overlay_match_the_goldens(path):
    PIL = pytest.importorskip("PIL.Image")
    from obia_amd.image import find_boundaries, mark_boundaries_u8
    from obia_amd.segmentation import Segments
    g = np.load(path)
    lab, img = g["labels"], g["image"]
    same(find_boundaries(lab), g["boundaries"])
    same(find_boundaries(lab.astype(np.int64)), g["boundaries"])
    same(mark_boundaries_u8(img, lab), g["marked"])
    seg = Segments(lab, None, "slic")
    pil = seg.to_segmented_image(PIL.fromarray(img))
    assert pil.mode == "RGB"
    same(np.array(pil), g["marked"])
    dev = Segments(torch.as_tensor(lab).cuda(), None, "slic").to_segmented_image(PIL.fromarray(img), as_array=True)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda
    same(dev, g["marked"])
    other = mark_boundaries_u8(torch.as_tensor(img).cuda(), lab, color=(0, 128, 255))
    assert isinstance(other, torch.Tensor)
    same(other, R.mark_u8(img, lab, color=(0, 128, 255)))


def test_overlay_of_a_real_slic_call():
    PIL = pytest.importorskip("PIL.Image")
    from obia_amd.image import find_boundaries, to_image
    from obia_amd.segmentation import Segments, slic
    raw = np.stack([raster((64, 80), 20 + c) for c in range(4)], -1)
    yy, xx = np.mgrid[0:64, 0:80]
    raw += (200 * np.sin(xx / 9.0) * np.cos(yy / 7.0))[..., None].astype(np.float32)
    mask = np.ones((64, 80), bool)
    mask[20:31, 33:50] = False                                   # a hole: -1 under scikit-image's maskSLIC numbering
    lab = slic(raw, n_segments=40, compactness=10.0, mask=mask, start_label=0, _normalize_bands=True)
    lab = np.asarray(lab)
    assert (lab == -1).any() and (lab == 0).any() and lab.max() > 5
    same(find_boundaries(lab), R.find_boundaries(lab.astype(np.int32)).astype(np.uint8))
    rgb = to_image(raw, [2, 1, 0], as_array=True)
    got = Segments(lab, None, "slic").to_segmented_image(PIL.fromarray(rgb), as_array=True)
    same(got, R.mark_u8(rgb, lab.astype(np.int32)))
    grey = PIL.fromarray(rgb[..., 0].copy())
    same(Segments(lab, None, "slic").to_segmented_image(grey, as_array=True), R.mark_u8(rgb[..., 0], lab.astype(np.int32)))


def test_overlay_table_on_all_256_values():
    from obia_amd.image import mark_boundaries_u8
    allv = np.arange(256, dtype=np.uint8).reshape(16, 16)
    lab = np.full((16, 16), 4, np.int32)                         # one region: no boundary, every pixel goes through the table
    want = np.stack([R.mark_table()[allv]] * 3, -1)
    assert (want[..., 0] != allv).sum() == 24
    same(mark_boundaries_u8(allv, lab), want)
    rgb = np.stack([allv, allv[::-1], allv.T], -1)
    same(mark_boundaries_u8(rgb, lab), R.mark_table()[rgb])
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        mark_boundaries_u8(rgb, np.full((16, 16), 2 ** 31 - 1, np.int32))


# ---- determinism --------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_byte_identical():
    from obia_amd import image as I
    x = raster((64, 257, 3), 30)
    img = u8((75, 131, 3), 31)
    lab = (np.add.outer(np.arange(75) // 9, np.arange(131) // 11) % 5 - 1).astype(np.int32)
    ops = {"rescale": lambda: I.rescale_to_8bit(x), "equalize": lambda: I.apply_histogram_equalization(img),
           "clahe": lambda: I.apply_clahe(img), "boundaries": lambda: I.find_boundaries(lab),
           "mark": lambda: I.mark_boundaries_u8(img, lab),
           "to_image": lambda: I.to_image(np.concatenate([x[:, :, :2]] * 2, -1), [3, 0, 1], stretch_type="clahe", as_array=True)}
    for name, op in ops.items():
        a, b = op(), op()
        assert a.tobytes() == b.tobytes(), name
