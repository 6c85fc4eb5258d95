"""The sharpness raster on the GPU (obia_amd.image.rgb_to_gray / box_filter / variance_of_laplacian / laplacian) against the NumPy
restatement (tests/sharpness_restatement.py) and, for the box filter, against the committed SciPy 1.15.3 goldens.  Every comparison
is exact equality of float32 bit patterns (``view(uint32)``, so NaNs compare).

Shapes: the smallest at which the kernels can go wrong -- single pixels and lines, (2, 2), odd sizes, and (130, 517): more rows than
the band of 64 rows one axis-1 workgroup owns (BOX_ROWS, csrc/sharpness.hip) and more columns than two LDS chunks of 64 (BOX_CH1; 32
for the variance), so that a band and its ragged neighbour, an inner chunk that needs no reflection (the unrolled path) and the ragged
last chunk are all taken; axis 0 unrolls 16 rows (BOX_UNROLL): 130 rows give whole blocks and a remainder; the plane also spans nine
64 x 32 tiles of the Laplacian across and five down.  Windows: 1 (a copy), 2, 3, 4, 15 and one longer than twice the longer side."""
import functools
import glob
import hashlib
import os

import numpy as np
import pytest

from tests import sharpness_restatement as S

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "sharpness", "*.npz")))
SHAPES = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 13), (9, 4), (33, 17), (67, 130), (130, 517)]


def big_win(shape):
    return 300 if shape == (67, 130) else 2 * max(shape) + 12


CASES = [(shape, win) for shape in SHAPES for win in (1, 2, 3, 4, 15, big_win(shape))]
IDS = [f"{s[0]}x{s[1]}-w{w}" for s, w in CASES]


def same(got, want):
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape
    diff = S.bits(got) != S.bits(want)
    assert not diff.any(), f"{int(diff.sum())} of {want.size} differ, first at {tuple(np.argwhere(diff)[0])}"


@functools.lru_cache(maxsize=None)
def raster01(shape, C=5, seed=2):
    """a [0, 1] raster (H, W, C) float32; read-only"""
    a = np.random.RandomState(seed).rand(shape[0], shape[1], C).astype(np.float32)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def want_box(data, shape, win):
    return S.box_filter(S.golden_plane(data, shape), win)


@functools.lru_cache(maxsize=None)
def want_variance(shape, win):
    return S.variance_of_laplacian(S.golden_plane("n50", shape), win)


@functools.lru_cache(maxsize=None)
def want_laplacian(shape, win):
    return S.laplacian(raster01(shape), win)


# ---- box filter --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[:-4] for p in GOLDENS])
def test_box_filter_is_scipy_through_the_goldens(path):
    from obia_amd.image import box_filter
    assert len(GOLDENS) == 13
    g = np.load(path)
    data, shp = os.path.basename(path)[:-4].split("_")
    shape = tuple(int(v) for v in shp.split("x"))
    plane = g["plane"] if "plane" in g else S.golden_plane(data, shape)
    assert hashlib.sha256(plane.tobytes()).hexdigest() == str(g["sha_plane"])
    for w in (int(v) for v in g["wins"]):
        got = box_filter(plane, w)
        assert got.dtype == np.float32 and got.shape == shape
        if f"out_{w}" in g:
            same(got, g[f"out_{w}"])
        else:
            assert hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest() == str(g[f"sha_{w}"]), (data, shape, w)


@pytest.mark.parametrize("shape,win", CASES, ids=IDS)
def test_box_filter_is_the_restatement(shape, win):
    from obia_amd.image import box_filter
    same(box_filter(S.golden_plane("n50", shape), win), want_box("n50", shape, win))


@pytest.mark.parametrize("win", [3, 4])
@pytest.mark.parametrize("shape", [(67, 130), (130, 517)])
def test_box_filter_wide_range_needs_the_serial_sum(shape, win):
    from obia_amd.image import box_filter
    same(box_filter(S.golden_plane("wide", shape), win), want_box("wide", shape, win))


def test_box_filter_takes_other_dtypes_as_float32():
    from obia_amd.image import box_filter
    rs = np.random.RandomState(5)
    for plane in (rs.randint(0, 60000, (21, 40)).astype(np.uint16), rs.randint(0, 256, (21, 40)).astype(np.uint8),
                  rs.randint(-3000, 3000, (21, 40)).astype(np.int16), rs.standard_normal((21, 40)) * 1e3):
        same(box_filter(plane, 5), S.box_filter(plane.astype(np.float32), 5))


# ---- variance of the Laplacian ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,win", CASES, ids=IDS)
def test_variance_of_laplacian_is_the_restatement(shape, win):
    from obia_amd.image import variance_of_laplacian
    same(variance_of_laplacian(S.golden_plane("n50", shape), win), want_variance(shape, win))


def test_gray_is_the_numpy_expression():
    from obia_amd.image import rgb_to_gray
    rgb = raster01((33, 65), C=3, seed=3)
    coeffs = np.array([0.299, 0.587, 0.114], dtype=np.float32)
    same(rgb_to_gray(rgb), (rgb * coeffs).sum(axis=-1))
    t = rgb_to_gray(torch.as_tensor(rgb).cuda())
    assert t.is_cuda and t.dtype == torch.float32
    same(t.cpu().numpy(), (rgb * coeffs).sum(axis=-1))


# ---- laplacian -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,win", CASES, ids=IDS)
def test_laplacian_is_the_restatement(shape, win):
    from obia_amd.image import laplacian
    same(laplacian(raster01(shape), None, win), want_laplacian(shape, win))


@pytest.mark.parametrize("bands", [(1, 2, 4), (4, 0, 3)])
@pytest.mark.parametrize("dtype", [np.uint16, np.float32, np.float64, np.uint8, np.int16])
def test_laplacian_dtypes_and_bands(dtype, bands):
    from obia_amd.image import Image, laplacian
    rs = np.random.RandomState(12)
    hi = 255 if dtype == np.uint8 else 3000
    img = (rs.rand(64, 257, 5) * hi).astype(dtype)
    want = S.laplacian(img, 7, bands)
    same(laplacian(img, None, 7, bands=bands), want)
    same(Image(img).laplacian(7, bands=list(bands)), want)


def test_laplacian_constant_band_and_constant_raster():
    from obia_amd.image import laplacian
    img = raster01((40, 70)).copy()
    img[..., 2] = 0.25                                                       # a used band that is constant: zeros, not NaN
    want = S.laplacian(img, 5)
    assert not np.isnan(want).any()
    same(laplacian(img, None, 5), want)
    flat = np.full((40, 70, 5), 7.0, np.float32)                             # hi == lo, taken literally: 0 / 0 everywhere
    out = laplacian(flat, None, 5)
    assert np.isnan(out).all()
    same(out, S.laplacian(flat, 5))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_input_raises(bad):
    from obia_amd.image import box_filter, laplacian, variance_of_laplacian
    img = raster01((33, 70)).copy()
    img[32, 69, 4] = bad
    with pytest.raises(ValueError, match="1 NaN or infinite values in bands"):
        laplacian(img, None, 3)
    if np.isnan(bad):                                                        # an unused band may hold anything
        same(laplacian(img, None, 3, bands=(0, 1, 2)), S.laplacian(img, 3, (0, 1, 2)))
        other = raster01((33, 70)).copy()
        other[0, 0, 3] = other[5, 5, 0] = bad
        same(laplacian(other, None, 3), S.laplacian(raster01((33, 70)), 3))
        same(laplacian(torch.as_tensor(other).cuda(), None, 3).cpu().numpy(), S.laplacian(raster01((33, 70)), 3))
    plane = S.golden_plane("n50", (33, 70)).copy()
    plane[0, 0] = plane[32, 69] = bad
    for fn in (box_filter, variance_of_laplacian):
        with pytest.raises(ValueError, match="2 NaN or infinite values"):
            fn(plane, 3)
        with pytest.raises(ValueError, match="2 NaN or infinite values"):
            fn(plane, 1)


def test_cuda_tensor_in_gives_cuda_tensor_out():
    from obia_amd.image import Image, box_filter, laplacian, variance_of_laplacian
    img = raster01((67, 130))
    t = torch.as_tensor(np.array(img)).cuda()
    out = laplacian(t, None, 4)
    assert isinstance(out, torch.Tensor) and out.device == t.device and out.dtype == torch.float32
    same(out.cpu().numpy(), want_laplacian((67, 130), 4))
    same(Image(t).laplacian(4).cpu().numpy(), want_laplacian((67, 130), 4))
    same(laplacian(t.to(torch.float64), None, 4).cpu().numpy(), want_laplacian((67, 130), 4))      # float32 values: the cast is exact
    same(laplacian(t[:, 1:].contiguous(), None, 4).cpu().numpy(), S.laplacian(img[:, 1:], 4))      # a view's copy, 129 columns
    plane = torch.as_tensor(S.golden_plane("n50", (67, 130))).cuda()
    for fn, want in ((box_filter, want_box("n50", (67, 130), 4)), (variance_of_laplacian, want_variance((67, 130), 4))):
        got = fn(plane, 4)
        assert isinstance(got, torch.Tensor) and got.device == plane.device
        same(got.cpu().numpy(), want)


def test_two_runs_agree_bit_for_bit():
    from obia_amd.image import laplacian, variance_of_laplacian
    img = raster01((130, 517))
    a, b = laplacian(img, None, 15), laplacian(img, None, 15)
    assert np.array_equal(S.bits(a), S.bits(b))
    plane = S.golden_plane("wide", (130, 517))
    assert np.array_equal(S.bits(variance_of_laplacian(plane, 4)), S.bits(variance_of_laplacian(plane, 4)))
