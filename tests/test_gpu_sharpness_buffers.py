"""The entry points of include/obia_sharpness.h on buffers that start 0, 1 and 3 floats off a 16-byte boundary, with poisoned guards
around every output, work plane and counter (tests/offset_views.py, tests/guarded.py), as tests/test_gpu_image_buffers.py does it for
obia_image.h.  Per case: the result equals the CPU restatement (tests/sharpness_restatement.py) bit for bit whatever the offsets, no
guard byte changed, no element left unwritten (for both poisons), the inputs byte-identical afterwards.

Shapes: 11 rows at widths 1, 3, 5, 64 and 67 (one ragged row band; one LDS chunk and a tail), and 140 x 131 with win = 5: three row bands
and three column chunks of 64 (five of 32 for the variance), the inner ones taking the unrolled paths of both axes (csrc/sharpness.hip)."""
import ctypes

import numpy as np
import pytest

from tests import sharpness_restatement as S
from tests.guarded import POISONS, guarded, snapshot, unchanged
from tests.offset_views import offset_view, residue
from tests.refusal_text import refused_saying

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KS = (0, 1, 3)
SHAPES = ((11, 1), (11, 3), (11, 5), (11, 64), (11, 67), (140, 131))
WIN = {(11, 1): 2, (11, 3): 3, (11, 5): 4, (11, 64): 15, (11, 67): 30, (140, 131): 5}

# every name of obia_amd._lib._SHARPNESS_SIGNATURES: the test below that runs it here, or the reason of a sentence why none does
EXERCISED = {
    "obia_sharp_gray_lap_dev": "test_gray_lap",
    "obia_sharp_laplacian_dev": "test_laplacian",
    "obia_sharp_box_dev": "test_box",
    "obia_sharp_variance_dev": "test_variance",
    "obia_sharp_stretch_f32_dev": "test_stretch",
}
NOT_EXERCISED = {}


def env():
    from obia_amd import _lib
    lib = _lib.load()
    return _lib, lib, _lib.default_context(0)


def dev_off(a, k):
    t = offset_view(torch.as_tensor(np.ascontiguousarray(a)).cuda(), k)
    assert residue(t) == (k * t.element_size()) % 16
    return t


def run(_lib, lib, c, fn, *args, expect=0):
    torch.cuda.synchronize()
    rc = fn(c.handle, *args)
    assert rc == expect, (rc, _lib.last_error())
    _lib.check(lib.obia_synchronize(c.handle))


def judge(g, want, name):
    """the guarded output holds `want` (bit patterns), nothing around it changed, nothing in it was left as it was"""
    got = g.host()
    gb, wb = got.view(np.uint32 if want.dtype == np.float32 else want.dtype), want.view(np.uint32 if want.dtype == np.float32 else want.dtype)
    assert np.array_equal(gb, wb), f"{name}: {int((gb != wb).sum())} of {want.size} differ"
    poison = np.frombuffer(bytes([g.poison]) * want.dtype.itemsize, want.dtype)[0]
    assert g.findings(exempt=(wb == poison.view(wb.dtype)), name=name) == []


def normal(shape, seed):
    return (np.random.RandomState(seed).standard_normal(shape) * 50).astype(np.float32)


CASES = [(k, shape, p) for k in KS for shape in SHAPES for p in POISONS]
IDS = [f"k{k}-{s[0]}x{s[1]}-{p:02X}" for k, s, p in CASES]


@pytest.mark.parametrize("k,shape,poison", CASES, ids=IDS)
def test_gray_lap(k, shape, poison):
    _lib, lib, c = env()
    H, W = shape
    img = np.random.RandomState(W).rand(H, W, 5).astype(np.float32) * 900
    bands = (4, 0, 2)
    want = S.laplacian3(S.rgb_to_gray(S.normalise_bands(img[:, :, list(bands)])))
    it = dev_off(img, k)
    snap = snapshot(it)
    g = guarded((H, W), np.float32, poison, "cuda", k)
    cnt = guarded((1,), np.int64, poison, "cuda", k)
    run(_lib, lib, c, lib.obia_sharp_gray_lap_dev, it.data_ptr(), H, W, 5, (ctypes.c_int32 * 3)(*bands), g.ptr, cnt.ptr)
    judge(g, want, "gray_lap")
    judge(cnt, np.zeros(1, np.int64), "gray_lap counter")
    assert unchanged(it, snap)
    g2 = guarded((H, W), np.float32, poison, "cuda", k)                                       # without the counter
    run(_lib, lib, c, lib.obia_sharp_gray_lap_dev, it.data_ptr(), H, W, 5, (ctypes.c_int32 * 3)(*bands), g2.ptr, None)
    judge(g2, want, "gray_lap alone")
    bad = img.copy()
    bad[H - 1, W - 1, 0] = np.inf
    bad[0, 0, 1] = np.nan                                                                     # band 1 is not used
    cnt2 = guarded((1,), np.int64, poison, "cuda", k)
    run(_lib, lib, c, lib.obia_sharp_gray_lap_dev, dev_off(bad, k).data_ptr(), H, W, 5, (ctypes.c_int32 * 3)(*bands), g2.ptr, cnt2.ptr)
    judge(cnt2, np.ones(1, np.int64), "gray_lap counter of one")
    # a null output, an output one byte on (the raster is compared with nothing), a counter off its boundary: the refusals in full
    g3, b3, I = guarded((H, W), np.float32, poison, "cuda", k), (ctypes.c_int32 * 3)(*bands), it.data_ptr()
    refused_saying("sharp gray_lap: bad arguments", lib.obia_sharp_gray_lap_dev, (c.handle, I, H, W, 5, b3, None, None),
                   (c.handle, I, H, W, 5, b3, g3.ptr + 1, None), (c.handle, I + 1, H, W, 5, b3, g3.ptr, None))
    refused_saying("sharp gray_lap: nonfinite_out must be 8-byte aligned", lib.obia_sharp_gray_lap_dev, (c.handle, I, H, W, 5, b3, g3.ptr, cnt2.ptr + 4))
    assert g3.untouched()


@pytest.mark.parametrize("k,shape,poison", CASES, ids=IDS)
def test_laplacian(k, shape, poison):
    _lib, lib, c = env()
    H, W = shape
    gray = normal(shape, 10 + W)
    want = S.laplacian3(gray)
    gt = dev_off(gray, k)
    snap = snapshot(gt)
    g = guarded((H, W), np.float32, poison, "cuda", k)
    cnt = guarded((1,), np.int64, poison, "cuda", k)
    run(_lib, lib, c, lib.obia_sharp_laplacian_dev, gt.data_ptr(), H, W, g.ptr, cnt.ptr)
    judge(g, want, "laplacian")
    judge(cnt, np.zeros(1, np.int64), "laplacian counter")
    assert unchanged(gt, snap)
    g2 = guarded((H, W), np.float32, poison, "cuda", k)
    run(_lib, lib, c, lib.obia_sharp_laplacian_dev, gt.data_ptr(), H, W, g2.ptr, None)
    judge(g2, want, "laplacian alone")
    # a null output, an output one byte on, an output where the input starts: the refusal in full
    g3 = guarded((H, W), np.float32, poison, "cuda", k)
    refused_saying("sharp laplacian: bad arguments", lib.obia_sharp_laplacian_dev, (c.handle, gt.data_ptr(), H, W, None, None),
                   (c.handle, gt.data_ptr(), H, W, g3.ptr + 1, None), (c.handle, gt.data_ptr(), H, W, gt.data_ptr(), None))
    assert g3.untouched() and unchanged(gt, snap)


@pytest.mark.parametrize("k,shape,poison", CASES, ids=IDS)
def test_box(k, shape, poison):
    _lib, lib, c = env()
    H, W = shape
    plane = normal(shape, 20 + W)
    pt = dev_off(plane, k)
    snap = snapshot(pt)
    for win in (WIN[shape], 1):
        g = guarded((H, W), np.float32, poison, "cuda", k)
        work = guarded((H, W), np.float32, poison, "cuda", k)
        cnt = guarded((1,), np.int64, poison, "cuda", k)
        run(_lib, lib, c, lib.obia_sharp_box_dev, pt.data_ptr(), H, W, win, work.ptr, g.ptr, cnt.ptr)
        judge(g, S.box_filter(plane, win), f"box win {win}")
        judge(cnt, np.zeros(1, np.int64), "box counter")
        if win > 1:
            judge(work, S.uniform_filter1d(plane, win, 0), "box work plane")
        else:
            assert work.untouched() and work.findings(exempt=np.ones(shape, bool)) == []       # a copy needs no work plane
    assert unchanged(pt, snap)
    g = guarded((H, W), np.float32, poison, "cuda", k)                                        # refused: nothing is written
    work = guarded((H, W), np.float32, poison, "cuda", k)
    run(_lib, lib, c, lib.obia_sharp_box_dev, pt.data_ptr(), H, W, 0, work.ptr, g.ptr, None, expect=_lib.E_INVALID)
    run(_lib, lib, c, lib.obia_sharp_box_dev, pt.data_ptr(), H, W, _lib.SHARP_MAX_WIN + 1, work.ptr, g.ptr, None, expect=_lib.E_UNSUPPORTED)
    # a null output, an output one byte on, and each of the three pairs at one start: the refusal in full
    P = pt.data_ptr()
    refused_saying("sharp box: bad arguments", lib.obia_sharp_box_dev, (c.handle, P, H, W, 3, work.ptr, None, None),
                   (c.handle, P, H, W, 3, work.ptr, g.ptr + 1, None), (c.handle, P, H, W, 3, work.ptr, P, None), (c.handle, P, H, W, 3, P, g.ptr, None),
                   (c.handle, P, H, W, 3, g.ptr, g.ptr, None))
    assert unchanged(pt, snap)
    assert g.untouched() and work.untouched() and g.findings(exempt=np.ones(shape, bool)) == []


@pytest.mark.parametrize("k,shape,poison", CASES, ids=IDS)
def test_variance(k, shape, poison):
    _lib, lib, c = env()
    H, W = shape
    lap = normal(shape, 30 + W)
    lt = dev_off(lap, k)
    snap = snapshot(lt)
    for win in (WIN[shape], 1):
        g = guarded((H, W), np.float32, poison, "cuda", k)
        work = guarded((2, H, W), np.float32, poison, "cuda", k)
        run(_lib, lib, c, lib.obia_sharp_variance_dev, lt.data_ptr(), H, W, win, work.ptr, g.ptr)
        mean, mean2 = S.box_filter(lap, win), S.box_filter(lap * lap, win)
        judge(g, mean2 - mean * mean, f"variance win {win}")
        if win > 1:
            judge(work, np.stack([S.uniform_filter1d(lap, win, 0), S.uniform_filter1d(lap * lap, win, 0)]), "variance work planes")
        else:
            assert work.untouched()
    # a null output, an output one byte on, and each of the three pairs at one start: the refusal in full
    g, work, L = guarded((H, W), np.float32, poison, "cuda", k), guarded((2, H, W), np.float32, poison, "cuda", k), lt.data_ptr()
    refused_saying("sharp variance: bad arguments", lib.obia_sharp_variance_dev, (c.handle, L, H, W, 3, work.ptr, None),
                   (c.handle, L, H, W, 3, work.ptr + 1, g.ptr), (c.handle, L, H, W, 3, work.ptr, L), (c.handle, L, H, W, 3, L, g.ptr),
                   (c.handle, L, H, W, 3, g.ptr, g.ptr))
    assert g.untouched() and work.untouched()
    assert unchanged(lt, snap)


@pytest.mark.parametrize("k,shape,poison", CASES, ids=IDS)
def test_stretch(k, shape, poison):
    _lib, lib, c = env()
    x = normal(shape, 40 + shape[1]) ** 2
    x.flat[0] = 3.0
    lo, hi = np.percentile(x, [2, 98])
    xt = dev_off(x, k)
    snap = snapshot(xt)
    g = guarded(shape, np.float32, poison, "cuda", k)
    run(_lib, lib, c, lib.obia_sharp_stretch_f32_dev, xt.data_ptr(), x.size, float(lo), float(hi), g.ptr)
    with np.errstate(invalid="ignore", divide="ignore"):
        judge(g, np.clip((x - lo) / (hi - lo), 0, 1).astype(np.float32), "stretch")
        z = guarded(shape, np.float32, poison, "cuda", k)                                     # lo == hi: NaN at lo, 0 below, 1 above
        run(_lib, lib, c, lib.obia_sharp_stretch_f32_dev, xt.data_ptr(), x.size, 3.0, 3.0, z.ptr)
        judge(z, np.clip((x - np.float64(3.0)) / np.float64(0.0), 0, 1).astype(np.float32), "stretch lo == hi")
    assert np.isnan(z.host().flat[0])
    # a null output, an output one byte on (the input is compared with nothing): the refusal in full
    g3 = guarded(shape, np.float32, poison, "cuda", k)
    refused_saying("sharp stretch: bad arguments", lib.obia_sharp_stretch_f32_dev, (c.handle, xt.data_ptr(), x.size, 0.0, 1.0, None),
                   (c.handle, xt.data_ptr(), x.size, 0.0, 1.0, g3.ptr + 1), (c.handle, xt.data_ptr() + 1, x.size, 0.0, 1.0, g3.ptr))
    assert g3.untouched()
    assert unchanged(xt, snap)


def test_every_sharpness_entry_point_is_exercised_here_or_says_why_not():
    from obia_amd import _lib
    assert not set(EXERCISED) & set(NOT_EXERCISED)
    assert set(EXERCISED) | set(NOT_EXERCISED) == set(_lib._SHARPNESS_SIGNATURES)
    assert all(name in globals() and callable(globals()[name]) for name in EXERCISED.values())
    assert all(len(reason.split()) >= 6 and reason.rstrip().endswith(".") for reason in NOT_EXERCISED.values())
