"""The entry points of include/obia_image.h on buffers that start 0, 1 and 3 elements off a 16-byte boundary -- for the uint8 rasters
1 and 3 BYTES -- at widths 1, 3, 5, 64 and 67, with poisoned guards around every output (tests/offset_views.py, tests/guarded.py).
The dword stores of these kernels are chosen from the output's address and a row of 3 W bytes is rarely a multiple of four: heads and
tails are where they would go wrong.  Per case: the result equals the CPU restatement (tests/image_restatement.py) whatever the
offsets, no guard byte changed, no element left unwritten (for both poisons), the inputs byte-identical afterwards.

CLAHE refuses a side below 8 (OBIA_E_INVALID): at widths 1, 3 and 5 the test asserts the refusal and an untouched output, and runs the
smallest legal odd widths 9, 11 and 13 in their place."""
import ctypes

import numpy as np
import pytest

from tests import image_restatement as R
from tests.guarded import POISONS, guarded, snapshot, unchanged
from tests.offset_views import offset_view, residue

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KS = (0, 1, 3)
WIDTHS = (1, 3, 5, 64, 67)
H = 11

# every name of obia_amd._lib._IMAGE_SIGNATURES: the test below that runs it here, or the reason of a sentence why none does
EXERCISED = {
    "obia_image_stretch_u8_dev": "test_stretch",
    "obia_image_gray_hist_dev": "test_gray_hist",
    "obia_image_lut_u8_dev": "test_lut",
    "obia_image_clahe_u8_dev": "test_clahe",
    "obia_image_boundaries_dev": "test_boundaries",
    "obia_image_mark_u8_dev": "test_mark",
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
    """the guarded output holds `want`, nothing around it changed, nothing in it was left as it was"""
    got = g.host()
    assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} of {want.size} differ"
    poison = np.frombuffer(bytes([g.poison]) * want.dtype.itemsize, want.dtype)[0]
    assert g.findings(exempt=(want == poison), name=name) == []


def u8(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(np.uint8)


def labels(Hh, W, seed):
    rs = np.random.RandomState(seed)
    lab = (np.add.outer(np.arange(Hh) // 3, np.arange(W) // 4) % 4 - 1).astype(np.int32)       # -1, 0, 1, 2 in blocks
    lab[rs.randint(Hh), rs.randint(W)] = 77
    return lab


CASES = [(k, W, p) for k in KS for W in WIDTHS for p in POISONS]


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("k,W,poison", CASES)
def test_stretch(k, W, poison, f64):
    _lib, lib, c = env()
    x = np.random.RandomState(W).normal(500, 200, (H, W, 3)).astype(np.float64 if f64 else np.float32)
    lo, hi = np.percentile(x, (2, 98))
    want = R.rescale_to_8bit(x)
    xt = dev_off(x, k)
    snap = snapshot(xt)
    g = guarded(x.shape, np.uint8, poison, "cuda", k)
    run(_lib, lib, c, lib.obia_image_stretch_u8_dev, xt.data_ptr(), int(f64), x.size, float(lo), float(hi), g.ptr)
    judge(g, want, "stretch")
    assert unchanged(xt, snap)
    z = guarded(x.shape, np.uint8, poison, "cuda", k)                                         # lo == hi: zeros, every one written
    run(_lib, lib, c, lib.obia_image_stretch_u8_dev, xt.data_ptr(), int(f64), x.size, 3.0, 3.0, z.ptr)
    judge(z, np.zeros(x.shape, np.uint8), "stretch zeros")


@pytest.mark.parametrize("nch", [3, 1])
@pytest.mark.parametrize("k,W,poison", CASES)
def test_gray_hist(k, W, poison, nch):
    _lib, lib, c = env()
    img = u8((H, W, 3) if nch == 3 else (H, W), 100 + W)
    gray = R.rgb_to_gray(img) if nch == 3 else img
    hist = np.bincount(gray.ravel(), minlength=256).astype(np.int64)
    it = dev_off(img, k)
    snap = snapshot(it)
    gg = guarded((H, W), np.uint8, poison, "cuda", k)
    gh = guarded((256,), np.int64, poison, "cuda", k)
    run(_lib, lib, c, lib.obia_image_gray_hist_dev, it.data_ptr(), nch, H * W, gg.ptr, gh.ptr)
    judge(gg, gray, "gray")
    judge(gh, hist, "hist")
    assert unchanged(it, snap)
    gh2 = guarded((256,), np.int64, poison, "cuda", k)                                        # without the grey plane
    run(_lib, lib, c, lib.obia_image_gray_hist_dev, it.data_ptr(), nch, H * W, None, gh2.ptr)
    judge(gh2, hist, "hist alone")


@pytest.mark.parametrize("rep", [1, 3])
@pytest.mark.parametrize("k,W,poison", CASES)
def test_lut(k, W, poison, rep):
    _lib, lib, c = env()
    plane = u8((H, W), 200 + W)
    lut = u8((256,), 7)
    want = lut[plane] if rep == 1 else np.stack([lut[plane]] * 3, -1)
    pt, lt = dev_off(plane, k), dev_off(lut, k)
    snaps = snapshot(pt), snapshot(lt)
    g = guarded(want.shape, np.uint8, poison, "cuda", k)
    run(_lib, lib, c, lib.obia_image_lut_u8_dev, pt.data_ptr(), H * W, lt.data_ptr(), rep, g.ptr)
    judge(g, want, "lut")
    assert unchanged(pt, snaps[0]) and unchanged(lt, snaps[1])


@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("k,W,poison", CASES)
def test_clahe(k, W, poison, nch):
    _lib, lib, c = env()
    if W < 8:                                                                                 # refused: nothing is written
        img = u8((H, W, nch), W)
        it = dev_off(img, k)
        g = guarded(img.shape, np.uint8, poison, "cuda", k)
        run(_lib, lib, c, lib.obia_image_clahe_u8_dev, it.data_ptr(), H, W, nch, 0, g.ptr, expect=_lib.E_INVALID)
        assert g.untouched() and g.findings(exempt=np.ones(img.shape, bool)) == []
        W = {1: 9, 3: 11, 5: 13}[W]
    img = u8((H, W, nch), 300 + W)
    want = R.apply_clahe(img)
    it = dev_off(img, k)
    snap = snapshot(it)
    g = guarded(img.shape, np.uint8, poison, "cuda", k)
    for ch in range(nch):
        run(_lib, lib, c, lib.obia_image_clahe_u8_dev, it.data_ptr(), H, W, nch, ch, g.ptr)
        if ch == 0 and nch == 3:                                                              # one channel: the others are not touched
            part = g.host()
            assert np.array_equal(part[..., 0], want[..., 0]) and (part[..., 1:] == poison).all()
    judge(g, want, "clahe")
    assert unchanged(it, snap)


@pytest.mark.parametrize("k,W,poison", CASES)
def test_boundaries(k, W, poison):
    _lib, lib, c = env()
    lab = labels(H, W, W)
    want = R.find_boundaries(lab).astype(np.uint8)
    lt = dev_off(lab, k)
    snap = snapshot(lt)
    g = guarded((H, W), np.uint8, poison, "cuda", k)
    run(_lib, lib, c, lib.obia_image_boundaries_dev, lt.data_ptr(), H, W, g.ptr)
    judge(g, want, "boundaries")
    assert unchanged(lt, snap)


@pytest.mark.parametrize("nch", [3, 1])
@pytest.mark.parametrize("k,W,poison", CASES)
def test_mark(k, W, poison, nch):
    _lib, lib, c = env()
    lab = labels(H, W, 50 + W)
    img = u8((H, W, 3) if nch == 3 else (H, W), 400 + W)
    color = (255, 255, 0) if poison == POISONS[0] else (1, 128, 254)
    want = R.mark_u8(img, lab, color)
    it, lt, tt = dev_off(img, k), dev_off(lab, k), dev_off(R.mark_table(), k)
    snaps = [snapshot(t) for t in (it, lt, tt)]
    g = guarded((H, W, 3), np.uint8, poison, "cuda", k)
    run(_lib, lib, c, lib.obia_image_mark_u8_dev, it.data_ptr(), nch, lt.data_ptr(), H, W, tt.data_ptr(), (ctypes.c_uint8 * 3)(*color), g.ptr)
    judge(g, want, "mark")
    assert all(unchanged(t, s) for t, s in zip((it, lt, tt), snaps))


def test_every_image_entry_point_is_exercised_here_or_says_why_not():
    from obia_amd import _lib
    assert not set(EXERCISED) & set(NOT_EXERCISED)
    assert set(EXERCISED) | set(NOT_EXERCISED) == set(_lib._IMAGE_SIGNATURES)
    assert all(name in globals() and callable(globals()[name]) for name in EXERCISED.values())
    assert all(len(reason.split()) >= 6 and reason.rstrip().endswith(".") for reason in NOT_EXERCISED.values())
