"""obia_amd.training on the GPU against the NumPy restatement (tests/training_restatement.py), bit for bit: the Gaussian blur, the chamfer
distance (against OpenCV's two-pass sweep restated, not the closed form the kernels evaluate), darkening and the two blends, the min-max
scaling; every new entry point once through guarded outputs (tests/guarded.py, both poisons) at view offsets 1, 2 and 3
(tests/offset_views.py); tile_and_process end to end.

cv2.GaussianBlur and cv2.distanceTransform are restated from OpenCV's algorithms and are NOT compared with cv2 anywhere."""
import functools
import json
import math

import numpy as np
import pytest

from tests import training_restatement as T
from tests.guarded import POISONS, guarded, snapshot, unchanged
from tests.offset_views import offset_view, residue
from tests.refusal_text import refused_saying

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BLUR_SHAPES = ((1, 1), (2, 3), (3, 7), (9, 4), (13, 17), (70, 131))
BLUR_KERNELS = ((5, 5), (11, 11), (11, 5), (7, 31), (1, 9))


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


def judge(g, want, name, written=None):
    """the guarded output holds `want` (bit patterns) where `written` (everywhere by default), nothing around it changed, nothing in it
    was left as it was"""
    got = g.host()
    bits = np.uint32 if want.dtype == np.float32 else want.dtype
    gb, wb = got.view(bits), want.view(bits)
    if written is None:
        written = np.ones(want.shape, bool)
    assert np.array_equal(gb[written], wb[written]), f"{name}: {int((gb != wb)[written].sum())} of {int(written.sum())} differ"
    poison = np.frombuffer(bytes([g.poison]) * want.dtype.itemsize, want.dtype)[0]
    assert g.findings(exempt=(wb == poison.view(bits)) | ~written, name=name) == []
    if not written.all():
        assert (got.view(np.uint8).reshape(want.shape + (-1,))[~written] == g.poison).all(), f"{name}: written where nothing belongs"


def image_u8(shape, nch, seed):
    return np.random.RandomState(seed).randint(0, 256, tuple(shape) + ((3,) if nch == 3 else ()), dtype=np.uint8)


def random_mask(shape, density, seed):
    """uint8 plane, non-zero (255) with probability `density`"""
    return (np.random.RandomState(seed).rand(*shape) < density).astype(np.uint8) * 255


def blob_mask(shape):
    """0 / 1 canopy mask: two discs and a bar"""
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    m = ((yy - 0.4 * shape[0]) ** 2 + (xx - 0.3 * shape[1]) ** 2 < (0.22 * min(shape)) ** 2)
    m |= ((yy - 0.75 * shape[0]) ** 2 + (xx - 0.8 * shape[1]) ** 2 < (0.15 * min(shape)) ** 2)
    m |= (abs(yy - 0.9 * shape[0]) < 1.5) & (xx > 0.1 * shape[1]) & (xx < 0.6 * shape[1])
    return m.astype(np.uint8)


# ---- blur ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blur_case(shape, nch):
    img = image_u8(shape, nch, 7 * shape[0] + shape[1] + nch)
    return img, {k: T.blur_u8(img, k) for k in BLUR_KERNELS}


@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("shape", BLUR_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in BLUR_SHAPES])
def test_blur(shape, nch):
    """the small shapes have sides shorter than half the kernel; widths that are no multiple of 4 take the byte heads and tails of
    every row; 70 x 131 crosses workgroup blocks in both directions (32 rows, 256 bytes of a row)"""
    from obia_amd.training import gaussian_blur_u8
    img, want = blur_case(shape, nch)
    for k in BLUR_KERNELS:
        got = gaussian_blur_u8(img, k)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == img.shape
        assert np.array_equal(got, want[k]), (k, int((got != want[k]).sum()))
    t = gaussian_blur_u8(torch.as_tensor(img).cuda(), 5)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), T.blur_u8(img, 5))
    assert np.array_equal(gaussian_blur_u8(img, (5, 5)), gaussian_blur_u8(img, 5))


def test_blur_rows_wider_than_one_block_with_the_widest_kernel():
    from obia_amd.training import gaussian_blur_u8
    img = image_u8((37, 301), 3, 5)                                          # 903 bytes a row: four column blocks, the last ragged
    assert np.array_equal(gaussian_blur_u8(img, 31), T.blur_u8(img, 31))
    assert np.array_equal(gaussian_blur_u8(img, 1), img)


# ---- distance --------------------------------------------------------------------------------------------------------------------
def distance_planes():
    corner = np.full((40, 50), 255, np.uint8)
    corner[39, 0] = 0
    outside = np.full((9, 9), 255, np.uint8)
    outside[0, 0] = 0
    return {"no-zero": np.full((11, 13), 7, np.uint8), "all-zero": np.zeros((6, 9), np.uint8), "corner": corner,
            "half": random_mask((33, 41), 0.5, 1), "sparse": random_mask((40, 37), 0.99, 2), "row": random_mask((1, 70), 0.9, 3),
            "column": random_mask((300, 1), 0.97, 4), "one": np.full((1, 1), 1, np.uint8), "outside": outside,
            "wide": random_mask((5, 700), 0.995, 5)}


@functools.lru_cache(maxsize=None)
def distance_want(name, R):
    src = distance_planes()[name]
    return T.chamfer_sweep(src) if R is None else T.chamfer_windowed(src, R)


@pytest.mark.parametrize("R", [None, 0, 1, 3])
@pytest.mark.parametrize("name", sorted(distance_planes()))
def test_distance(name, R):
    """R = None: the full transform, against the two-pass sweep; a window: against the closed form over the zero pixels inside it"""
    from obia_amd.training import chamfer_distance
    src = distance_planes()[name]
    got = chamfer_distance(src, R)
    want = distance_want(name, R)
    assert got.dtype == np.float32 and got.shape == src.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    if name == "no-zero":
        assert (got == 8192.0).all()
    if name == "all-zero":
        assert not got.any()
    if name == "outside" and R == 3:
        assert got[4, 4] == 8192.0 and got[3, 3] == np.float32(3 * T.DG) / 65536


def test_distance_full_window_by_number_and_tensor_in_tensor_out():
    from obia_amd.training import chamfer_distance
    src = distance_planes()["corner"]
    full = distance_want("corner", None)
    assert np.array_equal(chamfer_distance(src, 49), full) and np.array_equal(chamfer_distance(src, 10 ** 6), full)
    t = chamfer_distance(torch.as_tensor(src).cuda())
    assert t.is_cuda and t.dtype == torch.float32 and np.array_equal(t.cpu().numpy(), full)
    assert full[0, 49] == np.float32(39 * T.DG + 10 * T.HV) / 65536


# ---- compose ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def compose_case():
    shape = (23, 29)
    tile, blurred = image_u8(shape, 3, 11), image_u8(shape, 3, 12)
    mask = blob_mask(shape)
    dist = T.chamfer_sweep(255 - mask * 255)
    return tile, blurred, mask, dist


def compose(tile, blurred, mask, dist, darken_factor, feather, k=0, poison=None, expect=0):
    """obia_train_compose_u8_dev on inputs at view offset k; (output, counter) as arrays, or the guarded buffers when `poison` is given"""
    from obia_amd.training import _Settings
    _lib, lib, c = env()
    H, W = mask.shape
    lut = _Settings(0.0, 0, darken_factor, False, False).darken_lut()
    ins = [dev_off(a, k) for a in (tile, blurred, mask)] + [dev_off(dist, k) if dist is not None else None, dev_off(lut, k)]
    snaps = [snapshot(t) for t in ins if t is not None]
    out = guarded((H, W, 3), np.uint8, POISONS[0] if poison is None else poison, "cuda", k)
    cnt = guarded((1,), np.int64, POISONS[0] if poison is None else poison, "cuda", 0)
    run(_lib, lib, c, lib.obia_train_compose_u8_dev, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(),
        ins[3].data_ptr() if dist is not None else None, H, W, ins[4].data_ptr(), float(feather), out.ptr, cnt.ptr, expect=expect)
    assert all(unchanged(t, s) for t, s in zip([t for t in ins if t is not None], snaps))
    return (out, cnt) if poison is not None else (out.host(), int(cnt.host()[0]))


@pytest.mark.parametrize("darken_factor", [0, 0.2, 0.8, 1])
def test_compose_hard(darken_factor):
    tile, blurred, mask, _ = compose_case()
    got, bad = compose(tile, blurred, mask, None, darken_factor, 0.0)
    assert bad == 0 and np.array_equal(got, T.blend_hard(tile, T.darken(blurred, darken_factor), mask))
    if darken_factor in (0, 1):
        assert np.array_equal(got[mask == 0], blurred[mask == 0])            # 0 skips the darkening, as the reference does


@pytest.mark.parametrize("darken_factor", [0, 0.2, 0.8, 1])
@pytest.mark.parametrize("feather", [0.5, 0.955, 3.0, 7.5])
def test_compose_feathered(feather, darken_factor):
    """0.955 puts dist == feather on the axis neighbours of the canopy: alpha is exactly 0 there"""
    tile, blurred, mask, dist = compose_case()
    got, bad = compose(tile, blurred, mask, dist, darken_factor, feather)
    want = T.blend_feather(tile, T.darken(blurred, darken_factor), dist, feather)
    assert bad == 0 and np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(got[mask == 1], tile[mask == 1])
    assert (dist == np.float32(T.HV) / 65536).any()


def test_compose_counts_mask_bytes_other_than_0_and_1_and_refuses_a_feather_of_zero():
    _lib, _, _ = env()
    tile, blurred, mask, dist = compose_case()
    odd = mask.copy()
    odd[0, 0], odd[22, 28], odd[5, 7] = 2, 255, 128
    for d, f in ((None, 0.0), (dist, 3.0)):
        assert compose(tile, blurred, odd, d, 0.8, f)[1] == 3
    out, cnt = compose(tile, blurred, mask, dist, 0.8, 0.0, poison=POISONS[0], expect=_lib.E_INVALID)
    assert out.untouched() and cnt.untouched()


def test_process_tile_refuses_a_mask_byte_of_2():
    from obia_amd.training import process_tile
    tile = np.random.RandomState(3).rand(16, 18, 3).astype(np.float32)
    mask = blob_mask((16, 18))
    mask[3, 3] = 2
    for feather in (0.0, 2.0):
        with pytest.raises(ValueError, match="1 mask values other than 0 and 1"):
            process_tile(tile, mask, feather_radius=feather)


# ---- min-max ---------------------------------------------------------------------------------------------------------------------
def test_minmax():
    from obia_amd.training import process_tile
    rs = np.random.RandomState(8)
    kw = dict(rescale=False, apply_clahe_flag=False)
    for tile in (np.full((4, 6, 3), 3.25, np.float32), (rs.standard_normal((9, 11, 3)) * 300 - 100).astype(np.float32),
                 rs.rand(3, 5, 3).astype(np.float32), rs.rand(70, 90, 3).astype(np.float32) * 4000,      # 45 values: no multiple of 4
                 np.array([[[0.0, -0.0, 1e-30]]], np.float32), np.array([[[-1e37, 1e37, 0.0]]], np.float32)):
        got = process_tile(tile, **kw)
        with np.errstate(over="ignore"):                                     # 255 * (x - min) overflows in the last tile, on both sides
            want = T.minmax_u8(tile)
        assert got.dtype == np.uint8 and np.array_equal(got, want), tile.shape
    assert T.minmax_u8(np.full((4, 6, 3), 3.25, np.float32)).max() == 0
    bad = rs.rand(9, 11, 3).astype(np.float32)
    bad[4, 5, 1] = np.nan
    with pytest.raises(ValueError, match="1 NaN or infinite"):
        process_tile(bad, **kw)
    with pytest.raises(ValueError, match="NaN"):
        process_tile(bad, rescale=True, apply_clahe_flag=False)                # as the stretch already does


# ---- buffers ---------------------------------------------------------------------------------------------------------------------
KS = (1, 2, 3)
BUFFER_CASES = [(k, p) for k in KS for p in POISONS]
BUFFER_IDS = [f"k{k}-{p:02X}" for k, p in BUFFER_CASES]


@pytest.mark.parametrize("k,poison", BUFFER_CASES, ids=BUFFER_IDS)
def test_blur_buffers(k, poison):
    from obia_amd.training import gaussian_weights
    _lib, lib, c = env()
    for shape, nch, ksize in (((13, 17), 3, (11, 5)), ((70, 131), 3, (11, 5)), ((70, 131), 1, (7, 31)), ((9, 4), 1, (5, 5))):
        img, want = blur_case(shape, nch)
        it, wx, wy = dev_off(img, k), dev_off(gaussian_weights(ksize[0]), k), dev_off(gaussian_weights(ksize[1]), k)
        snaps = [snapshot(t) for t in (it, wx, wy)]
        outs = []
        for _ in range(2):
            g = guarded(img.shape, np.uint8, poison, "cuda", k)
            run(_lib, lib, c, lib.obia_train_blur_u8_dev, it.data_ptr(), shape[0], shape[1], nch, ksize[0], ksize[1], wx.data_ptr(),
                wy.data_ptr(), g.ptr)
            judge(g, want[ksize], f"blur {shape} x {nch} {ksize}")
            outs.append(g.host())
        assert np.array_equal(outs[0], outs[1])
        assert all(unchanged(t, s) for t, s in zip((it, wx, wy), snaps))
        g = guarded(img.shape, np.uint8, poison, "cuda", k)                   # refused: nothing is written
        for bad in ((4, 5), (5, 33), (0, 5), (-1, 3)):
            run(_lib, lib, c, lib.obia_train_blur_u8_dev, it.data_ptr(), shape[0], shape[1], nch, bad[0], bad[1], wx.data_ptr(), wy.data_ptr(),
                g.ptr, expect=_lib.E_INVALID)
        run(_lib, lib, c, lib.obia_train_blur_u8_dev, it.data_ptr(), shape[0], shape[1], 2, 5, 5, wx.data_ptr(), wy.data_ptr(), g.ptr,
            expect=_lib.E_INVALID)
        # a null output, the weights (the output is of bytes) one byte on, the output where the image starts: the refusal in full
        I, X, Y = it.data_ptr(), wx.data_ptr(), wy.data_ptr()
        refused_saying("train blur: bad arguments", lib.obia_train_blur_u8_dev, (c.handle, I, shape[0], shape[1], nch, 5, 5, X, Y, None),
                       (c.handle, I, shape[0], shape[1], nch, 5, 5, X + 1, Y, g.ptr), (c.handle, I, shape[0], shape[1], nch, 5, 5, X, Y, I))
        assert g.untouched()


def row_distance(src, R):
    """pass 1: per pixel the distance along its row to the row's nearest zero pixel, capped at R + 1"""
    H, W = src.shape
    out = np.full((H, W), R + 1, np.int32)
    for y in range(H):
        zeros = np.flatnonzero(src[y] == 0)
        if len(zeros):
            out[y] = np.minimum(np.abs(np.arange(W)[:, None] - zeros[None, :]).min(1), R + 1)
    return out


@pytest.mark.parametrize("k,poison", BUFFER_CASES, ids=BUFFER_IDS)
def test_distance_buffers(k, poison):
    _lib, lib, c = env()
    for name, R in (("half", 3), ("sparse", 39), ("wide", 4096), ("column", 1), ("no-zero", 12)):
        src = distance_planes()[name]
        H, W = src.shape
        st = dev_off(src, k)
        snap = snapshot(st)
        outs = []
        for _ in range(2):
            g = guarded((H, W), np.float32, poison, "cuda", k)
            work = guarded((H, W), np.int32, poison, "cuda", k)
            run(_lib, lib, c, lib.obia_train_distance_dev, st.data_ptr(), H, W, R, work.ptr, g.ptr)
            judge(g, distance_want(name, None if R >= max(H, W) - 1 else R), f"distance {name} R {R}")
            judge(work, row_distance(src, R), f"distance work plane {name} R {R}")
            outs.append(g.host())
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
        assert unchanged(st, snap)
    g = guarded((4, 4), np.float32, poison, "cuda", k)
    work = guarded((4, 4), np.int32, poison, "cuda", k)
    run(_lib, lib, c, lib.obia_train_distance_dev, st.data_ptr(), 4, 4, -1, work.ptr, g.ptr, expect=_lib.E_INVALID)
    run(_lib, lib, c, lib.obia_train_distance_dev, st.data_ptr(), 1, _lib.TRAIN_MAX_SIDE + 1, 1, work.ptr, g.ptr, expect=_lib.E_UNSUPPORTED)
    # a null output, an output one byte on, the output where the work plane starts (the only pair compared): the refusal in full
    refused_saying("train distance: bad arguments", lib.obia_train_distance_dev, (c.handle, st.data_ptr(), 4, 4, 1, work.ptr, None),
                   (c.handle, st.data_ptr(), 4, 4, 1, work.ptr, g.ptr + 1), (c.handle, st.data_ptr(), 4, 4, 1, work.ptr + 1, g.ptr),
                   (c.handle, st.data_ptr(), 4, 4, 1, work.ptr, work.ptr))
    assert g.untouched() and work.untouched()


@pytest.mark.parametrize("k,poison", BUFFER_CASES, ids=BUFFER_IDS)
def test_compose_buffers(k, poison):
    tile, blurred, mask, dist = compose_case()
    for d, feather in ((None, 0.0), (dist, 3.0)):
        bg = T.darken(blurred, 0.8)
        want = T.blend_hard(tile, bg, mask) if d is None else T.blend_feather(tile, bg, d, feather)
        outs = []
        for _ in range(2):
            out, cnt = compose(tile, blurred, mask, d, 0.8, feather, k=k, poison=poison)
            judge(out, want, "compose")
            judge(cnt, np.zeros(1, np.int64), "compose counter")
            outs.append(out.host())
        assert np.array_equal(outs[0], outs[1])
    # a null output, the distances (the output is of bytes) one byte on, the output where the tile or the blurred tile starts: the
    # refusal in full, and nothing written
    _lib, lib, c = env()
    (H, W), lut = mask.shape, np.arange(256, dtype=np.uint8)
    t, b, m, d, lu = (dev_off(a, k).data_ptr() for a in (tile, blurred, mask, dist, lut))
    out, cnt = guarded((H, W, 3), np.uint8, poison, "cuda", k), guarded((1,), np.int64, poison, "cuda", 0)
    refused_saying("train compose: bad arguments", lib.obia_train_compose_u8_dev, (c.handle, t, b, m, d, H, W, lu, 3.0, None, cnt.ptr),
                   (c.handle, t, b, m, d + 1, H, W, lu, 3.0, out.ptr, cnt.ptr), (c.handle, t, b, m, d, H, W, lu, 3.0, t, cnt.ptr),
                   (c.handle, t, b, m, d, H, W, lu, 3.0, b, cnt.ptr))
    refused_saying("train compose: the counter must be an 8-byte aligned device pointer", lib.obia_train_compose_u8_dev,
                   (c.handle, t, b, m, d, H, W, lu, 3.0, out.ptr, cnt.ptr + 4), (c.handle, t, b, m, d, H, W, lu, 3.0, out.ptr, None))
    assert out.untouched() and cnt.untouched()


@pytest.mark.parametrize("k,poison", BUFFER_CASES, ids=BUFFER_IDS)
def test_minmax_buffers(k, poison):
    _lib, lib, c = env()
    rs = np.random.RandomState(13)
    for n in (1, 45, 256, 1000, 70001):
        x = (rs.standard_normal(n) * 50).astype(np.float32)
        xt = dev_off(x, k)
        snap = snapshot(xt)
        nparts = min(-(-n // 256), _lib.TRAIN_MINMAX_WORK // 2)
        written = np.zeros(_lib.TRAIN_MINMAX_WORK, bool)
        written[:nparts] = written[_lib.TRAIN_MINMAX_WORK // 2:_lib.TRAIN_MINMAX_WORK // 2 + nparts] = True
        outs = []
        for _ in range(2):
            g = guarded((n,), np.uint8, poison, "cuda", k)
            work = guarded((_lib.TRAIN_MINMAX_WORK,), np.float32, poison, "cuda", k)
            cnt = guarded((1,), np.int64, poison, "cuda", 0)
            run(_lib, lib, c, lib.obia_train_minmax_u8_dev, xt.data_ptr(), n, work.ptr, g.ptr, cnt.ptr)
            judge(g, T.minmax_u8(x), f"minmax n {n}")
            judge(cnt, np.zeros(1, np.int64), "minmax counter")
            parts = work.host()
            assert parts[:nparts].min() == x.min() and parts[_lib.TRAIN_MINMAX_WORK // 2:][:nparts].max() == x.max()
            judge(work, parts, "minmax work", written=written)                # no stray write; the slots beyond the partials untouched
            outs.append(g.host())
        assert np.array_equal(outs[0], outs[1])
        assert unchanged(xt, snap)
    x[5] = np.inf
    x[9] = np.nan
    cnt = guarded((1,), np.int64, poison, "cuda", 0)
    run(_lib, lib, c, lib.obia_train_minmax_u8_dev, dev_off(x, k).data_ptr(), n, work.ptr, g.ptr, cnt.ptr)
    judge(cnt, np.full(1, 2, np.int64), "minmax counter of two")
    # a null work buffer, one a byte on (the output is of bytes), one where the input starts (the only pair compared): the refusal in full
    g, cnt, X = guarded((n,), np.uint8, poison, "cuda", k), guarded((1,), np.int64, poison, "cuda", 0), xt.data_ptr()
    refused_saying("train minmax: bad arguments", lib.obia_train_minmax_u8_dev, (c.handle, X, n, None, g.ptr, cnt.ptr),
                   (c.handle, X, n, work.ptr, None, cnt.ptr), (c.handle, X, n, work.ptr + 1, g.ptr, cnt.ptr), (c.handle, X, n, X, g.ptr, cnt.ptr))
    refused_saying("train minmax: the counter must be an 8-byte aligned device pointer", lib.obia_train_minmax_u8_dev,
                   (c.handle, X, n, work.ptr, g.ptr, cnt.ptr + 4))
    assert g.untouched() and cnt.untouched()


def test_every_training_entry_point_is_exercised_by_a_buffer_test():
    from obia_amd import _lib
    exercised = {"obia_train_blur_u8_dev": test_blur_buffers, "obia_train_distance_dev": test_distance_buffers,
                 "obia_train_compose_u8_dev": test_compose_buffers, "obia_train_minmax_u8_dev": test_minmax_buffers}
    assert set(exercised) == set(_lib._TRAINING_SIGNATURES) and all(callable(f) for f in exercised.values())


# ---- one tile --------------------------------------------------------------------------------------------------------------------
def test_process_tile_variants():
    from obia_amd.training import process_tile
    rs = np.random.RandomState(21)
    tile = (rs.rand(37, 45, 3) * 3000).astype(np.float32)
    mask = blob_mask((37, 45))
    for kw in (dict(), dict(feather_radius=4.0, blur_kernel=11), dict(feather_radius=0.955, blur_kernel=(3, 7), darken_factor=0.2),
               dict(blur_kernel=0, darken_factor=0), dict(rescale=False), dict(apply_clahe_flag=False, feather_radius=7.5)):
        got = process_tile(tile, mask, **kw)
        want = T.process_tile(tile, mask, **kw)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (kw, int((got != want).sum()))
    assert np.array_equal(process_tile(tile), T.process_tile(tile))           # no mask: nothing is blurred
    assert np.array_equal(process_tile(tile, mask.astype(bool)), T.process_tile(tile, mask))
    t = process_tile(torch.as_tensor(tile).cuda(), torch.as_tensor(mask).cuda(), feather_radius=4.0)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), T.process_tile(tile, mask, feather_radius=4.0))


# ---- end to end ------------------------------------------------------------------------------------------------------------------
SHAPE, AFFINE, CRS = (98, 120, 5), [0.5, 0.0, 0.0, -0.5, 1000.0, 5000.0], "EPSG:32610"
TILING = dict(tile_size=20.0, overlap=5.0, selected_bands=(4, 2, 1))
BOXES = np.array([[1002.3, 4960.2, 1006.8, 4966.9], [1016.2, 4953.1, 1018.9, 4955.7], [1047.5, 4985.2, 1058.1, 4996.0]])
VARIANTS = {"hard": dict(), "feathered": dict(feather_radius=4, blur_kernel=11), "minmax": dict(rescale=False),
            "no-clahe": dict(apply_clahe_flag=False), "no-mask": None}


@functools.lru_cache(maxsize=None)
def scene():
    rs = np.random.RandomState(33)
    yy, xx = np.mgrid[0:SHAPE[0], 0:SHAPE[1]]
    raster = np.stack([600 + 300 * np.sin(xx / (5.0 + b)) * np.cos(yy / (7.0 + b)) + rs.normal(0, 40, SHAPE[:2]) for b in range(SHAPE[2])],
                      -1).astype(np.float32)
    mask = blob_mask(SHAPE[:2])
    return raster, mask


@functools.lru_cache(maxsize=None)
def scene_want(variant):
    raster, mask = scene()
    kw = VARIANTS[variant]
    return T.tile_and_process(raster, AFFINE, CRS, mask if kw is not None else None, BOXES, **TILING, **(kw or {}))


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_tile_and_process(variant):
    """40-pixel tiles every 30 pixels over 98 x 120: 16 tiles, the right column 30 wide, the third row 38 high, the top row 8 high"""
    from obia_amd.training import TrainingTiles, tile_and_process
    raster, mask = scene()
    kw = VARIANTS[variant]
    names, images, transforms, annotations = scene_want(variant)
    got = tile_and_process(raster, AFFINE, CRS, mask if kw is not None else None, BOXES, **TILING, **(kw or {}))
    assert isinstance(got, TrainingTiles) and len(got) == 16
    assert got.names == names == [f"img_{i:03d}.jpg" for i in range(1, 17)]
    assert got.transforms == transforms and list(got.transforms) == names
    assert got.annotations == annotations and sorted(annotations) == ["img_001", "img_002", "img_012"]
    assert [im.shape for im in got.images] == [im.shape for im in images]
    assert {im.shape for im in images} == {(40, 40, 3), (40, 30, 3), (38, 40, 3), (38, 30, 3), (8, 40, 3), (8, 30, 3)}
    for name, a, b in zip(names, got.images, images):
        assert isinstance(a, np.ndarray) and a.dtype == np.uint8 and np.array_equal(a, b), (name, int((a != b).sum()))


def test_tile_and_process_on_device_tensors_and_twice():
    from obia_amd.training import tile_and_process
    raster, mask = scene()
    _, images, transforms, annotations = scene_want("feathered")
    rt, mt = torch.as_tensor(raster).cuda(), torch.as_tensor(mask).cuda()
    runs = [tile_and_process(rt, AFFINE, CRS, mt, BOXES, **TILING, **VARIANTS["feathered"], as_array=True) for _ in range(2)]
    for got in runs:
        assert all(t.is_cuda and t.dtype == torch.uint8 for t in got.images)
        assert all(np.array_equal(t.cpu().numpy(), b) for t, b in zip(got.images, images))
        assert got.transforms == transforms and got.annotations == annotations
    assert np.array_equal(rt.cpu().numpy(), raster) and np.array_equal(mt.cpu().numpy(), mask)
    host = tile_and_process(raster, AFFINE, CRS, mask, **TILING, **VARIANTS["feathered"], as_array=True)
    assert all(t.is_cuda for t in host.images) and host.annotations is None


def test_tile_and_process_writes_its_files(tmp_path):
    from PIL import Image
    from obia_amd.training import tile_and_process
    raster, mask = scene()
    names, images, transforms, annotations = scene_want("hard")
    out = tmp_path / "tiles"
    got = tile_and_process(raster, AFFINE, CRS, mask, BOXES, str(out), **TILING)
    assert json.load(open(out / "transforms.json")) == transforms == got.transforms
    assert json.load(open(out / "annotations.json")) == annotations
    assert open(out / "transforms.json").read() == json.dumps(transforms, indent=2)
    assert sorted(p.name for p in out.iterdir()) == sorted(names + ["annotations.json", "transforms.json"])
    for name, want in zip(names, images):
        with Image.open(out / name) as im:
            assert im.format == "JPEG" and im.mode == "RGB" and im.size == (want.shape[1], want.shape[0])
    bare = tmp_path / "bare"
    tile_and_process(raster, AFFINE, CRS, None, None, str(bare), **TILING)
    assert not (bare / "annotations.json").exists() and (bare / "transforms.json").exists()


def test_tile_and_process_names_the_tile_it_refuses():
    from obia_amd.training import tile_and_process
    raster, mask = scene()
    with pytest.raises(ValueError, match=r"img_004\.jpg: apply_clahe needs at least 8 x 8 pixels.*40 x 5"):
        tile_and_process(raster[:, :95], AFFINE, CRS, mask[:, :95], **TILING)
    assert len(tile_and_process(raster[:, :95], AFFINE, CRS, mask[:, :95], **TILING, apply_clahe_flag=False).images) == 16
    odd = mask.copy()
    odd[60, 100] = 3                                                         # in tiles 4 and 8 (rows 58..97 / 28..67, columns 90..119)
    with pytest.raises(ValueError, match=r"img_004\.jpg: 1 mask values other than 0 and 1"):
        tile_and_process(raster, AFFINE, CRS, odd, **TILING)
    nan = raster.copy()
    nan[97, 0, 4] = np.nan                                                   # the bottom-left tile only
    for rescale in (True, False):
        with pytest.raises(ValueError, match=r"img_001\.jpg: .*NaN"):
            tile_and_process(nan, AFFINE, CRS, mask, **TILING, rescale=rescale)
    assert math.isnan(nan[97, 0, 4])
