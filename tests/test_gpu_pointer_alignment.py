"""Every operator on device buffers that do NOT start on a 16-byte boundary ("Buffer alignment").

A fresh torch allocation is aligned to 256 bytes or more, so the rest of the suite never takes the library's branches for a
misaligned base pointer: the dword kernels chosen instead of the float4 / int4 ones (band_minmax_kernel<1>, mask_pack4_kernel and
tile_mask_kernel without `vec`, ids_apply_kernel with n4 = 0), the refusal of the fused feature pass, the head and tail bytes of
count_valid_kernel, the 16-byte loads at dword alignment (features, zonal raster, rasterize vertices) and the wrapper copy of
obia_amd.cost._as_dev.  Here each operator runs once on aligned inputs -- judged against the reference its own test file uses -- and
once per offset on `offset_view`s of the same data (tests/offset_views.py), which must give

  * the SAME result as the aligned run, value for value and NaN for NaN, for every operator whose contract is bit-reproducible
    (integer or ordered sums, no floating-point atomics): everything but zonal statistics.  The operation is defined on values, not
    addresses: no tolerance;
  * for zonal statistics and moments (floating-point atomics: two aligned runs need not agree in the last bit) the bars of
    tests/zonal_reference.py against the float64 reference, exactly as tests/test_gpu_zonal_f64.py::check judges the aligned run,
    with count, min and max equal.

Offsets in elements: float32 / int32 1, 2, 3 (residues 4, 8, 12); uint8 masks 1, 2, 3, 5 (odd, even but no multiple of 4, 4 + 1);
float64 / int64 1 (residue 8).  Every test asserts the residue of a pointer it really passes: where a wrapper would copy (the cost and
seeds wrappers realign, others upload host tables), the entry point is called through ctypes.

The last test runs one aligned case of every operator on a context whose workspace two other calls have filled first: the arena
keeps its memory between calls, so an operator must write every workspace buffer before it reads it."""
import ctypes
import functools
import warnings

import numpy as np
import pytest

from tests import cost_restatement as CR
from tests import forest_restatement as fr
from tests import mlp_restatement as mr
from tests import mlp_shap_restatement as MS
from tests import rasterize_restatement as RR
from tests import seeds_restatement as SR
from tests import shap_restatement as SH
from tests import slic_stages as S
from tests.metrics import adjusted_rand_index, label_disagreement
from tests.offset_views import offset_view, residue
from tests.zonal_reference import compare, tolerances, zonal_reference

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32_OFFSETS = (1, 2, 3)          # float32 / int32: residues 4, 8, 12
U8_OFFSETS = (1, 2, 3, 5)        # masks: odd, even but no multiple of 4, 4 + 1
F64_OFFSET = 1                   # float64 / int64: residue 8


# ---- helpers ------------------------------------------------------------------------------------------------------------------
def dev(a):
    t = torch.as_tensor(np.array(a, order="C")).cuda()                 # (a writable copy: the shared inputs are read-only)
    assert t.data_ptr() % 16 == 0
    return t


def off(a, k):
    """host array -> device tensor `k` elements off a 16-byte boundary (k = 0: a fresh, aligned tensor)"""
    t = dev(a)
    if k == 0:
        return t
    v = offset_view(t, k)
    assert residue(v) == (k * t.element_size()) % 16
    return v


def misaligned(t, mod=16):
    """`t` really is off the boundary, and what the wrappers do with an input (`.to(dtype).contiguous()`) hands the same memory on"""
    assert t.is_contiguous() and t.data_ptr() % mod != 0, f"data_ptr() % {mod} = {t.data_ptr() % mod}"
    assert t.to(t.dtype).contiguous().data_ptr() == t.data_ptr()
    return t


def host(x):
    if isinstance(x, dict):
        return {k: host(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(host(v) for v in x)
    return x.cpu().numpy() if torch.is_tensor(x) else x


def same(a, b):
    """equal values and equal NaN positions"""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na], b[~nb]))


def synth(H, W, C, seed=0):
    from tests.test_gpu_tiling import synth as tiling_synth
    return tiling_synth(H, W, C, seed=seed)


def hole_mask(H, W, frac=0.3):
    """valid everywhere but a disc in the middle that hides about `frac` of the raster"""
    yy, xx = np.mgrid[0:H, 0:W]
    r2 = frac * H * W / np.pi
    return ((yy - H / 2.0) ** 2 + (xx - W / 2.0) ** 2 >= r2).astype(np.uint8)


# ---- SLIC, single raster ------------------------------------------------------------------------------------------------------
SLIC_KW = dict(n_segments=60, compactness=10.0)


@functools.lru_cache(maxsize=None)
def slic_inputs(H, W, C, masked):
    img = synth(H, W, C, seed=10 + C)
    mask = hole_mask(H, W) if masked else None
    img.setflags(write=False)
    return img, mask


@functools.lru_cache(maxsize=None)
def slic_reference(orc, H, W, C, masked):
    """(labels, labels before connectivity) of the oracle (the conftest fixture) for the case: computed once, read-only"""
    img, mask = slic_inputs(H, W, C, masked)
    lab, pre, _ = orc.slic(orc.normalize(img), mask=mask, return_all=True, **SLIC_KW)
    lab.setflags(write=False), pre.setflags(write=False)
    return lab, pre


def run_slic(img_t, mask_t, stage, ctx=None):
    """(labels on the host, feature_fused_px of the call)"""
    from obia_amd import _lib
    from obia_amd.segmentation import slic
    from tests.test_gpu_fused_features import fuse_switch
    own = ctx is None
    c = _lib.Context(0) if own else ctx
    try:
        with fuse_switch(None):
            lab = slic(img_t, mask=mask_t, _normalize_bands=True, _stage=stage, ctx=c, **SLIC_KW).cpu().numpy()
        px = c.timing()["feature_fused_px"]
    finally:
        if own:
            c.close()
    return lab, px


def check_slic_aligned(oracle, lab, H, W, C, masked, stage):
    """the aligned run against the oracle, with the bars of tests/test_gpu_parity.py and tests/test_gpu_edge_cases.py: before
    connectivity at most 1e-4 of the pixels differ (5e-4 through Lab), after it ARI >= 0.99 over all pixels; masked pixels carry 0"""
    ref, ref_pre = slic_reference(oracle, H, W, C, masked)
    _, mask = slic_inputs(H, W, C, masked)
    if masked:
        # (after connectivity a valid pixel may carry 0: the reference merges a component below min_size into a neighbour, and the
        # masked region is one -- the oracle does so at one pixel of the 3-band case)
        assert (lab[mask == 0] == 0).all() and (stage == "full" or (lab[mask != 0] > 0).all())
    if stage == "pre":
        d = label_disagreement(lab, ref_pre)
        print(f"{H}x{W}x{C} masked={masked}: {d:.2e} of the pixels differ from the oracle before connectivity")
        assert d <= (5e-4 if C == 3 else 1e-4)
    else:
        ari = adjusted_rand_index(lab, ref)
        print(f"{H}x{W}x{C} masked={masked}: ARI against the oracle {ari:.6f}")
        assert ari >= 0.99


@pytest.mark.parametrize("stage", ["pre", "full"])
@pytest.mark.parametrize("masked", [False, True], ids=["unmasked", "masked"])
@pytest.mark.parametrize("C", [4, 8, 3, 5])
def test_slic_single_raster(oracle, C, masked, stage):
    """96 x 128: C = 4 and 8 take band_minmax_kernel<4> and the float4 feature reads, C = 3 (Lab) and 5 the scalar paths; image and mask
    are offset independently.  Masked C = 4 / 8: the counter of the fused feature pass says that the dispatch really went two ways."""
    H, W = 96, 128
    img, mask = slic_inputs(H, W, C, masked)
    lab0, px0 = run_slic(dev(img), dev(mask) if masked else None, stage)
    check_slic_aligned(oracle, lab0, H, W, C, masked, stage)
    fusable = masked and C % 4 == 0
    if fusable:
        assert px0 > 0, "aligned, masked, C % 4 == 0: the fused feature pass must run"
    runs = [(k, 0) for k in F32_OFFSETS] + ([(0, k) for k in U8_OFFSETS] + [(3, 5)] if masked else [])
    for ki, km in runs:
        it = off(img, ki)
        mt = off(mask, km) if masked else None
        misaligned(it if ki else mt, 16 if ki else 4)
        lab, px = run_slic(it, mt, stage)
        assert np.array_equal(lab, lab0), f"image offset {ki}, mask offset {km}: {(lab != lab0).sum()} px differ from the aligned run"
        if fusable:
            assert (px == 0) if ki else (px > 0), f"image offset {ki}, mask offset {km}: feature_fused_px {px}"


def test_slic_row_width_no_multiple_of_four(oracle):
    """W = 127: the `W % 4` term of mask_pack4_kernel's `vec` is false at the same time as the pointer terms"""
    H, W, C = 96, 127, 4
    img, mask = slic_inputs(H, W, C, True)
    for stage in ("pre", "full"):
        lab0, px0 = run_slic(dev(img), dev(mask), stage)
        check_slic_aligned(oracle, lab0, H, W, C, True, stage)
        assert px0 > 0
        for ki, km in [(1, 0), (0, 1), (0, 2), (2, 3), (0, 5)]:
            it, mt = off(img, ki), off(mask, km)
            misaligned(it if ki else mt, 16 if ki else 4)
            lab, px = run_slic(it, mt, stage)
            assert np.array_equal(lab, lab0), f"{stage}, image offset {ki}, mask offset {km}: {(lab != lab0).sum()} px differ"
            assert (px == 0) if ki else (px > 0)


@pytest.mark.parametrize("shape", [(33, 37), (2, 4), (3, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_count_valid_heads_and_tails(shape):
    """count_valid_kernel reads 16 mask bytes per load between a head and a tail of single bytes: one run at every mask offset 0 .. 15
    on 1221 pixels (no multiple of 16) and on rasters of 8 and 15 pixels, smaller than one head.  Every valid pixel gets a label and
    no other does, and the labels are those of the aligned run."""
    H, W = shape
    img = synth(H, W, 4, seed=3)
    rs = np.random.RandomState(H)
    if H * W > 100:
        mask = hole_mask(H, W)
        mask[0, :5] = 0                                       # zeros in the head bytes, ones in the tail
        n_seg = 20
    else:
        mask = np.ones((H, W), np.uint8)
        mask.flat[rs.choice(H * W, 2, replace=False)] = 0
        mask.flat[0] = 1
        n_seg = 2
    from obia_amd.segmentation import slic
    labs = []
    for k in range(16):
        mt = off(mask, k)
        assert residue(mt) == k and mt.contiguous().data_ptr() == mt.data_ptr()
        pre = slic(dev(img), mask=mt, n_segments=n_seg, compactness=10.0, _normalize_bands=True, _stage="pre").cpu().numpy()
        assert int((pre >= 1).sum()) == int(mask.sum()), f"mask offset {k}: {int((pre >= 1).sum())} labelled pixels, mask.sum() = {int(mask.sum())}"
        assert np.array_equal(pre >= 1, mask != 0)
        labs.append(pre)
    for k in range(1, 16):
        assert np.array_equal(labs[k], labs[0]), f"mask offset {k} differs from the aligned run"


def mask_with(H, W, n_valid):
    """the holed mask of the test above with exactly `n_valid` valid pixels: pixels next to the hole are switched, the zeros in the
    head bytes and the ones in the tail stay"""
    mask = hole_mask(H, W)
    mask[0, :5] = 0
    flat = mask.reshape(-1)
    inner = np.arange(2 * W, (H - 2) * W)
    d = n_valid - int(mask.sum())
    pick = inner[flat[inner] == (0 if d > 0 else 1)][:abs(d)]
    flat[pick] = 1 if d > 0 else 0
    assert int(mask.sum()) == n_valid and not mask[0, :5].any() and mask[-1].all()
    return mask


# (valid pixels, n_segments, segments the seeding must ask the grid for): n_eff = nearbyint(n_segments * H * W / n_valid) sits next to
# a rounding point, and the seed grid of 33 x 37 changes between 99 (steps of 4: 72 seeds) and 100 (steps of 3: 132 seeds)
GRID_CASES = [(846, 69, 100),       # 69 * 1221 / 846 = 99.585: ONE pixel counted too many (847: 99.468) gives 99
              (847, 69, 99)]        # 69 * 1221 / 847 = 99.468: ONE pixel counted too few (846) gives 100


@pytest.mark.parametrize("n_valid,n_seg,n_eff", GRID_CASES, ids=[f"valid{c[0]}" for c in GRID_CASES])
def test_count_valid_decides_the_seed_grid(oracle, n_valid, n_seg, n_eff):
    """The count reaches the result through the seeding alone (n_segments scaled by the valid share, then the regular grid): here a
    count off by one in either direction changes the grid from 132 seeds to 72 or back, so that the labels before connectivity -- equal
    to the oracle's, which counts with mask.sum() -- show it.  Every mask residue 0 .. 15."""
    from obia_amd.segmentation import _slic_stages, slic
    H, W = 33, 37
    assert int(np.rint(n_seg * H * W / n_valid)) == n_eff and {int(np.rint(n_seg * H * W / (n_valid + d))) for d in (-1, 1)} == {99, 100}
    grids = {n: tuple(oracle.regular_grid(H, W, n)) for n in (99, 100)}
    assert grids[99] != grids[100]
    K_ref = len(oracle.masked_grid_centroids(mask_with(H, W, n_valid), n_seg)[0])      # the grid points on valid pixels: 91 / 48
    assert K_ref == {100: 91, 99: 48}[n_eff]
    img = synth(H, W, 4, seed=3)
    mask = mask_with(H, W, n_valid)
    kw = dict(n_segments=n_seg, compactness=10.0, _normalize_bands=True)
    _, ref_pre, _ = oracle.slic(oracle.normalize(img), mask=mask, return_all=True, n_segments=n_seg, compactness=10.0)
    for k in range(16):
        mt = off(mask, k)
        assert residue(mt) == k and mt.contiguous().data_ptr() == mt.data_ptr()
        pre = slic(dev(img), mask=mt, _stage="pre", **kw).cpu().numpy()
        assert label_disagreement(pre, ref_pre) <= 1e-4, f"mask offset {k}: {(pre != ref_pre).sum()} px differ from the oracle's labels"
        assert np.array_equal(pre >= 1, mask != 0)
        g = _slic_stages(dev(img), mask=mt, max_num_iter=1, **kw)
        assert g["K"] == K_ref, f"mask offset {k}: {g['K']} seeds, the oracle's rule gives {K_ref}"


def test_count_valid_on_a_mask_that_hides_nothing():
    """n_valid == H * W is the sweeps' licence not to read the packed mask: every residue of an all-ones mask gives the same labels"""
    from obia_amd.segmentation import slic
    H, W = 33, 37
    img, mask = synth(H, W, 4, seed=3), np.ones((H, W), np.uint8)
    labs = [slic(dev(img), mask=off(mask, k), n_segments=20, compactness=10.0, _normalize_bands=True, _stage="pre").cpu().numpy() for k in range(16)]
    assert (labs[0] >= 1).all() and all(np.array_equal(lab, labs[0]) for lab in labs)


def run_stages(img_t, mask_t, kw, ctx=None):
    from obia_amd.segmentation import _slic_stages
    return host(_slic_stages(img_t, ctx=ctx, **dict(kw, mask=mask_t)))


def test_slic_stages(oracle):
    """_slic_stages on the masked 4-band case of tests/slic_stages.py: features, seeds, centroids and labels_pre of the offset runs equal
    the aligned run's, which equals the references of tests/test_gpu_slic_stages.py (features bit for bit, the sweep at every pixel)"""
    case = next(c for c in S.FIXED_CASES if c["name"] == "mask_disc_c4")
    img, mask, seeds = S.make_inputs(case)
    kw = dict(S.slic_kwargs(case, mask, seeds), max_num_iter=case["iters"])
    a = run_stages(dev(img), dev(mask), kw)
    ref32 = S.features_ref32(oracle, img, case)
    assert np.array_equal(a["features"].view(np.uint32), ref32.view(np.uint32))
    assert a["fscale"] == S.expected_fscale(a["features"])
    ref = S.sweep_ref32(oracle, a["features"], a["centroids"], a["step"], mask=mask, ignore_color=False, start_label=case["start_label"])
    fill = case["start_label"] - 1
    valid = mask != 0
    assert (a["labels_pre"][~valid] == fill).all()
    assert not (valid & (ref != fill) & (a["labels_pre"] != ref)).any()
    for ki, km in [(k, 0) for k in F32_OFFSETS] + [(0, k) for k in U8_OFFSETS] + [(2, 3)]:
        it, mt = off(img, ki), off(mask, km)
        misaligned(it if ki else mt, 16 if ki else 4)
        b = run_stages(it, mt, kw)
        for k in ("features", "seeds_yx", "centroids", "labels_pre", "K", "step", "prescale", "fscale"):
            assert same(a[k], b[k]), f"image offset {ki}, mask offset {km}: `{k}` differs from the aligned run"


# ---- tiled driver -------------------------------------------------------------------------------------------------------------
TILED_KW = dict(tile_size=128, buffer=16, crown_radius=4, pixel_size=(1.0, 1.0), compactness=10.0)


@functools.lru_cache(maxsize=None)
def tiled_inputs():
    H = W = 256
    img = synth(H, W, 4, seed=3)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = (((yy - 120) ** 2 + (xx - 130) ** 2) < 118 ** 2).astype(np.uint8)
    img.setflags(write=False), mask.setflags(write=False)
    return img, mask


def run_tiled(img_t, mask_t, ctx=None):
    from obia_amd.tiling import create_tiled_segments
    lab, n = create_tiled_segments(img_t, input_mask=mask_t, ctx=ctx, **TILED_KW)
    return lab.cpu().numpy(), n


@functools.lru_cache(maxsize=None)
def tiled_aligned(orc):                                   # (the conftest fixture: the oracle is built)
    from oracle import tiler
    img, mask = tiled_inputs()
    ref, n_ref = tiler.create_tiled_segments(img, mask.astype(bool), **TILED_KW)
    lab, n = run_tiled(dev(img), dev(mask))
    assert n == n_ref and np.array_equal(lab, ref), f"{(lab != ref).sum()} px differ from the oracle's tiler, n {n} vs {n_ref}"
    assert (lab[mask == 0] == 0).all()
    lab.setflags(write=False)
    return lab, n


def test_tiled_segments(oracle):
    """create_tiled_segments, 256 x 256 x 4 in four tiles with an input mask: tile_mask_kernel<true> (vec4) on the aligned run,
    <false> for every misaligned mask; band_minmax_kernel<1> and no fused feature pass for every misaligned image"""
    img, mask = tiled_inputs()
    lab0, n0 = tiled_aligned(oracle)
    for ki, km in [(k, 0) for k in F32_OFFSETS] + [(0, k) for k in U8_OFFSETS]:
        it, mt = off(img, ki), off(mask, km)
        misaligned(it if ki else mt, 16 if ki else 4)
        lab, n = run_tiled(it, mt)
        assert n == n0 and np.array_equal(lab, lab0), f"image offset {ki}, mask offset {km}: {(lab != lab0).sum()} px differ, n {n} vs {n0}"


@pytest.mark.parametrize("k", F32_OFFSETS)
def test_tiled_segments_into_a_misaligned_label_raster(oracle, k):
    """obia_tiled_slic_f32_dev with labels_out off the boundary: ids_apply_kernel with n4 = 0 and tile_mask_kernel without vec4 (it
    reads the label raster four at a time)"""
    from obia_amd import _lib
    from obia_amd.segmentation import make_params
    img, mask = tiled_inputs()
    lab0, n0 = tiled_aligned(oracle)
    H, W, C = img.shape
    it, mt = dev(img), dev(mask)
    out = misaligned(offset_view(torch.full((H, W), -5, dtype=torch.int32, device="cuda"), k))
    tp = _lib.TilingParams()
    tp.tile_size, tp.buffer, tp.crown_radius, tp.pixel_width, tp.pixel_height = 128, 16, 4.0, 1.0, 1.0
    params = make_params(n_segments=0, compactness=10.0, normalize_bands=True)
    n = ctypes.c_int64(0)
    torch.cuda.synchronize()
    _lib.check(_lib.load().obia_tiled_slic_f32_dev(_lib.default_context(0).handle, it.data_ptr(), mt.data_ptr(), H, W, C, ctypes.byref(tp),
                                                   ctypes.byref(params), out.data_ptr(), ctypes.byref(n)))
    got = out.cpu().numpy()
    assert n.value == n0 and np.array_equal(got, lab0), f"labels_out offset {k}: {(got != lab0).sum()} px differ"


# ---- quickshift ---------------------------------------------------------------------------------------------------------------
QS_CASES = {"lds_48x64x3": (48, 64, 3, 3.0, 8.0), "global_40x40x5": (40, 40, 5, 2.0, 6.0)}


@functools.lru_cache(maxsize=None)
def qs_inputs(name):
    H, W, C, ks, md = QS_CASES[name]
    rs = np.random.RandomState(C * 10 + int(ks))
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([((yy // 20 + xx // 25 + c) % 3) / 2.0 for c in range(C)], -1)
    img = np.clip(base + 0.04 * rs.normal(size=base.shape), 0, 1).astype(np.float32)
    noise = np.ascontiguousarray(np.random.RandomState(11).normal(scale=0.00001, size=(H, W)), np.float64)
    return img, noise


def run_quickshift(img_t, noise_t, ks, md, ctx=None):
    """obia_quickshift_f32_dev itself: the wrapper uploads the tie noise it draws, so it never passes a misaligned one"""
    from obia_amd import _lib
    c = ctx or _lib.default_context(0)
    H, W, C = img_t.shape
    out = torch.empty((H, W), dtype=torch.int32, device="cuda")
    n = ctypes.c_int(0)
    torch.cuda.synchronize()
    _lib.check(_lib.load().obia_quickshift_f32_dev(c.handle, img_t.data_ptr(), H, W, C, 1.0, float(ks), float(md), 0.0, 0, noise_t.data_ptr(), 0,
                                                   out.data_ptr(), ctypes.byref(n)))
    return out.cpu().numpy(), n.value


@pytest.mark.parametrize("name", list(QS_CASES))
def test_quickshift(oracle, name):
    """3 bands, kernel_size 3: the LDS-staged kernel; 5 bands, kernel_size 2: the same arithmetic on global memory.  The aligned run
    against the oracle with the bars of tests/test_gpu_quickshift.py::test_quickshift_any_band_count_and_kernel_size"""
    from obia_amd.segmentation import quickshift
    H, W, C, ks, md = QS_CASES[name]
    img, noise = qs_inputs(name)
    lab0, n0 = run_quickshift(dev(img), dev(noise), ks, md)
    ref = oracle.quickshift_core(img.astype(np.float64), noise, ks, md)
    assert adjusted_rand_index(lab0, ref) >= 0.99
    assert lab0.min() == 0 and lab0.max() == n0 - 1 == len(np.unique(lab0)) - 1
    assert abs(n0 - len(np.unique(ref))) <= max(1, 0.02 * len(np.unique(ref)))
    assert np.array_equal(quickshift(img, ratio=1.0, kernel_size=ks, max_dist=md, convert2lab=False, random_seed=11), lab0)   # the wrapper's call
    for ki, kn in [(k, 0) for k in F32_OFFSETS] + [(0, F64_OFFSET), (3, F64_OFFSET)]:
        it, nt = off(img, ki), off(noise, kn)
        misaligned(it if ki else nt)
        lab, n = run_quickshift(it, nt, ks, md)
        assert n == n0 and np.array_equal(lab, lab0), f"image offset {ki}, noise offset {kn}: {(lab != lab0).sum()} px differ"


# ---- connectivity -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cc_inputs():
    rs = np.random.RandomState(21)
    H, W = 70, 90
    lab = rs.randint(1, 4, (H, W)).astype(np.int32)
    lab[30:34, :] = 0                                          # a masked band
    return lab


def run_cc(lab_t, ctx=None):
    from obia_amd.segmentation import enforce_connectivity
    out, n = enforce_connectivity(lab_t, 9, lab_t.numel() + 1, start_label=1, ctx=ctx)
    return out.cpu().numpy(), n


def test_enforce_connectivity(oracle):
    lab = cc_inputs()
    ref = oracle.enforce_connectivity(lab, 9, lab.size + 1, start_label=1)
    out0, n0 = run_cc(dev(lab))
    assert np.array_equal(out0, ref) and n0 == len(np.unique(ref[ref > 0]))
    for k in F32_OFFSETS:
        out, n = run_cc(misaligned(off(lab, k)))
        assert n == n0 and np.array_equal(out, out0), f"labels offset {k}: {(out != out0).sum()} px differ"


# ---- zonal statistics and moments ---------------------------------------------------------------------------------------------
ZONAL_CASES = ["dispatch_C3_all", "dispatch_C4_all", "dispatch_C8_all", "shape_37x129"]


@functools.lru_cache(maxsize=None)
def zonal_case(name):
    from tests.test_gpu_zonal_f64 import CASES
    case = CASES[name]()
    ref = zonal_reference(case["raw"], case["lab"], bands=case.get("bands"), start_label=case.get("start_label", 1), n_labels=case.get("n_labels"))
    assert not ref["near_threshold"].any()
    return case, ref, tolerances(ref)


def run_zonal(raw_t, lab_t, case, moments, ctx=None):
    from obia_amd.statistics import zonal_stats
    return host(zonal_stats(raw_t, lab_t, bands=case.get("bands"), start_label=case.get("start_label", 1), n_labels=case.get("n_labels"),
                            moments=moments, ctx=ctx))


def judge_zonal(st, ref, tol, moments, tag):
    bad = compare(st, ref, tol, moments=moments)
    assert not bad, (tag, bad)


@pytest.mark.parametrize("name", ZONAL_CASES)
def test_zonal(name):
    """z_v3f / z_v4f: 12 and 16 bytes per lane at dword alignment (C = 3: every second pixel of an aligned raster is off the boundary
    already; with an offset base no lane is on it).  Raw and labels offset independently."""
    case, ref, tol = zonal_case(name)
    raw, lab = case["raw"], case["lab"]
    first = {}
    for moments in (False, True):
        first[moments] = run_zonal(dev(raw), dev(lab), case, moments)
        judge_zonal(first[moments], ref, tol, moments, f"{name}: aligned, moments {moments}")
    for kr, kl in [(k, 0) for k in F32_OFFSETS] + [(0, k) for k in F32_OFFSETS] + [(3, 1)]:
        rt, lt = off(raw, kr), off(lab, kl)
        misaligned(rt if kr else lt)
        for moments in (False, True):
            st = run_zonal(rt, lt, case, moments)
            tag = f"{name}: raw offset {kr}, labels offset {kl}, moments {moments}"
            judge_zonal(st, ref, tol, moments, tag)
            for k in ("count", "min", "max"):
                assert same(st[k], first[moments][k]), f"{tag}: `{k}` differs from the aligned run"


# ---- texture ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def texture_inputs(name):
    """the inputs of tests/test_gpu_texture_cases.py::test_thin_strips, and of test_bbox_4096_4097[(65, 63)]: the dense path"""
    from tests.test_gpu_texture_cases import bbox_inputs, thin_strips_inputs
    return thin_strips_inputs() if name == "thin_strips" else bbox_inputs(65, 63)


def run_texture(raw_t, lab_t, ctx=None):
    from obia_amd.statistics import texture_stats
    tx = texture_stats(raw_t, lab_t, ctx=ctx)
    return {k: v.cpu().numpy() for k, v in tx.items() if k != "bands"}


@pytest.mark.parametrize("name", ["thin_strips", "dense_65x63"])
def test_texture(name):
    from oracle.glcm import PROPS
    from tests.test_gpu_texture_cases import texture_reference
    raw, lab = texture_inputs(name)
    ref = texture_reference(raw, lab)
    tx0 = run_texture(dev(raw), dev(lab))
    for p in PROPS:
        assert np.array_equal(np.isnan(tx0[p]), np.isnan(ref[p])), p
        np.testing.assert_allclose(tx0[p], ref[p], rtol=1e-9, atol=1e-12, equal_nan=True, err_msg=p)
    for kr, kl in [(k, 0) for k in F32_OFFSETS] + [(0, k) for k in F32_OFFSETS] + [(1, 3)]:
        rt, lt = off(raw, kr), off(lab, kl)
        misaligned(rt if kr else lt)
        tx = run_texture(rt, lt)
        assert same(tx, tx0), f"{name}: raw offset {kr}, labels offset {kl}: differs from the aligned run"


# ---- polygon rings and rasterize ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def polygon_map(case):
    """the "donut" and "salt" maps of tests/test_gpu_polygons.py::test_rings_equal_the_oracle_on_small_maps"""
    from tests.test_gpu_polygons import small_map
    return small_map(case)


def run_polygons(lab_t, start, ctx=None):
    from obia_amd.polygons import polygonize
    from tests.test_gpu_polygons import rings_as_tuples
    return rings_as_tuples(polygonize(lab_t, start_label=start, ctx=ctx))


@pytest.mark.parametrize("case", ["donut", "salt"])
def test_polygon_rings(case):
    from tests.test_gpu_polygons import oracle_grouped
    lab, start = polygon_map(case)
    rings0 = run_polygons(dev(lab), start)
    assert rings0 == oracle_grouped(lab, start)
    for k in F32_OFFSETS:
        assert run_polygons(misaligned(off(lab, k)), start) == rings0, f"labels offset {k}"


@functools.lru_cache(maxsize=None)
def raster_shapes():
    """small shapes of every kind of tests/test_gpu_rasterize.py and one rectangle a row taller than the one-wave path takes"""
    from obia_amd.polygons import rasterize_info
    from tests.test_gpu_rasterize import _random_shapes
    H, W = 100, 100
    shapes, values = _random_shapes(4, H, W, 60)
    side = rasterize_info()["max_side"]
    shapes = shapes[:30] + [[RR.rect(10.2, 5.2, 30.2, 5.2 + side + 1)]] + shapes[30:]
    values = np.concatenate([values[:30], [77], values[30:]]).astype(np.int32)
    xy, ring_off, owner = RR.pack(shapes)
    want = RR.burn(xy, ring_off, owner, values, (H, W), fill=-7)
    return (H, W), xy, ring_off, owner, values, want


def run_rasterize(xy_t, off_t, owner_t, val_t, shape, ctx=None):
    """obia_rasterize_polygons_dev itself (the wrapper uploads the ring tables it has checked on the host); returns the raster and the
    (small, large) counts of obia_rasterize_info"""
    from obia_amd import _lib
    from obia_amd.polygons import rasterize_info
    c = ctx or _lib.default_context(0)
    H, W = shape
    out = torch.empty((H, W), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.load().obia_rasterize_polygons_dev(c.handle, xy_t.data_ptr(), off_t.data_ptr(), owner_t.numel(), owner_t.data_ptr(),
                                                       val_t.data_ptr(), val_t.numel(), H, W, -7, out.data_ptr()))
    _lib.check(_lib.load().obia_synchronize(c.handle))
    info = rasterize_info()
    return out.cpu().numpy(), (info["small"], info["large"])


def test_rasterize():
    """xy_pix is read as double2 at 8-byte alignment; ring_offset (int64), ring_shape and shape_value are offset too"""
    from obia_amd.polygons import rasterize, rasterize_info
    shape, xy, ring_off, owner, values, want = raster_shapes()
    got = rasterize((xy, ring_off, owner), shape, values=values, fill=-7)
    info = rasterize_info()
    assert np.array_equal(got, want) and (info["small"], info["large"]) == (60, 1) and (want == 77).sum() > 500
    out0, info0 = run_rasterize(dev(xy), dev(ring_off), dev(owner), dev(values), shape)
    assert np.array_equal(out0, want) and info0 == (60, 1)
    for kx, ko, ks, kv in [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 1, 1, 1), (1, 1, 2, 3), (0, 0, 3, 2)]:
        ts = off(xy, kx), off(ring_off, ko), off(owner, ks), off(values, kv)
        misaligned(next(t for t, k in zip(ts, (kx, ko, ks, kv)) if k))
        out, info = run_rasterize(*ts, shape)
        assert np.array_equal(out, out0) and info == info0, f"offsets xy {kx}, ring_offset {ko}, ring_shape {ks}, shape_value {kv}"


# ---- consumers ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_labels():
    """9 x 1030 random labels in 0 .. 2: label_edges_kernel strides the columns by 1024 per trip, so its column loop makes a second
    trip here, and that trip has a partial four-wide group"""
    return np.random.RandomState(5).randint(0, 3, (9, 1030)).astype(np.int32)


def run_edges(lab_t, ctx=None):
    from obia_amd.consumers import slic_edge
    return slic_edge(lab_t, ctx=ctx).cpu().numpy()


def test_slic_edge():
    from oracle.consumers import edge_raster
    lab = edge_labels()
    e0 = run_edges(dev(lab))
    assert e0.dtype == np.float32 and np.array_equal(e0, edge_raster(lab).astype(np.float32))
    for k in F32_OFFSETS:
        assert np.array_equal(run_edges(misaligned(off(lab, k))), e0), f"labels offset {k}"


SHEAR = [0.5, 0.5, 0.0, -0.5, 1000.0, 2000.0]    # x' = 0.5 x + 0.5 y + 1000, y' = -0.5 y + 2000: sheared, and its inverse is exact


@functools.lru_cache(maxsize=None)
def sample_inputs():
    """1000 points (four workgroups) given in pixel coordinates on a grid of eighths, so that the map coordinates and the inverse
    transform are exact: the first ones sit on pixel corners, on the right and bottom edges and at negative coordinates in (-1, 0)"""
    H, W = 40, 60
    rs = np.random.RandomState(8)
    lab = rs.randint(1, 500, (H, W)).astype(np.int32)
    special = [(0.0, 0.0), (7.0, 3.0), (59.0, 39.0), (60.0, 10.0), (10.0, 40.0), (60.0, 40.0), (59.875, 39.875), (-0.5, 5.0), (5.0, -0.125),
               (-0.875, -0.875), (-0.125, 39.5), (59.5, -0.5), (-1.0, 3.0), (3.0, -1.0), (12.0, 0.0), (0.0, 17.0)]
    cr = np.concatenate([np.array(special), np.round(rs.uniform(-1.5, [W + 1.5, H + 1.5], (1000 - len(special), 2)) * 8) / 8])
    col, row = cr[:, 0], cr[:, 1]
    Y = (4000.0 - row) / 2.0                                   # row = -2 Y + 4000
    X = (col + 6000.0 - 2.0 * Y) / 2.0                         # col = 2 X + 2 Y - 6000
    pts = np.ascontiguousarray(np.stack([X, Y], 1))
    return lab, pts, col, row


def sample_restatement(lab, pts, outside):
    """floor(a X + b Y + xoff), products and sums rounded one by one in float64 (the library is built with -ffp-contract=off)"""
    from obia_amd.consumers import invert_affine
    a, b, d, e, xoff, yoff = invert_affine(SHEAR)
    X, Y = pts[:, 0], pts[:, 1]
    col = np.floor((a * X + b * Y) + xoff)
    row = np.floor((d * X + e * Y) + yoff)
    H, W = lab.shape
    ok = (col >= 0) & (col < W) & (row >= 0) & (row < H)
    out = np.full(len(pts), outside, np.int32)
    out[ok] = lab[row[ok].astype(np.int64), col[ok].astype(np.int64)]
    return out


def run_sample(lab_t, pts_t, ctx=None):
    """obia_sample_labels_i32_dev itself (the wrapper uploads the points)"""
    from obia_amd import _lib
    from obia_amd.consumers import invert_affine
    c = ctx or _lib.default_context(0)
    H, W = lab_t.shape
    n = pts_t.shape[0]
    out = torch.full((n,), -9, dtype=torch.int32, device="cuda")
    inv = (ctypes.c_double * 6)(*invert_affine(SHEAR))
    torch.cuda.synchronize()
    _lib.check(_lib.load().obia_sample_labels_i32_dev(c.handle, lab_t.data_ptr(), H, W, inv, pts_t.data_ptr(), n, -9, out.data_ptr()))
    return out.cpu().numpy()


def test_sample_labels():
    from obia_amd.consumers import invert_affine, sample_labels
    lab, pts, col, row = sample_inputs()
    assert invert_affine(SHEAR) == [2.0, 2.0, -0.0, -2.0, -6000.0, 4000.0]
    want = sample_restatement(lab, pts, -9)
    H, W = lab.shape
    inside = (col >= 0) & (col < W) & (row >= 0) & (row < H)    # ... which is the pixel the point was drawn in
    assert np.array_equal(want[inside], lab[np.floor(row[inside]).astype(int), np.floor(col[inside]).astype(int)]) and (want[~inside] == -9).all()
    assert inside[:3].all() and not inside[3:6].any() and inside[6] and not inside[7:14].any() and inside[14:16].all()
    assert 300 < inside.sum() < 1000
    assert np.array_equal(sample_labels(lab, SHEAR, pts, outside=-9), want)
    out0 = run_sample(dev(lab), dev(pts))
    assert np.array_equal(out0, want)
    for kl, kp in [(k, 0) for k in F32_OFFSETS] + [(0, F64_OFFSET), (2, F64_OFFSET)]:
        lt, pt = off(lab, kl), off(pts, kp)
        misaligned(lt if kl else pt)
        assert np.array_equal(run_sample(lt, pt), want), f"labels offset {kl}, points offset {kp}"


# ---- cost surface -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cost_scene():
    from tests.test_gpu_cost_surface import _scene
    return _scene(33, 129, 5)


COST_WEIGHTS = (0.4, 0.3, 0.2, 0.1)


def cost_tensors(k):
    """(wv3, chm, labels, pan, red, nir) on the device, each `k` elements off a 16-byte boundary; pan / red / nir are the C, R and N1
    bands as contiguous planes of their own, so that the layer functions get the very pointer the test checks (a strided band slice
    would be copied to a fresh, aligned tensor by `.contiguous()` before the realigning branch is reached)"""
    wv3, chm, lab = cost_scene()
    planes = [np.ascontiguousarray(wv3[:, :, b]) for b in (0, 4, 6)]
    return tuple(off(a, k) for a in [wv3, chm, lab] + planes)


def run_cost_layers(wv3_t, chm_t, lab_t, pan_t, red_t, nir_t, ctx=None, seen=None):
    """every layer function and make_cost_surface; `seen`: a dict that receives, per function, the residues of the inputs that
    cost._as_dev had to move to an aligned buffer"""
    from obia_amd import cost
    calls = {"normalise": lambda: cost.normalise(chm_t, ctx=ctx), "chm_gradient": lambda: cost.chm_gradient(chm_t, ctx=ctx),
             "chm_gradient_raw": lambda: cost.chm_gradient(chm_t, ctx=ctx, _raw=True), "ndvi": lambda: cost.ndvi(red_t, nir_t, ctx=ctx),
             "texture_entropy": lambda: cost.texture_entropy(pan_t, ctx=ctx),
             "cost": lambda: cost.make_cost_surface(wv3_t, chm_t, slic=lab_t, weights=COST_WEIGHTS, ctx=ctx)}
    as_dev, out = cost._as_dev, {}

    def spy(x, dtype, dev_index):
        t = as_dev(x, dtype, dev_index)
        assert t.data_ptr() % 16 == 0 and t.is_contiguous()
        if torch.is_tensor(x) and x.is_contiguous() and x.dtype == dtype and t.data_ptr() != x.data_ptr():
            moved.append(x.data_ptr() % 16)
        return t
    cost._as_dev = spy
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for name, call in calls.items():
                moved = []
                out[name] = host(call())
                if seen is not None:
                    seen[name] = moved
    finally:
        cost._as_dev = as_dev
    return out


def test_cost_layers_realign_a_misaligned_input():
    """Every layer function and make_cost_surface on 33 x 129 inputs at residue 4 (and 8, 12): each of their inputs is a contiguous
    tensor whose residue is asserted, the wrapper's realigning copy (cost._as_dev) is seen to move every one of them, and the results
    are those of the aligned call, which are the restatement's bit for bit (tests/test_gpu_cost_surface.py)"""
    from tests.test_gpu_cost_surface import _same
    wv3, chm, lab = cost_scene()
    seen = {}
    a = run_cost_layers(*cost_tensors(0), seen=seen)
    assert all(m == [] for m in seen.values()), seen          # aligned inputs are passed on as they are
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = {"normalise": CR.normalise(chm), "chm_gradient": CR.chm_gradient(chm), "chm_gradient_raw": CR.hypot_plane(chm),
                "ndvi": CR.ndvi(np.ascontiguousarray(wv3[:, :, 4]), np.ascontiguousarray(wv3[:, :, 6])),
                "texture_entropy": CR.texture_entropy(np.ascontiguousarray(wv3[:, :, 0])), "cost": CR.make_cost_surface(wv3, chm, lab, COST_WEIGHTS)}
    for k in want:
        _same(a[k], want[k])
    inputs = {"normalise": 1, "chm_gradient": 1, "chm_gradient_raw": 1, "ndvi": 2, "texture_entropy": 1, "cost": 3}
    for k in F32_OFFSETS:
        ts = cost_tensors(k)
        for t in ts:
            misaligned(t)
            assert residue(t) == 4 * k
        seen = {}
        b = run_cost_layers(*ts, seen=seen)
        for name in want:
            assert seen[name] == [4 * k] * inputs[name], f"{name}, offset {k}: inputs moved by the wrapper (their residues): {seen[name]}"
            _same(b[name], a[name])


def test_cost_entry_points_refuse_a_misaligned_plane():
    """obia_cost_bands_f32_dev and obia_cost_select_dev read 16 bytes per lane and name the alignment in the header: a plane off the
    boundary is OBIA_E_INVALID, nothing is launched, and the context stays good"""
    from obia_amd import _lib
    lib, c = _lib.load(), _lib.default_context(0)
    wv3, chm, _ = cost_scene()
    H, W = chm.shape
    pan = torch.empty((H, W), dtype=torch.float32, device="cuda")
    gap = torch.empty_like(pan)
    n, bits = ctypes.c_int64(0), (ctypes.c_uint64 * 4)()
    torch.cuda.synchronize()
    for k in F32_OFFSETS:
        wt, ct = misaligned(off(wv3, k)), misaligned(off(chm, k))
        assert lib.obia_cost_bands_f32_dev(c.handle, wt.data_ptr(), H * W, pan.data_ptr(), gap.data_ptr()) == _lib.E_INVALID
        assert lib.obia_cost_select_dev(c.handle, ct.data_ptr(), 0, H * W, 0.02, 0.98, ctypes.byref(n), bits) == _lib.E_INVALID
    c64 = misaligned(off(chm.astype(np.float64), F64_OFFSET))
    assert lib.obia_cost_select_dev(c.handle, c64.data_ptr(), 1, H * W, 0.02, 0.98, ctypes.byref(n), bits) == _lib.E_INVALID
    wt, ct = dev(wv3), dev(chm)
    assert lib.obia_cost_bands_f32_dev(c.handle, wt.data_ptr(), H * W, pan.data_ptr(), gap.data_ptr()) == _lib.OBIA_OK
    assert lib.obia_cost_select_dev(c.handle, ct.data_ptr(), 0, H * W, 0.02, 0.98, ctypes.byref(n), bits) == _lib.OBIA_OK
    assert n.value == int((~np.isnan(chm)).sum())
    _lib.check(lib.obia_synchronize(c.handle))
    assert np.array_equal(pan.cpu().numpy(), wv3[:, :, 0])


# ---- seeds --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def peak_plane():
    from tests.test_gpu_seeds import surface
    return surface(50 * 1000 + 70, 50, 70)


def run_peaks(plane_t, ctx=None, v_min=12.0, d=3, sigma=1.0):
    """obia_seeds_peaks_dev + obia_seeds_peaks_gather_dev themselves, as obia_amd.seeds.detect_peaks calls them (the wrapper realigns
    its plane): (rows, cols, smoothed value, raw value, smoothed plane)"""
    from obia_amd import _lib, seeds
    lib = _lib.load()
    c = ctx or _lib.default_context(0)
    H, W = plane_t.shape
    nchunks = -(-(H * W) // seeds._CHUNK)
    i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
    smooth = torch.empty((H, W), **f32)
    flags = torch.empty(nchunks * seeds._CHUNK, dtype=torch.uint8, device="cuda")
    offsets = torch.empty(nchunks + 1, **i32)
    count = ctypes.c_int64(0)
    torch.cuda.synchronize()
    _lib.check(lib.obia_seeds_peaks_dev(c.handle, plane_t.data_ptr(), H, W, float(sigma), int(d), float(np.float32(v_min)), smooth.data_ptr(),
                                        flags.data_ptr(), offsets.data_ptr(), ctypes.byref(count)))
    k = int(count.value)
    rows, cols, gval, rval = torch.empty(k, **i32), torch.empty(k, **i32), torch.empty(k, **f32), torch.empty(k, **f32)
    _lib.check(lib.obia_seeds_peaks_gather_dev(c.handle, plane_t.data_ptr(), smooth.data_ptr(), flags.data_ptr(), offsets.data_ptr(), H, W, k,
                                               rows.data_ptr(), cols.data_ptr(), gval.data_ptr(), rval.data_ptr()))
    _lib.check(lib.obia_synchronize(c.handle))
    return host((rows, cols, gval, rval, smooth))


def test_seed_peaks():
    from obia_amd.seeds import detect_peaks
    a = peak_plane()
    p0 = run_peaks(dev(a))
    wr, wc = np.where(SR.peaks_scipy(a, 12.0, 3, 1))
    ref_g = SR.smooth(a, 1)
    assert len(wr) > 0 and np.array_equal(p0[0], wr) and np.array_equal(p0[1], wc)
    assert np.array_equal(p0[4], ref_g) and np.array_equal(p0[2], ref_g[wr, wc]) and np.array_equal(p0[3], a[wr, wc])
    assert same(detect_peaks(a, 12.0, 3, 1, _smooth=True), p0)                   # the wrapper's call
    for k in F32_OFFSETS:
        assert same(run_peaks(misaligned(off(a, k))), p0), f"plane offset {k}"


def test_seed_entry_points_refuse_a_misaligned_flag_plane():
    """The flag plane is read 16 bytes per lane and the header names its alignment: obia_seeds_peaks_dev and
    obia_seeds_peaks_gather_dev answer OBIA_E_INVALID to one off the boundary (the wrapper allocates it itself), launch nothing, and
    the same calls with the aligned plane go through"""
    from obia_amd import _lib, seeds
    lib, c = _lib.load(), _lib.default_context(0)
    a = peak_plane()
    H, W = a.shape
    nchunks = -(-(H * W) // seeds._CHUNK)
    plane = dev(a)
    i32, f32 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.float32, device="cuda")
    smooth, offsets = torch.empty((H, W), **f32), torch.empty(nchunks + 1, **i32)
    flags = torch.zeros(nchunks * seeds._CHUNK + 16, dtype=torch.uint8, device="cuda")
    rows, cols, gval, rval = torch.empty(64, **i32), torch.empty(64, **i32), torch.empty(64, **f32), torch.empty(64, **f32)
    count = ctypes.c_int64(-1)
    torch.cuda.synchronize()

    def peaks(fl):
        return lib.obia_seeds_peaks_dev(c.handle, plane.data_ptr(), H, W, 1.0, 3, 12.0, smooth.data_ptr(), fl.data_ptr(), offsets.data_ptr(),
                                        ctypes.byref(count))

    def gather(fl, k):
        return lib.obia_seeds_peaks_gather_dev(c.handle, plane.data_ptr(), smooth.data_ptr(), fl.data_ptr(), offsets.data_ptr(), H, W, k,
                                               rows.data_ptr(), cols.data_ptr(), gval.data_ptr(), rval.data_ptr())
    for k in (1, 4, 8, 15):
        fl = flags[k:k + nchunks * seeds._CHUNK]
        assert fl.is_contiguous() and residue(fl) == k
        assert peaks(fl) == _lib.E_INVALID and count.value == -1
        assert gather(fl, 0) == _lib.E_INVALID
    fl = flags[:nchunks * seeds._CHUNK]
    assert residue(fl) == 0 and peaks(fl) == _lib.OBIA_OK
    n = int(SR.peaks_scipy(a, 12.0, 3, 1).sum())
    assert count.value == n and 0 < n <= 64
    assert gather(fl, n) == _lib.OBIA_OK
    _lib.check(lib.obia_synchronize(c.handle))
    wr, wc = np.where(SR.peaks_scipy(a, 12.0, 3, 1))
    assert np.array_equal(rows[:n].cpu().numpy(), wr) and np.array_equal(cols[:n].cpu().numpy(), wc)


@functools.lru_cache(maxsize=None)
def pair_inputs():
    from tests.test_seeds_restatement_cpu import WEIGHT, XY_THRESH
    xs, ys, cost, aff = SR.pixel_centre_case(65, 65, 40, 50, 1.0)
    return np.ascontiguousarray(xs, np.float64), np.ascontiguousarray(ys, np.float64), cost, SR.inverse6(aff), WEIGHT, XY_THRESH


def run_pairs(xs_t, ys_t, cost_t, ctx=None):
    """obia_seeds_pair_matrix_dev through the wrapper's own call helper (pair_distances realigns its inputs first)"""
    from obia_amd import _lib, seeds
    _, _, _, inv, weight, thresh = pair_inputs()
    c = ctx or _lib.default_context(0)
    D = torch.empty((xs_t.numel(), xs_t.numel()), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _lib.check(seeds._pair_call(_lib.load().obia_seeds_pair_matrix_dev, c, xs_t, ys_t, cost_t, inv, weight, thresh, 12, D.data_ptr()))
    _lib.check(_lib.load().obia_synchronize(c.handle))
    return D.cpu().numpy()


def test_seed_pair_matrix():
    from obia_amd.seeds import pair_distances
    xs, ys, cost, inv, weight, thresh = pair_inputs()
    want = SR.distance_matrix(xs, ys, cost, inv, weight, thresh, 12)
    D0 = run_pairs(dev(xs), dev(ys), dev(cost))
    assert D0.dtype == np.float32 and np.array_equal(D0, want, equal_nan=True)
    assert same(pair_distances(xs, ys, cost, inv, weight, thresh, 12), D0)
    for kx, ky, kc in [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 2), (0, 0, 3), (1, 1, 3)]:
        ts = off(xs, kx), off(ys, ky), off(cost, kc)
        misaligned(next(t for t, k in zip(ts, (kx, ky, kc)) if k))
        assert same(run_pairs(*ts), D0), f"offsets xs {kx}, ys {ky}, cost {kc}"


# ---- classification -----------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def run_scale(table_t, wide, ctx=None):
    from obia_amd.classify import standard_scale
    return host(standard_scale(table_t, ctx=ctx, dtype=np.float64 if wide else np.float32))


@pytest.mark.parametrize("wide", [False, True], ids=["float32", "float64"])
def test_table_scale(wide):
    """obia_table_scale_dev / obia_table_scale_f64_dev on fixture "a" with the table one float64 off the boundary.  The aligned run
    against the exactly rounded column sums with the bounds of tests/test_gpu_classify.py::test_standard_scale"""
    from tests.test_gpu_classify import exact_columns
    c = fr.load_case("a")
    table = c["table"]
    X, mean, scale = run_scale(dev(table), wide)
    n, m_ref, v_ref, mabs = exact_columns(table)
    empty, const = n == 0, c["scale_"] == 1.0
    live = ~empty
    reg = live & ~const
    assert np.isnan(mean[empty]).all() and np.isnan(scale[empty]).all() and (scale[const] == 1.0).all()
    assert (np.abs(mean[live] - m_ref[live]) <= n[live] * 2.0 ** -52 * mabs[live]).all()
    s_ref = np.sqrt(v_ref[reg])
    assert (np.abs(scale[reg] - s_ref) <= (n[reg] * 2.0 ** -51 + 2.0 ** -52) * s_ref).all()
    with np.errstate(invalid="ignore"):
        want = ((table - mean) / scale).astype(X.dtype)
    assert X.dtype == (np.float64 if wide else np.float32) and same(X, want)
    got = run_scale(misaligned(off(table, F64_OFFSET)), wide)
    assert same(got, (X, mean, scale))


def forest_abi(c, k, x_t, acc_t=None, shap=False):
    """obia_forest_predict_dev / obia_forest_shap_dev with an obia_forest struct filled here: `threshold`, `value` (and `cover`) lie
    `k` float64 off the boundary.  `c`: the flat arrays of a fixture.  Returns what the wrappers return, on the host."""
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.default_context(0)
    t = {n: off(np.ascontiguousarray(c[n]), k if n in ("threshold", "value") else 0) for n in fr.ARRAYS}
    if k:
        assert residue(misaligned(t["threshold"])) == residue(misaligned(t["value"])) == 8
    tree_offset = np.ascontiguousarray(c["tree_offset"], np.int64)
    N, F = x_t.shape
    K = c["value"].shape[1]
    fs = _lib.Forest(*(t[n].data_ptr() for n in fr.ARRAYS[:6]), tree_offset.ctypes.data, t["value"].data_ptr(), len(c["threshold"]),
                     len(tree_offset), K)
    f64 = dict(dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    if shap:
        cover = off(np.ascontiguousarray(c["cover"], np.float64), k)
        phi, base = torch.empty((N, F, K), **f64), torch.empty((K,), **f64)
        _lib.check(lib.obia_forest_shap_dev(ctx.handle, x_t.data_ptr(), N, F, ctypes.byref(fs), cover.data_ptr(), phi.data_ptr(), base.data_ptr()))
        out = (phi, base)
    else:
        proba, pred, margin = torch.empty((N, K), **f64), torch.empty((N,), dtype=torch.int32, device="cuda"), torch.empty((N,), **f64)
        _lib.check(lib.obia_forest_predict_dev(ctx.handle, x_t.data_ptr(), N, F, ctypes.byref(fs), None if acc_t is None else acc_t.data_ptr(),
                                               proba.data_ptr(), pred.data_ptr(), margin.data_ptr()))
        out = (pred, margin, proba)
    _lib.check(lib.obia_synchronize(ctx.handle))
    return host(out)


def mlp_struct(c, k):
    """(obia_mlp, the tensors it points to): `weights` and `biases` `k` float64 off the boundary"""
    from obia_amd import _lib
    from obia_amd.classify import _HIDDEN_ACTIVATIONS, _OUT_ACTIVATIONS
    keep = [off(np.ascontiguousarray(c["weights"], np.float64), k), off(np.ascontiguousarray(c["biases"], np.float64), k),
            np.ascontiguousarray(c["layer_sizes"], np.int32)]
    if k:
        assert residue(misaligned(keep[0])) == residue(misaligned(keep[1])) == 8
    ms = _lib.Mlp(keep[0].data_ptr(), keep[1].data_ptr(), keep[2].ctypes.data, len(keep[2]) - 1, _HIDDEN_ACTIVATIONS.index(str(c["hidden_activation"])),
                  _OUT_ACTIVATIONS.index(str(c["out_activation"])), len(c["classes_"]))
    return ms, keep


def mlp_abi(c, k, x_t, acc_t=None, background_t=None):
    """obia_mlp_predict_dev -- or, with a background, obia_mlp_coalition_dev over all 2^F coalitions -- with the struct of mlp_struct"""
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.default_context(0)
    ms, keep = mlp_struct(c, k)
    N, F = x_t.shape
    K = len(c["classes_"])
    f64 = dict(dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    if background_t is not None:
        values = torch.empty((N, 1 << F, K), **f64)
        _lib.check(lib.obia_mlp_coalition_dev(ctx.handle, x_t.data_ptr(), N, F, ctypes.byref(ms), background_t.data_ptr(), background_t.shape[0],
                                              None, 1 << F, values.data_ptr()))
        out = values
    else:
        proba, pred, margin = torch.empty((N, K), **f64), torch.empty((N,), dtype=torch.int32, device="cuda"), torch.empty((N,), **f64)
        logits = torch.empty((N, int(keep[2][-1])), **f64)
        _lib.check(lib.obia_mlp_predict_dev(ctx.handle, x_t.data_ptr(), N, F, ctypes.byref(ms), None if acc_t is None else acc_t.data_ptr(),
                                            proba.data_ptr(), pred.data_ptr(), margin.data_ptr(), logits.data_ptr()))
        out = (pred, margin, proba, logits)
    _lib.check(lib.obia_synchronize(ctx.handle))
    return host(out)


@functools.lru_cache(maxsize=None)
def acceptable_rows(N, K):
    rs = np.random.RandomState(11)
    acc = rs.rand(N, K) < 0.5
    for i in np.flatnonzero(acc.sum(1) < 2):
        acc[i, rs.choice(K, 2, replace=False)] = True
    acc[rs.rand(N) < 0.33] = True
    return acc.astype(np.uint8)


def run_forest(forest, x_t, acc_t, ctx=None):
    from obia_amd.classify import forest_predict
    return host(forest_predict(forest, x_t, acceptable=acc_t, ctx=ctx))


def test_forest_predict():
    c = fr.load_case("a")
    X32 = c["transformed"].astype(np.float32)
    N, K = c["proba"].shape
    acc = acceptable_rows(N, K)
    want_pred, want_margin = fr.choose(c["proba"], acc.astype(bool))
    forest = fr.forest_of(c)
    r0 = run_forest(forest, dev(X32), dev(acc))
    assert same_bits(r0[2], c["proba"]) and np.array_equal(r0[0], want_pred) and same_bits(r0[1], want_margin)
    for kx, ka in [(k, 0) for k in F32_OFFSETS] + [(0, 1), (0, 3), (2, 3)]:
        xt, at = off(X32, kx), off(acc, ka)
        misaligned(xt if kx else at, 16 if kx else 4)
        assert same(run_forest(forest, xt, at), r0), f"x offset {kx}, acceptable offset {ka}"
    assert same(forest_abi(c, 0, dev(X32), dev(acc)), r0)                       # the struct filled here: the wrapper's result
    assert same(forest_abi(c, F64_OFFSET, dev(X32), dev(acc)), r0), "threshold / value one float64 off the boundary"
    assert same(forest_abi(c, F64_OFFSET, off(X32, 1), off(acc, 1)), r0)


def run_forest_shap(forest, x_t, ctx=None):
    from obia_amd.classify import forest_shap
    return host(forest_shap(forest, x_t, ctx=ctx))


def test_forest_shap():
    c = SH.load_case("a")
    forest = SH.forest_of(c)
    phi, base = run_forest_shap(forest, dev(c["X32"]))
    e_ref = float(c["e_ref"])
    assert float(np.abs(phi - c["phi_exact"]).max()) <= 8 * e_ref and float(np.abs(base - c["base_exact"]).max()) <= 8 * e_ref
    for k in F32_OFFSETS:
        assert same(run_forest_shap(forest, misaligned(off(c["X32"], k))), (phi, base)), f"x offset {k}"
    assert same(forest_abi(c, 0, dev(c["X32"]), shap=True), (phi, base))
    assert same(forest_abi(c, F64_OFFSET, dev(c["X32"]), shap=True), (phi, base)), "threshold / value / cover one float64 off the boundary"


def run_mlp(mlp, x_t, acc_t, ctx=None):
    from obia_amd.classify import mlp_predict
    return host(mlp_predict(mlp, x_t, acceptable=acc_t, ctx=ctx, _logits=True))


def test_mlp_predict():
    c = mr.load_case("a")
    X = c["transformed"]
    mlp = mr.mlp_of(c)
    N, K = c["proba"].shape
    acc = acceptable_rows(N, K)
    r0 = run_mlp(mlp, dev(X), dev(acc))
    assert same_bits(r0[3], mr.logits(c, X))                                     # relu: the ordered sums alone, bit for bit
    want_pred, want_margin = fr.choose(r0[2], acc.astype(bool))
    assert np.array_equal(r0[0], want_pred) and same_bits(r0[1], want_margin)
    assert float(np.abs(r0[2] - c["proba_ld"]).max()) <= 8 * mr.pooled_e_ref()
    for kx, ka in [(F64_OFFSET, 0), (0, 1), (0, 3), (F64_OFFSET, 3)]:
        xt, at = off(X, kx), off(acc, ka)
        misaligned(xt if kx else at, 16 if kx else 4)
        assert same(run_mlp(mlp, xt, at), r0), f"x offset {kx}, acceptable offset {ka}"
    assert same(mlp_abi(c, 0, dev(X), dev(acc)), r0)                            # the struct filled here: the wrapper's result
    assert same(mlp_abi(c, F64_OFFSET, dev(X), dev(acc)), r0), "weights / biases one float64 off the boundary"


def run_mlp_shap(mlp, x_t, bg_t, ctx=None):
    from obia_amd.classify import mlp_shap
    return host(mlp_shap(mlp, x_t, bg_t, ctx=ctx))


def test_mlp_shap():
    """fixture "author", the first of tests/golden/mlp_shap (there is no "a"): one row, nine features, 24 background rows"""
    c = MS.load_case("author")
    mlp = mr.mlp_of(c)
    phi, base = run_mlp_shap(mlp, dev(c["X"]), dev(c["background"]))
    E, e_comb = mr.pooled_e_ref(), float(c["e_comb"])
    assert float(np.abs(phi - c["phi_exact"]).max()) <= 16 * E + 8 * e_comb and float(np.abs(base - c["base_exact"]).max()) <= 8 * E
    for kx, kb in [(1, 0), (0, 1), (1, 1)]:
        xt, bt = off(c["X"], kx), off(c["background"], kb)
        misaligned(xt if kx else bt)
        assert same(run_mlp_shap(mlp, xt, bt), (phi, base)), f"x offset {kx}, background offset {kb}"
    # the coalition values behind them, with the struct filled here: the wrapper's, and the same with weights / biases off the boundary
    from obia_amd.classify import mlp_coalition_values
    values = mlp_coalition_values(mlp, c["X"], c["background"], MS.all_masks(c["X"].shape[1]))
    assert same_bits(values[0, 0], base)
    assert same(mlp_abi(c, 0, dev(c["X"]), background_t=dev(c["background"])), values)
    assert same(mlp_abi(c, F64_OFFSET, dev(c["X"]), background_t=dev(c["background"])), values), "weights / biases one float64 off the boundary"
    assert same(mlp_abi(c, F64_OFFSET, off(c["X"], 1), background_t=off(c["background"], 1)), values)


# ---- the same call on a used context ------------------------------------------------------------------------------------------
def _op_slic(C, masked, stage):
    def op(ctx):
        img, mask = slic_inputs(96, 128, C, masked)
        return run_slic(dev(img), dev(mask) if masked else None, stage, ctx=ctx)[0]
    return op


def _op_stages(ctx):
    case = next(c for c in S.FIXED_CASES if c["name"] == "mask_disc_c4")
    img, mask, seeds = S.make_inputs(case)
    g = run_stages(dev(img), dev(mask), dict(S.slic_kwargs(case, mask, seeds), max_num_iter=case["iters"]), ctx=ctx)
    return {k: g[k] for k in ("features", "seeds_yx", "centroids", "labels_pre", "K", "step", "prescale", "fscale")}


def _op_quickshift(name):
    def op(ctx):
        H, W, C, ks, md = QS_CASES[name]
        img, noise = qs_inputs(name)
        return run_quickshift(dev(img), dev(noise), ks, md, ctx=ctx)
    return op


def _op_zonal(moments):
    def op(ctx):
        case, _, _ = zonal_case("dispatch_C4_all")
        return run_zonal(dev(case["raw"]), dev(case["lab"]), case, moments, ctx=ctx)
    return op


def _op_rasterize(ctx):
    shape, xy, ring_off, owner, values, _ = raster_shapes()
    return run_rasterize(dev(xy), dev(ring_off), dev(owner), dev(values), shape, ctx=ctx)


def _op_forest(ctx):
    c = fr.load_case("a")
    return run_forest(fr.forest_of(c), dev(c["transformed"].astype(np.float32)), dev(acceptable_rows(*c["proba"].shape)), ctx=ctx)


def _op_forest_shap(ctx):
    c = SH.load_case("a")
    return run_forest_shap(SH.forest_of(c), dev(c["X32"]), ctx=ctx)


def _op_mlp(ctx):
    c = mr.load_case("a")
    return run_mlp(mr.mlp_of(c), dev(c["transformed"]), dev(acceptable_rows(*c["proba"].shape)), ctx=ctx)


def _op_mlp_shap(ctx):
    c = MS.load_case("author")
    return run_mlp_shap(mr.mlp_of(c), dev(c["X"]), dev(c["background"]), ctx=ctx)


OPS = {
    "slic_pre_c4": _op_slic(4, False, "pre"),
    "slic_full_c8_masked": _op_slic(8, True, "full"),
    "slic_full_c3_masked": _op_slic(3, True, "full"),
    "slic_stages": _op_stages,
    "tiled": lambda ctx: run_tiled(dev(tiled_inputs()[0]), dev(tiled_inputs()[1]), ctx=ctx),
    "quickshift_lds": _op_quickshift("lds_48x64x3"),
    "quickshift_global": _op_quickshift("global_40x40x5"),
    "enforce_connectivity": lambda ctx: run_cc(dev(cc_inputs()), ctx=ctx),
    "zonal_stats": _op_zonal(False),
    "zonal_moments": _op_zonal(True),
    "texture_thin_strips": lambda ctx: run_texture(*map(dev, texture_inputs("thin_strips")), ctx=ctx),
    "texture_dense": lambda ctx: run_texture(*map(dev, texture_inputs("dense_65x63")), ctx=ctx),
    "polygon_rings": lambda ctx: run_polygons(dev(polygon_map("salt")[0]), 0, ctx=ctx),
    "rasterize": _op_rasterize,
    "slic_edge": lambda ctx: run_edges(dev(edge_labels()), ctx=ctx),
    "sample_labels": lambda ctx: run_sample(dev(sample_inputs()[0]), dev(sample_inputs()[1]), ctx=ctx),
    "cost_layers": lambda ctx: run_cost_layers(*cost_tensors(0), ctx=ctx),
    "seed_peaks": lambda ctx: run_peaks(dev(peak_plane()), ctx=ctx),
    "seed_pair_matrix": lambda ctx: run_pairs(*map(dev, pair_inputs()[:3]), ctx=ctx),
    "table_scale": lambda ctx: run_scale(dev(fr.load_case("a")["table"]), False, ctx=ctx),
    "table_scale_f64": lambda ctx: run_scale(dev(fr.load_case("a")["table"]), True, ctx=ctx),
    "forest_predict": _op_forest,
    "forest_shap": _op_forest_shap,
    "mlp_predict": _op_mlp,
    "mlp_shap": _op_mlp_shap,
}


@pytest.mark.parametrize("name", list(OPS))
def test_operator_on_a_used_context(oracle, name):
    """All workspace buffers come from a bump allocator that keeps its memory between calls.  A tiled SLIC of 256 x 256 x 4 and a texture
    call with a dense-path box leave non-zero data across the first arena block; the operator then runs on that context and must
    give what it gives on a fresh one (same rule as above: equal, or for zonal the bars of the float64 reference with count, min and
    max equal).  The used context holds at least as much workspace as the fresh one after the operator, so no growth hands the
    operator fresh memory."""
    from obia_amd import _lib
    used, fresh = _lib.Context(0), _lib.Context(0)
    try:
        run_tiled(dev(tiled_inputs()[0]), dev(tiled_inputs()[1]), ctx=used)
        run_texture(*map(dev, texture_inputs("dense_65x63")), ctx=used)
        held = used.workspace_bytes()
        assert held > 0
        a = OPS[name](used)
        b = OPS[name](fresh)
        assert held >= fresh.workspace_bytes(), f"the operator needs {fresh.workspace_bytes()} bytes of workspace, the used context held {held}"
        if name.startswith("zonal"):
            moments = name == "zonal_moments"
            _, ref, tol = zonal_case("dispatch_C4_all")
            judge_zonal(a, ref, tol, moments, f"{name}: used context")
            judge_zonal(b, ref, tol, moments, f"{name}: fresh context")
            for k in ("count", "min", "max"):
                assert same(a[k], b[k]), f"{name}: `{k}` on the used context differs from the fresh one"
        else:
            assert same(a, b), f"{name}: the result on a used context differs from the one on a fresh context"
    finally:
        used.close()
        fresh.close()
