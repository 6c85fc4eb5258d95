"""Cost surface on the GPU (obia_amd.cost, cost.hip) against the CPU restatement of obia/utils/cost.py
(tests/cost_restatement.py): every comparison is bit for bit, except that +0.0 and -0.0 order statistics count as equal."""
import warnings

import numpy as np
import pytest

from tests import cost_restatement as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    bad = got.view(np.uint8).reshape(got.shape + (-1,)) != want.view(np.uint8).reshape(want.shape + (-1,))
    bad = bad.any(-1) & ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0]}: {got[bad][:4]} vs {want[bad][:4]}"


def _select(plane):
    """(lo, hi, n) of the GPU path for a host plane."""
    from obia_amd import _lib, cost
    c = _lib.default_context(0)
    t = torch.as_tensor(np.ascontiguousarray(plane)).cuda()
    return cost._select(_lib.load(), c, t)


def _want_lohi(plane):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return np.nanpercentile(plane, (2, 98))


# ------------------------------------------------------------------------------------------------------ percentile select
def _plane(kind, n, nan_frac, dtype, rs):
    if kind == "normal":
        a = rs.standard_normal(n) * 100
    elif kind == "three":
        a = rs.choice([-2.5, 0.0, 7.0], n)
    elif kind == "constant":
        a = np.full(n, 3.25)
    elif kind == "negative":
        a = -rs.exponential(1.0, n) * 1e6
    else:                                                  # subnormal (float32) / tiny (float64) with signed zeros
        a = rs.standard_normal(n) * (1e-42 if dtype == np.float32 else 1e-310)
        a[rs.rand(n) < 0.1] = -0.0
        a[rs.rand(n) < 0.1] = 0.0
    a = a.astype(dtype)
    a[rs.rand(n) < nan_frac] = np.nan
    if nan_frac == 1.0:
        a[:] = np.nan
    return a


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n", [1, 2, 3, 49, 50, 51, 1000, (1 << 20) + 7])
def test_percentile_select_is_exact(dtype, n):
    rs = np.random.RandomState(n % 1000 + (dtype == np.float64))
    for kind in ("normal", "three", "constant", "negative", "subnormal"):
        for nan_frac in (0.0, 0.5, 1.0):
            a = _plane(kind, n, nan_frac, dtype, rs)
            lo, hi, nv = _select(a)
            assert nv == int((~np.isnan(a)).sum())
            want = _want_lohi(a)
            for g, w in ((lo, want[0]), (hi, want[1])):
                assert (np.isnan(g) and np.isnan(w)) or g == w, (kind, nan_frac, g, w)   # == : +0.0 and -0.0 count as equal


def test_percentile_select_tie_heavy_large_plane():
    rs = np.random.RandomState(9)
    for vals in ([0.0, 1.0], [0.0], [0.125, 0.5, 0.75, 2.0]):
        a = rs.choice(vals, 3_000_001).astype(np.float64)
        lo, hi, n = _select(a)
        want = _want_lohi(a)
        assert n == a.size and lo == want[0] and hi == want[1]


# ---------------------------------------------------------------------------------------------------------------- sobel
@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (17, 63), (17, 64), (17, 65), (33, 129), (70, 191)])
@pytest.mark.parametrize("nan", ["none", "scattered", "clumped"])
def test_chm_gradient_matches(shape, nan):
    from obia_amd.cost import chm_gradient
    rs = np.random.RandomState(sum(shape))
    chm = (rs.uniform(0, 35, shape) * (rs.rand(*shape) < 0.7)).astype(np.float32)
    if nan == "scattered":
        chm[rs.rand(*shape) < 0.05] = np.nan
    elif nan == "clumped":
        chm[shape[0] // 3:shape[0] // 3 + 4, shape[1] // 4:shape[1] // 4 + 6] = np.nan
    _same(chm_gradient(chm, _raw=True), R.hypot_plane(chm))
    _same(chm_gradient(chm), R.chm_gradient(chm))
    got_t = chm_gradient(torch.as_tensor(chm).cuda())
    assert got_t.is_cuda
    _same(got_t.cpu().numpy(), R.chm_gradient(chm))


def test_chm_gradient_inf_and_huge_values():
    from obia_amd.cost import chm_gradient
    rs = np.random.RandomState(1)
    chm = (rs.standard_normal((40, 70)) * 10.0 ** rs.uniform(-3, 38, (40, 70))).astype(np.float32)
    chm[5, 5] = np.inf
    chm[20, 30] = -np.inf
    chm[30, 60] = np.nan
    _same(chm_gradient(chm, _raw=True), R.hypot_plane(chm))
    _same(chm_gradient(chm), R.chm_gradient(chm))


# ------------------------------------------------------------------------------------------------------ ndvi, entropy
@pytest.mark.parametrize("shape", [(1, 1), (3, 4), (6, 6), (64, 65)])
def test_ndvi_matches(shape):
    from obia_amd.cost import ndvi
    rs = np.random.RandomState(2)
    red = rs.uniform(-5, 1000, shape).astype(np.float32)
    nir = rs.uniform(-5, 1000, shape).astype(np.float32)
    red.flat[0] = 0.0; nir.flat[0] = 0.0
    if red.size > 3:
        red.flat[1] = np.nan; red.flat[2] = 5.0; nir.flat[2] = -5.0
    _same(ndvi(red, nir), R.ndvi(red, nir))


def _pan(shape, kind, rs):
    if kind == "smooth":
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        return (500 + 300 * np.sin(xx / 7.0) * np.cos(yy / 5.0) + rs.normal(0, 20, shape)).astype(np.float32)
    if kind == "few":
        return rs.choice([10.0, 20.0, 30.0], shape).astype(np.float32)
    if kind == "nan":
        p = rs.uniform(0, 1, shape).astype(np.float32)
        p[rs.rand(*shape) < 0.2] = np.nan
        return p
    return np.full(shape, 4.0, np.float32)


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (5, 6), (7, 7), (16, 64), (17, 65), (50, 131), (129, 70)])
@pytest.mark.parametrize("kind", ["smooth", "few", "nan", "constant"])
def test_texture_entropy_matches(shape, kind):
    from obia_amd.cost import texture_entropy
    rs = np.random.RandomState(shape[0] * 7 + shape[1])
    pan = _pan(shape, kind, rs)
    raw = R.texture_entropy(pan, raw=True)
    _same(texture_entropy(pan, _raw=True), raw)
    _same(texture_entropy(pan), R.normalise(raw))


def test_normalise_matches_for_both_dtypes():
    from obia_amd.cost import normalise
    rs = np.random.RandomState(3)
    for dt in (np.float32, np.float64):
        a = (rs.standard_normal((33, 47)) * 50).astype(dt)
        a[rs.rand(33, 47) < 0.1] = np.nan
        _same(normalise(a), R.normalise(a))
        _same(normalise(np.full((4, 5), 2, dt)), R.normalise(np.full((4, 5), 2, dt)))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _same(normalise(np.full((3, 3), np.nan, np.float32)), R.normalise(np.full((3, 3), np.nan, np.float32)))


# ---------------------------------------------------------------------------------------------------- make_cost_surface
def _scene(H, W, seed, nan_chm=True, labels=True):
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    wv3 = np.stack([300 + 200 * np.sin(xx / (9 + 2 * b)) * np.cos(yy / (7 + b)) + rs.normal(0, 15, (H, W)) for b in range(8)], -1)
    wv3 = wv3.astype(np.float32)
    chm = np.maximum(0, 20 * np.sin(xx / 13.0) * np.sin(yy / 11.0) + rs.normal(0, 1, (H, W))).astype(np.float32)
    if nan_chm:
        chm[rs.rand(H, W) < 0.01] = np.nan
        chm[H // 4:H // 4 + 5, W // 3:W // 3 + 9] = np.nan
    lab = ((yy // max(1, H // 7)) * 100 + xx // max(1, W // 9)).astype(np.int32) if labels else None
    return wv3, chm, lab


def _weights(rs):
    w = rs.dirichlet(np.ones(4))
    return (float(w[0]), float(w[1]), float(w[2]), float(1.0 - w[0] - w[1] - w[2]))


@pytest.mark.parametrize("case", range(20))
def test_cost_surface_matches_the_restatement(case):
    from obia_amd.cost import make_cost_surface
    rs = np.random.RandomState(100 + case)
    sizes = [(1, 1), (2, 9), (7, 5), (33, 70), (64, 64), (100, 257), (256, 256), (301, 199), (512, 384), (1024, 1024)]
    H, W = sizes[case % len(sizes)]
    with_slic = case % 2 == 0
    wv3, chm, lab = _scene(H, W, case, nan_chm=case % 3 != 0, labels=with_slic)
    w = _weights(rs)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = make_cost_surface(wv3, chm, slic=lab, weights=w)
        want = R.make_cost_surface(wv3, chm, lab, w)
    _same(got, want)


def test_cost_surface_with_this_packages_slic_labels():
    from obia_amd.cost import make_cost_surface
    from obia_amd.segmentation import slic
    wv3, chm, _ = _scene(160, 200, 7)
    lab = slic(wv3, n_segments=60, compactness=10.0, _normalize_bands=True).astype(np.int32)
    _same(make_cost_surface(wv3, chm, slic=lab), R.make_cost_surface(wv3, chm, lab))


def test_missing_slic_warns_and_renormalises():
    from obia_amd.cost import make_cost_surface
    wv3, chm, _ = _scene(40, 50, 8)
    with pytest.warns(UserWarning, match="No SLIC provided"):
        got = make_cost_surface(wv3, chm, weights=(0.5, 0.2, 0.2, 0.1))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _same(got, R.make_cost_surface(wv3, chm, None, (0.5, 0.2, 0.2, 0.1)))


def test_tensor_in_tensor_out_and_views_and_repeat():
    from obia_amd.cost import make_cost_surface
    wv3, chm, lab = _scene(120, 90, 11)
    want = R.make_cost_surface(wv3, chm, lab, (0.4, 0.3, 0.2, 0.1))
    got_np = make_cost_surface(wv3, chm, slic=lab, weights=(0.4, 0.3, 0.2, 0.1))
    _same(got_np, want)
    t = make_cost_surface(torch.as_tensor(wv3).cuda(), torch.as_tensor(chm).cuda(), slic=torch.as_tensor(lab).cuda(),
                          weights=(0.4, 0.3, 0.2, 0.1))
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32
    _same(t.cpu().numpy(), want)
    # non-contiguous HWC views: a band-major (CHW) tensor seen through a permute, and every other band of a wider one
    view = torch.as_tensor(np.ascontiguousarray(wv3.transpose(2, 0, 1))).cuda().permute(1, 2, 0)
    assert not view.is_contiguous()
    _same(make_cost_surface(view, torch.as_tensor(chm).cuda(), slic=torch.as_tensor(lab).cuda(),
                            weights=(0.4, 0.3, 0.2, 0.1)).cpu().numpy(), want)
    wide = torch.zeros((120, 90, 16), dtype=torch.float32, device="cuda")
    wide[:, :, ::2] = torch.as_tensor(wv3).cuda()
    _same(make_cost_surface(wide[:, :, ::2], chm, slic=lab, weights=(0.4, 0.3, 0.2, 0.1)).cpu().numpy(), want)
    again = make_cost_surface(wv3, chm, slic=lab, weights=(0.4, 0.3, 0.2, 0.1))
    _same(again, got_np)


def test_img_data_object_and_float64_input():
    from obia_amd.cost import make_cost_surface

    class Img:
        pass
    wv3, chm, lab = _scene(50, 61, 12)
    img = Img(); img.img_data = wv3.astype(np.float64)
    _same(make_cost_surface(img, chm, slic=lab), R.make_cost_surface(wv3.astype(np.float64), chm, lab))


def test_cost_surface_4096():
    from obia_amd.cost import make_cost_surface
    wv3, chm, lab = _scene(4096, 4096, 13)
    w = (0.45, 0.25, 0.2, 0.1)
    _same(make_cost_surface(wv3, chm, slic=lab, weights=w), R.make_cost_surface(wv3, chm, lab, w))


def test_full_size_properties():
    """16384^2 x 8 (the bench raster's shape): float32 in [0, 1], no NaN, deterministic, and every layer stretched by
    np.nanpercentile of the plane its stage function returns."""
    from obia_amd import cost
    H = W = 16384
    g = torch.Generator(device="cuda").manual_seed(5)
    wv3 = torch.rand((H, W, 8), generator=g, device="cuda") * 1000
    chm = torch.rand((H, W), generator=g, device="cuda") * 30
    chm[torch.rand((H, W), generator=g, device="cuda") < 1e-3] = float("nan")
    chm[1000:1100, 2000:2300] = float("nan")
    ys = torch.arange(H, device="cuda", dtype=torch.int32)[:, None] // 40
    xs = torch.arange(W, device="cuda", dtype=torch.int32)[None, :] // 40
    lab = ys * 1000 + xs
    layers = {}
    c1 = cost.make_cost_surface(wv3, chm, slic=lab, weights=(0.4, 0.3, 0.2, 0.1), _layers=layers)
    assert c1.dtype == torch.float32 and c1.shape == (H, W)
    assert not torch.isnan(c1).any() and float(c1.min()) >= 0.0 and float(c1.max()) <= 1.0
    c2 = cost.make_cost_surface(wv3, chm, slic=lab, weights=(0.4, 0.3, 0.2, 0.1))
    assert torch.equal(c1.view(torch.int32), c2.view(torch.int32))
    del c1, c2
    grad = cost.chm_gradient(chm, _raw=True).cpu().numpy()
    assert tuple(layers["grad"]) == tuple(_want_lohi(grad)); del grad
    pan = wv3[:, :, 0].contiguous().cpu().numpy()
    assert tuple(layers["pan"]) == tuple(_want_lohi(pan)); del pan
    gap = (1 - cost.ndvi(wv3[:, :, 4], wv3[:, :, 6])).cpu().numpy()
    assert tuple(layers["gap"]) == tuple(_want_lohi(gap)); del gap
    tex = cost.texture_entropy(wv3[:, :, 0], _raw=True).cpu().numpy()
    assert tuple(layers["tex"]) == tuple(_want_lohi(tex)); del tex
