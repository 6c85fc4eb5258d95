"""Zonal statistics (zonal_kernel, zonal_moments_kernel) against the float64 reference of tests/zonal_reference.py, at
every dispatch of zonal_stats_dev / zonal_moments_dev and at the shapes, labels and values where the kernels go wrong.

Bars (tests/zonal_reference.py: tolerances, from the error bound of the float64 arithmetic, not guessed):
  count, min, max equal; mean within C (n u R + u |mean|); variance within C n u (M2 + 3 R^2); skewness / kurtosis
  within the bound propagated from the first pass's mean error and the n-term sums of d^2, d^3, d^4 (u = 2^-53,
  n = non-NaN pixels, R = max - min, C = 8).  NaN patterns identical (skewness / kurtosis: except at pairs the reference
  flags near the (eps * mean)^2 threshold -- generated inputs are asserted to carry none).
Every case also asserts that its bars reject one pixel dropped or doubled in any band of its largest non-constant
segment.  The one exception is a single label over a whole 8192^2 raster: there n u R is larger than the move of one
pixel (about (x - mean) / n), so the exact count carries that check, and the mean / variance bars catch a whole
lost tile row of pixels or any systematic error above n u R (7e-9 R)."""
import functools

import numpy as np
import pytest

from tests.zonal_reference import assert_bars_detect_one_pixel, compare, tolerances, zonal_reference

torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu

ZTW, ZTH = 128, 64


# ---- the dispatch table of zonal.hip ----------------------------------------------------------------------------------
def zonal_dispatch(C, bands):
    """(LPP, BPL, MODE) of zonal_kernel for a raster of C bands and a band list (None = all)."""
    bl = list(range(C)) if bands is None else list(bands)
    nb = len(bl)
    ident = bl == list(range(nb)) and nb == C
    if ident and nb in (3, 6, 9):
        return (nb // 3, 3, 0)
    lpp = (nb + 3) // 4
    return (lpp, 4, 0 if ident and nb == 4 * lpp else 1 if ident else 2)


def moments_dispatch(C, bands):
    """(NBP, MODE) of zonal_moments_kernel."""
    bl = list(range(C)) if bands is None else list(bands)
    nb = len(bl)
    ident = bl == list(range(nb)) and nb == C
    nbp = 4 * ((nb + 3) // 4)
    return (nbp, 0 if ident and nb == nbp else 1 if ident else 2)


DISPATCH = ([(C, None) for C in range(1, 17)]                                 # identity lists: MODE 0 / 1, triples
            + [(16, list(range(k))) for k in (1, 3, 5, 8, 9, 12, 13, 15)]     # identity prefix of a wider raster: MODE 2
            + [(16, [15, 2, 7]), (5, [4, 1]), (9, [8, 0, 3, 5, 1, 7]), (12, [11, 10, 9, 8, 7, 6, 5, 4, 3, 2]),
               (16, list(range(15, -1, -1)))])


def test_dispatch_cases_reach_every_kernel_variant():
    zon = {zonal_dispatch(C, b) for C, b in DISPATCH}
    mom = {moments_dispatch(C, b) for C, b in DISPATCH}
    want_z = {(l, 4, m) for l in (1, 2, 3, 4) for m in (0, 1, 2)} | {(1, 3, 0), (2, 3, 0), (3, 3, 0)}
    want_m = {(n, m) for n in (4, 8, 12, 16) for m in (0, 1, 2)}
    assert zon == want_z and mom == want_m


# ---- inputs -----------------------------------------------------------------------------------------------------------
def smooth_raster(rs, H, W, C, base=1000.0, amp=300.0, noise=25.0):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([amp * np.sin(xx / (7 + c)) * np.cos(yy / (9 + c)) + base + 37 * c + rs.gamma(2.0, noise / 2, (H, W))
                     for c in range(C)], -1).astype(np.float32)


def block_labels(rs, H, W, s, jitter=1.5):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    lab = ((yy + jitter * rs.randn(H, W)) // s).astype(np.int64) * ((W + s - 1) // s + 2) + ((xx + jitter * rs.randn(H, W)) // s).astype(np.int64)
    return (lab - lab.min() + 1).astype(np.int32)


def case_dispatch(i):
    C, bands = DISPATCH[i]
    rs = np.random.RandomState(500 + i)
    H, W = 70 + 13 * (i % 3), 131 + 7 * (i % 4)
    raw = smooth_raster(rs, H, W, C)
    raw[rs.rand(H, W, C) < 0.02] = np.nan
    return dict(raw=raw, lab=block_labels(rs, H, W, 9), bands=bands)


def case_shape(H, W, s, C=4, seed=0):
    rs = np.random.RandomState(900 + H * 7 + W)
    raw = smooth_raster(rs, H, W, C)
    raw[rs.rand(H, W, C) < 0.01] = np.nan
    return dict(raw=raw, lab=block_labels(rs, H, W, s, jitter=0.5))


def case_columns_across_tiles():
    """Vertical stripes: runs of one label down a column that cross the tile borders (ZTH rows) and end off-grid."""
    rs = np.random.RandomState(31)
    H, W = 3 * ZTH + 5, ZTW + 9
    xx = np.mgrid[0:H, 0:W][1]
    lab = (xx // 3 + 1).astype(np.int32)
    lab[H // 2:, ::7] = 1000                      # one label that spans many tiles and columns
    return dict(raw=smooth_raster(rs, H, W, 6), lab=lab)


def case_many_labels_per_tile():
    """Salt-and-pepper labels: ~400 labels per 128 x 64 tile, so most go past the ZSLOTS LDS table to global atomics."""
    rs = np.random.RandomState(32)
    H, W = 150, 260
    raw = smooth_raster(rs, H, W, 5)
    raw[rs.rand(H, W, 5) < 0.05] = np.nan
    return dict(raw=raw, lab=rs.randint(1, 1500, (H, W)).astype(np.int32), bands=[4, 0, 2])


def case_label_ranges(start_label, n_labels_delta):
    """start_label 0 / 1, labels below the range, at and above start_label + n_labels, n_labels below and above the max."""
    rs = np.random.RandomState(40 + start_label * 10 + n_labels_delta)
    H, W = 97, 141
    raw = smooth_raster(rs, H, W, 3)
    lab = block_labels(rs, H, W, 11) - 1 + start_label
    lab[rs.rand(H, W) < 0.05] = start_label - 1
    lab[rs.rand(H, W) < 0.02] = -7
    n_labels = int(lab.max()) - start_label + 1 + n_labels_delta
    return dict(raw=raw, lab=lab, start_label=start_label, n_labels=n_labels)


def case_values():
    """NaN pixels per band, a band with no valid pixel, a segment with no valid pixel in one band, constant segments
    (variance exactly 0, skewness / kurtosis NaN), segments within a few ulps of a constant."""
    rs = np.random.RandomState(50)
    H, W, C = 96, 160, 5
    raw = smooth_raster(rs, H, W, C)
    lab = block_labels(rs, H, W, 16, jitter=0.0)
    raw[rs.rand(H, W, C) < 0.1] = np.nan
    raw[:, :, 3] = np.nan                         # a band without data
    ids = np.unique(lab)
    raw[lab == ids[1], 1] = np.nan                # one segment without a valid pixel in band 1
    raw[lab == ids[2]] = 1234.5                   # constant in every band
    raw[lab == ids[3], 0] = 0.0                   # constant zero
    for k, L in enumerate(ids[4:12]):             # a few ulps around a bright level
        m = lab == L
        base = np.float32(60000.0 if k % 2 else 4e6)
        raw[m, 2] = base + np.spacing(base) * rs.randint(-3, 4, int(m.sum()))
        raw[m, 4] = base
    return dict(raw=raw, lab=lab)


ILL = [(60000.0, 0.5, 2000), (60000.0, 2.0, 5000), (4e6, 1.0, 3000), (1000.0, 30.0, 400), (65535.0, 0.75, 1500)]


def case_ill_conditioned(C=1):
    """Bright, nearly flat segments (uint16 DN of water, shadow, saturated roofs) and one well-conditioned control."""
    rs = np.random.RandomState(60)
    W = 100
    rows = [int(np.ceil(n / W)) for _, _, n in ILL]
    H = sum(rows)
    raw = np.zeros((H, W, C), np.float32)
    lab = np.zeros((H, W), np.int32)
    y = 0
    for i, ((off, spread, n), r) in enumerate(zip(ILL, rows)):
        v = np.full(r * W, np.nan)
        v[:n] = off + rs.uniform(-spread, spread, n)
        if spread < 1.0:
            v[:n] = np.round(v[:n] * 2) / 2                 # DN-like half steps
        raw[y:y + r] = v.reshape(r, W, 1).astype(np.float32)
        lab[y:y + r] = np.where(np.isnan(v), 0, i + 1).reshape(r, W)
        y += r
    return dict(raw=raw, lab=lab)


CASES = {f"dispatch_C{DISPATCH[i][0]}_{'all' if DISPATCH[i][1] is None else '-'.join(map(str, DISPATCH[i][1]))}": (lambda i=i: case_dispatch(i))
         for i in range(len(DISPATCH))}
for (H, W, s) in [(1, 1, 1), (1, 300, 7), (300, 1, 7), (37, 127, 6), (37, 128, 6), (37, 129, 6), (63, 200, 8), (64, 200, 8),
                  (65, 200, 8), (7, 333, 5), (131, 77, 10)]:
    CASES[f"shape_{H}x{W}"] = (lambda H=H, W=W, s=s: case_shape(H, W, s))
CASES["columns_across_tiles"] = case_columns_across_tiles
CASES["many_labels_per_tile"] = case_many_labels_per_tile
for sl in (0, 1):
    for dn in (-5, 0, 9):
        CASES[f"labels_start{sl}_n{dn:+d}"] = (lambda sl=sl, dn=dn: case_label_ranges(sl, dn))
CASES["values_nan_constant_ulps"] = case_values
CASES["ill_conditioned"] = case_ill_conditioned


def run(case, entry, moments):
    from obia_amd.statistics import zonal_stats
    kw = dict(bands=case.get("bands"), start_label=case.get("start_label", 1), n_labels=case.get("n_labels"), moments=moments)
    if entry == "numpy":
        return zonal_stats(case["raw"], case["lab"], **kw)
    st = zonal_stats(torch.as_tensor(case["raw"]).cuda(), torch.as_tensor(case["lab"]).cuda(), **kw)
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in st.items()}


def check(case, entry, near_ok=False):
    raw, lab = case["raw"], case["lab"]
    sl = case.get("start_label", 1)
    ref = zonal_reference(raw, lab, bands=case.get("bands"), start_label=sl, n_labels=case.get("n_labels"))
    assert near_ok or not ref["near_threshold"].any(), "generated input sits on the (eps*mean)^2 threshold"
    tol = tolerances(ref)
    st = run(case, entry, False)
    bad = compare(st, ref, tol)
    assert not bad, bad
    st = run(case, entry, True)
    bad = compare(st, ref, tol, moments=True)
    assert not bad, bad
    if (ref["count"] > 1).any():
        assert_bars_detect_one_pixel(raw, lab, ref, tol, start_label=sl, bands=case.get("bands"), moments=True)
    return ref, st


@gpu
@pytest.mark.parametrize("entry", ["numpy", "device"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_zonal_vs_float64_reference(name, entry):
    check(CASES[name](), entry)


@gpu
def test_ill_conditioned_variance_beats_float32():
    """Relative variance error <= 1e-8 on the bright, nearly flat segments, and never above NumPy float32's own."""
    case = case_ill_conditioned()
    ref, _ = check(case, "device")
    for moments in (False, True):
        st = run(case, "device", moments)
        for i in range(len(ILL)):
            v = case["raw"][case["lab"] == i + 1, 0]
            exact = ref["variance"][i, 0]
            err = abs(st["variance"][i, 0] - exact) / exact
            f32 = abs(float(np.var(v)) - exact) / exact
            assert err <= 1e-8 and err <= max(f32, 1e-15), (ILL[i], moments, err, f32)


@functools.lru_cache(maxsize=1)
def raster_8192():
    S = 8192
    rs = np.random.RandomState(70)
    raw = np.empty((S, S, 2), np.float32)
    raw[:, :, 0] = rs.uniform(900.0, 1100.0, (S, S))
    raw[:, :, 1] = 60000.0 + np.round(rs.uniform(-2, 2, (S, S)) * 2) / 2
    raw[:, :, 1][rs.rand(S, S) < 0.01] = np.nan
    return raw


@gpu
@pytest.mark.parametrize("kind", ["one_label", "segments_300px"])
def test_zonal_8192_squared(kind):
    """8192^2 x 2 (band 1 with NaN pixels): one label over the whole raster, or ~220 000 segments of ~300 pixels."""
    from obia_amd.statistics import zonal_stats
    S = 8192
    raw = raster_8192()
    if kind == "one_label":
        lab = np.ones((S, S), np.int32)
    else:
        yy, xx = np.ogrid[0:S, 0:S]
        lab = ((yy // 17) * (S // 17 + 1) + (xx + (yy // 17) % 5) // 18 + 1).astype(np.int32)
    ref = zonal_reference(raw, lab)
    assert not ref["near_threshold"].any()
    tol = tolerances(ref)
    st = zonal_stats(torch.as_tensor(raw).cuda(), torch.as_tensor(lab).cuda(), moments=True)
    st = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in st.items()}
    bad = compare(st, ref, tol, moments=True)
    assert not bad, bad
    if kind == "segments_300px":
        assert_bars_detect_one_pixel(raw, lab, ref, tol, moments=True)
    else:
        # one pixel moves the mean by (x - mean) / n <= R / n, below the bound n u R: the exact count carries it
        assert st["count"].tolist() == [S * S] and np.all(tol["mean"] < 1e-6 * (ref["max"] - ref["min"]))
