"""Every launch clamp crossed on purpose: the second trip of the stride loops ("Launch clamps").

Almost every launch clamps its grid and lets the kernel walk the remainder in a stride loop; the second trip of that loop runs only
above the clamp, which the deliberately small shapes of the other test files never reach.  Each case here

  * takes its shape from tests/launch_grids.py, which finds it by asking the library (obia_test_launch_grid) for the smallest size
    with two trips on the intended axis -- and asserts that again through the library before it runs;
  * compares with the operator's existing restatement at the bar of the operator's own test file: bit for bit, NaN by position
    (quickshift: tests/qs_stages.py, as tests/test_gpu_quickshift_stages.py does);
  * takes every output from tests/guarded.py with one poison: an element the second trip failed to write cannot pass as correct
    because a recycled block happened to hold it, and a write past the end is seen.

Rasters are tall and narrow (or flat and long), so a case stays at a few seconds."""
import ctypes
import warnings

import numpy as np
import pytest

from tests import boxes_restatement as BR
from tests import cost_restatement as CR
from tests import crowns_restatement as WR
from tests import image_restatement as IR
from tests import launch_grids as LG
from tests import pointcloud_restatement as PR
from tests import rasterize_restatement as RR
from tests import seeds_restatement as SR
from tests import sharpness_restatement as SH
from tests import training_restatement as TR
from tests.guarded import POISONS, guarded, holds_poison, snapshot, unchanged

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

POISON = POISONS[0]
I32, U8, F32, F64, I64 = np.int32, np.uint8, np.float32, np.float64, np.int64


def env():
    from obia_amd import _lib
    return _lib, _lib.load(), _lib.default_context(0)


def dev(a):
    t = torch.as_tensor(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()                                    # the library runs on its own stream: the copy is complete first
    return t


def call(fn, *args):
    _lib, lib, c = env()
    rc = fn(c.handle, *args)
    assert rc == 0, (rc, _lib.last_error())
    _lib.check(lib.obia_synchronize(c.handle))
    torch.cuda.synchronize()


def crossed(name):
    """the case's shape, after the library has confirmed that it takes the second trip it is there for"""
    case = LG.cases()[name]
    LG.check(case)
    return case.sizes


def judge(g, want, name):
    """the guarded output holds `want` bit for bit (NaN by position), nothing around it changed, no element was left unwritten"""
    want = np.asarray(want)
    exempt = None
    if want.dtype.itemsize == 1:                                 # a byte that legitimately equals the poison is not "unwritten"
        exempt = want == POISON
    else:
        assert not holds_poison(want), f"{name}: the expected output holds an element that equals the poison"
    got = g.host()
    assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, want.dtype, got.shape, want.shape)
    bad = got.view(U8).reshape(got.shape + (-1,)) != want.view(U8).reshape(want.shape + (-1,))
    bad = bad.any(-1)
    if want.dtype.kind == "f":
        bad &= ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0].tolist()}: {got[bad][:4]} vs {want[bad][:4]}"
    assert g.findings(exempt=exempt, name=name) == []


def quiet(f, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return f(*a, **k)


def block_labels(H, W, seed, by=3, bx=2):
    """labels in blocks of by x bx pixels with a few strays: edges on well over 2 % and under 98 % of the pixels"""
    rs = np.random.RandomState(seed)
    lab = (np.add.outer((np.arange(H) // by) * 7, np.arange(W) // bx) % 5 - 1).astype(I32)          # -1 .. 3: background 0 included
    lab[rs.randint(0, H, 64), rs.randint(0, W, 64)] = 77
    lab[H - 1, W - 1] = 78                                       # the last pixel: the end of the last trip
    return lab


def u8(shape, seed):
    return np.random.RandomState(seed).randint(0, 256, shape).astype(U8)


# ---- rows past grid.y, columns past grid.x: the image previews --------------------------------------------------------------------
@pytest.mark.parametrize("case,k", [("boundaries_rows", 0), ("boundaries_cols", 0), ("boundaries_cols", 1)])
def test_boundaries(case, k):
    """find_boundaries; `_cols`: the output 0 and 1 byte off a 4-byte boundary (the kernel chunks its bytes by four)"""
    _lib, lib, c = env()
    H, W = crossed(case)
    lab = block_labels(H, W, 1)
    lt = dev(lab)
    snap = snapshot(lt)
    g = guarded((H, W), U8, POISON, "cuda", k)
    assert g.ptr % 4 == k
    call(lib.obia_image_boundaries_dev, lt.data_ptr(), H, W, g.ptr)
    judge(g, IR.find_boundaries(lab).astype(U8), case)
    assert unchanged(lt, snap)


@pytest.mark.parametrize("case,k,nch", [("mark_rows", 0, 3), ("mark_cols", 0, 3), ("mark_cols", 1, 1)])
def test_mark(case, k, nch):
    _lib, lib, c = env()
    H, W = crossed(case)
    lab = block_labels(H, W, 2)
    img = u8((H, W, 3) if nch == 3 else (H, W), 3)
    color = (255, 128, 1)
    it, lt, tt = dev(img), dev(lab), dev(IR.mark_table())
    g = guarded((H, W, 3), U8, POISON, "cuda", k)
    call(lib.obia_image_mark_u8_dev, it.data_ptr(), nch, lt.data_ptr(), H, W, tt.data_ptr(), (ctypes.c_uint8 * 3)(*color), g.ptr)
    judge(g, IR.mark_u8(img, lab, color), case)


def test_clahe_rows():
    """the interpolation pass past grid.y (its row blocks were an unclamped grid.y before): the whole raster against the restatement"""
    _lib, lib, c = env()
    H, W = crossed("clahe_rows")
    img = u8((H, W), 4)
    img[H // 2:] //= 2                                           # the tiles differ, so a row block read from the wrong tile row shows
    it = dev(img)
    g = guarded((H, W), U8, POISON, "cuda", 1)
    call(lib.obia_image_clahe_u8_dev, it.data_ptr(), H, W, 1, 0, g.ptr)
    judge(g, IR.apply_clahe(img), "clahe")


# ---- flat arrays past 8192 workgroups of four-byte chunks ---------------------------------------------------------------------------
def test_stretch():
    _lib, lib, c = env()
    n, = crossed("stretch")
    x = np.random.RandomState(5).normal(500, 200, n).astype(F32)
    x[-3:] = [9999.0, -9999.0, 500.0]                            # the tail chunk: both clips and a value inside
    lo, hi = np.percentile(x, (2, 98))
    xt = dev(x)
    g = guarded((n,), U8, POISON, "cuda", 1)
    call(lib.obia_image_stretch_u8_dev, xt.data_ptr(), 0, n, float(lo), float(hi), g.ptr)
    judge(g, IR.rescale_to_8bit(x), "stretch")


@pytest.mark.parametrize("rep", [1, 3])
def test_lut(rep):
    _lib, lib, c = env()
    n, _ = crossed(f"lut_rep{rep}")
    plane, lut = u8((n,), 6), u8((256,), 7)
    want = lut[plane] if rep == 1 else np.stack([lut[plane]] * 3, -1)
    pt, tt = dev(plane), dev(lut)
    g = guarded(want.shape, U8, POISON, "cuda", 1)
    call(lib.obia_image_lut_u8_dev, pt.data_ptr(), n, tt.data_ptr(), rep, g.ptr)
    judge(g, want, "lut")


@pytest.mark.parametrize("nch", [3, 1])
def test_gray_hist(nch):
    _lib, lib, c = env()
    n, = crossed("gray_hist")
    img = u8((n, 3) if nch == 3 else (n,), 8)
    gray = IR.rgb_to_gray(img[None])[0] if nch == 3 else img
    hist = np.bincount(gray.ravel(), minlength=256).astype(I64)
    it = dev(img)
    gg, gh = guarded((n,), U8, POISON, "cuda", 1), guarded((256,), I64, POISON, "cuda", 0)
    call(lib.obia_image_gray_hist_dev, it.data_ptr(), nch, n, gg.ptr, gh.ptr)
    judge(gg, gray, "gray")
    judge(gh, hist, "hist")


# ---- the cost surface ---------------------------------------------------------------------------------------------------------------
def test_cost_sobel_rows():
    _lib, lib, c = env()
    H, W = crossed("cost_sobel_rows")
    rs = np.random.RandomState(9)
    chm = (rs.rand(H, W) * 30).astype(F32)
    chm[rs.randint(0, H, 200), rs.randint(0, W, 200)] = np.nan
    ct = dev(chm)
    g = guarded((H, W), F32, POISON, "cuda", 1)
    call(lib.obia_cost_sobel_f32_dev, ct.data_ptr(), H, W, g.ptr)
    judge(g, quiet(CR.hypot_plane, chm), "sobel")


def test_cost_entropy_rows():
    from obia_amd import cost
    _lib, lib, c = env()
    H, W = crossed("cost_entropy_rows")
    pan = (np.random.RandomState(10).rand(H, W) * 1000).astype(F32)
    pt = dev(pan)
    lo, hi, _ = cost._select(lib, c, pt)
    table = cost._table_dev(0)
    g = guarded((H, W), F64, POISON, "cuda", 1)
    call(lib.obia_cost_entropy_f32_dev, pt.data_ptr(), H, W, lo, hi, table.data_ptr(), g.ptr)
    judge(g, CR.rank_entropy(CR.quantise(pan), rows=1 << 16), "entropy")


def test_cost_edge_count_cols():
    _lib, lib, c = env()
    H, W = crossed("cost_edge_count_cols")
    lab = block_labels(H, W, 11, by=5, bx=7)
    edge = np.zeros((H, W), bool)                                # tests/cost_restatement.py: slic_edge, before its stretch
    edge[:-1, :] |= lab[:-1, :] != lab[1:, :]
    edge[:, :-1] |= lab[:, :-1] != lab[:, 1:]
    assert edge[:, 4096:].any()
    n = ctypes.c_int64(-1)
    lt = dev(lab)
    call(lib.obia_cost_edge_count_dev, lt.data_ptr(), H, W, ctypes.byref(n))
    assert n.value == int(edge.sum())


def test_cost_combine_rows():
    """make_cost_surface on a raster of more rows than grid.y holds: the wrapper's layers, then the combine kernel into a guarded
    buffer, against tests/cost_restatement.py"""
    from obia_amd import cost
    _lib, lib, c = env()
    H, W = crossed("cost_combine_rows")
    rs = np.random.RandomState(12)
    yy, xx = np.mgrid[0:H, 0:W].astype(F32)
    wv3 = np.stack([300 + 200 * np.sin(yy / (9 + 2 * b)) + rs.normal(0, 15, (H, W)) for b in range(8)], -1).astype(F32)
    chm = np.maximum(0, 20 * np.sin(yy / 11.0) + rs.normal(0, 1, (H, W))).astype(F32)
    chm[rs.rand(H, W) < 0.01] = np.nan
    lab = block_labels(H, W, 13)
    weights = (0.4, 0.3, 0.2, 0.1)
    want = quiet(CR.make_cost_surface, wv3, chm, lab, weights)
    L = {}
    got = quiet(cost.make_cost_surface, wv3, chm, slic=lab, weights=weights, _layers=L)
    assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
    pt, gt = torch.empty((H, W), dtype=torch.float32, device="cuda"), torch.empty((H, W), dtype=torch.float32, device="cuda")
    wt, ct, lt = dev(wv3), dev(chm), dev(lab)
    call(lib.obia_cost_bands_f32_dev, wt.data_ptr(), H * W, pt.data_ptr(), gt.data_ptr())
    tex = cost._entropy_dev(lib, c, pt, *L["pan"])
    grad = cost._sobel_dev(lib, c, ct)
    lohi = [L["grad"], L["gap"], L["tex"], L["edge"]]
    lo4, hi4, w4 = np.array([p[0] for p in lohi], F64), np.array([p[1] for p in lohi], F64), np.array(L["weights"], F64)
    g = guarded((H, W), F32, POISON, "cuda", 1)
    call(lib.obia_cost_combine_dev, grad.data_ptr(), gt.data_ptr(), tex.data_ptr(), lt.data_ptr(), H, W, lo4.ctypes.data, hi4.ctypes.data,
         w4.ctypes.data, g.ptr)
    judge(g, want, "combine")


# ---- seeds, consumers, classify, boxes ----------------------------------------------------------------------------------------------
def test_seeds_flag_rows():
    _lib, lib, c = env()
    H, W = crossed("seeds_flag_rows")
    V_MIN, D = 12.0, 3
    a = (np.random.RandomState(14).rand(H, W) * 30).astype(F32)
    a[H - 1, 1] = 100.0                                          # a peak in the tile row only the second trip reaches
    peaks = SR.peaks_scipy(a, V_MIN, D, 0)
    nchunks = -(-H * W // 4096)
    want = np.zeros(nchunks * 4096, U8)
    want[:H * W] = peaks.reshape(-1)
    at = dev(a)
    flags = guarded((nchunks * 4096,), U8, POISON, "cuda", 0)
    offsets = guarded((nchunks + 1,), I32, POISON, "cuda", 1)
    count = ctypes.c_int64(-1)
    call(lib.obia_seeds_peaks_dev, at.data_ptr(), H, W, 0.0, D, float(F32(V_MIN)), None, flags.ptr, offsets.ptr, ctypes.byref(count))
    judge(flags, want, "flags")
    per_chunk = want.reshape(nchunks, 4096).sum(1, dtype=I64)
    judge(offsets, np.concatenate([[0], np.cumsum(per_chunk)]).astype(I32), "offsets")
    assert count.value == int(peaks.sum()) > 1000 and peaks[65535 * 16:].any()


def test_label_edges_rows():
    from oracle.consumers import edge_raster
    _lib, lib, c = env()
    H, = crossed("label_edges_rows")
    W = 5
    lab = block_labels(H, W, 15)
    ref = edge_raster(lab) != 0
    assert 0.02 * lab.size < ref.sum() < 0.98 * lab.size        # the oracle's stretch of a 0 / 1 raster is then the identity
    lt = dev(lab)
    g = guarded((H, W), U8, POISON, "cuda", 1)
    n = ctypes.c_int64(-1)
    call(lib.obia_label_edges_u8_dev, lt.data_ptr(), H, W, g.ptr, ctypes.byref(n))
    judge(g, ref.astype(U8), "label edges")
    assert n.value == int(ref.sum())


@pytest.mark.parametrize("wide", [False, True], ids=["float32", "float64"])
def test_scale_transform(wide):
    """the bars of tests/test_gpu_classify.py for mean and scale; the scaled table is ((t - mean) / scale) of the library's own mean
    and scale, bit for bit, as tests/test_gpu_output_guards.py judges it"""
    from tests.test_gpu_classify import exact_columns
    _lib, lib, c = env()
    N, F = crossed("scale_transform")
    rs = np.random.RandomState(16)
    t = rs.normal(3.0, 2.0, (N, F)) * (1 + np.arange(F))
    t[:, 5] = np.nan
    t[::17, 2] = np.nan
    tt = dev(t)
    gm, gs, gx = guarded((F,), F64, POISON, "cuda", 1), guarded((F,), F64, POISON, "cuda", 1), guarded((N, F), F64 if wide else F32, POISON, "cuda", 1)
    call(lib.obia_table_scale_f64_dev if wide else lib.obia_table_scale_dev, tt.data_ptr(), N, F, gm.ptr, gs.ptr, gx.ptr)
    mean, scale = gm.host(), gs.host()
    n, m_ref, v_ref, mabs = exact_columns(t)
    live = n > 0
    assert not live[5] and np.isnan(mean[~live]).all() and np.isnan(scale[~live]).all()
    assert (np.abs(mean[live] - m_ref[live]) <= n[live] * 2.0 ** -52 * mabs[live]).all()
    s_ref = np.sqrt(v_ref[live])
    assert (np.abs(scale[live] - s_ref) <= (n[live] * 2.0 ** -51 + 2.0 ** -52) * s_ref).all()
    with np.errstate(invalid="ignore"):
        want = ((t - mean) / scale).astype(F64 if wide else F32)
    judge(gx, want, "scaled")
    assert gm.findings(name="mean") == [] and gs.findings(name="scale") == []


def boxes(rs, n):
    lo = rs.rand(n, 2) * 100
    return np.concatenate([lo, lo + rs.rand(n, 2) * 40], 1)


def test_boxes_iou_a():
    _lib, lib, c = env()
    na, nb = crossed("boxes_iou_a")
    rs = np.random.RandomState(17)
    a, b = boxes(rs, na), boxes(rs, nb)
    at, bt = dev(a), dev(b)
    g = guarded((na, nb), F64, POISON, "cuda", 1)
    call(lib.obia_boxes_iou_dev, at.data_ptr(), na, bt.data_ptr(), nb, g.ptr)
    judge(g, BR.iou_matrix(a, b), "iou")


def test_boxes_iou_b():
    """b is 997 boxes repeated (997 is prime: no stride of the kernel is a multiple of it), so the restatement's Python loop runs over
    one period and every column of the matrix still has its own expected value"""
    _lib, lib, c = env()
    na, nb = crossed("boxes_iou_b")
    rs = np.random.RandomState(18)
    a, base = boxes(rs, na), boxes(rs, 997)
    idx = np.arange(nb) % 997
    b = np.ascontiguousarray(base[idx])
    at, bt = dev(a), dev(b)
    g = guarded((na, nb), F64, POISON, "cuda", 1)
    call(lib.obia_boxes_iou_dev, at.data_ptr(), na, bt.data_ptr(), nb, g.ptr)
    judge(g, np.ascontiguousarray(BR.iou_matrix(a, base)[:, idx]), "iou")


# ---- the other users of the flat grid: boxes, crowns, points ---------------------------------------------------------------------------
def test_boxes_assign_fill_and_winner():
    """boxes_fill_i32_kernel and boxes_winner_kernel walk the n_labels + 1 rows of the assignment: a small raster whose ids reach past
    the clamp, three boxes"""
    _lib, lib, c = env()
    m, = crossed("flat")
    nl = m - 1
    H, W = 12, 17
    rs = np.random.RandomState(19)
    lab = rs.randint(1, 6, (H, W)).astype(I32)
    lab[:, 9:] += nl - 8                                         # ids next to the last row of the table: written by the second trip
    lab[0, 0] = nl
    bx = np.array([[0.5, 0.25, 9.5, 7.0], [8.0, 3.0, 16.5, 11.75], [2.0, 2.0, 12.0, 10.0]], F64)
    want_a, want_area = BR.assign(lab, bx, nl)
    assert (want_a[-8:] >= 0).any() and (want_a[:8] >= 0).any() and (want_a == -1).sum() > nl - 20
    lt, bt = dev(lab), dev(bx)
    ga, gr = guarded((m,), I32, POISON, "cuda", 1), guarded((m,), F64, POISON, "cuda", 1)
    call(lib.obia_boxes_assign_dev, lt.data_ptr(), H, W, bt.data_ptr(), len(bx), nl, ga.ptr, gr.ptr)
    judge(ga, want_a, "assigned")
    judge(gr, want_area, "area")


def test_boxes_dissolve():
    _lib, lib, c = env()
    n, = crossed("flat")
    rs = np.random.RandomState(20)
    lab = rs.randint(-1, 40, n).astype(I32)
    assigned = rs.randint(-1, 9, 33).astype(I32)
    lt, at = dev(lab), dev(assigned)
    g = guarded((n,), I32, POISON, "cuda", 1)
    call(lib.obia_boxes_dissolve_dev, lt.data_ptr(), n, at.data_ptr(), len(assigned) - 1, g.ptr)
    judge(g, BR.dissolve(lab, assigned), "dissolve")


def test_crowns_init_and_finish():
    """Rows of NaN cost cut the raster into independent bands of seven rows; seeds lie in the first band, in the band that holds the
    first pixel of the second trip and in the last one.  Those bands are tests/crowns_restatement.py band by band; everywhere else
    the expected +inf / 0 is exactly what crowns_init_kernel and crowns_finish_kernel write, most of it in their second trip."""
    import math
    _lib, lib, c = env()
    n, = crossed("flat")
    W = 33
    H = -(-n // W) + 8
    assert H * W >= n
    rs = np.random.RandomState(21)
    cost = rs.rand(H, W).astype(F32)
    cost[7::8] = np.nan
    first_second_trip = LG.crossing("flat", (1,), 0, "x") - 1    # flat index of the first pixel one past the clamp
    bands = sorted({0, (first_second_trip // W) // 8, (H - 1) // 8})
    bands = [b for b in bands if b * 8 + 6 < H] or bands
    want_d, want_l = np.full((H, W), np.inf, F64), np.zeros((H, W), I32)
    rows, cols, ids = [], [], []
    for i, b in enumerate(bands):
        r0, r1 = b * 8, min(b * 8 + 7, H)
        sr, sc, si = np.array([1, min(5, r1 - r0 - 1)]), np.array([3 + i, 28 - i]), np.array([10 * i + 1, 10 * i + 2])
        d, l = WR.allocate(cost[r0:r1], sr, sc, si)
        want_d[r0:r1], want_l[r0:r1] = d, l
        rows += list(sr + r0); cols += list(sc); ids += list(si)
    assert len(bands) == 3 and (want_l > 0).sum() == 3 * 7 * W
    rc = np.ascontiguousarray(np.stack([rows, cols], 1), I32)
    ct, rt, it = dev(cost), dev(rc), dev(np.array(ids, I32))
    gd, gl = guarded((H, W), F64, POISON, "cuda", 1), guarded((H, W), I32, POISON, "cuda", 1)
    call(lib.obia_crowns_allocate_dev, ct.data_ptr(), None, H, W, rt.data_ptr(), it.data_ptr(), len(ids), 0.5, 1.0, 1.0, math.sqrt(2.0), 8, -1.0,
         gd.ptr, gl.ptr, (ctypes.c_int32 * 2)())
    judge(gd, want_d, "dist")
    judge(gl, want_l, "labels")


def test_points_segments():
    """more points than 1280 workgroups take in one trip (the state arrays are accumulators the caller zeroes, so they are not
    guarded); most points fall into a handful of segments"""
    from obia_amd.pointcloud import SegmentPoints
    from tests.test_gpu_pointcloud import np_state, same_state
    n, = crossed("points_segments")
    H, W = 20, 30
    rs = np.random.RandomState(22)
    labels = np.ones((H, W), I32)
    labels[:4] = np.arange(2, 2 + 4 * W, dtype=I32).reshape(4, W)
    labels[10] = 0                                               # pixels without a row
    affine = [1.0, 0.0, 0.0, -1.0, 0.0, float(H)]
    x, y = rs.uniform(-1, W + 1, n), rs.uniform(-1, H + 1, n)
    z = rs.uniform(-0.5, 8.5, n).astype(F32)
    z[::1001] = np.nan
    inten = rs.randint(0, 65536, n).astype(np.uint16)
    N = int(labels.max())
    sp = SegmentPoints(labels, affine, 1.0, 7.5, n_labels=N).add({"X": x, "Y": y, "Z": z, "Intensity": inten})
    want = PR.segments_state(x, y, z, inten, PR.invert_affine(affine), labels, 1, N, 8, 1.0)
    assert all(int(v) > 0 for v in want["counters"]) and int(want["counters"].sum()) == n
    same_state(np_state(sp), want)


def test_points_rasters_and_finish():
    """points_rasters_kernel over more points, points_finish_kernel over more pixels than the flat grid takes in one trip"""
    from obia_amd.pointcloud import PointRasters
    n, = crossed("flat")
    H, W = 1025, 2049
    assert crossed("flat_plane") == (H * W,)
    rs = np.random.RandomState(23)
    affine = [0.5, 0.0, 0.0, -0.5, 0.0, 0.5 * H]
    x, y = rs.uniform(-1, 0.5 * W + 1, n), rs.uniform(-1, 0.5 * H + 1, n)
    x[-1], y[-1] = 0.5 * W - 0.25, 0.25                          # the last point into the last pixel
    z = rs.uniform(-2, 40, n).astype(F32)
    z[::997] = np.nan
    res = PointRasters((H, W), affine).add({"X": x, "Y": y, "Z": z}).result()
    zk, count = PR.rasters_state(x, y, z, PR.invert_affine(affine), H, W)
    chm, density = PR.rasters_finish(zk, count, 0.25)
    assert count[H - 1, W - 1] >= 1 and (count == 0).any() and (count > 1).any()
    assert np.array_equal(res["chm"].view(np.uint32), chm.view(np.uint32))
    assert np.array_equal(res["density"].view(np.uint32), density.view(np.uint32))
    assert np.array_equal(np.asarray(res["count"]).astype(I64), count.astype(I64))


# ---- sharpness and training tiles: the flat passes ------------------------------------------------------------------------------------
def test_sharpness_stretch():
    _lib, lib, c = env()
    n, = crossed("flat")
    x = (np.random.RandomState(24).standard_normal(n) ** 2).astype(F32)
    x[-1] = 3.0
    lo, hi = np.percentile(x, [2, 98])
    xt = dev(x)
    g = guarded((n,), F32, POISON, "cuda", 1)
    call(lib.obia_sharp_stretch_f32_dev, xt.data_ptr(), n, float(lo), float(hi), g.ptr)
    judge(g, np.clip((x - lo) / (hi - lo), 0, 1).astype(F32), "stretch")


def test_sharpness_gray_lap_minmax():
    """band_minmax_kernel, the reduction in front of the grey plane, over more pixels than its workgroups take in one trip"""
    _lib, lib, c = env()
    npx, = crossed("sharpness_minmax")
    W = 727
    H = npx // W
    img = np.random.RandomState(30).rand(H, W, 5).astype(F32) * 900
    img[H - 1, W - 1] = [1000.0, 5.0, -3.0, 7.0, -20.0]          # the extremes of bands 0, 2 and 4 in the last pixel
    bands = (4, 0, 2)
    want = SH.laplacian3(SH.rgb_to_gray(SH.normalise_bands(img[:, :, list(bands)])))
    it = dev(img)
    g, cnt = guarded((H, W), F32, POISON, "cuda", 1), guarded((1,), I64, POISON, "cuda", 0)
    call(lib.obia_sharp_gray_lap_dev, it.data_ptr(), H, W, 5, (ctypes.c_int32 * 3)(*bands), g.ptr, cnt.ptr)
    judge(g, want, "gray_lap")
    judge(cnt, np.zeros(1, I64), "gray_lap counter")


def test_sharpness_window_of_one():
    """a box filter of one pixel is flat_pass_kernel: a copy that counts the non-finite values (box), lap * lap - lap * lap (variance)"""
    _lib, lib, c = env()
    H, W = 1025, 2049
    assert crossed("flat_plane") == (H * W,)
    plane = np.random.RandomState(25).standard_normal((H, W)).astype(F32)
    pt = dev(plane)
    g, cnt = guarded((H, W), F32, POISON, "cuda", 1), guarded((1,), I64, POISON, "cuda", 0)
    work = guarded((H, W), F32, POISON, "cuda", 1)
    call(lib.obia_sharp_box_dev, pt.data_ptr(), H, W, 1, work.ptr, g.ptr, cnt.ptr)
    judge(g, SH.box_filter(plane, 1), "box of one")
    judge(cnt, np.zeros(1, I64), "box counter")
    assert work.untouched()
    v, work2 = guarded((H, W), F32, POISON, "cuda", 1), guarded((2, H, W), F32, POISON, "cuda", 1)
    call(lib.obia_sharp_variance_dev, pt.data_ptr(), H, W, 1, work2.ptr, v.ptr)
    mean, mean2 = SH.box_filter(plane, 1), SH.box_filter(plane * plane, 1)
    judge(v, mean2 - mean * mean, "variance of one")


def test_training_minmax_scale():
    _lib, lib, c = env()
    n, = crossed("minmax_scale")
    x = (np.random.RandomState(26).standard_normal(n) * 50).astype(F32)
    x[-2:] = [x.max() + 1, x.min() - 1]                          # the extremes in the tail chunk
    xt = dev(x)
    g, cnt = guarded((n,), U8, POISON, "cuda", 1), guarded((1,), I64, POISON, "cuda", 0)
    work = torch.empty(_lib.TRAIN_MINMAX_WORK, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    call(lib.obia_train_minmax_u8_dev, xt.data_ptr(), n, work.data_ptr(), g.ptr, cnt.ptr)
    judge(g, TR.minmax_u8(x), "minmax")
    judge(cnt, np.zeros(1, I64), "minmax counter")


@pytest.mark.parametrize("feather", [0.0, 3.0])
def test_training_compose(feather):
    from obia_amd.training import _Settings
    _lib, lib, c = env()
    npx, = crossed("compose")
    H, W = 1399, npx // 1399
    tile, blurred = u8((H, W, 3), 27), u8((H, W, 3), 28)
    rs = np.random.RandomState(29)
    mask = (rs.rand(H, W) < 0.5).astype(U8)
    dist = (rs.rand(H, W) * 6 * (mask == 0)).astype(F32) if feather else None
    lut = _Settings(0.0, 0, 0.8, False, False).darken_lut()
    bg = TR.darken(blurred, 0.8)
    want = TR.blend_feather(tile, bg, dist, feather) if feather else TR.blend_hard(tile, bg, mask)
    ins = [dev(a) for a in (tile, blurred, mask)] + [dev(dist) if feather else None, dev(lut)]
    g, cnt = guarded((H, W, 3), U8, POISON, "cuda", 1), guarded((1,), I64, POISON, "cuda", 0)
    call(lib.obia_train_compose_u8_dev, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr() if feather else None, H, W,
         ins[4].data_ptr(), float(feather), g.ptr, cnt.ptr)
    judge(g, want, "compose")
    judge(cnt, np.zeros(1, I64), "bad mask bytes")


# ---- quickshift: tile rows past grid.y ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 2], ids=["staged", "global"])
def test_quickshift_rows(oracle, C):
    """tests/test_gpu_quickshift_stages.py's col_257x1 made tall: every stage against oracle.quickshift_stages (tier A: the oracle
    flags no near-tie on these inputs, so the labels must be identical), then the labels once more into a guarded buffer.  One band
    runs the kernel that stages its window in LDS, two bands the one that reads global memory"""
    from tests.test_gpu_quickshift_stages import run_case, textured
    _lib, lib, c = env()
    H, W = crossed("quickshift_rows")
    img = textured(H, W, C, seed=4)
    g, _ = run_case(oracle, img, 3.0, 10.0, seed=11, name="col_tall")
    it, nt = dev(img), dev(g["noise"])
    out = guarded((H, W), I32, POISON, "cuda", 1)
    n = ctypes.c_int(-1)
    call(lib.obia_quickshift_f32_dev, it.data_ptr(), H, W, C, 1.0, 3.0, 10.0, 0.0, 0, nt.data_ptr(), 0, out.ptr, ctypes.byref(n))
    judge(out, g["labels"].astype(I32), "labels")
    assert n.value == g["n_labels"]


# ---- the rasteriser's large shapes: vertices of one shape past grid.y, column tiles of one band past grid.y --------------------------
def rasterize_guarded(xy, ring_offset, ring_shape, values, H, W, fill, want, name):
    """obia_rasterize_polygons_dev into a guarded raster, judged against `want`; returns rasterize_info()"""
    from obia_amd.polygons import rasterize_info
    _lib, lib, c = env()
    ts = [dev(np.asarray(xy, F64)), dev(np.asarray(ring_offset, I64)), dev(np.asarray(ring_shape, I32)), dev(np.asarray(values, I32))]
    snaps = [snapshot(t) for t in ts]
    g = guarded((H, W), I32, POISON, "cuda", 1)
    call(lib.obia_rasterize_polygons_dev, ts[0].data_ptr(), ts[1].data_ptr(), len(ring_shape), ts[2].data_ptr(), ts[3].data_ptr(), len(values),
         H, W, fill, g.ptr)
    judge(g, want, name)
    assert all(unchanged(t, s) for t, s in zip(ts, snaps))
    return rasterize_info()


def test_rast_band_bin():
    """one shape of more vertices than the 64 x 256 threads of rast_band_bin_kernel take in one trip: a star, a shuffled (self-
    intersecting) star whose closing edge and ring boundary lie among the second trip's vertices, a small hole after it"""
    _, nv = crossed("rast_band_bin")
    first_trip = LG.crossing("rast_band_bin", (1, 1), 1, "y") - 1
    H = W = 300
    rs = np.random.RandomState(33)
    n_a, n_hole = first_trip * 9 // 16, 85
    n_b = nv - n_a - n_hole
    assert n_a < first_trip < n_a + n_b - 100                    # the second trip: the end of the second ring, its closing edge, the hole
    rings = [RR.star(rs, 150.3, 149.6, n_a, 60, 140), RR.star(rs, 148.7, 151.2, n_b, 20, 130, shuffle=True), RR.star(rs, 150.1, 150.4, n_hole, 3, 9)]
    xy, off, owner = RR.pack([rings])
    assert len(xy) == nv and off[2] > first_trip
    want = RR.burn(xy, off, owner, [6], (H, W), fill=-3)
    assert 10000 < (want == 6).sum() < 60000
    info = rasterize_guarded(xy, off, owner, [6], H, W, -3, want, "band bin")
    assert (info["large"], info["small"]) == (1, 0)


def test_rast_large():
    """a band of more column tiles than grid.y holds: a zigzag over the whole width of a 9-row raster (two bands), a small shape burned
    before it and one after it inside the tiles only the second trip reaches"""
    n_bands, w = crossed("rast_large")
    H, W = 9, w
    T = LG.unit("rast_large", (1, 1), 1, "y")
    second = (LG.crossing("rast_large", (1, 1), 1, "y") - 1)     # first column (the shape starts at column 0) of the second trip's tiles
    assert second % T == 0 and 32 <= W - second <= T
    xs = np.linspace(0.3, W - 0.3, 40)
    top = np.stack([xs, np.where(np.arange(40) % 2 == 0, 0.2, 3.8)], 1)
    bottom = np.stack([xs[::-1], np.where(np.arange(40) % 2 == 0, 8.8, 5.2)], 1)
    zigzag = np.concatenate([top, bottom])
    shapes = [[RR.rect(W - 38.2, 0.4, W - 20.1, 8.6)], [zigzag], [RR.rect(W - 30.4, 2.3, W - 5.6, 7.7)]]
    values = np.array([5, 9, 13], I32)
    xy, off, owner = RR.pack(shapes)
    assert len(zigzag) == 80
    c0, c1 = max(RR._first_centre_ge(zigzag[:, 0].min()) - 1, 0), min(RR._first_centre_ge(zigzag[:, 0].max()), W - 1)
    assert c0 == 0 and LG.trips("rast_large", (n_bands, c1 - c0 + 1), "y") >= 2
    want = RR.burn(xy, off, owner, values, (H, W), fill=0)
    tail = want[:, second:]
    assert {0, 5, 9, 13} <= set(np.unique(tail).tolist()) and (want[:, :second] == 9).sum() > W
    info = rasterize_guarded(xy, off, owner, values, H, W, 0, want, "large")
    assert (info["large"], info["small"]) == (1, 2)


# ---- the seed merge: pair tiles past grid.x -------------------------------------------------------------------------------------------
PAIRS_EPS = 1.25                                                 # several hundred clusters on this case (2.0 merges everything)


@pytest.fixture(scope="module")
def pairs():
    """n seeds whose pair tiles outnumber the workgroups of walk_pairs, the restated distance matrix (once), and which pairs lie in
    tiles of index >= grid.x: the second trip's"""
    from tests.test_seeds_restatement_cpu import WEIGHT, XY_THRESH
    n, = crossed("seeds_pairs")
    xs, ys, cost, aff = SR.pixel_centre_case(41, n, 130, 160, 0.5)
    order = np.random.RandomState(42).permutation(n)
    xs, ys = np.ascontiguousarray(xs[order]), np.ascontiguousarray(ys[order])
    inv = SR.inverse6(aff)
    D = SR.distance_matrix(xs, ys, cost, inv, WEIGHT, XY_THRESH, 12)
    P = LG.unit("seeds_pairs", (1,), 0, "x")                     # side of a pair tile
    nt, gx = -(-n // P), LG.grid("seeds_pairs", n)[0]
    assert nt * (nt + 1) // 2 > gx
    bi, bj = np.minimum.outer(np.arange(n) // P, np.arange(n) // P), np.maximum.outer(np.arange(n) // P, np.arange(n) // P)
    tile = bi * nt - bi * (bi - 1) // 2 + (bj - bi)              # tile pairs of the upper triangle, rows first (seeds.hip: tile_of)
    return dict(n=n, xs=xs, ys=ys, cost=cost, inv=inv, D=D, second=tile >= gx, args=(WEIGHT, XY_THRESH))


def test_seeds_pairs_link(pairs):
    from obia_amd import seeds as S
    p = pairs
    want = SR.components(p["D"], PAIRS_EPS)
    assert 1 < want.max() + 1 < p["n"]
    # the second trip matters: without the links of its tile pairs the components are others
    assert not np.array_equal(SR.components(np.where(p["second"], np.float32(np.inf), p["D"]), PAIRS_EPS), want)
    for prune in (None, False):
        got = S.merge_clusters(p["xs"], p["ys"], p["cost"], p["inv"], *p["args"], PAIRS_EPS, prune=prune)
        assert got.dtype == I32 and np.array_equal(got, want), prune


def test_seeds_pairs_stats(pairs):
    from obia_amd import seeds as S
    p = pairs
    want = np.array(SR.triu_stats(p["D"]), F32)
    iu = np.triu_indices(p["n"], 1)
    dv, first = p["D"][iu], ~p["second"][iu]
    assert 0 < (~first).sum() < first.sum()
    assert not np.array_equal(np.array([dv[first].min(), np.median(dv[first]), dv[first].max()], F32), want)     # the second trip matters
    got = S.pair_stats(p["xs"], p["ys"], p["cost"], p["inv"], *p["args"], 12)
    assert all(isinstance(v, F32) for v in got) and np.array_equal(np.array(got), want), (got, want)


# ---- masked SLIC on one tall window: the mask packing past grid.x, and with it the min/max, feature and max-distance rows --------------
@pytest.mark.parametrize("W", [16, 18], ids=["vector", "bytes"])
def test_tall_masked_slic(oracle, W):
    """one band, a window of more rows than mask_pack4_kernel's workgroups take four at a time; labels before and after connectivity
    equal the oracle's, as tests/test_gpu_random_parity.py demands at compactness >= 5.  W = 16: the kernel's vector path, 18: bytes"""
    from obia_amd.segmentation import make_params
    _lib, lib, c = env()
    H, _ = crossed("slic_mask_pack")
    first_trip = LG.crossing("slic_mask_pack", (1, 1), 0, "x") - 1
    for name, rows in (("slic_band_minmax", H), ("slic_feature_rows", H // 16), ("slic_maxdist", H)):
        assert LG.trips(name, (rows, 1), "x") >= 2, name
    rs = np.random.RandomState(50 + W)
    yy, xx = np.mgrid[0:H, 0:W].astype(F64)
    img = (300 * np.sin(yy / 9.0) * np.cos(xx / 3.0) + 800 + rs.normal(0, 25, (H, W))).astype(F32)[:, :, None]
    mask = rs.rand(H, W) >= 0.03
    mask[1000:1050, 5:14] = False
    mask[first_trip + 40:first_trip + 90, 3:12] = False          # a block only the second trip packs
    assert first_trip + 90 < H
    n_seg = H * W // 64
    ref, ref_pre, _ = oracle.slic(oracle.normalize(img), n_segments=n_seg, compactness=10.0, max_iter=10, start_label=1, convert2lab=False,
                                  mask=mask.astype(U8), return_all=True)
    assert (ref[~mask] == 0).all() and ref[first_trip:].max() > ref[:first_trip].max() > 1000
    params = make_params(n_segments=n_seg, compactness=10.0, convert2lab=False, normalize_bands=True)
    it, mt = dev(img), dev(mask.astype(U8))
    snaps = snapshot(it), snapshot(mt)
    for fn, want, name in ((lib.obia_slic_assign_only_f32_dev, ref_pre, "before connectivity"), (lib.obia_slic_f32_dev, ref, "labels")):
        g = guarded((H, W), I32, POISON, "cuda", 1)
        n = ctypes.c_int(-1)
        call(fn, it.data_ptr(), H, W, 1, mt.data_ptr(), ctypes.byref(params), g.ptr, ctypes.byref(n))
        judge(g, np.ascontiguousarray(want, I32), name)
    assert n.value == len(np.unique(ref[ref >= 1]))
    assert unchanged(it, snaps[0]) and unchanged(mt, snaps[1])
