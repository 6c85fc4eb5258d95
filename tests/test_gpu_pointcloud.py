"""Point clouds on the GPU (obia_amd.pointcloud, include/obia_points.h) against the restatement (tests/pointcloud_restatement.py): the
state bit for bit -- it is integer sums and integer maxima, so the order of the points and the cut of the cloud change nothing -- and
the columns within bounds that are derived, not fitted:

  ch, n_points, mean_intensity   equal the float64 restatement exactly; mean_intensity is within 1 ulp of the exact rational
  variance_intensity             within 4 ulp of the exact rational: at most four roundings (the two-word numerator conversion is two,
                                 n^2, the division)
  pai, fhd, pad                  within max(8 D, 4) ulp of the long-double restatement, D the largest distance of the float64 NumPy
                                 restatement from it on the same inputs: the device's log is not correctly rounded (the margin of 3.5j)
"""
import functools

import numpy as np
import pytest

from tests import pointcloud_restatement as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NZ = 106                                                                     # floor(31.7 / 0.3) + 1


def cloud(c, sel=slice(None), intensity=True):
    d = {"X": c["x"][sel], "Y": c["y"][sel], "HeightAboveGround": c["z"][sel]}
    if intensity:
        d["Intensity"] = c["intensity"][sel]
    return d


def np_state(sp):
    st = sp.state()
    return {"profile": st["profile"].astype(np.uint32), "top": st["top"].astype(np.uint32), "n_int": st["n_int"].astype(np.uint32),
            "s1": st["s1"].view(np.uint64), "s2": st["s2"].view(np.uint64), "counters": st["counters"].view(np.uint64)}


def same_state(got, want):
    for k, w in want.items():
        assert got[k].dtype == w.dtype and got[k].shape == w.shape and np.array_equal(got[k], w), (k, int((got[k] != w).sum()))


@functools.lru_cache(maxsize=None)
def reference(which):
    """the case, its restated state and rasters: computed once, shared, never changed"""
    affine, start = {"base": (R.AFFINE, 1), "rotated": (R.AFFINE_ROTATED, 1), "start0": (R.AFFINE, 0)}[which]
    c = R.base_case(affine)
    N = R.NSEG + 1 - start
    st = R.segments_state(c["x"], c["y"], c["z"], c["intensity"], c["inv"], c["labels"], start, N, NZ, R.DZ)
    zk, count = R.rasters_state(c["x"], c["y"], c["z"], c["inv"], R.H, R.W)
    area = abs(affine[0] * affine[3] - affine[1] * affine[2])
    chm, density = R.rasters_finish(zk, count, area)
    # every class of points and of rows is there before anything is judged
    assert all(int(v) > 0 for v in st["counters"])
    empty = st["profile"].sum(1) == 0
    assert 0 < empty.sum() < N and (st["n_int"] == 0).sum() > 0
    assert np.isnan(c["z"]).any() and (c["z"] < 0).any() and (c["z"] == np.float32(R.ZMAX)).any() and (zk == 0).any() and (count > 1).any()
    return dict(c=c, N=N, start=start, st=st, zkey=zk, count=count, chm=chm, density=density)


def run_segments(c, start, N, parts=(slice(None),), intensity=True):
    from obia_amd.pointcloud import SegmentPoints
    sp = SegmentPoints(c["labels"], c["affine"], R.DZ, R.ZMAX, start_label=start, n_labels=N)
    for sel in parts:
        sp.add(cloud(c, sel, intensity))
    return sp


@pytest.mark.parametrize("which", ["base", "rotated", "start0"])
def test_state_bit_for_bit(which):
    from obia_amd.pointcloud import PointRasters
    r = reference(which)
    c = r["c"]
    sp = run_segments(c, r["start"], r["N"])
    assert sp.nz == NZ and sp.N == r["N"]
    same_state(np_state(sp), r["st"])
    assert sp.counters() == dict(zip(("outside", "unlabelled", "out_of_range", "in_profile"), (int(v) for v in r["st"]["counters"])))
    pr = PointRasters((R.H, R.W), c["affine"]).add(cloud(c))
    st, res = pr.state(), pr.result()
    assert np.array_equal(st["zkey"].astype(np.uint32), r["zkey"]) and np.array_equal(st["count"].astype(np.uint32), r["count"])
    assert res["chm"].dtype == np.float32 and np.array_equal(res["chm"].view(np.uint32), r["chm"].view(np.uint32))
    assert res["density"].dtype == np.float32 and np.array_equal(res["density"].view(np.uint32), r["density"].view(np.uint32))
    assert np.array_equal(res["count"], r["count"].astype(np.int64))


def test_without_intensity_the_radiometric_state_stays_zero():
    r = reference("base")
    sp = run_segments(r["c"], 1, r["N"], intensity=False)
    want = dict(r["st"], n_int=np.zeros_like(r["st"]["n_int"]), s1=np.zeros_like(r["st"]["s1"]), s2=np.zeros_like(r["st"]["s2"]))
    same_state(np_state(sp), want)
    col = sp.columns()
    assert np.isnan(col["mean_intensity"]).all() and np.isnan(col["variance_intensity"]).all()


def test_order_and_chunking_change_no_bit():
    from obia_amd.pointcloud import PointRasters
    r = reference("base")
    c = r["c"]
    n = len(c["x"])
    perm = np.random.RandomState(11).permutation(n)
    shuffled = dict(c, x=c["x"][perm], y=c["y"][perm], z=c["z"][perm], intensity=c["intensity"][perm])
    same_state(np_state(run_segments(shuffled, 1, r["N"])), r["st"])
    parts = (slice(0, 2049), slice(2049, 2049), slice(2049, 7000), slice(7000, n))         # ragged, one of them empty
    same_state(np_state(run_segments(c, 1, r["N"], parts)), r["st"])
    pr = PointRasters((R.H, R.W), c["affine"])
    for sel in parts:
        pr.add(cloud(shuffled, sel))
    st = pr.state()
    assert np.array_equal(st["zkey"].astype(np.uint32), r["zkey"]) and np.array_equal(st["count"].astype(np.uint32), r["count"])


def test_more_rows_in_a_chunk_than_any_table_holds():
    """128 x 128 pixels, every pixel its own label, 20 000 shuffled points: a chunk of 2048 points meets about 2000 rows and as many
    (row, bin) keys, four times the row table and as much as the whole profile table, so keys fall through to global memory"""
    from obia_amd.pointcloud import SegmentPoints
    rs = np.random.RandomState(3)
    H = W = 128
    labels = np.arange(1, H * W + 1, dtype=np.int32).reshape(H, W)
    affine = [1.0, 0.0, 0.0, -1.0, 0.0, float(H)]
    n = 20000
    x, y = rs.uniform(0, W, n), rs.uniform(0, H, n)
    z = rs.uniform(0, 8, n).astype(np.float32)
    inten = rs.randint(0, 65536, n).astype(np.uint16)
    sp = SegmentPoints(labels, affine, 1.0, 7.5).add({"X": x, "Y": y, "Z": z, "Intensity": inten})
    want = R.segments_state(x, y, z, inten, R.invert_affine(affine), labels, 1, H * W, 8, 1.0)
    assert want["counters"][3] == n and (want["profile"] > 0).sum() > 15000
    same_state(np_state(sp), want)


def test_one_counter_past_sixteen_bits():
    """70 000 points in one segment and one bin, all of intensity 65535"""
    from obia_amd.pointcloud import SegmentPoints
    labels = np.full((4, 4), 3, np.int32)
    affine = [1.0, 0.0, 0.0, -1.0, 0.0, 4.0]
    n = 70000
    rs = np.random.RandomState(5)
    x, y = rs.uniform(0, 4, n), rs.uniform(0, 4, n)
    z = np.full(n, 2.5, np.float32)
    inten = np.full(n, 65535, np.uint16)
    sp = SegmentPoints(labels, affine, 1.0, 5.0).add({"X": x, "Y": y, "Z": z, "Intensity": inten})
    st = np_state(sp)
    assert st["profile"].shape == (3, 6) and st["profile"][2, 2] == n and st["profile"].sum() == n
    assert st["n_int"][2] == n and st["s1"][2] == n * 65535 and st["s2"][2] == n * 65535 ** 2
    col = sp.columns()
    assert col["n_points"].tolist() == [0, 0, n] and col["mean_intensity"][2] == 65535.0 and col["variance_intensity"][2] == 0.0
    assert col["ch"][2] == 2.5 and np.isnan(col["ch"][:2]).all()


@pytest.mark.parametrize("dz,z_max,nz", [(50.0, 10.0, 1), (0.16, 31.9, 200)])
def test_bin_counts(dz, z_max, nz):
    from obia_amd.pointcloud import SegmentPoints
    r = reference("base")
    c = r["c"]
    sp = SegmentPoints(c["labels"], c["affine"], dz, z_max, n_labels=r["N"]).add(cloud(c))
    assert sp.nz == nz
    want = R.segments_state(c["x"], c["y"], c["z"], c["intensity"], c["inv"], c["labels"], 1, r["N"], nz, dz)
    same_state(np_state(sp), want)
    got, ref = sp.columns(pad=True), R.columns(want, dz, pad=True)
    assert np.array_equal(got["n_points"], ref["n_points"])
    assert np.array_equal(np.isnan(got["pad"]), np.isnan(ref["pad"])) and got["pad"].shape == (r["N"], nz)


@pytest.mark.parametrize("n", [0, 1, 257])
def test_small_clouds(n):
    from obia_amd.pointcloud import PointRasters
    r = reference("base")
    c = r["c"]
    sel = slice(100, 100 + n)
    sp = run_segments(c, 1, r["N"], (sel,))
    want = R.segments_state(c["x"][sel], c["y"][sel], c["z"][sel], c["intensity"][sel], c["inv"], c["labels"], 1, r["N"], NZ, R.DZ)
    same_state(np_state(sp), want)
    assert sum(sp.counters().values()) == n
    res = PointRasters((R.H, R.W), c["affine"]).add(cloud(c, sel)).result()
    zk, count = R.rasters_state(c["x"][sel], c["y"][sel], c["z"][sel], c["inv"], R.H, R.W)
    chm, density = R.rasters_finish(zk, count, 0.25)
    assert np.array_equal(res["chm"].view(np.uint32), chm.view(np.uint32)) and np.array_equal(res["density"].view(np.uint32), density.view(np.uint32))


def test_columns():
    r = reference("base")
    st = r["st"]
    sp = run_segments(r["c"], 1, r["N"])
    got = sp.columns(min_height=1.0, beer_lambert_constant=0.5, pad=True)
    f64 = R.columns(st, R.DZ, 1.0, 0.5, np.float64, pad=True)
    ld = R.columns(st, R.DZ, 1.0, 0.5, np.longdouble, pad=True)
    exact = R.exact_intensity(st)
    for name in R.COLUMNS + ("pad",):                                        # NaN rows are exactly the restatement's
        assert got[name].shape == f64[name].shape and got[name].dtype == (np.int64 if name == "n_points" else np.float64)
        if name != "n_points":
            assert np.array_equal(np.isnan(got[name]), np.isnan(f64[name])), name
    assert np.isnan(f64["ch"]).sum() == 4 and np.isnan(f64["pai"]).sum() > 4 and np.isnan(f64["mean_intensity"]).sum() == 4
    assert np.array_equal(got["n_points"], f64["n_points"])
    assert np.array_equal(got["ch"].view(np.uint64), f64["ch"].view(np.uint64))
    assert np.array_equal(got["mean_intensity"].view(np.uint64), f64["mean_intensity"].view(np.uint64))
    rows = [i for i, e in enumerate(exact) if e is not None]
    u_mean = R.ulps(got["mean_intensity"][rows], [exact[i][0] for i in rows])
    u_var = R.ulps(got["variance_intensity"][rows], [exact[i][1] for i in rows])
    print(f"mean_intensity: {u_mean.max():.3f} ulp of the exact rational; variance_intensity: {u_var.max():.3f} ulp")
    assert u_mean.max() <= 1.0 and u_var.max() <= 4.0
    for name in ("pai", "fhd", "pad"):
        ok = ~np.isnan(f64[name])
        D = float(R.ulps(f64[name][ok], ld[name][ok]).max())
        bound = max(8.0 * D, 4.0)
        u = float(R.ulps(got[name][ok], ld[name][ok]).max())
        print(f"{name}: restatement {D:.3f} ulp from long double, bound {bound:.3f} ulp, kernel {u:.3f} ulp")
        assert u <= bound, name
    # the profile above min_height telescopes to pai (a property of the definitions, checked on the kernel's own output)
    j0 = R.j0_of(1.0, R.DZ, NZ)
    tel = np.nansum(got["pad"][:, j0:], 1) * R.DZ
    ok = ~np.isnan(got["pai"]) & ~np.isnan(got["pad"][:, j0:]).any(1)
    assert ok.sum() > 40 and np.allclose(tel[ok], got["pai"][ok], rtol=1e-12, atol=1e-12)


class _Image:
    def __init__(self, img, affine):
        self.img_data, self.affine_transformation, self.crs = img, affine, None


def test_create_objects_fills_the_five_columns():
    from obia_amd.pointcloud import segment_point_stats
    from obia_amd.statistics import create_objects
    r = reference("base")
    c = r["c"]
    rs = np.random.RandomState(2)
    img = _Image(rs.uniform(0, 1000, (R.H, R.W, 2)).astype(np.float32), c["affine"])
    pc = cloud(c)
    kw = dict(calculate_textural=False, geometry=False)
    plain = create_objects(c["labels"], img, **kw)
    full = create_objects(c["labels"], img, voxel_resolution=(1.0, 1.0, R.DZ), calculate_structural=True, calculate_radiometric=True,
                          pointcloud=pc, **kw)
    assert list(full.columns) == list(plain.columns) and len(full) == len(plain) == R.NSEG
    stats = segment_point_stats(pc, c["labels"], c["affine"], R.DZ, n_labels=R.NSEG)
    present = np.ones(R.NSEG, bool)                                          # every id 1 .. 60 has pixels
    five = ("pai", "fhd", "ch", "mean_intensity", "variance_intensity")
    for name in five:
        assert np.array_equal(full[name].to_numpy().view(np.uint64), stats[name][present].view(np.uint64)), name
        assert plain[name].isna().all() and not full[name].isna().all()
    spectral = [n for n in plain.columns if n not in five and n != "geometry"]
    assert full[spectral].equals(plain[spectral])
    # a family that was not asked for stays NaN, a flag that is off drops its column as before
    only = create_objects(c["labels"], img, voxel_resolution=(1.0, 1.0, R.DZ), calculate_radiometric=True, calc_fhd=False, pointcloud=pc, **kw)
    assert "fhd" not in only.columns and only["pai"].isna().all() and only["ch"].isna().all()
    assert np.array_equal(only["mean_intensity"].to_numpy().view(np.uint64), full["mean_intensity"].to_numpy().view(np.uint64))


def test_the_chm_feeds_the_seed_chain_as_a_tensor():
    from obia_amd.pointcloud import points_to_rasters
    from obia_amd.seeds import make_chm_seeds, make_density_seeds
    r = reference("base")
    c = r["c"]
    t = {"X": torch.as_tensor(c["x"]).cuda(), "Y": torch.as_tensor(c["y"]).cuda(), "HeightAboveGround": torch.as_tensor(c["z"]).cuda()}
    res = points_to_rasters(t, c["affine"], (R.H, R.W))
    assert all(v.is_cuda for v in res.values()) and res["chm"].dtype == torch.float32
    assert np.array_equal(res["chm"].cpu().numpy().view(np.uint32), r["chm"].view(np.uint32))
    a = make_chm_seeds(res["chm"], h_min_m=2.5, min_dist_px=3, gauss_sigma=1, affine_transformation=c["affine"])
    b = make_chm_seeds(r["chm"], h_min_m=2.5, min_dist_px=3, gauss_sigma=1, affine_transformation=c["affine"])
    assert len(b["id"]) > 0 and set(a) == set(b)
    for k in b:
        assert np.array_equal(np.asarray(a[k].cpu() if hasattr(a[k], "cpu") else a[k]), np.asarray(b[k])), k
    d = make_density_seeds(res["density"], d_min=4.5, min_dist_px=4, gauss_sigma=2)
    e = make_density_seeds(r["density"], d_min=4.5, min_dist_px=4, gauss_sigma=2)
    assert len(e["id"]) > 0 and all(np.array_equal(np.asarray(d[k].cpu() if hasattr(d[k], "cpu") else d[k]), np.asarray(e[k])) for k in e)
