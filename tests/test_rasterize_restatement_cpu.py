"""Polygons -> label raster, host side: hand-made answers that pin the NumPy restatement of the rule
(tests/rasterize_restatement.py) pixel by pixel, and the argument checks of obia_amd.polygons.rasterize and
obia_amd.cost.rasterise_slic_gpkg that fire before any device use."""
import struct

import numpy as np
import pytest

from tests import rasterize_restatement as R


def burn(shapes, values, shape=(5, 6), fill=0, **kw):
    xy, off, owner = R.pack(shapes)
    return R.burn(xy, off, owner, values, shape, fill, **kw)


def grid(rows):
    return np.array([[int(ch) for ch in row] for row in rows], np.int32)


def test_rectangle_of_3_by_2_pixels():
    assert np.array_equal(burn([[R.rect(1, 1, 4, 3)]], [7]), 7 * grid(["000000", "011100", "011100", "000000", "000000"]))


def test_closing_vertex_and_direction_do_not_matter():
    open_ring = R.rect(1, 1, 4, 3)
    want = burn([[open_ring]], [1])
    assert np.array_equal(burn([[open_ring + open_ring[:1]]], [1]), want)
    assert np.array_equal(burn([[open_ring[::-1]]], [1]), want)


def test_ring_with_a_hole():
    got = burn([[R.rect(0, 0, 6, 6), R.rect(2, 2, 4, 4)]], [3], shape=(6, 6))
    assert np.array_equal(got, 3 * grid(["111111", "111111", "110011", "110011", "111111", "111111"]))


def test_two_parts_of_one_shape():
    got = burn([[R.rect(0, 0, 2, 2), R.rect(3, 3, 5, 5)]], [4])
    assert np.array_equal(got, 4 * grid(["110000", "110000", "000000", "000110", "000110"]))


def test_overlap_is_won_by_the_later_shape_in_both_orders():
    a, b = [R.rect(0, 0, 4, 4)], [R.rect(2, 2, 6, 5)]
    assert np.array_equal(burn([a, b], [5, 9]), grid(["555500", "555500", "559999", "559999", "009999"]))
    assert np.array_equal(burn([b, a], [9, 5]), grid(["555500", "555500", "555599", "555599", "009999"]))


def test_triangle_with_its_vertices_on_pixel_centres():
    """Closed on the left and top, open on the right and bottom: of the three vertex pixels only the top-left one is covered."""
    got = burn([[[(0.5, 0.5), (3.5, 0.5), (0.5, 3.5)]]], [1], shape=(4, 4))
    assert np.array_equal(got, grid(["1110", "1100", "1000", "0000"]))


def test_horizontal_edges_through_rows_of_centres():
    """Top edge through the centres of row 1: covered.  Bottom edge through the centres of row 3: not covered."""
    got = burn([[R.rect(1, 1.5, 4, 3.5)]], [1])
    assert np.array_equal(got, grid(["000000", "011100", "011100", "000000", "000000"]))


def test_vertical_edges_through_columns_of_centres():
    """Left edge through the centres of column 1: covered.  Right edge through the centres of column 3: not covered."""
    got = burn([[R.rect(1.5, 1, 3.5, 3)]], [1])
    assert np.array_equal(got, grid(["000000", "011000", "011000", "000000", "000000"]))


def test_slivers_that_contain_no_centre():
    assert not burn([[R.rect(1.6, 1.6, 4.4, 2.4)]], [1]).any()
    assert not burn([[R.rect(1.6, -1, 1.9, 7)]], [1]).any()
    assert not burn([[[(0.6, 0.6), (5.4, 0.9), (5.4, 0.6)]]], [1]).any()


def test_ring_wholly_outside_the_raster():
    for ring in (R.rect(10, 10, 12, 12), R.rect(-9, -9, -1, -1), R.rect(-5, 1, -0.6, 3), R.rect(1, 5.6, 3, 9)):
        assert np.array_equal(burn([[ring]], [1], fill=-3), np.full((5, 6), -3, np.int32))


def test_ring_that_sticks_out_on_all_four_sides():
    assert np.array_equal(burn([[R.rect(-3, -2, 9, 8)]], [2]), np.full((5, 6), 2, np.int32))
    got = burn([[R.rect(-3, -2, 9, 8), R.rect(2, -4, 3, 20)]], [2])          # a hole that sticks out too
    assert np.array_equal(got, 2 * grid(["110111"] * 5))


def test_degenerate_rings_cover_nothing():
    for ring in ([(1, 1)], [(1, 1), (4, 4)], [(1, 1), (4, 4), (1, 1)], [(1, 1), (1, 1), (1, 1), (1, 1)],
                 [(0, 2.5), (6, 2.5), (3, 2.5)], [(1, 0), (1, 5), (1, 2)], [(0, 0), (4, 4), (2, 2)],
                 [(0.5, 0.5), (4.5, 4.5), (0.5, 0.5), (4.5, 4.5)], []):
        assert not burn([[ring]], [1]).any(), ring
    # ... and leave the shapes around them alone
    got = burn([[R.rect(1, 1, 4, 3)], [[(0, 0), (6, 5)]]], [7, 8])
    assert np.array_equal(got, 7 * grid(["000000", "011100", "011100", "000000", "000000"]))


def test_shape_without_rings_and_fill():
    xy, off, owner = R.pack([[R.rect(1, 1, 2, 2)]])
    got = R.burn(xy, off, owner + 2, [4, 5, 6, 7], (3, 3), fill=-7)          # shapes 0, 1 and 3 own no ring
    assert np.array_equal(got, np.array([[-7, -7, -7], [-7, 6, -7], [-7, -7, -7]], np.int32))


@pytest.mark.parametrize("seed", range(6))
def test_bounding_box_search_equals_the_whole_raster_search(seed):
    rs = np.random.RandomState(seed)
    H, W = 23, 31
    shapes = []
    for i in range(25):
        ring = R.star(rs, rs.uniform(-8, W + 8), rs.uniform(-8, H + 8), rs.randint(3, 30), 0.3, 14, shuffle=i % 3 == 0,
                      on_centres=i % 4 == 0)
        shapes.append([ring] if i % 5 else [ring, R.star(rs, ring[0, 0], ring[0, 1], 5, 0.5, 3)])
    vals = rs.randint(1, 9, len(shapes))
    a, b = burn(shapes, vals, (H, W), fill=-7), burn(shapes, vals, (H, W), fill=-7, full=True)
    assert np.array_equal(a, b)
    assert (a != -7).any() and (a == -7).any()


# ------------------------------------------------------------------------------------------ argument checks, no device
@pytest.fixture
def no_device(monkeypatch):
    """Any use of the library fails the test."""
    from obia_amd import _lib

    def boom(*a, **k):
        raise AssertionError("the device library was used")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(_lib, "default_context", boom)


def wkb_polygon(rings):
    b = struct.pack("<BII", 1, 3, len(rings))
    for r in rings:
        r = list(r) + [r[0]]
        b += struct.pack("<I", len(r)) + np.asarray(r, "<f8").tobytes()
    return b


def test_public_names():
    import obia_amd
    from obia_amd import cost, polygons
    assert obia_amd.rasterize is polygons.rasterize
    assert obia_amd.rasterise_slic_gpkg is cost.rasterise_slic_gpkg


def test_to_pixel_uses_the_inverse_of_the_image_transform():
    from obia_amd.polygons import to_pixel
    from obia_amd.seeds import invert_affine
    aff = [0.5, 0.0, 0.0, -0.5, 443210.0, 6012345.5]
    xy = np.array([[443210.0, 6012345.5], [443215.25, 6012340.0]])
    ra, rb, rc, rd, re, rf = invert_affine(aff)
    want = np.stack([ra * xy[:, 0] + rb * xy[:, 1] + rc, rd * xy[:, 0] + re * xy[:, 1] + rf], 1)
    assert np.array_equal(to_pixel(xy, aff), want)
    assert np.array_equal(want, [[0.0, 0.0], [10.5, 11.0]])
    assert np.array_equal(to_pixel(xy, None), xy)


def test_rasterize_argument_checks(no_device):
    from obia_amd.polygons import rasterize
    sq = wkb_polygon([R.rect(0, 0, 2, 2)])
    for bad in ((4,), (0, 4), (4, -1), (4.5, 4), "ab", None, (4, 4, 4)):
        with pytest.raises(ValueError, match="out_shape"):
            rasterize([sq], bad)
    with pytest.raises(ValueError, match="values"):
        rasterize([sq, sq], (4, 4), values=[1])
    with pytest.raises(ValueError, match="values"):
        rasterize([sq], (4, 4), values=[1.5])
    with pytest.raises(ValueError, match="values"):
        rasterize([sq], (4, 4), values=[2 ** 31])
    with pytest.raises(ValueError, match="shapes must be"):
        rasterize(sq, (4, 4))
    with pytest.raises(ValueError, match="shapes must be"):
        rasterize(7, (4, 4))
    with pytest.raises(ValueError, match="not WKB"):
        rasterize([sq, "POLYGON ((0 0, 1 0, 1 1, 0 0))"], (4, 4))
    with pytest.raises(ValueError, match="Polygon or MultiPolygon"):
        rasterize([struct.pack("<BI2d", 1, 1, 0.0, 0.0)], (4, 4))                 # a Point
    with pytest.raises(ValueError, match="Polygon or MultiPolygon"):
        rasterize([b"\x00" + sq[1:]], (4, 4))                                      # big-endian flag
    with pytest.raises(ValueError, match="truncated"):
        rasterize([sq[:-8]], (4, 4))
    with pytest.raises(ValueError, match="finite"):
        rasterize([wkb_polygon([[(0, 0), (np.nan, 1), (1, 1)]])], (4, 4))
    with pytest.raises(ValueError, match="singular"):
        rasterize([sq], (4, 4), affine_transformation=[1, 1, 1, 1, 0, 0])
    with pytest.raises(ValueError, match="six values"):
        rasterize([sq], (4, 4), affine_transformation=[1, 0, 0, 1, 0])
    with pytest.raises(ValueError, match="fill"):
        rasterize([sq], (4, 4), fill=2 ** 31)
    xy, off, owner = R.pack([[R.rect(0, 0, 2, 2)], [R.rect(1, 1, 3, 3)]])
    with pytest.raises(ValueError, match=r"\(V, 2\)"):
        rasterize((xy.ravel(), off, owner), (4, 4))
    with pytest.raises(ValueError, match="one more entry"):
        rasterize((xy, off[:-1], owner), (4, 4))
    with pytest.raises(ValueError, match="ring_offset"):
        rasterize((xy, off[::-1].copy(), owner), (4, 4))
    with pytest.raises(ValueError, match="ring_offset"):
        rasterize((xy[:-1], off, owner), (4, 4))
    with pytest.raises(ValueError, match="ring_shape"):
        rasterize((xy, off, owner[::-1].copy()), (4, 4))
    with pytest.raises(ValueError, match="ring_shape"):
        rasterize((xy, off, owner), (4, 4), values=[1])
    with pytest.raises(NotImplementedError, match="2\\^31"):
        rasterize([sq], (65536, 32768))


def test_rasterize_has_no_cpu_path():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from obia_amd.polygons import rasterize
    with pytest.raises(RuntimeError):
        rasterize([wkb_polygon([R.rect(0, 0, 2, 2)])], (4, 4))


def _gpkg(tmp_path, wkbs, ids, epsg=32610, name="segments.gpkg"):
    from obia_amd.geopackage import write_geopackage
    return write_geopackage(str(tmp_path / name), wkbs, {"segment_id": ids}, srs_epsg=epsg)


PROFILE = {"height": 8, "width": 9, "transform": (1.0, 0.0, 100.0, 0.0, -1.0, 50.0)}


def test_rasterise_slic_gpkg_argument_errors(no_device, tmp_path):
    from obia_amd.cost import rasterise_slic_gpkg
    path = _gpkg(tmp_path, [wkb_polygon([R.rect(101, 45, 104, 48)])], [1])
    with pytest.raises(ValueError, match="height, width and transform"):
        rasterise_slic_gpkg(path, {"height": 8, "width": 9})
    with pytest.raises(ValueError, match="height, width and transform"):
        rasterise_slic_gpkg(path, None)
    with pytest.raises(ValueError, match="positive"):
        rasterise_slic_gpkg(path, dict(PROFILE, height=0))
    with pytest.raises(ValueError, match="transform"):
        rasterise_slic_gpkg(path, dict(PROFILE, transform=(1.0, 0.0, 100.0)))
    with pytest.raises(ValueError, match="bounds"):
        rasterise_slic_gpkg(path, dict(PROFILE, bounds=(0, 1, 2)))
    with pytest.raises(ValueError, match="not a GeoPackage|no feature table"):
        import sqlite3
        other = str(tmp_path / "other.gpkg")
        sqlite3.connect(other).close()
        rasterise_slic_gpkg(other, PROFILE)


def test_rasterise_slic_gpkg_exits_like_the_reference(no_device, tmp_path):
    from obia_amd.cost import rasterise_slic_gpkg
    sq = wkb_polygon([R.rect(101, 45, 104, 48)])
    empty = struct.pack("<BII", 1, 3, 0)
    with pytest.raises(SystemExit, match="SLIC GPKG has no polygons over this tile."):
        rasterise_slic_gpkg(_gpkg(tmp_path, [], []), PROFILE)
    path = _gpkg(tmp_path, [sq, sq], [1, 2])
    with pytest.raises(SystemExit, match="SLIC GPKG has no polygons over this tile."):
        rasterise_slic_gpkg(path, dict(PROFILE, bounds=(200.0, 0.0, 300.0, 40.0)))
    with pytest.raises(SystemExit, match="No valid SLIC polygons with 'segment_id' found."):
        rasterise_slic_gpkg(_gpkg(tmp_path, [sq, sq], ["a", "b"]), PROFILE)
    import sqlite3
    path = _gpkg(tmp_path, [sq, sq], [1, 2])                 # one empty geometry (flag bit 4, no envelope), one NULL
    con = sqlite3.connect(path)
    con.execute("UPDATE segments SET geom = ? WHERE fid = 1", (b"GP" + struct.pack("<BBi", 0, 0x11, 32610) + empty,))
    con.execute("UPDATE segments SET geom = NULL WHERE fid = 2")
    con.commit()
    con.close()
    with pytest.raises(SystemExit, match="No valid SLIC polygons with 'segment_id' found."):
        rasterise_slic_gpkg(path, PROFILE)
    with pytest.raises(SystemExit, match="SLIC GPKG has no polygons over this tile."):
        rasterise_slic_gpkg(path, dict(PROFILE, bounds=(100.0, 42.0, 109.0, 50.0)))


def test_rasterise_slic_gpkg_does_not_reproject(no_device, tmp_path):
    from obia_amd.cost import rasterise_slic_gpkg
    path = _gpkg(tmp_path, [wkb_polygon([R.rect(101, 45, 104, 48)])], [1], epsg=32610)
    with pytest.raises(NotImplementedError, match="reprojection"):
        rasterise_slic_gpkg(path, dict(PROFILE, crs="EPSG:4326"))
    with pytest.raises(NotImplementedError, match="reprojection"):
        rasterise_slic_gpkg(path, dict(PROFILE, crs="a WKT string"))
    with pytest.raises(AssertionError, match="device library"):                  # the same code goes on to the device
        rasterise_slic_gpkg(path, dict(PROFILE, crs="EPSG:32610", bounds=(100.0, 42.0, 109.0, 50.0)))


def test_profile_transform_forms():
    from obia_amd.cost import _profile_transform

    class Affine:
        a, b, c, d, e, f = 0.5, 0.0, 443210.0, 0.0, -0.5, 6012345.5
    assert _profile_transform(Affine()) == [0.5, 0.0, 0.0, -0.5, 443210.0, 6012345.5]
    assert _profile_transform((0.5, 0.0, 443210.0, 0.0, -0.5, 6012345.5)) == [0.5, 0.0, 0.0, -0.5, 443210.0, 6012345.5]
