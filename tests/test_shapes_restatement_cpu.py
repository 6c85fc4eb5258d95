"""The shape columns without a GPU: the restatement (tests/shapes_restatement.py) against a double loop over pixels with Python
integers and against scikit-image's regionprops (tests/golden/shapes/*.npz, written by tests/golden/gen_goldens_shapes.py); closed
forms; translation; merge and pair_shapes against recomputation on the relabelled raster; the perimeter against the adjacency
restatement; what the header says; what the source file must not do; the refusals of the Python functions that fire before the library is loaded; the overflow rule at its threshold.

COMPARISON WITH SCIKIT-IMAGE 0.18.3.  Integer fields (area, bbox) are equal.  For the float fields the restatement's largest deviation
from the goldens over the three maps was measured (NumPy 2.x, x86-64) and the bound is 8 x the measured value:

    field                     measured              bound
    centroid  (relative)      0                     0        (equal)
    extent    (relative)      0                     0        (equal)
    mu / trace of the tensor  6.50e-16              5.20e-15
    eigenvalues (relative)    3.28e-15              2.62e-14
    eccentricity (relative)   5.53e-15              4.42e-14
    major axis (relative)     4.34e-16              3.47e-15
    minor axis (relative)     1.62e-15              1.30e-14
    orientation (absolute)    2.78e-15              2.22e-14

No segment of the three maps has equal eigenvalues (smallest relative gap 0.043), so none is left out of the orientation comparison."""
import os
import re

import numpy as np
import pytest

from tests import adjacency_restatement as R
from tests import shapes_restatement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MAPS = ("c2s_256x256x4_c025", "quickstart_128x128x3", "mask_128x160x4_c025")
F64, I32, I64 = np.float64, np.int32, np.int64
# 8 x the measured deviations of the module docstring
BOUNDS = {"mu": 8 * 6.50e-16, "eigenvalues": 8 * 3.28e-15, "eccentricity": 8 * 5.53e-15, "major_axis_length": 8 * 4.34e-16,
          "minor_axis_length": 8 * 1.62e-15, "orientation": 8 * 2.78e-15}


def rasters():
    """30 random rasters of at most 12 x 12: labels in -1 .. 6, start_label 1 or 0, n_labels 5 (so 0 or -1, and 6, are background)"""
    rs = np.random.RandomState(17)
    out = []
    for k in range(30):
        H, W = rs.randint(1, 13), rs.randint(1, 13)
        lab = rs.randint(-1, (3, 7, 7)[k % 3], (H, W))
        if k % 5 == 4:
            lab = np.kron(lab, np.ones((2, 3), int))[:H, :W]
        out.append((lab.astype(I32), k % 2, 5))
    return out


def blob(h=9, w=13, seed=2):
    """an irregular blob of one segment inside an (h, w) window"""
    rs = np.random.RandomState(seed)
    m = rs.uniform(size=(h, w)) < 0.7
    m[h // 2, :] = True
    m[:, w // 2] = True
    return m


# ------------------------------------------------------------------------------------------------------------ the integer tables
def test_the_restatement_is_the_double_loop_over_pixels():
    for lab, start, N in rasters():
        got, want = S.tables(lab, start, N), S.tables_loop(lab, start, N)
        assert S.same_bits(got[0], want[0]) and S.same_bits(got[1], want[1]), (lab.tolist(), start)
        empty = got[0][:, 0] == 0
        assert not got[0][empty].any() and not got[1][empty].any()                 # a row without pixels is all zeros
    sums, box = S.tables(np.zeros((3, 4), I32), 1, 0)
    assert sums.shape == (0, 7) and box.shape == (0, 4)


def test_the_perimeter_is_the_row_sum_of_the_adjacency_graph():
    for lab, start, N in rasters():
        indptr, _, border = R.graph(lab, start, N)
        assert np.array_equal(S.tables(lab, start, N)[0][:, 6], R.row_sum(indptr, border))


def test_one_label_in_two_places_is_one_row_and_a_known_answer():
    lab = np.array([[1, 2, 1],
                    [0, 2, 3]], I32)
    sums, box = S.tables(lab, 1, 3)
    assert sums.tolist() == [[2, 0, 2, 0, 4, 0, 8], [2, 1, 2, 1, 2, 1, 6], [1, 1, 2, 1, 4, 2, 4]]
    assert box.tolist() == [[0, 0, 1, 3], [0, 1, 2, 2], [1, 2, 2, 3]]


# ----------------------------------------------------------------------------------------------------- against scikit-image
@pytest.mark.parametrize("name", MAPS)
def test_against_regionprops_of_scikit_image(name):
    lab = np.load(os.path.join(GOLDEN, name + ".npz"))["labels"]
    g = np.load(os.path.join(GOLDEN, "shapes", name + ".npz"))
    assert str(g["skimage_version"]) == "0.18.3"
    N = int(lab.max())
    sums, box = S.tables(lab, 1, N)
    d = S.derived(sums, box)
    idx = g["label"].astype(I64) - 1
    assert np.array_equal(np.flatnonzero(d["present"]), idx)
    assert np.array_equal(d["area"][idx], g["area"]) and np.array_equal(box[idx], g["bbox"]) and g["area"].min() >= 3
    assert np.array_equal(d["centroid"][idx], g["centroid"]) and np.array_equal(d["extent"][idx], g["extent"])
    T, ev = g["inertia_tensor"], g["inertia_tensor_eigvals"]
    assert (ev[:, 0] > ev[:, 1]).all()                                             # no isotropic segment: every orientation is compared
    trace = T[:, 0, 0] + T[:, 1, 1]
    mu = d["mu"][idx]
    measured = {"mu": max(np.max(np.abs(mu[:, 0] - T[:, 1, 1]) / trace), np.max(np.abs(mu[:, 1] - T[:, 0, 0]) / trace),
                          np.max(np.abs(mu[:, 2] + T[:, 0, 1]) / trace)),
                "eigenvalues": np.max(np.abs(d["eigenvalues"][idx] - ev) / ev),
                "orientation": np.max(np.abs(d["orientation"][idx] - g["orientation"]))}
    for k in ("eccentricity", "major_axis_length", "minor_axis_length"):
        measured[k] = np.max(np.abs(d[k][idx] - g[k]) / g[k])
    print(name, {k: float(v) for k, v in measured.items()})
    for k, v in measured.items():
        assert v <= BOUNDS[k], (k, float(v), BOUNDS[k])


# ------------------------------------------------------------------------------------------------------------------ closed forms
def one_segment(mask, at=(0, 0), shape=None):
    h, w = mask.shape
    lab = np.zeros(shape or (at[0] + h + 1, at[1] + w + 2), I32)
    lab[at[0]:at[0] + h, at[1]:at[1] + w] = mask
    sums, box = S.tables(lab, 1, 1)
    return S.derived(sums, box), sums, box


@pytest.mark.parametrize("k", [1, 2, 5, 16])
def test_a_square(k):
    d, sums, box = one_segment(np.ones((k, k), bool), (3, 4))
    assert d["area"][0] == k * k and d["perimeter"][0] == 4 * k and box.tolist() == [[3, 4, 3 + k, 4 + k]]
    assert d["compactness"][0] == (F64(4.0) * F64(np.pi) * F64(k * k)) / F64(16 * k * k) and abs(d["compactness"][0] - np.pi / 4) < 1e-15
    assert d["shape_index"][0] == 1.0 and d["extent"][0] == 1.0 and d["smoothness"][0] == 1.0
    assert d["centroid"][0].tolist() == [3 + (k - 1) / 2, 4 + (k - 1) / 2]
    assert d["mu"][0].tolist() == [(k * k - 1) / 12, (k * k - 1) / 12, 0.0]
    assert d["eigenvalues"][0, 0] == d["eigenvalues"][0, 1] and d["eccentricity"][0] == 0.0
    assert d["orientation"][0] == np.pi / 4                                       # isotropic, mu_rc == 0: scikit-image's +pi/4


def test_a_rectangle_a_pixel_and_a_row_of_pixels():
    a, b = 5, 7                                                                  # (k^2 - 1) / 12 = 2 and 4: exact in binary
    d, _, _ = one_segment(np.ones((a, b), bool), (1, 2))
    assert d["area"][0] == a * b and d["perimeter"][0] == 2 * (a + b) and d["extent"][0] == 1.0 and d["smoothness"][0] == 1.0
    assert d["mu"][0].tolist() == [(a * a - 1) / 12, (b * b - 1) / 12, 0.0]
    assert d["eigenvalues"][0].tolist() == [(b * b - 1) / 12, (a * a - 1) / 12]
    assert d["major_axis_length"][0] == 4 * np.sqrt(F64((b * b - 1) / 12)) and d["minor_axis_length"][0] == 4 * np.sqrt(F64((a * a - 1) / 12))
    assert d["orientation"][0] == 0.5 * np.arctan2(F64(0.0), F64((a * a - 1) / 12 - (b * b - 1) / 12)) == np.pi / 2   # along the columns
    assert d["shape_index"][0] == F64(2 * (a + b)) / (4 * np.sqrt(F64(a * b)))
    d, _, box = one_segment(np.ones((1, 1), bool), (5, 6))
    assert d["area"][0] == 1 and d["perimeter"][0] == 4 and box.tolist() == [[5, 6, 6, 7]] and d["centroid"][0].tolist() == [5.0, 6.0]
    assert d["mu"][0].tolist() == [0, 0, 0] and d["eigenvalues"][0].tolist() == [0, 0] and d["eccentricity"][0] == 0 and d["major_axis_length"][0] == 0
    d, _, _ = one_segment(np.ones((1, 7), bool), (2, 0))
    assert d["eigenvalues"][0].tolist() == [4.0, 0.0] and d["eccentricity"][0] == 1.0 and d["minor_axis_length"][0] == 0 and d["perimeter"][0] == 16
    d, _, _ = one_segment(np.ones((7, 1), bool), (2, 0))
    assert d["eigenvalues"][0].tolist() == [4.0, 0.0] and d["eccentricity"][0] == 1.0 and d["orientation"][0] == 0.0
    # a diagonal pair: mu_rr == mu_cc, mu_rc > 0 -> -pi/4 (scikit-image's b = -mu_rc < 0)
    d, _, _ = one_segment(np.eye(2, dtype=bool))
    assert d["mu"][0].tolist() == [0.25, 0.25, 0.25] and d["orientation"][0] == -np.pi / 4
    d, _, _ = one_segment(np.eye(2, dtype=bool)[::-1])
    assert d["orientation"][0] == np.pi / 4


def test_an_empty_row_is_the_quiet_nan_in_every_float_column():
    d = S.derived(*S.tables(np.array([[1, 3]], I32), 1, 3))
    assert d["present"].tolist() == [True, False, True]
    for k in S.FLOAT_COLUMNS:
        assert S.same_bits(np.atleast_2d(d[k][1]).ravel(), np.full(np.atleast_2d(d[k][1]).size, S.NAN)), k
        assert not np.isnan(d[k][[0, 2]]).any(), k
    for k in S.INT_COLUMNS:
        assert d[k][1] == 0 and d[k].dtype == I64


def test_a_blob_moved_by_whole_pixels_keeps_its_bits():
    m = blob()
    here, s0, _ = one_segment(m, (0, 0), (40, 40))
    there, s1, _ = one_segment(m, (30000, 21), (30040, 40))
    assert s1[0, 3] > 2 ** 33 and not np.array_equal(s0, s1)
    for k in S.FLOAT_COLUMNS:
        if k != "centroid":
            assert S.same_bits(here[k], there[k]), k
    assert np.abs(there["centroid"] - (here["centroid"] + [30000, 21])).max() < 1e-9
    xy = S.centroid_xy(here["centroid"], [0.5, 0.0, 0.0, -0.5, 100.0, 200.0])
    assert xy[0].tolist() == [100.0 + 0.5 * (here["centroid"][0, 1] + 0.5), 200.0 - 0.5 * (here["centroid"][0, 0] + 0.5)]


# --------------------------------------------------------------------------------------------------------- merge and pair shapes
def test_merge_is_the_recomputation_on_the_relabelled_raster():
    rs = np.random.RandomState(9)
    tried = 0
    for lab, start, N in rasters():
        indptr, nb, border = R.graph(lab, start, N)
        sums, box = S.tables(lab, start, N)
        for p in (0.0, 0.4, 1.0):
            link = rs.uniform(size=len(nb)) < p
            root = R.components(indptr, nb, N, link)
            msums, mbox = S.merge(sums, box, root, indptr, nb, border)
            off = np.ones(N, bool)
            off[root] = False
            assert not msums[off].any() and not mbox[off].any()                    # stored at row root[i], every other row empty
            table = R.compact_roots(root, start, sums[:, 0] > 0)
            relab = R.relabel(lab, table, start)
            n_new = max(int(table.max()) - start + 1, 0) if N else 0
            want = S.tables(relab, start, n_new)
            keep = np.flatnonzero(msums[:, 0] > 0)                                 # the objects with pixels, in ascending order of root
            assert S.same_bits(msums[keep], want[0]) and S.same_bits(mbox[keep], want[1]), (lab.tolist(), start, p)
            tried += len(keep) < (sums[:, 0] > 0).sum()
    assert tried > 10


def test_pair_shapes_is_the_shape_of_the_union():
    for lab, start, N in rasters()[:12]:
        indptr, nb, border = R.graph(lab, start, N)
        sums, box = S.tables(lab, start, N)
        pairs = S.pair_shapes(indptr, nb, border, sums, box)
        rows = R.rows_of(indptr)
        for e in range(len(nb)):
            i, j = int(rows[e]), int(nb[e])
            if j >= N:
                assert pairs["area"][e] == 0 and pairs["perimeter"][e] == 0 and not pairs["box"][e].any()
                assert all(S.same_bits(pairs[k][e:e + 1], np.array([S.NAN])) for k in ("compactness", "shape_index", "smoothness"))
                continue
            both = np.where(np.asarray(lab) == j + start, i + start, lab)
            usums, ubox = S.tables(both, start, N)
            d = S.derived(usums, ubox)
            assert pairs["area"][e] == usums[i, 0] and pairs["perimeter"][e] == usums[i, 6] and pairs["box"][e].tolist() == ubox[i].tolist()
            assert all(S.same_bits(pairs[k][e:e + 1], d[k][i:i + 1]) for k in ("compactness", "shape_index", "smoothness"))


# ------------------------------------------------------------------------------------------------- the header and the source
def test_the_header_says_there_is_no_overflow_path():
    full = open(os.path.join(ROOT, "include", "obia_shapes.h")).read()
    assert "THERE IS NO OVERFLOW PATH" in full and "NO SUM OVERFLOWS" in full and "The reference has no counterpart" in full


def test_the_source_takes_no_workspace_and_every_atomic_is_on_an_integer():
    src = open(os.path.join(ROOT, "obia_amd", "csrc", "shapes.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"arena\.(get|alloc)\b|\bA\.get<|\.arena\b", src)   # every buffer is the caller's
    assert not re.search(r"hipMalloc|hipFree|hipHostMalloc|Staging|upload_async|read_back", code)
    assert not re.search(r"\b(float|double)\b", code)                        # no floating-point value anywhere, so no such atomic
    targets = {"keys": r"\bint keys\[", "acc": r"\bint acc\[", "s_n": r"\bint s_n\b", "row": r"unsigned long long \*row\b", "corner": r"\bint \*corner\b"}
    found = list(re.finditer(r"\batomic([A-Za-z]+)\s*\(\s*&(\w+)", code))
    assert len(found) == len(re.findall(r"\batomic[A-Z]\w*\s*\(", code)) >= 10
    for m in found:
        assert m.group(1) in ("Add", "Max", "Or", "CAS") and m.group(2) in targets, m.group(0)
        assert re.search(targets[m.group(2)], code), m.group(2)
    assert "unsafeAtomic" not in code and not re.search(r"__hip_atomic_fetch|__atomic_fetch", code)
    # every launch takes its grid from launch_grids.hpp, by name; no dim3 carries a clamp
    sites = re.findall(r"hipLaunchKernelGGL\([^;]*;", code)
    assert len(sites) == 2
    for site in sites:
        assert re.search(r"to_dim3\(grids::(flat|adj_tiles)\(", site) and "dim3(256)" in site, site
    assert not re.search(r"std::min|std::max", code)
    mk = open(os.path.join(ROOT, "obia_amd", "csrc", "Makefile")).read()
    assert " shapes.o" in mk and "../../include/obia_shapes.h" in mk


# ------------------------------------------------------------------------------------------------------------------- the wrappers
def test_public_names_and_refusals_before_any_device_use(monkeypatch):
    pytest.importorskip("torch")
    import torch
    import obia_amd
    from obia_amd import _lib, shapes as SH
    for name in ("ShapeTable", "segment_shapes", "pair_shapes", "shape_columns"):
        assert getattr(obia_amd, name) is getattr(SH, name)
    for prop in ("sums", "box", "present", "area", "perimeter", "bbox_height", "bbox_width", "centroid", "mu", "eigenvalues", "major_axis_length",
                 "minor_axis_length", "eccentricity", "orientation", "extent", "compactness", "shape_index", "smoothness"):
        assert isinstance(getattr(SH.ShapeTable, prop), property), prop
    assert callable(SH.ShapeTable.merge) and callable(SH.ShapeTable.centroid_xy)

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    lab = np.ones((4, 5), np.int32)
    for bad in (np.ones(5, np.int32), np.ones((0, 5), np.int32), np.ones((2, 2, 2), np.int32)):
        with pytest.raises(ValueError, match="non-empty"):
            SH.segment_shapes(bad)
    with pytest.raises(ValueError, match="n_labels"):
        SH.segment_shapes(lab, n_labels=-1)
    with pytest.raises(ValueError, match="n_labels"):
        SH.segment_shapes(lab, n_labels=2 ** 31 - 2)
    with pytest.raises(ValueError, match="start_label"):
        SH.segment_shapes(lab, start_label=1.5)
    with pytest.raises(ValueError, match="GPU"):
        SH.segment_shapes(torch.ones((4, 5), dtype=torch.int32))              # a CPU tensor is refused: its pointer reaches no kernel
    with pytest.raises(NotImplementedError, match="2\\^31"):
        SH.segment_shapes(np.broadcast_to(np.int32(1), (65536, 32768)))
    with pytest.raises(NotImplementedError, match="2\\^63"):
        SH.segment_shapes(np.broadcast_to(np.int32(1), (1, 2 ** 21)))         # no allocation: a broadcast view


def test_the_overflow_rule_is_at_its_threshold():
    pytest.importorskip("torch")
    from obia_amd import shapes as SH
    for H in (1, 4, 1000):
        lo, hi = H, 2 ** 31
        while hi - lo > 1:                                                      # the smallest refused W >= H, by bisection of the exact rule
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if mid * mid * H * mid >= 2 ** 63 else (mid, hi)
        assert lo ** 3 * H < 2 ** 63 <= hi ** 3 * H and lo * H < 2 ** 31
        for shape in ((H, lo), (lo, H)):
            SH._check_sums_fit(*shape)                                          # one below: served
        for shape in ((H, hi), (hi, H)):
            with pytest.raises(NotImplementedError):
                SH._check_sums_fit(*shape)
    assert 2 ** 21 - 1 == max(w for w in (2 ** 21 - 1, 2 ** 21) if w ** 3 < 2 ** 63)      # the header's example
    # the largest sum a served raster can hold fits: every pixel one segment, sum r^2 and sum c^2 and sum r c
    for H, W in ((1, 2 ** 21 - 1), (46340, 46340), (2 ** 15, 2 ** 16 - 1)):
        SH._check_sums_fit(H, W)
        assert max(H - 1, W - 1) ** 2 * H * W < 2 ** 63
