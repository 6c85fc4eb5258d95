"""tests/guarded.py on NumPy buffers: every planted fault is reported where it was planted, and a correctly written payload gives no
finding.  No GPU."""
import numpy as np
import pytest

from tests.guarded import GUARD_MIN, POISONS, guard_bytes, guarded, guarded_array, holds_poison, poison_value, snapshot, unchanged

DTYPES = [np.uint8, np.int32, np.float32, np.int64, np.float64]
SHAPES = [(37, 53), (5,), (3, 700), (2, 3, 4)]


def written(g, seed=0):
    """fill the payload with values of which no element is all-poison"""
    rs = np.random.RandomState(seed)
    if g.dtype.kind == "f":
        v = rs.uniform(-3, 3, g.shape).astype(g.dtype)
    else:
        v = rs.randint(0, 80, g.shape).astype(g.dtype)
    assert not holds_poison(v)
    g.t[...] = v
    return v


def test_poison_values():
    assert poison_value(np.int32, 0xA5) == -1515870811 and poison_value(np.int32, 0x5A) == 1515870810
    for p in POISONS:
        assert poison_value(np.uint8, p) not in (0, 1)
        for dt in (np.float32, np.float64):
            assert np.isfinite(poison_value(dt, p))
    assert holds_poison(np.array([0, -1515870811], np.int32)) and holds_poison(np.array([poison_value(np.float64, 0x5A)]))
    assert not holds_poison(np.arange(100, dtype=np.int32)) and not holds_poison(np.zeros(0, np.float32))


def test_guard_size_is_4096_or_two_rows():
    assert guard_bytes((37, 53), 4) == GUARD_MIN == 4096
    assert guard_bytes((3, 700), 8) == 2 * 700 * 8                      # two rows of 5600 bytes
    assert guard_bytes((3, 701), 1) == 4096 and guard_bytes((3, 2051), 1) == 4112     # 4102 rounded up to a multiple of 16
    assert guard_bytes((5,), 8) == 4096
    g = guarded_array((3, 700), np.float64, 0xA5)
    assert g.guard == 11200 and g.front == 11200 and len(g.buf) >= 2 * 11200 + g.nbytes


@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("poison", POISONS, ids=hex)
def test_layout_and_a_clean_write(dtype, k, poison):
    for shape in SHAPES:
        g = guarded(shape, dtype, poison, "numpy", k)
        it = np.dtype(dtype).itemsize
        assert g.t.shape == shape and g.t.dtype == np.dtype(dtype) and g.t.flags["C_CONTIGUOUS"]
        assert g.ptr == g.t.ctypes.data and g.ptr % 16 == (k * it) % 16
        assert (g.buf == poison).all() and g.untouched()
        assert g.front == g.guard + k * it
        assert len(g.unwritten()) == g.t.size and len(g.stray()) == 0          # nothing written yet: every element, no stray byte
        v = written(g)
        assert g.findings() == [] and not g.untouched()
        assert np.array_equal(g.host(), v)


def test_torch_cpu_twin():
    torch = pytest.importorskip("torch")
    for k in (0, 1, 3):
        g = guarded((7, 9), torch.int32, 0x5A, "cpu", k)
        assert g.t.dtype == torch.int32 and tuple(g.t.shape) == (7, 9) and g.t.is_contiguous() and g.t.data_ptr() % 16 == (4 * k) % 16
        assert len(g.unwritten()) == 63
        g.t.copy_(torch.arange(63, dtype=torch.int32).view(7, 9))
        assert g.findings() == []
        g.buf[g.lo + g.nbytes] = 0
        assert g.stray().tolist() == [0]


@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("dtype", [np.uint8, np.int32, np.float64], ids=lambda d: np.dtype(d).name)
def test_stray_bytes_are_found_where_they_were_planted(dtype, k):
    shape = (6, 700)
    it = np.dtype(dtype).itemsize
    row = 700 * it
    plants = {"the byte before the payload": -1, "the first byte past the end": 0, "one row beyond the end": row,
              "one row before the start": -row - 1}
    for what, o in plants.items():
        g = guarded_array(shape, dtype, 0xA5, k)
        written(g)
        g.buf[g.lo + (g.nbytes + o if o >= 0 else o)] ^= 0xFF
        assert g.stray().tolist() == [o], what
        f = g.findings(name="out")
        assert len(f) == 1 and "stray" in f[0] and str(o) in f[0], what
    g = guarded_array(shape, dtype, 0x5A, k)
    written(g)
    g.buf[g.lo + g.nbytes + g.guard - 1] = 0                         # the last guard byte
    g.buf[g.lo - g.front] = 0                                         # the first one
    assert g.stray().tolist() == [-g.front, g.guard - 1] and g.guard >= 2 * row
    if k:                                                             # the slack between guard and payload is watched too
        g = guarded_array(shape, dtype, 0x5A, k)
        written(g)
        g.buf[g.lo - k * it] = 1
        assert g.stray().tolist() == [-k * it]


def test_a_stray_write_of_the_poison_value_itself_cannot_be_seen_but_the_other_poison_sees_it():
    """why the driver runs every case at both poisons"""
    hit = {}
    for p in POISONS:
        g = guarded_array((4, 4), np.uint8, p)
        written(g)
        g.buf[g.lo + g.nbytes] = 0xA5
        hit[p] = g.stray().tolist()
    assert hit == {0xA5: [], 0x5A: [0]}


@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("poison", POISONS, ids=hex)
def test_one_unwritten_element_is_found(dtype, k, poison):
    shape = (37, 53)
    n = 37 * 53
    for where in (0, n // 2, n - 1):
        g = guarded_array(shape, dtype, poison, k)
        v = written(g)
        g.t.reshape(-1)[where] = poison_value(dtype, poison)
        assert g.unwritten().tolist() == [where]
        f = g.findings(name="labels")
        assert len(f) == 1 and "unwritten" in f[0] and str(tuple(int(x) for x in np.unravel_index(where, shape))) in f[0]
        ex = np.zeros(shape, bool)
        ex.reshape(-1)[where] = True
        assert g.findings(exempt=ex) == []                            # ... unless the header promises nothing for it
        assert len(g.stray()) == 0
        del v
    if np.dtype(dtype).itemsize > 1:                                  # an element of which ONE byte changed is written
        g = guarded_array(shape, dtype, poison, k)
        g.buf[g.lo] ^= 1
        assert 0 not in g.unwritten().tolist() and len(g.unwritten()) == n - 1


def test_empty_payload():
    g = guarded_array((0, 5), np.int32, 0xA5, 1)
    assert g.findings() == [] and g.ptr % 16 == 4 and g.untouched()
    g.buf[g.lo] = 0
    assert g.stray().tolist() == [0]


def test_a_modified_input_is_seen():
    a = np.random.RandomState(1).normal(size=(9, 11)).astype(np.float32)
    a[3, 3] = np.nan                                                  # bytes are compared: a NaN equals itself
    s = snapshot(a)
    assert unchanged(a, s) and unchanged(a.copy(), s)
    b = a.copy()
    b.view(np.uint32)[8, 10] ^= 1                                     # one bit
    assert not unchanged(b, s)
    assert not unchanged(a.astype(np.float64), s) and not unchanged(a.reshape(11, 9), s)
    c = a.copy()
    c[0, 0] = -c[0, 0]
    assert not unchanged(c, s)
    torch = pytest.importorskip("torch")
    t = torch.as_tensor(a.copy())
    st = snapshot(t)
    assert st == s and unchanged(t, st)
    t[8, 10] += 1
    assert not unchanged(t, st)


def test_every_entry_point_with_an_output_has_a_decision():
    """Every name of obia_amd/_lib.py: _SIGNATURES is in exactly one of three lists of tests/test_gpu_output_guards.py: the registry
    of guarded cases, LEFT_OUT (takes a caller output, no case, with the reason: DESIGN.md 3.8) or NO_OUTPUT_BUFFER.  A new entry
    point fails this test until somebody decides where it belongs."""
    pytest.importorskip("torch")
    from obia_amd import _lib
    from tests import test_gpu_output_guards as G
    covered = G.covered_entry_points()
    assert covered == set(COVERED), sorted(covered ^ set(COVERED))
    groups = [covered, set(G.LEFT_OUT), set(G.NO_OUTPUT_BUFFER)]
    for i, a in enumerate(groups):
        for b in groups[i + 1:]:
            assert not a & b, sorted(a & b)
    assert set().union(*groups) == set(_lib._SIGNATURES), sorted(set().union(*groups) ^ set(_lib._SIGNATURES))
    assert all(len(reason) > 20 for reason in G.LEFT_OUT.values())
    for c in G.REGISTRY.values():                           # label rasters also run 3 elements off the boundary
        assert c.ks in ((0, 1), (0, 1, 3)) and c.entries


# the entry points the registry of tests/test_gpu_output_guards.py must cover (kept here by hand, see the test above)
COVERED = [
    "obia_slic_f32", "obia_slic_f32_dev", "obia_slic_assign_only_f32_dev", "obia_slic_seeded_f32_dev", "obia_enforce_connectivity_i32_dev",
    "obia_mask_centroids_dev", "obia_slic_stages_f32_dev", "obia_quickshift_f32", "obia_quickshift_f32_dev", "obia_quickshift_stages_f32_dev",
    "obia_tiled_slic_f32", "obia_tiled_slic_f32_dev", "obia_tiled_slic_seeded_f32", "obia_tiled_slic_seeded_f32_dev",
    "obia_zonal_stats_f32", "obia_zonal_stats_f32_dev", "obia_zonal_moments_f32", "obia_zonal_moments_f32_dev", "obia_texture_stats_f32_dev",
    "obia_polygon_rings_i32_dev", "obia_rasterize_polygons_dev", "obia_label_edges_u8_dev", "obia_sample_labels_i32_dev",
    "obia_cost_bands_f32_dev", "obia_cost_ndvi_f32_dev", "obia_cost_sobel_f32_dev", "obia_cost_select_dev", "obia_cost_entropy_f32_dev",
    "obia_cost_normalise_dev", "obia_cost_combine_dev",
    "obia_seeds_peaks_dev", "obia_seeds_peaks_gather_dev", "obia_seeds_pair_link_dev", "obia_seeds_pair_stats_dev", "obia_seeds_pair_matrix_dev",
    "obia_table_scale_dev", "obia_table_scale_f64_dev", "obia_forest_predict_dev", "obia_forest_shap_dev", "obia_mlp_predict_dev",
    "obia_mlp_coalition_dev", "obia_shapley_combine_dev",
]
