"""Region merging on the GPU (include/obia_merging.h, obia_amd/csrc/merging.hip, obia_amd/merging.py) against the restatement
(tests/merging_restatement.py), bit for bit: the fusion cost, the pair merge with every defensive reading of `partner`, the
contraction against the restatement AND against ``segment_graph(relabel(...))``, rows around OBIA_MERGE_ROW_CAP, a path long enough
for second trips of the clamped launches, the driver round by round, the state after every round against a recomputation on the
relabelled raster, reproducibility and both input types.

MEAN AND M2 AFTER MERGING against ``zonal_stats`` of the relabelled raster (test_state_after_every_round).  On that case -- the recovery
case, seed 0, all ten rounds, one MI355X -- the state's distance from NumPy float64 (np.mean, np.var of the float32 pixels taken as
float64) was measured: mean 1.453e-16 of the range of the segment means, m2 / area 1.450e-14 of the largest variance
(``zonal_stats`` itself: 0 and 1.492e-14).  The bound on the distance between the two is 8 x those figures, MEAN_MEASURED and
VAR_MEASURED below; the distances seen were at most 1.453e-16 and 2.095e-15.  The test prints what it sees."""
import functools
import os

import numpy as np
import pytest

from tests import adjacency_restatement as R
from tests import merging_restatement as M

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MAPS = ("c2s_256x256x4_c025", "quickstart_128x128x3", "mask_128x160x4_c025")
F64, I32, I64 = np.float64, np.int32, np.int64
TH, TW = 16, 32
H, W, START, N = 2 * TH + 3, 2 * TW + 5, 1, 40
# measured on the recovery case, seed 0 (the module docstring)
MEAN_MEASURED, VAR_MEASURED = 1.453e-16, 1.450e-14


def block_map(seed=31):
    """(2 16 + 3) x (2 32 + 5) pixels in blocks of 3 x 4: absent labels, background below and above the table, the frame"""
    rs = np.random.RandomState(seed)
    lab = np.kron(rs.randint(-1, N + 2, (-(-H // 3), -(-W // 4))), np.ones((3, 4), int))[:H, :W].astype(I32)
    lab[lab == 5] = 4
    lab[lab == 17] = 16
    return lab


@functools.lru_cache(maxsize=None)
def case(F):
    lab = block_map()
    rs = np.random.RandomState(100 + F)
    raw = (rs.uniform(0, 50, (H, W, F)) + 20.0 * (lab[:, :, None] % 7)).astype(np.float32)
    st = M.state_of(raw, lab, START, n_labels=N)
    assert st.N == N and (st.area == 0).sum() >= 2 and (lab < START).any() and (lab >= START + N).any()
    return lab, raw, st


def device_state(st, as_tensor=False):
    from obia_amd import RegionState, SegmentGraph
    g = SegmentGraph(st.indptr, st.neighbor, st.border, st.N, START, as_tensor=as_tensor)
    return RegionState(st.area, st.mean, st.m2, st.perimeter, st.box, g, st.root, as_tensor=as_tensor)


def host(x):
    return x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def same_state(got, want, what=""):
    for name in ("area", "mean", "m2", "perimeter", "box", "root"):
        assert R.same_bits(host(getattr(got, name)), getattr(want, name)), (what, name)
    same_graph(got.graph, want.graph(), what)


def same_graph(g, want, what=""):
    for name, w in zip(("indptr", "neighbor", "border"), want):
        assert R.same_bits(host(getattr(g, name)), w), (what, name)


# ------------------------------------------------------------------------------------------------------------------------ cost
@pytest.mark.parametrize("F", [1, 3, 9])
def test_cost_equals_the_restatement_bit_for_bit(F):
    from obia_amd import fusion_cost
    lab, raw, st = case(F)
    w = np.linspace(0.25, 2.0, F)
    dev = device_state(st)
    for shape, compactness in ((0.0, 0.5), (0.1, 0.5), (1.0, 0.3), (0.4, 0.0), (0.4, 1.0)):
        got = fusion_cost(dev, w, shape, compactness)
        want = M.cost(st, w, shape, compactness)
        assert R.same_bits(got, want), (F, shape, compactness, np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))[:5])
    real = st.neighbor < N
    assert np.isnan(got[~real]).all() and not np.isnan(got[real]).any() and real.sum() > 50 and (~real).sum() > 10
    rows = R.rows_of(st.indptr)
    back = {(int(i), int(j)): e for e, (i, j) in enumerate(zip(rows, st.neighbor))}
    for e in np.flatnonzero(real):
        assert got.view(np.uint64)[e] == got.view(np.uint64)[back[(int(st.neighbor[e]), int(rows[e]))]]
    assert R.same_bits(fusion_cost(dev), M.cost(st))                                 # the defaults: unit weights


def test_the_hand_check_on_the_device():
    from obia_amd import RegionState, fusion_cost
    lab = np.array([[1, 1, 2, 2], [1, 1, 2, 2]], I32)
    raw = np.zeros((2, 4, 1), np.float32)
    raw[:, 2:] = 2
    state = RegionState.from_raster(raw, lab)
    assert state.area.tolist() == [4, 4] and state.mean.tolist() == [[0.0], [2.0]] and state.m2.tolist() == [[0.0], [0.0]]
    c = fusion_cost(state, shape=0.1, compactness=0.5)
    assert c[0] == c[2] == 7.297056274847714 and np.isnan(c[1]) and np.isnan(c[3])


# ------------------------------------------------------------------------------------------------------------------ pair merge
def test_pair_merge_with_every_defensive_reading_of_partner():
    from obia_amd import merge_pairs
    lab, raw, st = case(3)
    partner, pairs, _ = M.round_partner(st, 1e9)
    assert pairs >= 5
    dev = device_state(st)
    same_state(merge_pairs(dev, partner), M.merge_pairs(st, partner), "a round")
    free = [i for i in range(N) if partner[i] < 0 and st.area[i] > 0]
    rows = R.rows_of(st.indptr)
    adjacent = {(int(i), int(j)) for i, j in zip(rows, st.neighbor)}
    far = next((i, j) for i in free[3:] for j in free[3:] if i < j and (i, j) not in adjacent)
    odd = partner.copy()
    odd[free[0]] = N + 5                                                             # outside 0 .. N - 1
    odd[free[1]] = -7
    odd[free[2]] = free[2]                                                           # itself
    odd[far[0]], odd[far[1]] = far[1], far[0]                                        # not in the row: border 0
    single = next(i for i in free if i not in far and i not in free[:3])
    odd[single] = int(np.flatnonzero(partner >= 0)[0])                               # does not point back
    want = M.merge_pairs(st, odd)
    assert want.area[far[0]] == st.area[far[0]] + st.area[far[1]] and want.perimeter[far[0]] == st.perimeter[far[0]] + st.perimeter[far[1]]
    assert want.area[single] == st.area[single] and want.area[free[0]] == st.area[free[0]]
    same_state(merge_pairs(dev, odd), want, "defensive")
    none = np.full(N, -1, I32)
    same_state(merge_pairs(dev, none), M.merge_pairs(st, none), "no pair")


# ----------------------------------------------------------------------------------------------------------------- contraction
def by_the_raster(lab, root, start, n):
    from obia_amd import relabel, segment_graph
    return segment_graph(relabel(lab, (np.asarray(root, I64) + start).astype(I32), start), start, n_labels=n)


def test_contract_for_pair_roots_and_component_roots():
    from obia_amd import SegmentGraph
    lab, raw, st = case(1)
    g = SegmentGraph(*st.graph(), N, START)
    rs = np.random.RandomState(3)
    roots = [M.pair_root(M.round_partner(st, 1e9)[0], N), np.arange(N, dtype=I32), np.zeros(N, I32)]
    for p in (0.2, 0.5, 0.9):
        roots.append(R.components(st.indptr, st.neighbor, N, rs.uniform(size=len(st.neighbor)) < p))
    far = rs.permutation(N)                                                          # members that do not touch: any root is served
    hop = np.arange(N, dtype=I32)
    hop[far[:20]] = far[:20].min()
    roots.append(hop)
    for k, root in enumerate(roots):
        got = g.contract(root)
        same_graph(got, M.contract(*st.graph(), N, root), k)
        ref = by_the_raster(lab, root, START, N)
        same_graph(got, (ref.indptr, ref.neighbor, ref.border), k)
        assert got.n_labels == N and got.start_label == START
    with pytest.raises(ValueError, match="root\\[root"):
        g.contract(np.roll(np.arange(N, dtype=I32), 1))
    with pytest.raises(ValueError, match="rows 0"):
        g.contract(np.full(N, N, I32))
    t = g.contract(torch.as_tensor(roots[3]).cuda())
    assert not torch.is_tensor(t.neighbor)                                           # a graph answers as it was made


def comb(width, split=False):
    """row 0 one segment (two halves with `split`), below it segments one pixel wide"""
    lab = np.empty((2, width), I32)
    lab[0] = 1
    if split:
        lab[0, width // 2:] = 2
    lab[1] = np.arange(width) + 1 + lab[0].max()
    return lab


@pytest.mark.parametrize("length", ["cap-1", "cap", "cap+1", "32", "33", "8", "9", "2cap+700"])
def test_rows_around_the_limits_of_every_path(length):
    from obia_amd import _lib, segment_graph
    cap = _lib.MERGE_ROW_CAP
    L = {"cap-1": cap - 1, "cap": cap, "cap+1": cap + 1, "32": 32, "33": 33, "8": 8, "9": 9, "2cap+700": 2 * cap + 700}[length]
    lab = comb(L - 1)                                                                # row 0: L - 1 teeth and the frame
    n = L
    g = segment_graph(lab, 1)
    assert int(g.indptr[1]) == L
    same_graph(g.contract(np.arange(n, dtype=I32)), (g.indptr, g.neighbor, g.border), "identity")
    # teeth united in runs of 300 (runs of equal keys across the chunks of the combine step) and in pairs
    for run in (300, 2):
        root = np.arange(n, dtype=I32)
        root[1:] = 1 + ((np.arange(n - 1) // run) * run)
        got = g.contract(root)
        ref = by_the_raster(lab, root, 1, n)
        same_graph(got, (ref.indptr, ref.neighbor, ref.border), run)
        same_graph(got, M.contract(host(g.indptr), host(g.neighbor), host(g.border), n, root), run)


@pytest.mark.parametrize("extra", [-1, 0, 1])
def test_a_row_made_by_uniting_two_shorter_ones(extra):
    from obia_amd import _lib, segment_graph
    cap = _lib.MERGE_ROW_CAP
    width = cap + extra - 4                                                          # each half: its teeth, the other half, the frame
    lab = comb(width, split=True)
    n = width + 2
    g = segment_graph(lab, 1)
    assert int(g.indptr[1]) + int(g.indptr[2] - g.indptr[1]) == cap + extra and int(g.indptr[1]) < cap
    root = np.arange(n, dtype=I32)
    root[1] = 0
    got = g.contract(root)
    ref = by_the_raster(lab, root, 1, n)
    same_graph(got, (ref.indptr, ref.neighbor, ref.border))
    assert int(got.indptr[1]) == width + 1 and int(got.indptr[2]) == width + 1


# ---------------------------------------------------------------------------------------------------------------- launch clamps
def test_a_path_of_70000_segments():
    """a 1 x 70 000 path: 70 000 x 32 lanes pass the clamp of a flat launch (8192 workgroups of 256), so the second trip of the
    32-lane sort runs; cost and tables are held to the restatement on a sample of rows, the graph to the raster"""
    from obia_amd import RegionState, fusion_cost, merge_pairs
    n = 70000
    lab = np.arange(1, n + 1, dtype=I32).reshape(1, n)
    rs = np.random.RandomState(5)
    raw = rs.uniform(0, 100, (1, n, 2)).astype(np.float32)
    state = RegionState.from_raster(raw, lab)
    st = M.State(state.area, state.mean, state.m2, state.perimeter, state.box, state.graph.indptr, state.graph.neighbor, state.graph.border)
    got = fusion_cost(state, [1.0, 0.5])
    rows = R.rows_of(st.indptr)
    for e in np.concatenate([np.arange(40), rs.randint(0, len(rows), 200), np.arange(len(rows) - 40, len(rows))]):
        i, j = int(rows[e]), int(st.neighbor[e])
        want = M.cost_of_pair(st, min(i, j), max(i, j), st.border[e], [1.0, 0.5], F64(1.0) - F64(0.1), 0.5)[0] if j < n else M.NAN
        assert got.view(np.uint64)[e] == np.array([want], F64).view(np.uint64)[0], e
    partner = np.full(n, -1, I32)
    left = np.arange(0, n - 1, 3)
    partner[left], partner[left + 1] = left + 1, left
    merged = merge_pairs(state, partner)
    root = M.pair_root(partner, n)
    assert R.same_bits(merged.root, root)
    ref = by_the_raster(lab, root, 1, n)
    same_graph(merged.graph, (ref.indptr, ref.neighbor, ref.border))
    want = M.merge_tables(st, partner)
    for name, w in zip(("area", "mean", "m2", "perimeter", "box"), want):
        g = getattr(merged, name)
        pick = np.concatenate([np.arange(50), np.arange(n - 50, n), rs.randint(0, n, 300)])
        assert R.same_bits(g[pick], w[pick]), name
    assert R.same_bits(merged.area, want[0]) and R.same_bits(merged.perimeter, want[3]) and R.same_bits(merged.box, want[4])


# -------------------------------------------------------------------------------------------------------------------- the driver
def recovery(seed):
    r, c = np.mgrid[0:48, 0:64]
    lab = ((r // 4) * 16 + c // 4 + 1).astype(I32)
    patch = (r // 24) * 2 + c // 32
    raw = np.stack([100.0 * (patch + 1), 50.0 * (4 - patch), np.where(patch % 2 == 0, 10.0, 90.0)], -1)
    raw = (raw + np.random.RandomState(seed).normal(0, 1, (48, 64, 3))).astype(np.float32)
    return raw, lab, (patch + 1).astype(I32)


def golden_case(name):
    lab = np.load(os.path.join(GOLDEN, name + ".npz"))["labels"].astype(I32)
    rs = np.random.RandomState(len(name))
    yy, xx = np.mgrid[0:lab.shape[0], 0:lab.shape[1]]
    raw = np.stack([60 * np.sin(xx / 17.0) + 80, 40 * np.cos(yy / 23.0) + 50, (xx + yy) * 0.2], -1) + rs.normal(0, 2, lab.shape + (3,))
    return raw.astype(np.float32), lab


def drive_both(raw, lab, scale, **kw):
    """the device's rounds and the restatement's from ONE initial state, the device's: the first zonal pass sums about pivots that
    workgroups claim, so two passes over one raster need not give the same last bits; everything after it is a pure function"""
    from obia_amd import RegionState, compact_roots, merge_regions, relabel
    first = RegionState.from_raster(raw, lab)
    st = M.State(first.area, first.mean, first.m2, first.perimeter, first.box, first.graph.indptr, first.graph.neighbor, first.graph.border)
    states, counts, final = M.drive(st, scale, **kw)
    dkw = {("band_weights" if k == "w" else k): v for k, v in kw.items()}
    state, got_counts = merge_regions(first, scale, **dkw)
    assert got_counts == counts, (got_counts, counts)
    same_state(state, final, "final")
    out = relabel(lab, compact_roots(state.root, 1, present=first.area > 0), 1)
    assert R.same_bits(out, M.labels_of(lab, final, 1, st.area > 0))
    return out, counts, states, first, dkw


@pytest.mark.parametrize("name", MAPS)
def test_the_driver_on_the_golden_label_rasters(name):
    from obia_amd import merge_regions, multiresolution_merge
    raw, lab = golden_case(name)
    out, counts, states, first, dkw = drive_both(raw, lab, 100.0, w=[1.0, 0.5, 2.0], shape=0.3, compactness=0.4)
    assert len(counts) >= 3 and counts[-1] == counts[-2] < counts[0] and counts[-1] == len(np.unique(out[out >= 1]))
    # a limited run is the run's beginning
    k = 2
    state_k, counts_k = merge_regions(first, 100.0, max_rounds=k, **dkw)
    assert counts_k == counts[:k]
    same_state(state_k, states[k - 1], "two rounds")
    assert merge_regions(first, 100.0, max_rounds=0)[1] == []
    assert multiresolution_merge(raw, lab, 100.0, max_rounds=0)[1] == []


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_recovery_case(seed):
    from obia_amd import multiresolution_merge
    raw, lab, patches = recovery(seed)
    out, counts, states, first, dkw = drive_both(raw, lab, 30.0)
    assert np.array_equal(out, patches) and counts[-1] == 4 and counts[0] < 192
    whole, whole_counts = multiresolution_merge(raw, lab, 30.0, shape=0.1, compactness=0.5)
    assert np.array_equal(whole, patches) and whole_counts == counts


def test_state_after_every_round():
    """area, perimeter, box and the graph of every round equal segment_shapes / segment_graph of the relabelled raster to the bit;
    mean and m2 / area lie within 8 x the measured distance of zonal_stats of the relabelled raster"""
    from obia_amd import RegionState, merging, relabel, segment_graph, segment_shapes, zonal_stats
    raw, lab, _ = recovery(0)
    state = RegionState.from_raster(raw, lab)
    n = state.n_labels
    w = np.ones(3)
    px = raw.astype(F64)
    span = float(np.ptp(host(state.mean)))
    worst_mean = worst_var = ours_mean = ours_var = 0.0
    rounds = 0
    while True:
        partner, pairs = merging._round(state, w, 0.9, 0.5, 900.0)
        if not pairs:
            break
        state = merging._merge_pairs(state, partner)
        rounds += 1
        root = host(state.root)
        relab = relabel(lab, (root.astype(I64) + 1).astype(I32), 1)
        g, sh = segment_graph(relab, 1, n_labels=n), segment_shapes(relab, 1, n_labels=n)
        same_graph(state.graph, (g.indptr, g.neighbor, g.border), rounds)
        assert R.same_bits(state.area, sh.area) and R.same_bits(state.perimeter, sh.perimeter) and R.same_bits(state.box, sh.box)
        t = state.shape_table()
        assert R.same_bits(t.compactness, sh.compactness) and R.same_bits(t.smoothness, sh.smoothness)
        z = zonal_stats(raw, relab, n_labels=n)
        has = host(state.area) > 0
        assert np.array_equal(has, z["count"] > 0) and np.isnan(host(state.mean)[~has]).all() and np.isnan(host(state.m2)[~has]).all()
        exact_mean = np.stack([px[relab == i + 1].mean(0) for i in np.flatnonzero(has)])
        exact_var = np.stack([px[relab == i + 1].var(0) for i in np.flatnonzero(has)])
        vmax = float(exact_var.max())
        worst_mean = max(worst_mean, np.abs(z["mean"][has] - exact_mean).max() / span)
        worst_var = max(worst_var, np.abs(z["variance"][has] - exact_var).max() / vmax)
        ours_mean = max(ours_mean, np.abs(host(state.mean)[has] - exact_mean).max() / span)
        ours_var = max(ours_var, np.abs(host(state.variance)[has] - exact_var).max() / vmax)
        dm = np.abs(host(state.mean)[has] - z["mean"][has]).max() / span
        dv = np.abs(host(state.variance)[has] - z["variance"][has]).max() / vmax
        print(f"round {rounds}: regions {int(has.sum())}, mean vs zonal {dm:.3e}, variance vs zonal {dv:.3e}")
        assert dm <= 8 * MEAN_MEASURED and dv <= 8 * VAR_MEASURED, (rounds, dm, dv)
    print(f"against NumPy float64: zonal mean {worst_mean:.3e} var {worst_var:.3e}; merged mean {ours_mean:.3e} var {ours_var:.3e}")
    assert rounds >= 5 and state.n_regions == 4


# ------------------------------------------------------------------------------------------- reproducibility and input types
def test_two_runs_give_equal_bytes_and_tensors_come_back_as_tensors():
    from obia_amd import RegionState, merge_regions, multiresolution_merge
    raw, lab, patches = recovery(1)
    a = multiresolution_merge(raw, lab, 30.0, return_state=True)
    b = multiresolution_merge(raw, lab, 30.0, return_state=True)
    t = multiresolution_merge(torch.as_tensor(raw).cuda(), torch.as_tensor(lab).cuda(), 30.0, return_state=True)
    assert isinstance(a[0], np.ndarray) and torch.is_tensor(t[0]) and t[0].is_cuda and torch.is_tensor(t[2].mean) and torch.is_tensor(t[2].graph.neighbor)
    assert isinstance(a[2].mean, np.ndarray) and isinstance(a[2].graph.neighbor, np.ndarray)
    for x, y in ((a, b), (a, t)):                                                    # from the raster: everything that is an integer
        assert x[1] == y[1] and host(x[0]).tobytes() == host(y[0]).tobytes()
        for name in ("area", "perimeter", "box", "root"):
            assert host(getattr(x[2], name)).tobytes() == host(getattr(y[2], name)).tobytes(), name
        for name in ("indptr", "neighbor", "border"):
            assert host(getattr(x[2].graph, name)).tobytes() == host(getattr(y[2].graph, name)).tobytes(), name
    first = RegionState.from_raster(raw, lab)                                        # from one state: every byte
    x, y = merge_regions(first, 30.0), merge_regions(first, 30.0)
    assert x[1] == y[1] == a[1]
    for name in ("area", "mean", "m2", "perimeter", "box", "root"):
        assert host(getattr(x[0], name)).tobytes() == host(getattr(y[0], name)).tobytes(), name
    for name in ("indptr", "neighbor", "border"):
        assert host(getattr(x[0].graph, name)).tobytes() == host(getattr(y[0].graph, name)).tobytes(), name
    with pytest.raises(ValueError, match="NaN in a used band"):
        bad = raw.copy()
        bad[5, 5, 1] = np.nan
        multiresolution_merge(bad, lab, 30.0)
    bad = raw.copy()
    bad[5, 5, 1] = np.nan
    assert multiresolution_merge(bad, lab, 30.0, bands=[0, 2])[1][-1] == 4           # a NaN in a band that is not used is nobody's business
