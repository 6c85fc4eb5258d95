"""Region merging without a GPU: the restatement (tests/merging_restatement.py) against the hand check of include/obia_merging.h,
against the adjacency restatement's graph of the relabelled raster, against np.mean and np.var of a union's pixels; the fixed point;
the recovery of four patches from 192 blocks; what the header says; what the source file must not do; the refusals of the Python functions that fire before the library is loaded.

THE CHAN MERGE AGAINST NUMPY.  Over every region of every round of six random block maps merged down to one region, the largest
relative distance of the merged mean from np.mean of the union's pixels (float64) and of m2 / area from np.var was measured (NumPy
2.x, x86-64); the bound is 8 x the measured value:

    field                  measured      bound
    mean     (relative)    2.21e-16      1.77e-15
    variance (relative)    1.51e-15      1.21e-14"""
import os
import re

import numpy as np
import pytest

from tests import adjacency_restatement as R
from tests import merging_restatement as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, I32, I64 = np.float64, np.int32, np.int64
BOUNDS = {"mean": 8 * 2.21e-16, "variance": 8 * 1.51e-15}


def rasters():
    """six block maps of at most 24 x 24 with blocks of up to 3 x 3, labels 0 .. 13 (0 is background), two bands"""
    rs = np.random.RandomState(23)
    out = []
    for k in range(6):
        H, W = rs.randint(9, 25), rs.randint(9, 25)
        bh, bw = rs.randint(1, 4), rs.randint(1, 4)
        lab = np.kron(rs.randint(0, 14, (-(-H // bh), -(-W // bw))), np.ones((bh, bw), int))[:H, :W].astype(I32)
        raw = (rs.uniform(0, 255, (H, W, 2)) + 1000 * (k % 2)).astype(np.float32)
        out.append((raw, lab))
    return out


def bits(x):
    return np.array([x], F64).view(np.uint64)[0]


# ------------------------------------------------------------------------------------------------------------------- arithmetic
def test_the_hand_check_to_the_bit():
    lab = np.array([[1, 1, 2, 2], [1, 1, 2, 2]], I32)
    raw = np.zeros((2, 4, 1))
    raw[:, 2:] = 2
    st = M.state_of(raw, lab)
    assert st.area.tolist() == [4, 4] and st.perimeter.tolist() == [8, 8] and st.mean.tolist() == [[0.0], [2.0]] and st.m2.tolist() == [[0.0], [0.0]]
    c, colour, hc, hs = M.cost_of_pair(st, 0, 1, 2, [1.0], 0.9, 0.5)
    assert bits(colour) == bits(8.0) and bits(hc) == bits(1.9411254969542782) and bits(hs) == bits(0.0) and bits(c) == bits(7.297056274847714)
    full = M.cost(st, None, 0.1, 0.5)
    assert st.neighbor.tolist() == [1, 3, 0, 3] and bits(full[0]) == bits(full[2]) == bits(7.297056274847714)
    assert bits(full[1]) == bits(full[3]) == R.QNAN                            # the frame: the quiet NaN


def test_both_directions_hold_the_same_bits_and_pseudo_entries_nan():
    for raw, lab in rasters():
        st = M.state_of(raw, lab)
        c = M.cost(st, [0.5, 2.0], 0.3, 0.7)
        rows = R.rows_of(st.indptr)
        at = {(int(i), int(j)): e for e, (i, j) in enumerate(zip(rows, st.neighbor))}
        real = st.neighbor < st.N
        assert real.any() and (~real).any()
        for e in range(len(c)):
            if real[e]:
                assert not np.isnan(c[e]) and c.view(np.uint64)[e] == c.view(np.uint64)[at[(int(st.neighbor[e]), int(rows[e]))]]
            else:
                assert c.view(np.uint64)[e] == R.QNAN


# ------------------------------------------------------------------------------------------------------------------ restatement
def test_the_contraction_is_the_graph_of_the_relabelled_raster():
    rs = np.random.RandomState(4)
    tried = 0
    for raw, lab in rasters():
        st = M.state_of(raw, lab)
        N = st.N
        roots = [M.pair_root(M.round_partner(st, 1e9)[0], N), np.arange(N, dtype=I32), np.zeros(N, I32)]
        for p in (0.2, 0.6, 1.0):
            roots.append(R.components(st.indptr, st.neighbor, N, rs.uniform(size=len(st.neighbor)) < p))
        hop = np.arange(N, dtype=I32)                                           # members that need not touch
        pick = rs.permutation(N)[:N // 2]
        hop[pick] = pick.min()
        roots.append(hop)
        for root in roots:
            assert np.array_equal(root[root], root)
            got = M.contract(*st.graph(), N, root)
            want = R.graph(R.relabel(lab, (root.astype(I64) + 1).astype(I32), 1), 1, N)
            assert all(R.same_bits(g, w) for g, w in zip(got, want)), root.tolist()
            off = np.ones(N, bool)
            off[root] = False
            assert not np.diff(got[0])[off].any()                               # every other row is empty
            tried += 1
    assert tried == 42


def test_the_chan_merge_stays_close_to_numpy():
    worst = {"mean": 0.0, "variance": 0.0}
    for raw, lab in rasters():
        st = M.state_of(raw, lab)
        states, counts, final = M.drive(st, 1e9)
        assert counts[-1] == 1 and len(states) >= 4
        px = raw.astype(F64)
        for s in states:
            for r in np.flatnonzero(s.area > 0):
                p = px[np.isin(lab, np.flatnonzero(s.root == r) + 1)]
                assert len(p) == s.area[r]
                worst["mean"] = max(worst["mean"], float(np.max(np.abs(s.mean[r] - p.mean(0)) / np.abs(p.mean(0)))))
                worst["variance"] = max(worst["variance"], float(np.max(np.abs(s.m2[r] / s.area[r] - p.var(0)) / p.var(0))))
            empty = s.area == 0
            assert np.isnan(s.mean[empty]).all() and np.isnan(s.m2[empty]).all() and not s.perimeter[empty].any() and not s.box[empty].any()
    print(worst)
    for k, v in worst.items():
        assert v <= BOUNDS[k], (k, v, BOUNDS[k])


def test_every_round_is_the_recomputation_on_the_relabelled_raster():
    from tests import shapes_restatement as S
    for raw, lab in rasters()[:3]:
        st = M.state_of(raw, lab)
        for s in M.drive(st, 40.0, shape=0.5)[0]:
            relab = R.relabel(lab, (s.root.astype(I64) + 1).astype(I32), 1)
            sums, box = S.tables(relab, 1, s.N)
            assert R.same_bits(s.area, sums[:, 0]) and R.same_bits(s.perimeter, sums[:, 6]) and R.same_bits(s.box, box)
            assert all(R.same_bits(g, w) for g, w in zip(s.graph(), R.graph(relab, 1, s.N)))


@pytest.mark.parametrize("scale", [0.0, 15.0, 60.0, 1e9])
def test_at_the_fixed_point_no_real_edge_costs_the_scale_or_less(scale):
    for raw, lab in rasters():
        states, counts, final = M.drive(M.state_of(raw, lab), scale, shape=0.2)
        c = M.cost(final, None, 0.2, 0.5)
        real = final.neighbor < final.N
        assert not (c[real] <= scale * scale).any() and len(counts) == len(states) + 1 and counts[-1] == (final.area > 0).sum()
        assert M.drive(M.state_of(raw, lab), scale, shape=0.2, max_rounds=1)[1] == counts[:1]


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_recovery_case(seed):
    r, c = np.mgrid[0:48, 0:64]
    lab = ((r // 4) * 16 + c // 4 + 1).astype(I32)
    patch = (r // 24) * 2 + c // 32
    raw = np.stack([100.0 * (patch + 1), 50.0 * (4 - patch), np.where(patch % 2 == 0, 10.0, 90.0)], -1)
    raw = (raw + np.random.RandomState(seed).normal(0, 1, (48, 64, 3))).astype(np.float32)
    st = M.state_of(raw, lab)
    assert st.N == 192
    states, counts, final = M.drive(st, 30.0, shape=0.1, compactness=0.5)
    assert counts[-1] == 4 and np.array_equal(M.labels_of(lab, final), patch + 1)


# ------------------------------------------------------------------------------------------------- the header and the source
def test_the_header_says_no_row_is_dropped():
    full = open(os.path.join(ROOT, "include", "obia_merging.h")).read()
    assert "NO ROW IS EVER DROPPED OR TRUNCATED" in full and "The reference has no counterpart" in full and "compared with eCognition" in full


def test_the_source_takes_no_workspace_and_every_atomic_is_on_an_integer():
    src = open(os.path.join(ROOT, "obia_amd", "csrc", "merging.hip")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert not re.search(r"arena\.(get|alloc)\b|\bA\.get<|\.arena\b", src)   # every buffer is the caller's
    assert not re.search(r"hipMalloc|hipFree|hipHostMalloc|Staging|upload_async|read_back", code)
    targets = {"raw_count": r"unsigned long long \*raw_count\b", "cursor": r"\bint \*cursor\b", "acc": r"unsigned long long acc\["}
    found = list(re.finditer(r"\batomic([A-Za-z]+)\s*\(\s*&(\w+)", code))
    assert len(found) == len(re.findall(r"\batomic[A-Z]\w*\s*\(", code)) == 3
    for m in found:
        assert m.group(1) == "Add" and m.group(2) in targets, m.group(0)
        assert re.search(targets[m.group(2)], code), m.group(2)
    assert "unsafeAtomic" not in code and not re.search(r"__hip_atomic_fetch|__atomic_fetch", code)
    # every launch takes its grid from launch_grids.hpp, by name; no dim3 carries a clamp
    sites = re.findall(r"hipLaunchKernelGGL\([^;]*;", code)
    assert len(sites) == 8
    for site in sites:
        assert re.search(r"to_dim3\(grids::flat\(", site) and "dim3(256)" in site, site
    assert not re.search(r"std::min|std::max", code)
    # the square roots are the builtin on doubles, and nothing is contracted: the Makefile's flag
    assert "__builtin_sqrt(" in code and not re.search(r"\bsqrtf?\s*\(|\bfma\s*\(|__fma", code.replace("__builtin_sqrt(", ""))
    mk = open(os.path.join(ROOT, "obia_amd", "csrc", "Makefile")).read()
    assert " merging.o" in mk and "../../include/obia_merging.h" in mk and "-ffp-contract=off" in mk


# ------------------------------------------------------------------------------------------------------------------- the wrappers
def test_public_names_and_refusals_before_any_device_use(monkeypatch):
    pytest.importorskip("torch")
    import obia_amd
    from obia_amd import _lib, adjacency, merging as MG
    for name in ("RegionState", "fusion_cost", "merge_pairs", "merge_regions", "multiresolution_merge"):
        assert getattr(obia_amd, name) is getattr(MG, name)
    assert callable(adjacency.SegmentGraph.contract) and callable(MG.RegionState.from_raster) and callable(MG.RegionState.shape_table)
    for prop in ("area", "mean", "m2", "perimeter", "box", "root", "present", "variance"):
        assert isinstance(getattr(MG.RegionState, prop), property), prop

    def no_load():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(_lib, "load", no_load)
    lab = np.ones((4, 5), np.int32)
    raw = np.zeros((4, 5, 3), np.float32)
    run = MG.multiresolution_merge
    for kw, match in ((dict(scale=-1.0), "scale"), (dict(scale=float("nan")), "scale"), (dict(scale=1.0, shape=-0.1), "shape"),
                      (dict(scale=1.0, shape=1.5), "shape"), (dict(scale=1.0, compactness=1.01), "compactness"),
                      (dict(scale=1.0, compactness=float("nan")), "compactness"), (dict(scale=1.0, band_weights=[1.0, -1.0, 1.0]), "band_weights"),
                      (dict(scale=1.0, band_weights=[1.0, float("nan"), 1.0]), "band_weights"), (dict(scale=1.0, band_weights=[1.0, 1.0]), "band_weights"),
                      (dict(scale=1.0, band_weights=[1.0, 1.0, 1.0], bands=[0, 2]), "band_weights"), (dict(scale=1.0, max_rounds=-1), "max_rounds"),
                      (dict(scale=1.0, max_rounds=1.5), "max_rounds"), (dict(scale=1.0, max_rounds=True), "max_rounds")):
        with pytest.raises(ValueError, match=match):
            run(raw, lab, **kw)
    with pytest.raises(ValueError, match="non-empty"):
        run(raw, np.ones(5, np.int32), 1.0)
    with pytest.raises(ValueError, match="raw must be"):
        run(raw[:3], lab, 1.0)
