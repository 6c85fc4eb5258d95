"""Stream ordering of every wrapper: inputs that arrive late on torch's stream, a context stream that runs late.

A wrapper uses two streams -- torch's current one (`t`) and the context's (`s`) -- and nothing orders them but the waits the wrappers
make: `_device.begin` (and the hand-written copies of it) before the library reads what torch wrote, the library's own
hipStreamSynchronize in the synchronous entry points, `_device.end` after the asynchronous families.  On the suite's small inputs a
missing wait gives the right answer, because torch's kernels have finished before ctypes has marshalled the next call.  Here every
case runs under tests/stream_order.py, which makes the streams late with bounded delay kernels and checks the ordering at every ABI
call, in three arrangements:

  A  torch on a fresh stream t, the context on a stream of its own (obia_create).  Every input is made by late(): it holds poison
     until a delay on t has passed.  At every ABI entry t must be idle; the result is the plain run's.
  B  as A, with the context on a second torch stream s (obia_create_on_stream), a delay on s in front of every call's kernels: the
     entry points that return with s busy are exactly the ones the headers declare asynchronous (ASYNC below agrees with the headers
     line for line), s is idle when the wrapper returns, the result is the plain run's, and s still works after the context is gone.
  C  the context on t itself, no delays: the "run on my stream" integration.  The result is the plain run's.

Cases: every case of tests/test_gpu_workspace_history.py but the "guards:" ones (they call entry points through ctypes on buffers of
their own); and the cases below for every public wrapper those do not reach, each judged by its operator's restatement.  Late inputs:
under A and B every `.cuda()` upload of a host tensor returns a late() tensor -- the inputs of this file's cases, of the helpers of
tests/test_gpu_pointer_alignment.py and the *_buffers files, and of the session, connectivity and tiled cases.  NOT late are inputs
handed over as NumPy arrays, which the wrapper uploads itself: `crowns_mask`, `boxes_table`, `boxes_passes`, the mask of
`tiled_skimage` and `tiled_orphan_repeat`, and all of the `host:` cases (the host-pointer entry points, there for the completeness
test; all but one are judged by their own plain run only).  `cost_allocation` gets CUDA tensors in `crowns:cost_allocation`.
"forest_predict's chunked path (classify.py:543)" of the issue is the piece loop of `mlp_shap`, where that line stands:
`classify:mlp_shap_in_pieces`.  Delays: 4 x the largest host gap between two ABI calls of a
plain, logged run of the case, at least 5 ms (FLOOR_MS: 20 ms for the shape and merging wrappers); no case may need more than 100 ms
(test_no_case_needs_more_than_the_cap; profiles/stream_order_notes.md has the figures).

Stale blocks.  A wrongly ordered read must see poison, not the previous run's correct answer in a block torch's caching allocator
hands out again.  Before an instrumented run the test drops what it holds, then allocates, fills with 0xA5 and frees tensors of the
sizes the case's plain run allocated.  This is best effort: the allocator rounds and splits blocks as it sees fit, so a stale answer
can survive; the idle_t / pending_s log does not depend on it.

Nothing here provokes a fault: the two deliberately wrong mini-wrappers at the end touch valid buffers only and read stale data."""
import contextlib
import ctypes
import functools
import time

import numpy as np
import pytest

from tests import stream_order as SO
from tests import workspace_history as WH

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import test_gpu_pointer_alignment as PA                           # noqa: E402
from tests import test_gpu_workspace_history as WHT                          # noqa: E402

Op, same = WHT.Op, PA.same

# ---- the entry points that return with the context's stream busy, as the headers declare them ---------------------------------------
ASYNC = {
    # include/obia_hip.h, cost surface: "every call is asynchronous on the context's stream except the two that return a count"
    "obia_cost_bands_f32_dev", "obia_cost_ndvi_f32_dev", "obia_cost_sobel_f32_dev", "obia_cost_entropy_f32_dev", "obia_cost_normalise_dev",
    "obia_cost_combine_dev",
    # include/obia_hip.h, seeds: "the gather and the matrix are asynchronous" (the other three read a host value back)
    "obia_seeds_peaks_gather_dev", "obia_seeds_pair_matrix_dev",
    # include/obia_hip.h, the session: "obia_tiler_create queues its clears and returns"
    "obia_tiler_create",
    # include/obia_image.h: "every call is asynchronous on the context's stream"
    "obia_image_stretch_u8_dev", "obia_image_gray_hist_dev", "obia_image_lut_u8_dev", "obia_image_clahe_u8_dev", "obia_image_boundaries_dev",
    "obia_image_mark_u8_dev",
    # include/obia_sharpness.h: "every call is asynchronous on the context's stream"
    "obia_sharp_gray_lap_dev", "obia_sharp_laplacian_dev", "obia_sharp_box_dev", "obia_sharp_variance_dev", "obia_sharp_stretch_f32_dev",
    # include/obia_training.h: "every call is asynchronous on the context's stream"
    "obia_train_blur_u8_dev", "obia_train_distance_dev", "obia_train_compose_u8_dev", "obia_train_minmax_u8_dev",
}

# An entry that may be entered with torch's stream busy: name -> one-line proof, read from the code, that the pending torch work
# touches no buffer the call reads or writes.  None is expected.
IDLE_EXEMPT = {}

# Entry points arrangement B need not observe, each with its reason (the rest of what obia_amd/_lib.py binds must be logged).
NOT_OBSERVED = dict(SO.CONTEXT_FREE)
NOT_OBSERVED.update(SO.BOOKKEEPING)
NOT_OBSERVED.update({
    "obia_test_clear_ranges_dev": "obia_test_*: the clear kernel's own hook, driven by tests/test_gpu_clear_ranges.py only; no wrapper calls it",
    "obia_test_poison_workspace_dev": "obia_test_*: the instrument of tests/test_gpu_workspace_history.py; no wrapper calls it",
})

# The cases none of whose inputs is late: they hand NumPy arrays to the wrapper, which uploads them itself (module docstring).
NOT_LATE = {"crowns_mask", "boxes_table", "boxes_passes", "host:slic", "host:zonal_stats", "host:quickshift", "host:create_tiled_segments",
            "host:create_tiled_segments_skimage"}

# The delay in front of a call's kernels on s is at least this long.  pending_s is read in the statement after the call returns; a
# host thread that loses the processor between the two for longer than the delay would see an asynchronous entry point as
# synchronous.  20 ms is four scheduler quanta of a loaded machine; the t side keeps the 4 x gap rule, where a delay that runs out
# early can only hide a violation, never invent one.
S_MIN_MS = 20.0

def dev(a):
    """a test input on the device; under arrangements A and B the upload is late (late_inputs below)"""
    return torch.as_tensor(np.array(a, order="C")).cuda()


def host(v):
    if isinstance(v, torch.Tensor):
        return v.cpu().numpy()
    if isinstance(v, dict):
        return {k: host(x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return tuple(host(x) for x in v)
    return v


def bits_equal(got, want, what=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), f"{what}: {int((got.view(np.uint8) != want.view(np.uint8)).sum())} bytes differ"


# ---- new cases: run(ctx, oracle) -> host result, judge(result, oracle) against the operator's restatement -----------------------------
NEW = {}
FLOOR_MS = {}             # case -> the least delay in ms, where the 4 x gap rule alone would give too short a one
CALLS = {}                # case -> the entry points its wrappers call, in order (arrangement B's log but the obia_destroy of the test itself)


# -- image previews (tests/image_restatement.py)
def _image_case(make, call, want):
    inputs, wanted = functools.lru_cache(maxsize=None)(make), functools.lru_cache(maxsize=None)(lambda: want(make()))

    def run(ctx, oracle):
        return host(call(inputs()))

    def judge(got, oracle):
        bits_equal(got, wanted())
    return Op(run, judge=judge)


def _image_cases():
    from tests import image_restatement as R
    from tests import test_gpu_image as TI

    def raw5():
        return np.stack([TI.raster((40, 52), 10 + c) * (1 + 0.3 * c) for c in range(5)], -1).astype(np.float32)

    def I():
        from obia_amd import image
        return image
    NEW["image:rescale"] = _image_case(lambda: TI.raster((7, 13, 3), 1), lambda x: I().rescale_to_8bit(dev(x), 2, 98), lambda x: R.rescale_to_8bit(x, 2, 98))
    NEW["image:equalize"] = _image_case(lambda: TI.u8((33, 47, 3), 2), lambda x: I().apply_histogram_equalization(dev(x)), R.apply_histogram_equalization)
    for st in (None, "histogram_equalization", "clahe"):
        NEW[f"image:to_image_{st or 'plain'}"] = _image_case(raw5, lambda x, st=st: I().to_image(dev(x), (4, 0, 2), stretch_type=st, as_array=True),
                                                           lambda x, st=st: TI.want_image(x, (4, 0, 2), 2, 98, st))

    @functools.lru_cache(maxsize=None)
    def golden():
        g = np.load(TI.GOLDENS[0])
        return g["labels"], g["image"], g["boundaries"], g["marked"]

    def overlay(ctx, oracle):
        from PIL import Image as PILImage
        from obia_amd.segmentation import Segments
        lab, img = golden()[:2]
        return host((I().find_boundaries(dev(lab)), I().mark_boundaries_u8(dev(img), dev(lab)),
                     Segments(dev(lab), None, "slic").to_segmented_image(PILImage.fromarray(img), as_array=True)))

    def judge_overlay(got, oracle):
        _, _, boundaries, marked = golden()
        bits_equal(got[0], boundaries, "find_boundaries"), bits_equal(got[1], marked, "mark_boundaries_u8"), bits_equal(got[2], marked, "to_segmented_image")
    NEW["image:boundaries_mark_overlay"] = Op(overlay, judge=judge_overlay)


# -- the sharpness raster (tests/sharpness_restatement.py)
def _sharpness_cases():
    from tests import sharpness_restatement as S
    from tests import test_gpu_sharpness as TS
    shape, win = (33, 17), 3

    def I():
        from obia_amd import image
        return image
    NEW["sharp:box_filter"] = Op(lambda ctx, oracle: host(I().box_filter(dev(S.golden_plane("n50", shape)), win)),
                                 judge=lambda got, oracle: TS.same(got, TS.want_box("n50", shape, win)))
    NEW["sharp:variance_of_laplacian"] = Op(lambda ctx, oracle: host(I().variance_of_laplacian(dev(S.golden_plane("n50", shape)), win)),
                                            judge=lambda got, oracle: TS.same(got, TS.want_variance(shape, win)))
    NEW["sharp:laplacian"] = Op(lambda ctx, oracle: host(I().laplacian(dev(TS.raster01(shape)), None, win)),
                                judge=lambda got, oracle: TS.same(got, TS.want_laplacian(shape, win)))


# -- training tiles (tests/training_restatement.py)
TILE_SCENE = (slice(0, 30), slice(0, 60))                                   # two tiles: 30 x 40 and 30 x 30


def _training_cases():
    from tests import training_restatement as T
    from tests import test_gpu_training as TT

    def blur(ctx, oracle):
        from obia_amd.training import gaussian_blur_u8
        img, _ = TT.blur_case((13, 17), 3)
        return host((gaussian_blur_u8(dev(img), 5), gaussian_blur_u8(dev(img), (7, 31))))

    def judge_blur(got, oracle):
        _, want = TT.blur_case((13, 17), 3)
        bits_equal(got[0], want[(5, 5)], "5 x 5"), bits_equal(got[1], want[(7, 31)], "7 x 31")
    NEW["train:gaussian_blur"] = Op(blur, judge=judge_blur)

    def distance(ctx, oracle):
        from obia_amd.training import chamfer_distance
        src = TT.distance_planes()["half"]
        return host((chamfer_distance(dev(src)), chamfer_distance(dev(src), 3)))

    def judge_distance(got, oracle):
        bits_equal(got[0], TT.distance_want("half", None), "full"), bits_equal(got[1], TT.distance_want("half", 3), "R = 3")
    NEW["train:chamfer_distance"] = Op(distance, judge=judge_distance)

    @functools.lru_cache(maxsize=None)
    def want_tiles(variant):
        raster, mask = TT.scene()
        return T.tile_and_process(raster[TILE_SCENE], TT.AFFINE, TT.CRS, mask[TILE_SCENE], TT.BOXES, **TT.TILING, **TT.VARIANTS[variant])

    def tiles(variant):
        def run(ctx, oracle):
            from obia_amd.training import tile_and_process
            raster, mask = TT.scene()
            got = tile_and_process(dev(raster[TILE_SCENE]), TT.AFFINE, TT.CRS, dev(mask[TILE_SCENE]), TT.BOXES, **TT.TILING, **TT.VARIANTS[variant],
                                   as_array=True)
            assert all(t.is_cuda for t in got.images)
            return got.names, host(got.images), got.transforms, got.annotations

        def judge(got, oracle):
            names, images, transforms, annotations = want_tiles(variant)
            assert len(names) == 2 and got[0] == names and got[2] == transforms and got[3] == annotations
            for name, a, b in zip(names, got[1], images):
                bits_equal(a, b, name)
        return Op(run, judge=judge)
    for variant in ("hard", "feathered", "minmax"):                          # masked; feathered; without `rescale`
        NEW[f"train:tile_and_process_{variant}"] = tiles(variant)


# -- crowns (tests/crowns_restatement.py): cost_allocation is the case `crowns_mask`; grow_crowns from a seed table
def _crowns_cases():
    from tests import crowns_restatement as C
    from tests import test_gpu_crowns as TC

    @functools.lru_cache(maxsize=None)
    def want():
        c = TC.case("mask", TC.SHAPES[4])
        ids = (1 + np.searchsorted(np.unique(c["ids"]), c["ids"])).astype(np.int32)
        return C.allocate(c["cost"], c["rows"], c["cols"], ids, mask=c["mask"], weight=0.5, pixel_size=(1.0, 1.0), connectivity=8)

    def run(ctx, oracle):
        from obia_amd import grow_crowns
        c = TC.case("mask", TC.SHAPES[4])
        seeds = {"x": dev(c["cols"] + 0.5), "y": dev(c["rows"] + 0.5), "cluster": dev(c["ids"].astype(np.int64))}
        return host(grow_crowns(dev(c["cost"]), seeds, mask=dev(c["mask"]), return_distance=True))

    def judge(got, oracle):
        assert TC.same_bits(got[1], want()[0]) and np.array_equal(got[0], want()[1]) and got[0].dtype == np.int32
    NEW["crowns:grow_crowns"] = Op(run, judge=judge)


# -- point clouds (tests/pointcloud_restatement.py): rasters, per-segment state and columns
def _pointcloud_cases():
    from tests import pointcloud_restatement as R
    from tests import test_gpu_pointcloud as TP

    def cloud_t(c):
        return {"X": dev(c["x"]), "Y": dev(c["y"]), "HeightAboveGround": dev(c["z"]), "Intensity": dev(c["intensity"])}

    def rasters(ctx, oracle):
        from obia_amd.pointcloud import points_to_rasters
        c = TP.reference("base")["c"]
        t = cloud_t(c)
        del t["Intensity"]
        return host(points_to_rasters(t, c["affine"], (R.H, R.W)))

    def judge_rasters(got, oracle):
        r = TP.reference("base")
        bits_equal(got["chm"], r["chm"], "chm"), bits_equal(got["density"], r["density"], "density")
        assert np.array_equal(got["count"], r["count"].astype(np.int64))
    NEW["points:rasters"] = Op(rasters, judge=judge_rasters)

    def segments(ctx, oracle):
        from obia_amd.pointcloud import SegmentPoints
        r = TP.reference("base")
        c = r["c"]
        sp = SegmentPoints(dev(c["labels"]), c["affine"], R.DZ, R.ZMAX, start_label=1, n_labels=r["N"])
        sp.add(cloud_t(c))
        return host(sp.state()), host(sp.columns(min_height=1.0, beer_lambert_constant=0.5, pad=True)), sp.counters()

    def judge_segments(got, oracle):
        st = TP.reference("base")["st"]
        state, cols, counters = got
        as_bits = {"profile": np.uint32, "top": np.uint32, "n_int": np.uint32}
        TP.same_state({k: (state[k].astype(as_bits[k]) if k in as_bits else state[k].view(np.uint64)) for k in state}, st)
        assert list(counters.values()) == [int(v) for v in st["counters"]]
        f64 = R.columns(st, R.DZ, 1.0, 0.5, np.float64, pad=True)
        assert np.array_equal(cols["n_points"], f64["n_points"])
        bits_equal(cols["ch"], f64["ch"], "ch"), bits_equal(cols["mean_intensity"], f64["mean_intensity"], "mean_intensity")
        for name in ("pai", "fhd", "pad", "variance_intensity"):             # (their ulp bars are tests/test_gpu_pointcloud.py's; here: NaN rows)
            assert np.array_equal(np.isnan(cols[name]), np.isnan(f64[name])), name
    NEW["points:segments"] = Op(segments, judge=judge_segments)


# -- height above ground (tests/ground_restatement.py): k nearest ground points, and a DTM
def _ground_cases():
    from tests import ground_restatement as G
    from tests import test_gpu_ground as TG
    DTM_AFFINE, DTM_SHAPE = [1.5, 0.0, 0.0, -1.5, G.ORIGIN[0] - 4.0, G.ORIGIN[1] + 52.0], (37, 53)

    @functools.lru_cache(maxsize=None)
    def want():
        _, kept, x, y, z = TG.base()
        dtm = G.to_raster(kept, DTM_SHAPE, DTM_AFFINE, 1, 0.0)
        return G.hag(z, TG.base_want(3, 1.5)["zg"]), dtm, G.hag(z, G.dtm_z(x, y, dtm, DTM_AFFINE))

    def knn(ctx, oracle):
        from obia_amd.pointcloud import GroundIndex, normalize_heights
        _, _, x, y, z = TG.base()
        idx = GroundIndex(TG.cloud(*(dev(a) for a in G.base_ground())))
        out = normalize_heights(TG.cloud(dev(x), dev(y), dev(z)), idx, count=3, max_distance=1.5)
        return host(out["HeightAboveGround"])
    NEW["ground:normalize_heights_knn"] = Op(knn, judge=lambda got, oracle: TG.same(got, want()[0], "k nearest"))

    def dtm(ctx, oracle):
        from obia_amd.pointcloud import normalize_heights
        _, _, x, y, z = TG.base()
        out = normalize_heights(TG.cloud(dev(x), dev(y), dev(z)), dtm=dev(want()[1]), affine_transformation=DTM_AFFINE)
        return host(out["HeightAboveGround"])
    NEW["ground:normalize_heights_dtm"] = Op(dtm, judge=lambda got, oracle: TG.same(got, want()[2], "dtm"))


# -- the ground filter (tests/groundfilter_restatement.py)
def _groundfilter_cases():
    from tests import groundfilter_restatement as R
    from tests import pointcloud_restatement as PR
    from tests import test_gpu_groundfilter_buffers as TB
    SHAPE, AFFINE = (PR.H, PR.W), PR.AFFINE
    KW = dict(cell_size=0.5, slope=1.0, initial_distance=0.15, max_distance=2.5, max_window_size=3.0)

    def opening(ctx, oracle):
        from obia_amd.pointcloud import grey_opening
        return host(grey_opening(dev(TB.case()["plane"]), TB.RADIUS))

    def judge_opening(got, oracle):
        assert R.same_bits(got, R.dilation(TB.case()["erosion"], TB.RADIUS))
    NEW["gf:grey_opening"] = Op(opening, judge=judge_opening)

    @functools.lru_cache(maxsize=None)
    def want():
        c = TB.case()
        radii, dh = R.schedule(KW["cell_size"], KW["slope"], KW["initial_distance"], KW["max_distance"], KW["max_window_size"])
        return (radii, dh), R.ground_filter(c["x"], c["y"], c["z"], AFFINE, SHAPE, radii, dh)

    def cloud_t():
        c = TB.case()
        return {"X": dev(c["x"]), "Y": dev(c["y"]), "Z": dev(c["z"])}

    def gf(ctx, oracle):
        from obia_amd import ground_filter
        g = ground_filter(cloud_t(), affine_transformation=AFFINE, shape=SHAPE, **KW)
        return (g.radii, g.dh), host({"flags": g.ground, "zmin": g.zmin, "surface": g.surface, "threshold": g.threshold}), g.counters

    def judge_gf(got, oracle):
        schedule, w = want()
        assert tuple(got[0]) == tuple(schedule) and len(schedule[0]) >= 2
        assert np.array_equal(got[1]["flags"].astype(np.uint8), w["flags"])
        for name in ("zmin", "surface", "threshold"):
            assert R.same_bits(got[1][name], w[name]), name
        assert got[2] == dict(zip(R.COUNTERS, (int(v) for v in w["counters"])))
    NEW["gf:ground_filter"] = Op(gf, judge=judge_gf)

    def classify(ctx, oracle):
        from obia_amd import classify_ground
        out = classify_ground(cloud_t(), affine_transformation=AFFINE, shape=SHAPE, **KW)
        return host(out["Classification"])

    def judge_classify(got, oracle):
        assert got.dtype == np.uint8 and np.array_equal(got, np.where(want()[1]["flags"] == 1, 2, 1).astype(np.uint8))
    NEW["gf:classify_ground"] = Op(classify, judge=judge_classify)


# -- the adjacency graph (tests/adjacency_restatement.py): the table methods on the case of the *_buffers file, the drivers on blocks()
def _adjacency_cases():
    from tests import adjacency_restatement as R
    from tests import test_gpu_adjacency_buffers as TB

    def graph(ctx, oracle):
        from obia_amd import relabel, segment_graph
        r = TB.case()
        g = segment_graph(dev(r["labels"]), TB.START, n_labels=TB.N)
        best = g.best_neighbor(dev(r["dist"]))
        st = g.neighbor_stats(dev(r["values"]))
        return host({"indptr": g.indptr, "neighbor": g.neighbor, "border": g.border, "d2": g.d2(dev(r["values"])), "mean": st["mean"],
                     "min": st["min"], "max": st["max"], "used": st["used"], "cls": g.border_to_class(dev(r["classes"]), TB.K), "best": best[0],
                     "best_d2": best[1], "root": g.components(dev(r["link"])), "relabelled": relabel(dev(r["labels"]), dev(r["table"]), TB.START),
                     "perimeter": g.perimeter, "n_neighbors": g.n_neighbors})

    def judge_graph(got, oracle):
        r = TB.case()
        for name in ("indptr", "neighbor", "border", "d2", "mean", "min", "max", "used", "cls", "best", "best_d2", "root", "relabelled"):
            assert R.same_bits(got[name], r[name]), name
        real = r["neighbor"] < TB.N
        rows = np.repeat(np.arange(TB.N), np.diff(r["indptr"]))
        assert np.array_equal(got["perimeter"], np.bincount(rows, r["border"], TB.N).astype(np.int64))
        assert np.array_equal(got["n_neighbors"], np.bincount(rows[real], minlength=TB.N))
    NEW["adj:segment_graph_tables"] = Op(graph, judge=judge_graph)

    @functools.lru_cache(maxsize=None)
    def want_drivers():
        from tests import test_gpu_adjacency as TA
        raw, lab = TA.blocks()
        means = TA.zonal_means_np(raw, lab)
        classes = np.random.RandomState(5).randint(-1, 3, 35)
        sim, counts, _ = R.merge_similar(raw, lab, 10.0, TA.zonal_means_np, max_rounds=3)
        return raw, lab, classes, R.merge_by_threshold(means, lab, 2.5), (sim, counts), R.dissolve_by_class(lab, classes)

    def drivers(ctx, oracle):
        from obia_amd import dissolve_by_class, merge_by_threshold, merge_similar
        raw, lab, classes = want_drivers()[:3]
        a, na = merge_by_threshold(dev(raw), dev(lab), 2.5)
        b, counts = merge_similar(dev(raw), dev(lab), 10.0, max_rounds=3)
        c, nc = dissolve_by_class(dev(lab), dev(classes))
        return host((a, na, b, list(counts), c, nc))

    def judge_drivers(got, oracle):
        _, _, _, (wa, wna), (wb, wcounts), (wc, wnc) = want_drivers()
        assert got[1] == wna and R.same_bits(got[0], wa) and 1 < wna < 35, "merge_by_threshold"
        assert list(got[3]) == list(wcounts) and R.same_bits(got[2], wb), "merge_similar"
        assert got[5] == wnc and R.same_bits(got[4], wc) and wnc < 35, "dissolve_by_class"
    NEW["adj:merge_and_dissolve"] = Op(drivers, judge=judge_drivers)

    @functools.lru_cache(maxsize=None)
    def objects():
        from obia_amd import create_objects
        from tests import test_gpu_adjacency as TA
        raw, lab = TA.blocks()
        lab = np.where(lab == 17, 36, lab).astype(np.int32)                   # label 17 is absent: 36 rows in the graph, 35 in the table
        return lab, create_objects(lab, raw, calculate_textural=False, geometry=False)

    def context(ctx, oracle):
        from obia_amd import context_columns, segment_graph
        lab, table = objects()
        g = segment_graph(dev(lab))
        cc = context_columns(table, g, columns=["b0_mean", "b2_max"])
        return {c: np.asarray(cc[c].to_numpy()) for c in cc.columns}

    def judge_context(got, oracle):
        lab, table = objects()
        indptr, neighbor, border = R.graph(lab, 1, 36)
        present = np.diff(np.concatenate([[0], np.cumsum(border)])[indptr]) > 0
        values = np.full((36, 2), np.nan)
        values[present] = table[["b0_mean", "b2_max"]].to_numpy(dtype=np.float64)
        want = R.neighbor_stats(indptr, neighbor, border, 36, values)
        diff = values - want["mean"]
        for k, c in enumerate(("b0_mean", "b2_max")):
            for s, w in (("mean", want["mean"]), ("min", want["min"]), ("max", want["max"]), ("diff", diff)):
                assert R.same_bits(np.asarray(got[f"{c}_nb_{s}"], np.float64), w[present, k]), (c, s)
        assert (got["perimeter"] == 32).all() and len(got["perimeter"]) == 35
    NEW["adj:context_columns"] = Op(context, judge=judge_context)


# -- the shape columns and region merging: the wrappers on the cases of their *_buffers files.  Each makes ABI calls with no host gap to
#    scale a delay by, so the delay has a floor; and the calls a wrapper makes are pinned, in order.
def _shapes_cases():
    from tests import shapes_restatement as S
    from tests import test_gpu_shapes_buffers as TB

    def run(ctx, oracle):
        from obia_amd import segment_shapes
        table = segment_shapes(dev(TB.case()["labels"]), TB.START, n_labels=TB.N, ctx=ctx)
        return host((table.sums, table.box, table.orientation))

    def judge(got, oracle):
        r = TB.case()
        assert S.same_bits(got[0], r["sums"]) and S.same_bits(got[1], r["box"])
        want = S.derived(r["sums"], r["box"])["orientation"]
        assert np.array_equal(np.isnan(got[2]), np.isnan(want)) and np.nanmax(np.abs(got[2] - want)) <= 8 * 2.22e-16   # ORIENTATION_BOUND of tests/test_gpu_shapes.py
    NEW["shapes:segment_shapes"] = Op(run, judge=judge)
    FLOOR_MS["shapes:segment_shapes"], CALLS["shapes:segment_shapes"] = 20.0, TB.EXERCISED


def _merging_cases():
    from tests import adjacency_restatement as R
    from tests import test_gpu_merging_buffers as TB

    def run(ctx, oracle):
        from obia_amd import RegionState, SegmentGraph, fusion_cost, merge_pairs
        r = TB.case()
        st = r["st"]
        g = SegmentGraph(dev(st.indptr), dev(st.neighbor), dev(st.border), TB.N, TB.START, ctx=ctx)
        state = RegionState(dev(st.area), dev(st.mean), dev(st.m2), dev(st.perimeter), dev(st.box), g)
        cost = fusion_cost(state, TB.WEIGHTS, TB.SHAPE, TB.COMPACT)
        merged = merge_pairs(state, dev(r["ins"]["partner"]))
        return host(dict(cost=cost, area=merged.area, mean=merged.mean, m2=merged.m2, perimeter=merged.perimeter, box=merged.box,
                         neighbor=merged.graph.neighbor, border=merged.graph.border, root=merged.root))

    def judge(got, oracle):
        r = TB.case()
        for name in ("cost", "area", "mean", "m2", "perimeter", "box", "neighbor", "border"):
            assert R.same_bits(got[name], r["want"][name]), name
        assert R.same_bits(got["root"], r["ins"]["root"])
    NEW["merge:cost_and_pairs"] = Op(run, judge=judge)
    FLOOR_MS["merge:cost_and_pairs"], CALLS["merge:cost_and_pairs"] = 20.0, TB.EXERCISED


# -- seeds: the CHM seeds and the canonical seeds with every table option (tests/seeds_restatement.py, tests/seed_table_restatement.py)
def _seeds_cases():
    from tests import seeds_restatement as SR
    from tests import test_gpu_seed_table as TST

    @functools.lru_cache(maxsize=None)
    def plane():
        return PA.peak_plane()

    def chm_seeds(ctx, oracle):
        from obia_amd.seeds import make_chm_seeds
        aff = SR.pixel_affine(0.5, plane().shape[0])
        out = make_chm_seeds(dev(plane()), h_min_m=12.0, affine_transformation=aff)
        return host({k: out[k] for k in ("row", "col", "id", "ch_max", "x", "y")})

    def judge_chm(got, oracle):
        a = plane()
        aff = SR.pixel_affine(0.5, a.shape[0])
        wr, wc = np.where(SR.peaks_scipy(a, 12.0, 3, 1))
        assert len(wr) > 0 and np.array_equal(got["row"], wr) and np.array_equal(got["col"], wc) and np.array_equal(got["id"], np.arange(len(wr)))
        assert np.array_equal(got["ch_max"], a[wr, wc])
        assert np.array_equal(got["x"], aff[0] * (wc + 0.5) + aff[1] * (wr + 0.5) + aff[4])
        assert np.array_equal(got["y"], aff[2] * (wc + 0.5) + aff[3] * (wr + 0.5) + aff[5])
    NEW["seeds:make_chm_seeds"] = Op(chm_seeds, judge=judge_chm)

    def canonical(ctx, oracle):
        from obia_amd import seeds as S
        tabs, cost, aff, chm = TST.scene()
        a, b = TST.as_dicts(tabs)
        ta, tb = {k: dev(v) for k, v in a.items()}, {k: dev(v) for k, v in b.items()}
        got = S.canonical_seeds(ta, tb, dev(cost), chm=dev(chm), chm_affine=aff, cost_affine=aff, debug_dist=False, **TST.OPTION_SETS["all"])
        return {k: host(got[k]) for k in TST.KEYS}

    def judge_canonical(got, oracle):
        TST.same_table(got, TST.want_canonical("all"))
    NEW["seeds:canonical_seeds_all_options"] = Op(canonical, judge=judge_canonical)


# -- mlp_shap a piece of rows at a time (the wait of classify.py between the pieces): two rows, one row a piece
def _mlp_shap_pieces():
    from tests import mlp_restatement as mr
    from tests import mlp_shap_restatement as MS

    def run(ctx, oracle):
        import importlib
        K = importlib.import_module("obia_amd.classify")                      # (the package exports a function of the same name)
        c = MS.load_case("author")
        X = np.concatenate([c["X"], c["X"]])
        old = K._SHAP_VALUES_BYTES
        K._SHAP_VALUES_BYTES = 1                                               # one row a piece
        try:
            return host(K.mlp_shap(mr.mlp_of(c), dev(X), dev(c["background"])))
        finally:
            K._SHAP_VALUES_BYTES = old

    def judge(got, oracle):
        c = MS.load_case("author")
        E, e_comb = mr.pooled_e_ref(), float(c["e_comb"])
        phi, base = got
        assert phi.shape[0] == 2 and np.array_equal(phi[0], phi[1])           # a row's result does not depend on the piece it fell in
        assert float(np.abs(phi[0] - c["phi_exact"][0]).max()) <= 16 * E + 8 * e_comb and float(np.abs(base - c["base_exact"]).max()) <= 8 * E
    NEW["classify:mlp_shap_in_pieces"] = Op(run, judge=judge)


# -- the wrappers whose entry points only the "guards:" cases reach, on CUDA tensors, each judged by its operator's restatement
def _wrapper_cases():
    from tests import test_gpu_wrapper_plumbing as WP
    INV, WEIGHT, XY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0], 0.5, 0.8

    @functools.lru_cache(maxsize=None)
    def data():
        make = getattr(WP.data, "__wrapped__", None) or WP.data.__pytest_wrapped__.obj    # (the fixture's function, whatever pytest wraps it in)
        d = make()
        return dict(d, chm17=d["chm"][:17, :19].copy(), labels17=d["labels"][:17, :19].copy())

    @functools.lru_cache(maxsize=None)
    def pair_matrix():
        from tests import seeds_restatement as SR
        d = data()
        return SR.distance_matrix(d["xs"], d["ys"], d["cost"], INV, WEIGHT, XY, 12)

    def cost_surface(ctx, oracle):
        from obia_amd.cost import make_cost_surface
        d = data()
        return host(make_cost_surface(dev(d["wv3"]), dev(d["chm17"]), slic=dev(d["labels17"]), weights=PA.COST_WEIGHTS))

    def judge_cost_surface(got, oracle):
        import warnings
        from tests import cost_restatement as CR
        from tests.test_gpu_cost_surface import _same
        d = data()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _same(got, CR.make_cost_surface(d["wv3"], d["chm17"], d["labels17"], PA.COST_WEIGHTS))
    NEW["wrapper:make_cost_surface"] = Op(cost_surface, judge=judge_cost_surface)

    def seed_tables():
        from tests import test_gpu_seed_table as TST
        tabs, cost, aff, _ = TST.scene()
        return tabs[0], (tabs[1][0], tabs[1][1], np.full(len(tabs[1][0]), 7.5, np.float32)), cost, aff

    def canonical(ctx, oracle):
        from obia_amd import seeds as S
        from tests import test_gpu_seed_table as TST
        chm_tab, den_tab, cost, aff = seed_tables()
        a, b = TST.as_dicts((chm_tab, den_tab))
        got = S.make_canonical_seeds({k: dev(v) for k, v in a.items()}, {k: dev(v) for k, v in b.items()}, dev(cost), cost_affine=aff,
                                     debug_dist=False)
        return {k: host(got[k]) for k in TST.KEYS}

    @functools.lru_cache(maxsize=None)
    def want_canonical():
        from tests import seed_table_restatement as T
        chm_tab, den_tab, cost, aff = seed_tables()
        return T.canonical(chm_tab, den_tab, cost, cost_affine=aff)

    def judge_canonical(got, oracle):
        from tests import test_gpu_seed_table as TST
        want = want_canonical()
        assert 1 < len(np.unique(want["cluster"])) < len(want["x"])             # seeds were merged, and not into one
        TST.same_table(got, want)
    NEW["wrapper:make_canonical_seeds"] = Op(canonical, judge=judge_canonical)

    def merge(ctx, oracle):
        from obia_amd import seeds as S
        d = data()
        return host(S.merge_clusters(dev(d["xs"]), dev(d["ys"]), dev(d["cost"]), INV, WEIGHT, XY, 6.0))

    def judge_merge(got, oracle):
        from tests import seeds_restatement as SR
        want = SR.components(pair_matrix(), 6.0)
        assert got.dtype == np.int32 and np.array_equal(got, want) and 1 < want.max() + 1 < len(want)
    NEW["wrapper:merge_clusters"] = Op(merge, judge=judge_merge)

    def stats(ctx, oracle):
        from obia_amd import seeds as S
        d = data()
        return tuple(S.pair_stats(dev(d["xs"]), dev(d["ys"]), dev(d["cost"]), INV, WEIGHT, XY, 12))

    def judge_stats(got, oracle):
        from tests import seeds_restatement as SR
        assert all(isinstance(v, np.float32) for v in got)
        assert np.array_equal(np.array(got), np.array(SR.triu_stats(pair_matrix()), np.float32), equal_nan=True)
    NEW["wrapper:pair_stats"] = Op(stats, judge=judge_stats)

    def centroids(ctx, oracle):
        from obia_amd.segmentation import mask_centroids
        return host(mask_centroids(dev(data()["mask"]), 6))

    def judge_centroids(got, oracle):
        from tests import mask_seeds_restatement as MSR
        cent, steps = MSR.mask_centroids(data()["mask"] != 0, 6)
        assert got[0].shape == cent.shape and np.array_equal(got[0], cent) and np.array_equal(got[1], steps)
    NEW["wrapper:mask_centroids"] = Op(centroids, judge=judge_centroids)

    # slic(seeding="skimage") on a fixture scikit-image made: the centroids are its own seeds bit for bit, and the labels are those of
    # the seeded call with these seeds -- the bar of tests/test_gpu_mask_seeds.py, which inherits test_gpu_parity.py's against its labels
    FIXTURE = "maskones_96x96x4"

    @functools.lru_cache(maxsize=None)
    def seeded_labels():
        from obia_amd import segmentation as seg
        from tests import test_gpu_mask_seeds as TM
        z, params = TM.load(FIXTURE)
        want = seg.slic(torch.as_tensor(z["raw"].astype(np.float32)).cuda(), mask=z["mask"], seeds=(z["seeds_yx"], z["seed_steps_all"]),
                        **TM.slic_kwargs(params))
        return want.cpu().numpy()

    def slic_skimage(ctx, oracle):
        from obia_amd import segmentation as seg
        from tests import test_gpu_mask_seeds as TM
        z, params = TM.load(FIXTURE)
        lab = seg.slic(dev(z["raw"].astype(np.float32)), mask=dev(z["mask"]), seeding="skimage", **TM.slic_kwargs(params))
        cent, steps = seg.mask_centroids(dev(z["mask"]), params["n_segments"])
        return host(lab), host(cent), host(steps)

    def judge_slic_skimage(got, oracle):
        from tests import test_gpu_mask_seeds as TM
        z, _ = TM.load(FIXTURE)
        assert np.array_equal(got[1][:, 1:], z["seeds_yx"]) and not got[1][:, 0].any() and np.array_equal(got[2], z["seed_steps_all"])
        assert got[0].dtype == np.int32 and np.array_equal(got[0], seeded_labels())
    NEW["wrapper:slic_skimage"] = Op(slic_skimage, judge=judge_slic_skimage)

    # the stage entry of quickshift against the oracle's float64 stages (tests/qs_stages.py), the smallest case of its own test file
    QS = "below_window_9x13"

    @functools.lru_cache(maxsize=None)
    def qs_image():
        from tests import test_gpu_quickshift_stages as TQ
        H, W, C, ks, md, ratio, sigma, lab, kind, expect = TQ.CASES[QS]
        assert (ratio, sigma, lab, expect) == (1.0, 0, False, 0)
        return TQ.make_image(kind, H, W, C, seed=len(QS)), ks, md

    def quickshift_stages(ctx, oracle):
        from tests import qs_stages as Q
        img, ks, md = qs_image()
        return Q.run_gpu(dev(img), ratio=1.0, kernel_size=ks, max_dist=md, sigma=0.0, convert2lab=False, random_seed=7, ctx=ctx)

    def judge_quickshift_stages(g, oracle):
        from tests import qs_stages as Q
        img, ks, md = qs_image()
        ref_img = Q.oracle_image(oracle, img, 1.0, 0.0, False, False)
        assert np.array_equal(g["noise"], np.random.RandomState(7).normal(scale=0.00001, size=img.shape[:2]))
        Q.check(g, oracle.quickshift_stages(ref_img, g["noise"], ks, md, tau=Q.TAU), md, "A", expect_flags=0, staged_ref=ref_img, name=QS)
    NEW["wrapper:quickshift_stages"] = Op(quickshift_stages, judge=judge_quickshift_stages)

    # a session's set_segments / get_alive / set_alive against the oracle's tiler (oracle/tiler.py), image and mask late like the rest
    def session_flags(ctx, oracle):
        from obia_amd.distributed import HipTilerEngine
        it, mask = dev(np.array(WHT.session_inputs())), dev(np.ones((40, 40), np.uint8))
        e = HipTilerEngine(it, mask, 40, 0, 20, 5, 2.0, (1.0, 1.0), {}, 8, ctx=ctx)
        try:
            e.run(False, 0, 2)
            first = e.next_id()
            e.set_segments(first, dev(np.array([3, 2 ** 32 - 1], np.int64)))  # two imported segments, one that continues beyond the halo
            alive = e.get_alive(first + 2)
            flipped = alive.clone()
            flipped[1] = 0
            e.set_alive(flipped)
            return first, e.next_id(), host(alive), host(e.get_alive(first + 2))
        finally:
            e.close()

    def judge_session_flags(got, oracle):
        from oracle import tiler
        t = tiler.OracleTiler(WHT.session_inputs(), None, 40, 0, **WHT.SESSION_KW)
        t.run(False, 0, 2)
        first, after, alive, back = got
        assert first == t.next_id > 1 and after == first + 2
        t.set_segments(first, [3, tiler.HUGE])
        want = np.array([1 if t.alive.get(g) else 0 for g in range(1, t.next_id)], np.uint8)
        assert want[0] == 1 and want[-2:].tolist() == [1, 1] and np.array_equal(alive[1:], want)
        want[0] = 0                                                           # what set_alive cleared
        assert np.array_equal(back[1:], want) and back[0] == alive[0]
    NEW["session:set_segments_set_alive"] = Op(session_flags, judge=judge_session_flags)

    # cost_allocation on CUDA tensors (the reused `crowns_mask` hands it NumPy arrays)
    def allocation(ctx, oracle):
        from obia_amd import cost_allocation
        from tests import test_gpu_crowns as TC
        c = TC.case("mask", TC.SHAPES[4])
        return host(cost_allocation(dev(c["cost"]), dev(c["rows"]), dev(c["cols"]), dev(c["ids"]), mask=dev(c["mask"]), **c["kw"]))

    def judge_allocation(got, oracle):
        from tests import test_gpu_crowns as TC
        c = TC.case("mask", TC.SHAPES[4])
        assert TC.same_bits(got[0], c["want"][0]) and np.array_equal(got[1], c["want"][1])
    NEW["crowns:cost_allocation"] = Op(allocation, judge=judge_allocation)


# -- the six host-pointer entry points, on NumPy arrays (the wrappers of tests/test_gpu_wrapper_plumbing.py).  The NumPy path uploads
#    synchronously inside the library and is not what is at risk: these cases are there for the completeness test, nothing of theirs
#    is late, and five of them are judged by the same wrapper's plain run only (the sixth by the tiler's restatement).
def _host_cases():
    from tests import test_gpu_wrapper_plumbing as WP

    @functools.lru_cache(maxsize=None)
    def data():
        return (getattr(WP.data, "__wrapped__", None) or WP.data.__pytest_wrapped__.obj)()

    def wrapper(name):
        def run(ctx, oracle):
            names, call, _, _ = WP._cases()[name]
            return [host(v) for v in WP.leaves(call(data(), *[data()[n] for n in names]))]
        return Op(run)
    for name in ("slic", "zonal_stats", "quickshift", "create_tiled_segments"):
        NEW[f"host:{name}"] = wrapper(name)

    def tiled_skimage_host(ctx, oracle):
        from tests import test_gpu_tiling_skimage as TS
        img, mask, kw = TS.checkerboard_case()
        lab, n = TS.gpu(img, mask, device=False, seeding="skimage", **kw)
        TS.same(np.asarray(lab), n, *WHT._skimage_reference(oracle), "checkerboard, host arrays")
        return np.asarray(lab), n
    NEW["host:create_tiled_segments_skimage"] = Op(tiled_skimage_host)


# -- the device primitives' hook (tests/test_gpu_wave_ops.py): a one-workgroup scan and a per-workgroup rank on one late input each
def _wave_ops_cases():
    from tests import test_gpu_wave_ops as WO
    values = np.random.RandomState(5).randint(0, 8, 2 * 1024 + 3)
    calls = ((WO.SCAN_I64, 1024), (WO.BLOCK_FLAG_RANK, 256))

    def run(ctx, oracle):
        return tuple(a for op, nt in calls for a in WO.wave_ops(op, nt, values, ctx))

    def judge(got, oracle):
        want = tuple(a for op, nt in calls for a in WO.expected(op, nt, values))
        assert len(got) == len(want)
        for g, w in zip(got, want):
            bits_equal(g, w, "wave ops")
    NEW["test:wave_ops"] = Op(run, judge=judge)
    CALLS["test:wave_ops"] = ("obia_test_wave_ops_dev",) * len(calls)


for _build in (_image_cases, _sharpness_cases, _training_cases, _crowns_cases, _pointcloud_cases, _ground_cases, _groundfilter_cases,
               _adjacency_cases, _shapes_cases, _merging_cases, _seeds_cases, _mlp_shap_pieces, _wrapper_cases, _host_cases,
               _wave_ops_cases):
    _build()

REUSED = [name for name in WHT.OPS if not name.startswith("guards:")]
ALL = {name: WHT.OPS[name] for name in REUSED}
ALL.update(NEW)
CASES = list(ALL)


# ---- running a case -------------------------------------------------------------------------------------------------------------------
_plain = {}


def plain_result(name, oracle):
    """the case's result on a fresh context with nothing instrumented, judged by its reference: computed once, shared"""
    if name in REUSED:
        return WHT.fresh_result(name, oracle)[0]
    if name not in _plain:
        from obia_amd import _lib
        op, ctx = ALL[name], _lib.Context(0)
        try:
            with WHT.as_default(ctx):
                got = op.run(ctx, oracle)
                if op.judge is not None:
                    op.judge(got, oracle)
            _plain[name] = got
        finally:
            ctx.close()
    return _plain[name]


def compare(name, got, want, oracle, tag):
    if name in REUSED:
        WHT.compare(name, ALL[name], got, want, oracle, tag)
    else:
        assert same(got, want), f"{tag}: the result differs from the plain run's"
        if ALL[name].judge is not None:
            ALL[name].judge(got, oracle)


@contextlib.contextmanager
def late_inputs(t, delay):
    """inside: every upload of a host tensor with `.cuda()` -- dev() here, the helpers of the reused cases' own files, the raw
    uploads of the session, connectivity and tiled cases -- returns a late() tensor.  The wrappers never upload this way (they
    use torch.as_tensor(..., device=) and .to()), so only the tests' inputs are touched."""
    made = []                                                                  # (the shapes of the late tensors, for the test to count)
    if delay is None:
        yield made
        return
    plain = torch.Tensor.cuda

    def cuda(self, *args, **kwargs):
        out = plain(self, *args, **kwargs)
        if self.is_cuda:
            return out
        made.append(tuple(out.shape))
        return SO.late(out, t, delay)
    torch.Tensor.cuda = cuda
    try:
        yield made
    finally:
        torch.Tensor.cuda = plain


def stale_blocks(sizes):
    """best effort (module docstring): blocks of the sizes the case allocates hold 0xA5 when it asks for them"""
    import gc
    gc.collect()
    held = [torch.full((int(n),), 0xA5, dtype=torch.uint8, device="cuda") for n in sorted(sizes)[-64:] for _ in range(2) if 0 < n <= 1 << 28]
    torch.cuda.current_stream().synchronize()
    del held


class Arranged:
    """one run of a case: its result, the log, whether s was idle when the case returned, and s"""

    def __init__(self, name, oracle, arrangement, delay_ms=None, sizes=()):
        from obia_amd import _lib
        real = _lib.load()
        op = ALL[name]
        t = torch.cuda.Stream()
        s = torch.cuda.Stream() if arrangement == "B" else None
        delay = SO.Delay(delay_ms) if delay_ms else None
        delay_s = SO.Delay(max(delay_ms, S_MIN_MS)) if delay_ms else None
        self.s, self.s_idle, self.wall = s, None, time.perf_counter()
        with torch.cuda.stream(t):
            stale_blocks(sizes)
            ctx = _lib.Context(0, stream={"A": None, "L": None, "B": s and s.cuda_stream, "C": t.cuda_stream}[arrangement])
            try:
                with WHT.as_default(ctx), SO.Instrumented(real, t, s, delay, delay_s=delay_s) as ins, late_inputs(t, delay) as made:
                    if delay is not None:
                        delay(t)                                               # whatever the case uploads itself is late too
                    self.result = op.run(ctx, oracle)
                    if s is not None:
                        self.s_idle = s.query()
                    if op.after is not None:
                        op.after(ctx, oracle)
                    ctx.close()                                                # (obia_destroy is an entry point like the others)
            finally:
                t.synchronize()
                if s is not None:
                    s.synchronize()
                ctx.close()
        self.log, self.sizes, self.late = ins.log, ins.sizes, made
        self.wall = time.perf_counter() - self.wall


_measured = {}


def measured(name, oracle):
    """((largest gap in seconds, the two entry points around it), allocation sizes, ABI calls) of a plain, logged run: arrangement "L",
    no delays"""
    if name not in _measured:
        plain_result(name, oracle)                                             # (the references are cached before anything is timed)
        r = Arranged(name, oracle, "L")
        # (not the gap in front of the obia_destroy the test itself makes: that one is the test judging the result, and reads nothing)
        gaps = [(b.t_in - a.t_out, a.name, b.name) for a, b in zip(r.log, r.log[1:]) if b.name != "obia_destroy"]
        _measured[name] = (max(gaps, default=(0.0, "", "")), r.sizes, len(r.log))
    return _measured[name]


def delay_ms(name, oracle):
    return max(FLOOR_MS.get(name, 0.0), min(SO.MAX_MS, SO.delay_ms_for(measured(name, oracle)[0][0])))


def idle_violations(log):
    """(index in the log, entry point) of every served call that was entered with torch's stream busy.  A refused call (a negative
    status) reads and writes nothing on the device and is not judged."""
    return [(i, r.name) for i, r in enumerate(log) if not r.idle_t and not r.refused and r.name not in IDLE_EXEMPT]


def pending_violations(log):
    """(index, entry point, returned with s busy) of every served call that returned with s busy and is not declared asynchronous, or
    is and returned with s idle.  A refused call returns at once, whatever the delay in front of it does."""
    return [(i, r.name, r.pending_s) for i, r in enumerate(log) if not r.refused and r.pending_s != (r.name in ASYNC)]


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
def test_the_delay_is_calibrated_and_bounded():
    per_ms = SO.Delay.calibrate()
    t = torch.cuda.Stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(t):
        a.record()
        SO.Delay(20.0)(t)
        b.record()
    assert not t.query()                                                       # it is still running when the host gets here
    b.synchronize()
    ms = a.elapsed_time(b)
    print(f"calibration: {per_ms:.1f} {'cycles' if SO.Delay.how == '_sleep' else 'matmuls'} per ms ({SO.Delay.how}); a 20 ms delay took {ms:.2f} ms")
    assert 10.0 <= ms <= 60.0 and t.query()


@pytest.mark.parametrize("name", CASES)
def test_no_case_needs_more_than_the_cap(oracle, name):
    """the delay of a case is 4 x its largest host gap between two ABI calls; a case that needs more than the cap has a host-side
    computation between two calls and must be split"""
    (gap, before, after), _, calls = measured(name, oracle)
    print(f"{name}: {calls} ABI calls, largest gap {gap * 1e3:.3f} ms ({before} -> {after}), delay {delay_ms(name, oracle):.1f} ms")
    assert calls > 0, "the case calls the library"
    assert SO.delay_ms_for(gap) <= SO.MAX_MS, f"{name}: {gap * 1e3:.1f} ms of host time between {before} and {after}"


@pytest.mark.parametrize("name", CASES)
def test_a_default_context_late_inputs(oracle, name):
    want = plain_result(name, oracle)
    r = Arranged(name, oracle, "A", delay_ms(name, oracle), measured(name, oracle)[1])
    assert bool(r.late) != (name in NOT_LATE), f"late inputs: {r.late}"
    assert not idle_violations(r.log), f"entered with torch's stream busy: {idle_violations(r.log)}"
    compare(name, r.result, want, oracle, f"{name}, arrangement A")


_b_logs = {}


def arrangement_b(name, oracle):
    if name not in _b_logs:
        _b_logs[name] = Arranged(name, oracle, "B", delay_ms(name, oracle), measured(name, oracle)[1])
    return _b_logs[name]


@pytest.mark.parametrize("name", CASES)
def test_b_context_on_a_second_stream(oracle, name):
    want = plain_result(name, oracle)
    r = arrangement_b(name, oracle)
    assert bool(r.late) != (name in NOT_LATE), f"late inputs: {r.late}"
    assert not idle_violations(r.log), f"entered with torch's stream busy: {idle_violations(r.log)}"
    assert not pending_violations(r.log), f"not what the headers declare: {pending_violations(r.log)}"
    assert r.s_idle, "the context's stream was still busy when the wrapper returned"
    if name in CALLS:
        assert [rec.name for rec in r.log] == list(CALLS[name]) + ["obia_destroy"], [rec.name for rec in r.log]
    compare(name, r.result, want, oracle, f"{name}, arrangement B")
    with torch.cuda.stream(r.s):                                               # the context is closed: its caller's stream still works
        x = torch.full((257,), 7, dtype=torch.int32, device="cuda")
    r.s.synchronize()
    assert x.cpu().tolist() == [7] * 257


@pytest.mark.parametrize("name", CASES)
def test_c_one_stream(oracle, name):
    want = plain_result(name, oracle)
    r = Arranged(name, oracle, "C", None, measured(name, oracle)[1])
    compare(name, r.result, want, oracle, f"{name}, arrangement C")


def test_every_bound_entry_point_is_observed_in_arrangement_b(oracle):
    seen = set()
    for name in CASES:
        try:
            seen |= {r.name for r in arrangement_b(name, oracle).log}
        except Exception as e:                                                 # (that case's own test says why; here: what was not reached)
            print(f"{name}: {type(e).__name__}: {e}")
    bound = set(WH.bound_entry_points())
    assert all(len(reason) > 10 for reason in NOT_OBSERVED.values()) and set(NOT_OBSERVED) <= bound
    assert not seen & set(NOT_OBSERVED), sorted(seen & set(NOT_OBSERVED))
    missing = sorted(bound - set(NOT_OBSERVED) - seen)
    assert not missing, f"never called in arrangement B: {missing}"
    assert ASYNC <= seen, sorted(ASYNC - seen)


def test_the_asynchronous_table_is_the_headers():
    """every name of ASYNC is declared in the header its comment names, under a sentence that says so"""
    import os
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    text = {h: open(os.path.join(inc, h), encoding="utf-8").read() for h in ("obia_hip.h", "obia_image.h", "obia_sharpness.h", "obia_training.h")}
    for h in ("obia_image.h", "obia_sharpness.h", "obia_training.h"):
        assert "asynchronous on the context's stream" in " ".join(text[h].split()).replace(" * ", " ")
    for needle in ("every call is asynchronous on the context's stream except the two that return a count",
                   "the gather and the matrix are asynchronous", "obia_tiler_create queues its clears and returns"):
        assert needle in " ".join(text["obia_hip.h"].replace("\n *", " ").split()), needle
    import re
    declared = {h: set(re.findall(r"\b(obia_\w+)\s*\(", text[h])) for h in text}
    family = {"obia_image.h": "obia_image_", "obia_sharpness.h": "obia_sharp_", "obia_training.h": "obia_train_"}
    for h, prefix in family.items():
        assert {n for n in declared[h] if n.startswith(prefix)} == {n for n in ASYNC if n.startswith(prefix)}, h
    rest = {n for n in ASYNC if not n.startswith(tuple(family.values()))}
    assert rest <= declared["obia_hip.h"]
    assert {n for n in declared["obia_hip.h"] if n.startswith("obia_cost_")} - rest == {"obia_cost_select_dev", "obia_cost_edge_count_dev"}


# ---- the instrument must bite: two deliberately wrong mini-wrappers (valid buffers only, stale data, no fault) --------------------------
def test_bite_a_late_input_without_a_wait_is_seen():
    from oracle.consumers import edge_raster
    from obia_amd import _lib
    lab = PA.edge_labels()
    H, W = lab.shape
    want = edge_raster(lab).astype(np.uint8)
    assert want.any()
    real = _lib.load()
    t = torch.cuda.Stream()
    ctx = _lib.Context(0)
    try:
        with torch.cuda.stream(t), SO.Instrumented(real, t, None, SO.Delay(50.0)) as ins:
            src = torch.as_tensor(np.array(lab, np.int32)).cuda()
            out = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
            t.synchronize()
            x = SO.late(src, t, SO.Delay(50.0))
            n = ctypes.c_int64(-1)
            # the wrong wrapper: no wait for torch's stream before the library reads x
            _lib.check(_lib.load().obia_label_edges_u8_dev(ctx.handle, x.data_ptr(), H, W, out.data_ptr(), ctypes.byref(n)))
            t.synchronize()
            got = out.cpu().numpy()
    finally:
        ctx.close()
    assert [(r.name, r.idle_t) for r in ins.log] == [("obia_label_edges_u8_dev", False)]
    assert not np.array_equal(got, want) and n.value != int(want.sum()), "the call read the poison, not the labels"
    assert np.array_equal(x.cpu().numpy(), lab)                                # ... which arrived afterwards


def test_bite_a_return_without_obia_synchronize_is_seen():
    from obia_amd import _lib
    real = _lib.load()
    t, s = torch.cuda.Stream(), torch.cuda.Stream()
    ctx = _lib.Context(0, stream=s.cuda_stream)
    try:
        with torch.cuda.stream(t), SO.Instrumented(real, t, s, SO.Delay(50.0)) as ins:
            x = torch.linspace(0.0, 1.0, 4099, dtype=torch.float32, device="cuda")
            out = torch.zeros(4099, dtype=torch.uint8, device="cuda")
            t.synchronize()

            def wrong_wrapper():                                              # returns without obia_synchronize
                _lib.check(_lib.load().obia_image_stretch_u8_dev(ctx.handle, x.data_ptr(), 0, x.numel(), 0.0, 1.0, out.data_ptr()))
                return out
            wrong_wrapper()
            busy_at_return = not s.query()
            s.synchronize()
            t.synchronize()
            got = out.cpu().numpy()
    finally:
        ctx.close()
    assert busy_at_return and [(r.name, r.idle_t, r.pending_s) for r in ins.log] == [("obia_image_stretch_u8_dev", True, True)]
    assert got[0] == 0 and got[-1] == 255                                      # the buffers were valid: the work ran once s was waited for
