"""Every operator on a context whose workspace holds a KNOWN byte everywhere, twice: the result of a fresh context both times.

All scratch memory comes from the context's bump allocator, which keeps its memory between calls ("What a context holds between calls"): a counter,
flag table or min / max slot that an operator reads before it clears it holds what the call before left there.  On a fresh context
that is memory straight from hipMalloc, in practice zero -- so the rest of the suite cannot see such a read.  Here, for every case of
OPS (one or more per entry point: tests/workspace_history.py is the decision table) and every poison byte

    0x01   small positive integers, flags that are "true", tiny floats
    0x7F   large finite floats and integers: a missing initialisation of a maximum
    0xFF   -1, NaN, counters that are all ones

  1  the case runs on a fresh context and is judged by the operator's own reference, as its own test file judges it;
  2  a second context is poisoned (obia_test_poison_workspace_dev) with a reserve of what the fresh context holds afterwards: ONE block,
     every byte of it the poison, and the pinned host areas with it;
  3  the case runs there twice -- the first run sees the poison, the second its own leftovers -- and both results equal the fresh one,
     value for value and NaN for NaN (zonal statistics and moments, whose sums are floating-point atomics: the bars of
     tests/zonal_reference.py against the float64 reference, count, min and max equal -- the rule of tests/test_gpu_pointer_alignment.py);
  4  after each run the context holds what it held (no growth: every workspace byte the operator saw was poison or its own) and
  5  the visited map of the connectivity stage has no non-zero word.

Nothing here provokes a fault: every entry point's workspace use was read before its row ran (the `init` line of its row), so that no
poisoned word is ever used as an index."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import workspace_history as WH

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import cc_regimes as R                                            # noqa: E402
from tests import test_gpu_output_guards as G                                # noqa: E402
from tests import test_gpu_pointer_alignment as PA                           # noqa: E402

POISON_BYTES = (0x01, 0x7F, 0xFF)
same = PA.same


# ---- the instrument ----------------------------------------------------------------------------------------------------------------
def poison(ctx, reserve, byte):
    """(bytes held, non-zero words of the visited map)"""
    from obia_amd import _lib
    held, nz = ctypes.c_int64(-1), ctypes.c_int64(-1)
    torch.cuda.synchronize()
    _lib.check(_lib.load().obia_test_poison_workspace_dev(ctx.handle, int(reserve), int(byte), ctypes.byref(held), ctypes.byref(nz)))
    return held.value, nz.value


def visited_nonzero(ctx):
    from obia_amd import _lib
    nz = ctypes.c_int64(-1)
    _lib.check(_lib.load().obia_test_visited_nonzero(ctx.handle, ctypes.byref(nz)))
    return nz.value


@contextlib.contextmanager
def as_default(ctx):
    """`ctx` is what `_lib.default_context(0)` returns inside the block: the wrappers and the helpers of the other test files that take
    no context run on it"""
    from obia_amd import _lib
    old = _lib._default_ctx.get(0)
    _lib._default_ctx[0] = ctx
    try:
        yield
    finally:
        if old is None:
            _lib._default_ctx.pop(0, None)
        else:
            _lib._default_ctx[0] = old


# ---- cases: run(ctx, oracle) -> result; judged by the operator's reference inside `run` (every run) or by `judge` (the fresh run) ------
class Op:
    def __init__(self, run, judge=None, zonal=None, after=None):
        """`judge(result, oracle)`: the fresh result against the operator's reference (None: `run` judges every run itself); `zonal`:
        the moments flag of a zonal case, whose results are compared by the bars instead of whole; `after(ctx, oracle)`: a check of the
        context after every run (the regime a connectivity case took, the repeat a tiled case made)"""
        self.run, self.judge, self.zonal, self.after = run, judge, zonal, after


OPS = {}


# -- tests/test_gpu_pointer_alignment.py: OPS, each with the reference of its own test there
def _judge_slic(C, masked, stage):
    return lambda lab, oracle: PA.check_slic_aligned(oracle, lab, 96, 128, C, masked, stage)


def _judge_stages(a, oracle):
    from tests import slic_stages as S
    case = next(c for c in S.FIXED_CASES if c["name"] == "mask_disc_c4")
    img, mask, _ = S.make_inputs(case)
    assert np.array_equal(a["features"].view(np.uint32), S.features_ref32(oracle, img, case).view(np.uint32))
    assert a["fscale"] == S.expected_fscale(a["features"])
    ref = S.sweep_ref32(oracle, a["features"], a["centroids"], a["step"], mask=mask, ignore_color=False, start_label=case["start_label"])
    fill, valid = case["start_label"] - 1, mask != 0
    assert (a["labels_pre"][~valid] == fill).all() and not (valid & (ref != fill) & (a["labels_pre"] != ref)).any()


def _judge_tiled(r, oracle):
    lab0, n0 = PA.tiled_aligned(oracle)                                   # (which is the oracle's tiler, pixel for pixel)
    assert r[1] == n0 and np.array_equal(r[0], lab0)


def _judge_quickshift(name):
    def judge(r, oracle):
        from tests.metrics import adjusted_rand_index
        H, W, C, ks, md = PA.QS_CASES[name]
        img, noise = PA.qs_inputs(name)
        lab0, n0 = r
        ref = oracle.quickshift_core(img.astype(np.float64), noise, ks, md)
        assert adjusted_rand_index(lab0, ref) >= 0.99
        assert lab0.min() == 0 and lab0.max() == n0 - 1 == len(np.unique(lab0)) - 1
        assert abs(n0 - len(np.unique(ref))) <= max(1, 0.02 * len(np.unique(ref)))
    return judge


def _judge_cc(r, oracle):
    lab = PA.cc_inputs()
    ref = oracle.enforce_connectivity(lab, 9, lab.size + 1, start_label=1)
    assert np.array_equal(r[0], ref) and r[1] == len(np.unique(ref[ref > 0]))


def _judge_zonal(moments):
    def judge(st, oracle):
        _, ref, tol = PA.zonal_case("dispatch_C4_all")
        PA.judge_zonal(st, ref, tol, moments, f"fresh, moments {moments}")
    return judge


def _judge_texture(name):
    def judge(tx, oracle):
        from oracle.glcm import PROPS
        from tests.test_gpu_texture_cases import texture_reference
        ref = texture_reference(*PA.texture_inputs(name))
        for p in PROPS:
            assert np.array_equal(np.isnan(tx[p]), np.isnan(ref[p])), p
            np.testing.assert_allclose(tx[p], ref[p], rtol=1e-9, atol=1e-12, equal_nan=True, err_msg=p)
    return judge


def _judge_polygons(rings, oracle):
    from tests.test_gpu_polygons import oracle_grouped
    lab, start = PA.polygon_map("salt")
    assert start == 0 and rings == oracle_grouped(lab, start)


def _judge_rasterize(r, oracle):
    assert np.array_equal(r[0], PA.raster_shapes()[5]) and r[1] == (60, 1)


def _judge_edges(e, oracle):
    from oracle.consumers import edge_raster
    assert e.dtype == np.float32 and np.array_equal(e, edge_raster(PA.edge_labels()).astype(np.float32))


def _judge_sample(out, oracle):
    lab, pts, _, _ = PA.sample_inputs()
    assert np.array_equal(out, PA.sample_restatement(lab, pts, -9))


def _judge_cost(a, oracle):
    import warnings
    from tests import cost_restatement as CR
    from tests.test_gpu_cost_surface import _same
    wv3, chm, lab = PA.cost_scene()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = {"normalise": CR.normalise(chm), "chm_gradient": CR.chm_gradient(chm), "chm_gradient_raw": CR.hypot_plane(chm),
                "ndvi": CR.ndvi(np.ascontiguousarray(wv3[:, :, 4]), np.ascontiguousarray(wv3[:, :, 6])),
                "texture_entropy": CR.texture_entropy(np.ascontiguousarray(wv3[:, :, 0])), "cost": CR.make_cost_surface(wv3, chm, lab, PA.COST_WEIGHTS)}
    for k in want:
        _same(a[k], want[k])


def _judge_peaks(p0, oracle):
    from tests import seeds_restatement as SR
    a = PA.peak_plane()
    wr, wc = np.where(SR.peaks_scipy(a, 12.0, 3, 1))
    g = SR.smooth(a, 1)
    assert len(wr) > 0 and np.array_equal(p0[0], wr) and np.array_equal(p0[1], wc)
    assert np.array_equal(p0[4], g) and np.array_equal(p0[2], g[wr, wc]) and np.array_equal(p0[3], a[wr, wc])


def _judge_pairs(D0, oracle):
    from tests import seeds_restatement as SR
    xs, ys, cost, inv, weight, thresh = PA.pair_inputs()
    assert D0.dtype == np.float32 and np.array_equal(D0, SR.distance_matrix(xs, ys, cost, inv, weight, thresh, 12), equal_nan=True)


def _judge_scale(wide):
    def judge(r, oracle):
        from tests import forest_restatement as fr
        from tests.test_gpu_classify import exact_columns
        c = fr.load_case("a")
        table = c["table"]
        X, mean, scale = r
        n, m_ref, v_ref, mabs = exact_columns(table)
        empty, const = n == 0, c["scale_"] == 1.0
        live = ~empty
        reg = live & ~const
        assert np.isnan(mean[empty]).all() and np.isnan(scale[empty]).all() and (scale[const] == 1.0).all()
        assert (np.abs(mean[live] - m_ref[live]) <= n[live] * 2.0 ** -52 * mabs[live]).all()
        s_ref = np.sqrt(v_ref[reg])
        assert (np.abs(scale[reg] - s_ref) <= (n[reg] * 2.0 ** -51 + 2.0 ** -52) * s_ref).all()
        with np.errstate(invalid="ignore"):
            want = ((table - mean) / scale).astype(X.dtype)
        assert X.dtype == (np.float64 if wide else np.float32) and same(X, want)
    return judge


def _judge_forest(r0, oracle):
    from tests import forest_restatement as fr
    c = fr.load_case("a")
    acc = PA.acceptable_rows(*c["proba"].shape)
    want_pred, want_margin = fr.choose(c["proba"], acc.astype(bool))
    assert PA.same_bits(r0[2], c["proba"]) and np.array_equal(r0[0], want_pred) and PA.same_bits(r0[1], want_margin)


def _judge_forest_shap(r, oracle):
    from tests import shap_restatement as SH
    c = SH.load_case("a")
    e_ref = float(c["e_ref"])
    assert float(np.abs(r[0] - c["phi_exact"]).max()) <= 8 * e_ref and float(np.abs(r[1] - c["base_exact"]).max()) <= 8 * e_ref


def _judge_mlp(r0, oracle):
    from tests import forest_restatement as fr
    from tests import mlp_restatement as mr
    c = mr.load_case("a")
    acc = PA.acceptable_rows(*c["proba"].shape)
    assert PA.same_bits(r0[3], mr.logits(c, c["transformed"]))
    want_pred, want_margin = fr.choose(r0[2], acc.astype(bool))
    assert np.array_equal(r0[0], want_pred) and PA.same_bits(r0[1], want_margin)
    assert float(np.abs(r0[2] - c["proba_ld"]).max()) <= 8 * mr.pooled_e_ref()


def _judge_mlp_shap(r, oracle):
    from tests import mlp_restatement as mr
    from tests import mlp_shap_restatement as MS
    c = MS.load_case("author")
    E, e_comb = mr.pooled_e_ref(), float(c["e_comb"])
    assert float(np.abs(r[0] - c["phi_exact"]).max()) <= 16 * E + 8 * e_comb and float(np.abs(r[1] - c["base_exact"]).max()) <= 8 * E


PA_JUDGES = {
    "slic_pre_c4": _judge_slic(4, False, "pre"), "slic_full_c8_masked": _judge_slic(8, True, "full"),
    "slic_full_c3_masked": _judge_slic(3, True, "full"), "slic_stages": _judge_stages, "tiled": _judge_tiled,
    "quickshift_lds": _judge_quickshift("lds_48x64x3"), "quickshift_global": _judge_quickshift("global_40x40x5"),
    "enforce_connectivity": _judge_cc, "zonal_stats": _judge_zonal(False), "zonal_moments": _judge_zonal(True),
    "texture_thin_strips": _judge_texture("thin_strips"), "texture_dense": _judge_texture("dense_65x63"), "polygon_rings": _judge_polygons,
    "rasterize": _judge_rasterize, "slic_edge": _judge_edges, "sample_labels": _judge_sample, "cost_layers": _judge_cost,
    "seed_peaks": _judge_peaks, "seed_pair_matrix": _judge_pairs, "table_scale": _judge_scale(False), "table_scale_f64": _judge_scale(True),
    "forest_predict": _judge_forest, "forest_shap": _judge_forest_shap, "mlp_predict": _judge_mlp, "mlp_shap": _judge_mlp_shap,
}
assert set(PA_JUDGES) == set(PA.OPS)
for _name, _op in PA.OPS.items():
    OPS["pa:" + _name] = Op(lambda ctx, oracle, op=_op: op(ctx), judge=PA_JUDGES[_name],
                            zonal={"zonal_stats": False, "zonal_moments": True}.get(_name))


# -- tests/test_gpu_output_guards.py: a case of its registry, judged in every run as its own driver judges it
def _guards(name):
    def run(ctx, oracle):
        case = G.REGISTRY[name]
        w = case.want(oracle)                                             # (the wrapper on this context, against the operator's reference)
        r = G.Run(G.POISONS[0], 0)
        extra = case.call(r, w)
        assert r.findings() == [], (name, r.findings())
        got = r.results()
        got.update(extra)
        got = {k: v for k, v in got.items() if v is not None}
        if case.judge is not None:
            case.judge(got, w)
        else:
            want = G.public(w)
            assert got.keys() == want.keys(), (name, sorted(got), sorted(want))
            for key in want:
                assert same(got[key], want[key]), f"{name}: `{key}` differs from the wrapper's result"
        return got if case.deterministic else {k: got[k] for k in ("count", "min", "max") if k in got}
    return run


for _name in [c[len("guards:"):] for c in WH.cases() if c.startswith("guards:")]:
    OPS["guards:" + _name] = Op(_guards(_name))


# -- the body of an existing *_buffers test on the context: what its own judge() saw, in order (each is judged there, bit for bit)
def _body(module_name, call):
    def run(ctx, oracle):
        import importlib
        m = importlib.import_module(module_name)
        seen, judge = [], m.judge

        def recording(g, want, name):
            seen.append((name, np.array(g.host())))
            return judge(g, want, name)
        m.judge = recording
        try:
            call(m)
        finally:
            m.judge = judge
        assert seen
        return tuple(seen)
    return run


OPS["body:image_clahe"] = Op(_body("tests.test_gpu_image_buffers", lambda m: m.test_clahe(0, 67, G.POISONS[0], 3)))
OPS["body:sharp_gray_lap"] = Op(_body("tests.test_gpu_sharpness_buffers", lambda m: m.test_gray_lap(0, (140, 131), G.POISONS[0])))


def _seed_table_body(m):
    assert m.case()["rounds"] >= 3, "stage 1 must read both state planes"
    m.test_buffers_off_the_boundary_and_guarded_outputs(1, G.POISONS[0])


OPS["body:seed_table"] = Op(_body("tests.test_gpu_seed_table_buffers", _seed_table_body))
OPS["body:boxes"] = Op(_body("tests.test_gpu_boxes_buffers", lambda m: m.test_buffers_off_the_boundary_and_guarded_outputs(1, G.POISONS[0])))


# -- the ground filter's, the adjacency graph's, the shapes' and the merging's *_buffers files: run_all takes the context, judge_all judges every output bit for bit
def _groundfilter_body(ctx, oracle):
    from tests import test_gpu_groundfilter_buffers as m
    s, o, scratch, _ = m.run_all(ctx, 1, G.POISONS[0])
    m.judge_all(s, o, scratch)
    return {name: np.array(g.host()) for name, g in list(s.items()) + list(o.items())}


def _adjacency_body(ctx, oracle):
    from tests import test_gpu_adjacency_buffers as m
    o, scratch, _ = m.run_all(ctx, 1, G.POISONS[0])
    return {name: np.array(a) for name, a in m.judge_all(o, scratch).items()}   # (the records sorted inside their tiles, as it judges them)


def _shapes_body(ctx, oracle):
    from tests import test_gpu_shapes_buffers as m
    return {name: np.array(a) for name, a in m.judge_all(m.run_all(ctx, 1, G.POISONS[0])[0]).items()}


def _merging_body(ctx, oracle):
    from tests import test_gpu_merging_buffers as m
    o, scratch, _ = m.run_all(ctx, 1, G.POISONS[0])
    return {name: np.array(a) for name, a in m.judge_all(o, scratch).items()}


OPS["body:groundfilter"] = Op(_groundfilter_body)
OPS["body:adjacency"] = Op(_adjacency_body)
OPS["body:shapes"] = Op(_shapes_body)
OPS["body:merging"] = Op(_merging_body)


# -- boxes: every footprint fits the LDS table / a footprint of more labels than the table, split into passes
def _boxes(scene):
    def run(ctx, oracle):
        from obia_amd import assign_boxes, box_overlaps
        from tests import test_gpu_boxes as TB
        labels, boxes = scene()
        got = assign_boxes(labels, None, boxes, pixel=True)
        pairs = box_overlaps(labels, boxes)
        want_table, want = _boxes_reference(scene)
        assert TB.same(got.assigned, want[0]) and TB.same(got.area, want[1]) and TB.same_table(pairs, want_table)
        return (got.assigned, got.area, dict(pairs))
    return run


@functools.lru_cache(maxsize=None)
def _boxes_reference(scene):
    from tests import boxes_restatement as BR
    labels, boxes = scene()
    return BR.pair_table(labels, boxes), BR.assign(labels, boxes)


@functools.lru_cache(maxsize=None)
def _boxes_table_scene():
    from tests import test_gpu_boxes as TB
    labels, boxes = TB.scene()
    return labels, boxes[::10].copy()                                     # 301 of its boxes, the 40 x 40 one among them


@functools.lru_cache(maxsize=None)
def _boxes_passes_scene():
    """tests/test_gpu_boxes.py::test_a_footprint_with_more_labels_than_the_table_is_split_into_passes[dense-ids]"""
    from obia_amd import _lib
    side = 47
    assert side * side > 2 * _lib.BOXES_TABLE
    labels = np.arange(1, side * side + 1, dtype=np.int32).reshape(side, side)
    return labels, np.array([[3.3, 2.2, 40.7, 44.1], [-0.5, -0.5, side + 0.5, side + 0.5], [10.0, 10.0, 12.0, 12.0]])


OPS["boxes_table"] = Op(_boxes(_boxes_table_scene))
OPS["boxes_passes"] = Op(_boxes(_boxes_passes_scene))


# -- crowns
def _crowns(ctx, oracle):
    from obia_amd import cost_allocation
    from tests import test_gpu_crowns as TC
    c = TC.case("mask", TC.SHAPES[4])
    D, L = cost_allocation(c["cost"], c["rows"], c["cols"], c["ids"], mask=c["mask"], **c["kw"])
    assert TC.same_bits(D, c["want"][0]) and np.array_equal(L, c["want"][1])
    return D, L


OPS["crowns_mask"] = Op(_crowns)


# -- connectivity: one case per regime of tests/cc_regimes.py, and the batch entry on two problems
COUNTS = ("problems", "pixels", "surviving", "small", "small_px", "cut", "code", "evaluation", "side")
CC = {"cc_walks": ("slic_like_sparse", False, (0, R.WALKS, False)), "cc_lists": ("strips", False, (1, R.LISTS, False)),
      "cc_code_walks": ("comb", True, (1, R.WALKS, False)), "cc_cut": ("twin_bars_cut", False, (1, R.LISTS, True))}


@contextlib.contextmanager
def _worklist(on):
    old = os.environ.pop("OBIA_CC_WORKLIST", None)
    try:
        if on:
            os.environ["OBIA_CC_WORKLIST"] = "1"
        yield
    finally:
        os.environ.pop("OBIA_CC_WORKLIST", None)
        if old is not None:
            os.environ["OBIA_CC_WORKLIST"] = old


def _cc(name):
    case, worklist, regime = CC[name]

    def run(ctx, oracle):
        from obia_amd.segmentation import enforce_connectivity
        lab, mn, mx = R.CASES[case].make()
        with _worklist(worklist):
            out, n = enforce_connectivity(torch.as_tensor(lab.astype(np.int32)).cuda(), mn, mx, start_label=1)
        out = out.cpu().numpy()
        assert np.array_equal(out, oracle.enforce_connectivity(lab, mn, mx, start_label=1)), f"{(out != oracle.enforce_connectivity(lab, mn, mx, start_label=1)).sum()} px differ"
        return out, n

    def after(ctx, oracle):
        lab, mn, mx = R.CASES[case].make()
        rep = R.cc_report(ctx)
        want = R.predict(lab, mn, mx, start_label=1, worklist=worklist, oracle=oracle)
        assert {k: rep[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, rep
        assert (rep["code"], rep["evaluation"], rep["cut"] > 0) == regime, (name, rep)
    return Op(run, after=after)


for _name in CC:
    OPS[_name] = _cc(_name)


def _cc_batch(ctx, oracle):
    maps, probs = R.batch_touching()                                       # two problems whose touching rows carry the same labels
    assert len(maps) == 2
    flat = torch.as_tensor(np.concatenate([m.ravel() for m in maps]).astype(np.int32)).cuda()
    out = torch.full_like(flat, -5)
    rows = [(m.shape[0], m.shape[1], mn, mx) for m, (mn, mx) in zip(maps, probs)]
    n = R.enforce_connectivity_batch(flat, rows, 1, out)
    refs, n_ref = R.batch_reference(oracle, maps, probs, 1)
    out = out.cpu().numpy()
    assert np.array_equal(out, np.concatenate([r.ravel() for r in refs])) and n == n_ref
    return out, n


def _cc_batch_after(ctx, oracle):
    maps, probs = R.batch_touching()
    rep, want = R.cc_report(ctx), R.predict_batch(maps, probs, 1, oracle=oracle)
    assert rep["problems"] == 2 and {k: rep[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, rep


OPS["cc_batch"] = Op(_cc_batch, after=_cc_batch_after)


# -- tiled SLIC: the orphan repeat (the arena is rewound inside the call) and seeding="skimage" in every tile
@functools.lru_cache(maxsize=None)
def _orphan_reference(orc):
    from oracle import tiler
    from tests.test_gpu_tiling import orphan_islands_case
    img, mask, kw = orphan_islands_case()
    return tiler.create_tiled_segments(img, mask, **kw)


def _tiled_orphan(ctx, oracle):
    from obia_amd.tiling import create_tiled_segments
    from tests.test_gpu_tiling import orphan_islands_case
    img, mask, kw = orphan_islands_case()
    lab, n = create_tiled_segments(torch.as_tensor(img).cuda(), input_mask=mask, **kw)
    lab = lab.cpu().numpy()
    ref, n_ref = _orphan_reference(oracle)
    assert n == n_ref and np.array_equal(lab, ref) and (lab[~mask] == 0).all()
    return lab, n


def _repeated(ctx, oracle):
    assert ctx.timing()["batch_repeats"] >= 1, "the case is meant to take the repeat path"


OPS["tiled_orphan_repeat"] = Op(_tiled_orphan, after=_repeated)


@functools.lru_cache(maxsize=None)
def _skimage_reference(orc):
    from tests import test_gpu_tiling_skimage as TS
    from tests import tiler_skimage_restatement as TR
    img, mask, kw = TS.checkerboard_case()
    return TR.create_tiled_segments(img, mask, **kw)


def _tiled_skimage(ctx, oracle):
    from tests import test_gpu_tiling_skimage as TS
    img, mask, kw = TS.checkerboard_case()
    lab, n = TS.gpu(img, mask, seeding="skimage", **kw)
    TS.same(lab, n, *_skimage_reference(oracle), "checkerboard")
    return lab, n


OPS["tiled_skimage"] = Op(_tiled_skimage)


# -- a tiler session: create, black, two seam imports (one ranked by the LDS sort, one by counting), white, finalize
SESSION_KW = dict(tile_size=20, buffer=5, crown_radius=2.0, pixel_size=(1.0, 1.0))
ME, OWNER = 1, 2


@functools.lru_cache(maxsize=None)
def session_inputs():
    from tests.test_gpu_tiling import synth
    img = synth(40, 40, 2, seed=4)
    img.setflags(write=False)
    return img


def seam_codes(limit):
    """(codes of the first import: 100 new ids, of the second: limit + 1 new ids, each id twice, shuffled)"""
    from tests import seam_restatement as SR
    rs = np.random.RandomState(9)
    a = np.repeat(np.arange(1, 101), 2)
    b = np.repeat(np.arange(101, 101 + limit + 1), 2)
    rs.shuffle(a), rs.shuffle(b)
    return SR.code(OWNER, a), SR.code(OWNER, b)


def _session(ctx, oracle):
    from obia_amd import _lib
    from obia_amd.distributed import HipTilerEngine
    from oracle import tiler
    from tests import seam_restatement as SR
    lib = _lib.load()
    limit = int(lib.obia_test_seam_sort_limit())
    img = session_inputs()
    t = tiler.OracleTiler(img, None, 40, 0, **SESSION_KW)
    it = torch.as_tensor(np.array(img)).cuda()
    mask = torch.ones((40, 40), dtype=torch.uint8, device="cuda")
    extra = limit + 200
    e = HipTilerEngine(it, mask, 40, 0, 20, 5, 2.0, (1.0, 1.0), {}, extra, ctx=ctx)
    try:
        e.run(False, 0, 2)
        t.run(False, 0, 2)
        assert e.next_id() == t.next_id > 1 and np.array_equal(e.G.cpu().numpy(), t.G)
        cap = t.next_id + extra + 8
        fmap, code_of = np.zeros(101 + limit + 8, np.int32), np.zeros(cap, np.int32)
        fmap_t, code_of_t = torch.as_tensor(fmap).cuda(), torch.as_tensor(code_of).cuda()
        news = []
        for codes in seam_codes(limit):
            r = SR.import_seam(codes, ME, OWNER, fmap, code_of, t.next_id)
            ids, first, n_new, t_max = e.import_seam(torch.as_tensor(codes), ME, OWNER, fmap_t, code_of_t)
            assert (first, n_new, t_max) == (r["first"], r["n_new"], r["t_max"]) and np.array_equal(ids.cpu().numpy(), r["ids"])
            fmap, code_of = r["fmap"], r["code_of"]
            assert np.array_equal(fmap_t.cpu().numpy(), fmap) and np.array_equal(code_of_t.cpu().numpy(), code_of)
            t.set_segments(first, [tiler.HUGE] * n_new)                    # registered like the import: alive, never "within"
            news.append(n_new)
        assert news[0] == 100 <= limit < news[1] == limit + 1               # below and above the limit of the LDS sort
        e.run(True, 0, 2)
        t.run(True, 0, 2)
        assert e.next_id() == t.next_id
        G = e.G.cpu().numpy()
        alive = e.get_alive(t.next_id).cpu().numpy()
        assert np.array_equal(G, t.G) and np.array_equal(alive[1:], [1 if t.alive.get(g) else 0 for g in range(1, t.next_id)])
        n = ctypes.c_int64(-1)
        _lib.check(lib.obia_tiler_finalize(e.h, ctypes.byref(n)))
        final = e.G.cpu().numpy()
        ref, n_ref = t.finalize()
        assert n.value == n_ref and np.array_equal(final, ref)
    finally:
        e.close()
    return G, alive, final, n.value


OPS["session"] = Op(_session)


def _session_refusals(ctx, oracle):
    """every ordinary call is refused while the session is open -- and leaves the context as it was, the visited map included"""
    from obia_amd import _lib
    from obia_amd.distributed import HipTilerEngine
    it = torch.as_tensor(np.array(session_inputs())).cuda()
    mask = torch.ones((40, 40), dtype=torch.uint8, device="cuda")
    PA.run_cc(PA.dev(PA.cc_inputs()), ctx=ctx)                            # (a connectivity call first: the visited map exists)
    e = HipTilerEngine(it, mask, 40, 0, 20, 5, 2.0, (1.0, 1.0), {}, 8, ctx=ctx)
    try:
        with pytest.raises(ValueError, match="context is held by an open tiler session"):
            PA.run_cc(PA.dev(PA.cc_inputs()), ctx=ctx)
        assert visited_nonzero(ctx) == 0
        e.run(False, 0, 2)
        e.run(True, 0, 2)
        G, alive = e.G.cpu().numpy(), e.get_alive(e.next_id()).cpu().numpy()
    finally:
        e.close()
    return G, alive


OPS["session_refusals"] = Op(_session_refusals)

CASES = WH.cases()


def test_every_case_of_the_table_exists():
    assert set(CASES) == set(OPS), sorted(set(CASES) ^ set(OPS))


# ---- the test ----------------------------------------------------------------------------------------------------------------------
_fresh = {}


def fresh_result(name, oracle):
    """(result on a fresh context, judged; bytes the context held afterwards): computed once per case, shared by the three bytes"""
    if name not in _fresh:
        from obia_amd import _lib
        op, ctx = OPS[name], _lib.Context(0)
        try:
            with as_default(ctx):
                a = op.run(ctx, oracle)
                if op.judge is not None:
                    op.judge(a, oracle)
                if op.after is not None:
                    op.after(ctx, oracle)
            _fresh[name] = (a, ctx.workspace_bytes())
        finally:
            ctx.close()
    return _fresh[name]


def compare(name, op, got, want, oracle, tag):
    if op.zonal is not None:
        _, ref, tol = PA.zonal_case("dispatch_C4_all")
        PA.judge_zonal(got, ref, tol, op.zonal, tag)
        for k in ("count", "min", "max"):
            assert same(got[k], want[k]), f"{tag}: `{k}` differs from the fresh context's"
    else:
        assert same(got, want), f"{tag}: the result differs from the one on a fresh context"


@pytest.mark.parametrize("byte", POISON_BYTES, ids=[f"{b:02X}" for b in POISON_BYTES])
@pytest.mark.parametrize("name", CASES)
def test_operator_equals_its_fresh_context_result(oracle, name, byte):
    from obia_amd import _lib
    op = OPS[name]
    want, reserve = fresh_result(name, oracle)                             # (0: the entry point takes no workspace; the poison still fills a block)
    ctx = _lib.Context(0)
    try:
        held, nz = poison(ctx, reserve, byte)
        assert held >= max(reserve, 1) and nz == 0 and ctx.workspace_bytes() == held
        for run in (1, 2):
            tag = f"{name}, poison 0x{byte:02X}, run {run}"
            with as_default(ctx):
                got = op.run(ctx, oracle)
                if op.after is not None:
                    op.after(ctx, oracle)
            compare(name, op, got, want, oracle, tag)
            assert ctx.workspace_bytes() == held, f"{tag}: the workspace grew from {held} to {ctx.workspace_bytes()} bytes"
            assert visited_nonzero(ctx) == 0, f"{tag}: the visited map holds non-zero words"
    finally:
        ctx.close()


# ---- the instrument itself -----------------------------------------------------------------------------------------------------------
def test_the_poison_reaches_the_workspace_and_refuses_what_the_header_says():
    """The block is one, at least the reserve, and holds the byte: an operator that leaves its scratch in the arena (the connectivity
    stage's label planes) shows its own values after a call and the byte again after the next poison."""
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.Context(0)
    try:
        held, nz = poison(ctx, 1 << 20, 0x5A)
        assert held >= 1 << 20 and nz == 0 and ctx.workspace_bytes() == held
        big, _ = poison(ctx, 200 << 20, 0xFF)                              # more than the first block: grown, and still ONE block
        assert big >= 200 << 20
        assert poison(ctx, 1 << 20, 0x01)[0] == big                        # a smaller reserve keeps the block
        none = ctypes.c_int64(0)
        assert lib.obia_test_poison_workspace_dev(None, 0, 0, None, None) == _lib.E_INVALID
        for reserve, byte in ((0, -1), (0, 256), (-1, 0)):
            assert lib.obia_test_poison_workspace_dev(ctx.handle, reserve, byte, ctypes.byref(none), None) == _lib.E_INVALID
        assert lib.obia_test_visited_nonzero(None, ctypes.byref(none)) == _lib.E_INVALID
        assert lib.obia_test_visited_nonzero(ctx.handle, None) == _lib.E_INVALID
        assert ctx.workspace_bytes() == big
        out, n = PA.run_cc(PA.dev(PA.cc_inputs()), ctx=ctx)               # the context still serves
        lab = PA.cc_inputs()
        assert n > 0 and out.shape == lab.shape and ctx.workspace_bytes() == big and visited_nonzero(ctx) == 0
    finally:
        ctx.close()
