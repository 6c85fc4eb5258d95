"""Every caller-provided output buffer of the C ABI between poisoned guards ("Output buffers"; tests/guarded.py).

The rest of the suite judges what lies inside an output buffer that came from `torch.empty`: the caching allocator hands back the block
an earlier call of the same shape filled with the right answer, so an element the call under test never wrote still holds the expected
value, and a write next to the buffer lands in memory nobody looks at.  Here every entry point that takes a caller output is called
through ctypes with each output taken from `guarded(...)`: every byte of it and of at least 4096 bytes (two rows, if that is more) on
either side is 0xA5 in one run and 0x5A in the next, the payload sits k = 0 and k = 1 elements (int32 label rasters: also 3) off a
16-byte boundary, and the driver asserts

  A  no guard or slack byte changed, and no payload element is still all poison (the expected output is first checked, on the host, to
     hold no element that equals a poison) -- but for the elements the header promises nothing for, which each case names with the
     header's words (`exempt=` / `keep_poison=`: those must still be wholly poison);
  B  the payload equals what the operator's Python wrapper returns for the same inputs -- value for value and NaN for NaN, and the
     two poison runs equal each other -- where the wrapper's result has been judged against the operator's reference in the same test
     (zonal statistics, whose sums are floating-point atomics: count, min, max equal and the rest within tests/zonal_reference.py's
     bars of the float64 reference);
  C  every input, on the device or the host, holds the bytes it held before the call.

Nothing here provokes a fault: guards are memory the test owns, and reads past a buffer are out of scope."""
import ctypes
import functools
import warnings

import numpy as np
import pytest

from tests import cost_restatement as CR
from tests import forest_restatement as fr
from tests import mlp_restatement as mr
from tests import mlp_shap_restatement as MS
from tests import rasterize_restatement as RR
from tests import seeds_restatement as SR
from tests import shap_restatement as SH
from tests import slic_stages as S
from tests import test_gpu_pointer_alignment as PA
from tests.guarded import POISONS, guarded, holds_poison, snapshot, unchanged
from tests.metrics import adjusted_rand_index, label_disagreement
from tests.zonal_reference import compare, tolerances, zonal_reference

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

I32, U8, F32, F64, I64 = np.int32, np.uint8, np.float32, np.float64, np.int64


# ---- one run: the guarded outputs and the watched inputs of one call -------------------------------------------------------------
class Run:
    def __init__(self, poison, k):
        self.poison, self.k = poison, k
        self.outs, self.ins = {}, []

    def out(self, name, shape, dtype, labels=False, aligned=False, exempt=None, keep_poison=False, host=False):
        """a guarded output.  `labels`: an int32 label raster, which also runs 3 elements off the boundary (everything else: at most
        1); `aligned`: a pointer the header wants on a 16-byte boundary; `exempt` / `keep_poison`: see `exempt()`"""
        k = 0 if aligned else self.k if labels else min(self.k, 1)
        g = guarded(shape, dtype, self.poison, "numpy" if host else "cuda", k)
        self.outs[name] = [g, exempt, keep_poison]
        return g

    def exempt(self, name, mask):
        """elements of output `name` the header promises nothing for (boolean array, True = exempt from `unwritten`)"""
        self.outs[name][1] = mask

    def dev(self, name, a, k=0):
        """a device input: a fresh copy of the host array `a`, watched"""
        t = PA.off(np.asarray(a), k)
        torch.cuda.synchronize()                            # (the library runs on its own stream: the copy is complete first)
        self.ins.append((name, t, snapshot(t)))
        return t

    def host(self, name, a):
        """a host input: a contiguous copy, watched"""
        h = np.array(a, order="C")
        self.ins.append((name, h, snapshot(h)))
        return h

    def watch(self, name, t):
        self.ins.append((name, t, snapshot(t)))
        return t

    def findings(self):
        torch.cuda.synchronize()
        out = []
        for name, (g, exempt, keep) in self.outs.items():
            if keep:
                s = g.stray()
                if len(s) or not g.untouched():
                    out.append(f"{name}: the call must not write it, but {len(g.t.reshape(-1)) - len(g.unwritten())} elements and "
                               f"{len(s)} guard bytes changed")
            else:
                out += g.findings(exempt=exempt, name=name)
        out += [f"input `{name}` was modified" for name, t, snap in self.ins if not unchanged(t, snap)]
        return out

    def results(self):
        return {name: g.host() for name, (g, _, keep) in self.outs.items() if not keep}


def lib_ctx():
    from obia_amd import _lib
    return _lib, _lib.load(), _lib.default_context(0)


def ok(rc):
    from obia_amd import _lib
    _lib.check(rc)


def finish():
    _lib, lib, c = lib_ctx()
    ok(lib.obia_synchronize(c.handle))
    torch.cuda.synchronize()


def ptr(t):
    return None if t is None else t.data_ptr() if hasattr(t, "data_ptr") else t.ctypes.data


def to_host(x):
    return PA.host(x)


def same(a, b):
    return PA.same(a, b)


# ---- the registry ------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, entries, want, call, label_k3=False, judge=None, deterministic=True):
        self.name, self.entries, self.want, self.call = name, tuple(entries), want, call
        self.ks = (0, 1, 3) if label_k3 else (0, 1)
        self.judge, self.deterministic = judge, deterministic


REGISTRY = {}


def register(name, entries, want, call, **kw):
    assert name not in REGISTRY
    REGISTRY[name] = Case(name, entries, want, call, **kw)


def covered_entry_points():
    return {e for c in REGISTRY.values() for e in c.entries} | set(REFUSAL_ENTRIES)


# Entry points of obia_amd/_lib.py: _SIGNATURES that take a caller output and have no case here, with the reason.
LEFT_OUT = {
    "obia_tiler_create": "labels_local is the session's persistent label raster, read and written by every later call of the session: "
                         "not the output of one call",
    "obia_tiler_get_alive": "needs an open session and the host's picture of its ids: guarded in tests/test_gpu_seam_import.py "
                            "(alive_out_dev between poisoned guards after every import), not by a case of this registry",
    "obia_tiler_import_seam": "as obia_tiler_get_alive: tests/test_gpu_seam_import.py calls it on a HipTilerEngine's handle with ids_out_dev "
                              "between poisoned guards and the caller's fmap_dev and code_of_dev pre-filled and compared whole",
    "obia_rasterize_info": "four host integers of a developer aid, no device buffer",
    "obia_slic_default_params": "fills a host struct, no buffer",
}
# ... and the ones whose only outputs are host scalars passed by reference (counts, sizes), or that take no output at all
NO_OUTPUT_BUFFER = {
    "obia_abi_version", "obia_last_error", "obia_create", "obia_create_on_stream", "obia_destroy", "obia_synchronize", "obia_workspace_bytes",
    "obia_polygon_count_i32_dev", "obia_cost_edge_count_dev", "obia_tiler_set_seeding", "obia_tiler_destroy", "obia_tiler_run",
    "obia_tiler_next_id", "obia_tiler_set_segments", "obia_tiler_set_alive", "obia_tiler_finalize", "obia_set_profiling", "obia_last_timing",
}
REFUSAL_ENTRIES = ()          # (the refusal test calls entry points the registry has already)


# ---- SLIC, single raster ---------------------------------------------------------------------------------------------------------
def slic_setup(H, W, C, masked):
    img = PA.synth(H, W, C, seed=10 + C)
    mask = PA.hole_mask(H, W) if masked else None
    kw = dict(n_segments=12 if H > 1 else 5, compactness=10.0)
    return img, mask, kw


def slic_seeds(oracle, H, W, mask, n):
    yx, steps = oracle.grid_centroids(H, W, n) if mask is None else oracle.masked_grid_centroids(mask, n)
    return np.ascontiguousarray(yx, F64), np.ascontiguousarray(steps, F64)


def judge_slic(oracle, lab, img, mask, kw, stage, seeds=None):
    """the wrapper's labels against the oracle with the bars of tests/test_gpu_pointer_alignment.py::check_slic_aligned"""
    okw = dict(kw) if seeds is None else dict(kw, seeds_yx=seeds[0], seed_steps=seeds[1])
    ref, ref_pre, _ = oracle.slic(oracle.normalize(img), mask=mask, return_all=True, **okw)
    C = img.shape[2]
    if mask is not None:
        assert (lab[mask == 0] == 0).all() and (stage == "full" or (lab[mask != 0] > 0).all())
    if stage == "pre":
        d = label_disagreement(lab, ref_pre)
        print(f"{img.shape} masked={mask is not None}: {d:.2e} of the pixels differ from the oracle before connectivity")
        assert d <= (5e-4 if C == 3 else 1e-4)
    else:
        ari = adjusted_rand_index(lab, ref)
        print(f"{img.shape} masked={mask is not None}: ARI against the oracle {ari:.6f}")
        assert ari >= 0.99


def slic_case(entry, H, W, C, masked):
    stage = "pre" if entry in ("assign", "seeded1") else "full"
    seeded = entry.startswith("seeded")

    def want(oracle):
        from obia_amd.segmentation import slic
        img, mask, kw = slic_setup(H, W, C, masked)
        seeds = slic_seeds(oracle, H, W, mask, kw["n_segments"]) if seeded else None
        lab = slic(PA.dev(img), mask=None if mask is None else PA.dev(mask), seeds=seeds, _normalize_bands=True, _stage=stage, **kw).cpu().numpy()
        judge_slic(oracle, lab, img, mask, kw, stage, seeds)
        return {"labels": lab, "_seeds": seeds}

    def call(run, w):
        from obia_amd.segmentation import make_params
        _lib, lib, c = lib_ctx()
        img, mask, kw = slic_setup(H, W, C, masked)
        it = run.dev("img", img)
        mt = run.dev("mask", mask) if masked else None
        out = run.out("labels", (H, W), I32, labels=True)
        params = make_params(normalize_bands=True, **kw)
        n = ctypes.c_int(-1)
        if seeded:
            yx = run.host("seeds.yx", w["_seeds"][0])
            sd = _lib.SlicSeeds()
            sd.yx, sd.n = yx.ctypes.data, yx.shape[0]
            sd.steps_zyx[:] = [1.0] + [float(v) for v in w["_seeds"][1]]
            ok(lib.obia_slic_seeded_f32_dev(c.handle, ptr(it), H, W, C, ptr(mt), ctypes.byref(params), ctypes.byref(sd), 1 if stage == "pre" else 0,
                                            out.ptr, ctypes.byref(n)))
        else:
            fn = lib.obia_slic_assign_only_f32_dev if stage == "pre" else lib.obia_slic_f32_dev
            ok(fn(c.handle, ptr(it), H, W, C, ptr(mt), ctypes.byref(params), out.ptr, ctypes.byref(n)))
        finish()
        lab = out.host()
        if stage == "full":
            assert n.value == len(np.unique(lab[lab >= 1]))
        if masked:                                      # the masked pixels carry start_label - 1, and the call wrote it
            assert (lab[mask == 0] == 0).all()
        return {}
    return want, call


SLIC_ENTRIES = {"slic": "obia_slic_f32_dev", "assign": "obia_slic_assign_only_f32_dev", "seeded0": "obia_slic_seeded_f32_dev",
                "seeded1": "obia_slic_seeded_f32_dev"}
for _entry, _sym in SLIC_ENTRIES.items():
    for _H, _W in [(37, 53), (1, 67)]:
        for _C in (4, 3):
            for _m in (False, True):
                register(f"{_entry}_{_H}x{_W}x{_C}_{'masked' if _m else 'unmasked'}", [_sym], *slic_case(_entry, _H, _W, _C, _m), label_k3=True)


def cc_case():
    def want(oracle):
        lab = PA.cc_inputs()
        out, n = PA.run_cc(PA.dev(lab))
        ref = oracle.enforce_connectivity(lab, 9, lab.size + 1, start_label=1)
        assert np.array_equal(out, ref) and n == len(np.unique(ref[ref > 0]))
        return {"labels": out, "n": n}

    def call(run, w):
        _lib, lib, c = lib_ctx()
        lab = PA.cc_inputs()
        H, W = lab.shape
        lt = run.dev("labels_in", lab)
        out = run.out("labels", (H, W), I32, labels=True)
        n = ctypes.c_int(-1)
        ok(lib.obia_enforce_connectivity_i32_dev(c.handle, ptr(lt), H, W, 9, lab.size + 1, 1, out.ptr, ctypes.byref(n)))
        finish()
        return {"n": n.value}
    return want, call


register("enforce_connectivity_70x90", ["obia_enforce_connectivity_i32_dev"], *cc_case(), label_k3=True)


# ---- SLIC stage by stage ---------------------------------------------------------------------------------------------------------
def stages_case(name, exact_capacity):
    """the buffers of obia_slic_stages_f32_dev; `exact_capacity`: centroid_capacity = K, else H * W with the rows at and above K
    exempt (header: "centroid_capacity  rows that seeds_yx / centroids hold" -- the call writes K of them)"""
    case = next(c for c in S.FIXED_CASES if c["name"] == name)

    def setup():
        img, mask, seeds = S.make_inputs(case)
        return img, mask, dict(S.slic_kwargs(case, mask, seeds), max_num_iter=case["iters"])

    def want(oracle):
        img, mask, kw = setup()
        a = PA.run_stages(PA.dev(img), None if mask is None else PA.dev(mask), kw)
        if not case["lab"]:
            ref32 = S.features_ref32(oracle, img, case)
            assert np.array_equal(a["features"].view(np.uint32), ref32.view(np.uint32))
        assert a["fscale"] == S.expected_fscale(a["features"])
        ref = S.sweep_ref32(oracle, a["features"], a["centroids"], a["step"], mask=mask, ignore_color=False, start_label=case["start_label"])
        fill = case["start_label"] - 1
        valid = np.ones(ref.shape, bool) if mask is None else mask != 0
        assert (a["labels_pre"][~valid] == fill).all()
        assert not (valid & (ref != fill) & (a["labels_pre"] != ref)).any()
        return {k: a[k] for k in ("features", "seeds_yx", "centroids", "labels_pre", "K", "step", "prescale", "fscale")}

    def call(run, w):
        from obia_amd.segmentation import make_params
        _lib, lib, c = lib_ctx()
        img, mask, kw = setup()
        H, W, C = img.shape
        K = w["K"]
        cap = K if exact_capacity else H * W
        it = run.dev("img", img)
        mt = None if mask is None else run.dev("mask", mask)
        g = {"features": run.out("features", (H, W, C), F32), "seeds_yx": run.out("seeds_yx", (cap, 2), F32),
             "centroids": run.out("centroids", (cap, 2 + C), F32), "labels_pre": run.out("labels_pre", (H, W), I32, labels=True)}
        if not exact_capacity:
            for k in ("seeds_yx", "centroids"):
                ex = np.zeros(g[k].shape, bool)
                ex[K:] = True
                run.exempt(k, ex)
        params = make_params(kw["n_segments"], kw["compactness"], kw["max_num_iter"], kw["convert2lab"], False, 0.5, 3, kw["slic_zero"],
                             kw["start_label"], kw["_normalize_bands"], False, kw["sigma"], kw.get("spacing"))
        s = _lib.SlicStages()
        s.features, s.seeds_yx, s.centroids, s.labels_pre = (g[k].ptr for k in ("features", "seeds_yx", "centroids", "labels_pre"))
        s.centroid_capacity, s.prepass_only, s.prepass_iters = cap, 0, 0
        ok(lib.obia_slic_stages_f32_dev(c.handle, ptr(it), H, W, C, ptr(mt), ctypes.byref(params), None, ctypes.byref(s)))
        finish()
        assert s.K == K
        if not exact_capacity:                           # the rows above K: still wholly poison
            for k in ("seeds_yx", "centroids"):
                raw = g[k].host()[K:].view(np.uint8)
                assert (raw == run.poison).all(), f"{k}: rows at or above K = {K} were written"
        return {"seeds_yx": g["seeds_yx"].host()[:K], "centroids": g["centroids"].host()[:K], "K": int(s.K), "step": float(s.step),
                "prescale": float(s.prescale), "fscale": float(s.fscale)}
    return want, call


for _name, _exact in [("s33_c3_nolab", False), ("s33_c5_raw_dense", False), ("mask_disc_c4", True), ("lab_tiny_unit", True)]:
    register(f"slic_stages_{_name}_{'capK' if _exact else 'capHW'}", ["obia_slic_stages_f32_dev"], *stages_case(_name, _exact), label_k3=True)


# ---- quickshift ------------------------------------------------------------------------------------------------------------------
QS = {"lds_23x31x3": (23, 31, 3, 3.0, 6.0), "global_17x19x5": (17, 19, 5, 2.0, 5.0)}
QS_SEED = 11


def qs_image(name):
    from tests.test_gpu_quickshift_stages import textured
    H, W, C, ks, md = QS[name]
    return textured(H, W, C, seed=C + int(ks))


def qs_want(name):
    def want(oracle):
        from tests import qs_stages as qs
        from tests.test_gpu_quickshift_stages import run_case
        H, W, C, ks, md = QS[name]
        g, _ = run_case(oracle, qs_image(name), ks, md, seed=QS_SEED, name=name)      # every stage against the oracle (tier A)
        return {"labels": g["labels"], "n": g["n_labels"], "staged": np.ascontiguousarray(np.moveaxis(g["image"], -1, 0)), "noise": g["noise"],
                "dens": g["dens"], "parent": g["parent"], "dist_parent": g["dist_parent"], "roots": g["roots"]}
    return want


def qs_case(name, stages, host=False):
    def call(run, w):
        _lib, lib, c = lib_ctx()
        H, W, C, ks, md = QS[name]
        inp = run.host if host else run.dev
        it, nt = inp("img", qs_image(name)), inp("tie_noise", w["noise"])
        out = run.out("labels", (H, W), I32, labels=True, host=host)
        n = ctypes.c_int(-1)
        head = (c.handle, ptr(it), H, W, C, 1.0, float(ks), float(md), 0.0, 0, ptr(nt), 0, out.ptr, ctypes.byref(n))
        if stages:
            g = [run.out("staged", (C, H, W), F64), run.out("noise", (H, W), F64), run.out("dens", (H, W), F64),
                 run.out("parent", (H, W), I32, labels=True), run.out("dist_parent", (H, W), F64), run.out("roots", (H, W), I32, labels=True)]
            ok(lib.obia_quickshift_stages_f32_dev(*head, *(x.ptr for x in g)))
        else:
            ok((lib.obia_quickshift_f32 if host else lib.obia_quickshift_f32_dev)(*head))
        finish()
        return {"n": n.value}

    def want(oracle):
        w = qs_want(name)(oracle)
        return w if stages else {"labels": w["labels"], "n": w["n"], "_noise": w["noise"]}
    if stages:
        return want, call

    def call_plain(run, w):
        return call(run, {"noise": w["_noise"]})
    return want, call_plain


for _name in QS:
    register(f"quickshift_{_name}", ["obia_quickshift_f32_dev"], *qs_case(_name, False), label_k3=True)
    register(f"quickshift_stages_{_name}", ["obia_quickshift_stages_f32_dev"], *qs_case(_name, True), label_k3=True)
register("quickshift_host_lds_23x31x3", ["obia_quickshift_f32"], *qs_case("lds_23x31x3", False, host=True), label_k3=True)


# ---- tiled driver ----------------------------------------------------------------------------------------------------------------
TILED = dict(tile_size=64, buffer=8, crown_radius=4, pixel_size=(1.0, 1.0), compactness=10.0)


@functools.lru_cache(maxsize=None)
def tiled_inputs():
    """129 x 131 x 4 in 3 x 3 tiles of 64 with a mask: H * W = 16899 is odd, so the int4 body and the scalar tail of ids_apply_kernel
    both run on an aligned label raster"""
    H, W = 129, 131
    img = PA.synth(H, W, 4, seed=3)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = (((yy - 60) ** 2 + (xx - 66) ** 2) < 62 ** 2).astype(U8)
    mask[128, 130] = 1                                             # a valid pixel in the tail
    img.setflags(write=False), mask.setflags(write=False)
    return img, mask


def tiled_case(seeded, host=False):
    def want(oracle):
        from obia_amd.tiling import create_tiled_segments
        from oracle import tiler
        img, mask = tiled_inputs()
        ref, n_ref = tiler.create_tiled_segments(img, mask.astype(bool), **TILED)
        lab, n = create_tiled_segments(PA.dev(img), input_mask=PA.dev(mask), **TILED)
        lab = lab.cpu().numpy()
        assert n == n_ref and np.array_equal(lab, ref), f"{(lab != ref).sum()} px differ from the oracle's tiler, n {n} vs {n_ref}"
        assert (lab[mask == 0] == 0).all() and n > 9
        return {"labels": lab, "n": n}

    def call(run, w):
        from obia_amd.segmentation import make_params
        _lib, lib, c = lib_ctx()
        img, mask = tiled_inputs()
        H, W, C = img.shape
        inp = run.host if host else run.dev
        it, mt = inp("img", img), inp("mask", mask)
        out = run.out("labels", (H, W), I32, labels=True, host=host)
        tp = _lib.TilingParams()
        tp.tile_size, tp.buffer, tp.crown_radius, tp.pixel_width, tp.pixel_height = 64, 8, 4.0, 1.0, 1.0
        params = make_params(n_segments=0, compactness=10.0, normalize_bands=True)
        n = ctypes.c_int64(-1)
        head = (c.handle, ptr(it), ptr(mt), H, W, C, ctypes.byref(tp), ctypes.byref(params))
        if seeded:
            fn = lib.obia_tiled_slic_seeded_f32 if host else lib.obia_tiled_slic_seeded_f32_dev
            ok(fn(*head, _lib.SEEDING_GRID, ctypes.cast(None, _lib.PickFn), None, out.ptr, ctypes.byref(n)))
        else:
            ok((lib.obia_tiled_slic_f32 if host else lib.obia_tiled_slic_f32_dev)(*head, out.ptr, ctypes.byref(n)))
        finish()
        return {"n": n.value}
    return want, call


register("tiled_129x131x4", ["obia_tiled_slic_f32_dev"], *tiled_case(False), label_k3=True)
register("tiled_seeded_grid_129x131x4", ["obia_tiled_slic_seeded_f32_dev"], *tiled_case(True), label_k3=True)
register("tiled_host_129x131x4", ["obia_tiled_slic_f32"], *tiled_case(False, host=True), label_k3=True)
register("tiled_seeded_grid_host_129x131x4", ["obia_tiled_slic_seeded_f32"], *tiled_case(True, host=True), label_k3=True)


# ---- host entry points of SLIC and the maskSLIC seeds ----------------------------------------------------------------------------
def slic_host_case():
    H, W, C = 37, 53, 4

    def want(oracle):
        from obia_amd.segmentation import slic
        img, mask, kw = slic_setup(H, W, C, True)
        lab = slic(img, mask=mask, _normalize_bands=True, **kw).astype(I32)
        judge_slic(oracle, lab, img, mask, kw, "full")
        return {"labels": lab}

    def call(run, w):
        from obia_amd.segmentation import make_params
        _lib, lib, c = lib_ctx()
        img, mask, kw = slic_setup(H, W, C, True)
        ih, mh = run.host("img", img), run.host("mask", mask)
        out = run.out("labels", (H, W), I32, labels=True, host=True)
        params = make_params(normalize_bands=True, **kw)
        n = ctypes.c_int(-1)
        ok(lib.obia_slic_f32(c.handle, ptr(ih), H, W, C, ptr(mh), ctypes.byref(params), out.ptr, ctypes.byref(n)))
        finish()
        return {}
    return want, call


register("slic_host_37x53x4_masked", ["obia_slic_f32"], *slic_host_case(), label_k3=True)


def mask_centroids_case():
    H, W, n_seg = 37, 53, 12

    def want(oracle):
        from obia_amd.segmentation import mask_centroids
        from tests import mask_seeds_restatement as MR
        mask = PA.hole_mask(H, W)
        cent, steps = mask_centroids(mask, n_seg)
        ref_c, ref_s = MR.mask_centroids(mask, n_seg)
        assert np.array_equal(cent, ref_c) and np.array_equal(steps, ref_s)
        return {"centroids_yx": np.ascontiguousarray(cent[:, 1:]), "steps_zyx": steps}

    def call(run, w):
        from obia_amd.segmentation import _mask_seed_picks
        _lib, lib, c = lib_ctx()
        mask = PA.hole_mask(H, W)
        idx, dense = _mask_seed_picks(int(mask.sum()), n_seg)
        mt = run.dev("mask", mask)
        ih = run.host("picks", idx)
        dh = None if dense is None else run.host("dense_picks", dense)
        yx = run.out("centroids_yx", (len(idx), 2), F64, host=True)
        st = run.out("steps_zyx", (3,), F64, host=True)
        ok(lib.obia_mask_centroids_dev(c.handle, ptr(mt), H, W, ptr(ih), len(idx), ptr(dh), 0 if dense is None else len(dense), 5, yx.ptr, st.ptr))
        finish()
        return {}
    return want, call


register("mask_centroids_37x53", ["obia_mask_centroids_dev"], *mask_centroids_case())


# ---- zonal statistics, moments, texture ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def zonal_inputs(C, subset):
    """37 x 129: labels 1 .. with label 3 removed (an empty label), n_labels above the largest label (more empty ones), band 1 all NaN;
    `subset`: a band list that is no identity prefix"""
    from tests.test_gpu_zonal_f64 import block_labels, smooth_raster
    H, W = 37, 129
    rs = np.random.RandomState(80 + C)
    raw = smooth_raster(rs, H, W, C)
    raw[rs.rand(H, W, C) < 0.01] = np.nan
    raw[:, :, 1] = np.nan
    lab = block_labels(rs, H, W, 6, jitter=0.5)
    lab[lab == 3] = 4
    bands = ([C - 1, 0] if C < 9 else [8, 1, 3, 5, 0]) if subset else None
    case = dict(raw=raw, lab=lab, bands=bands, start_label=1, n_labels=int(lab.max()) + 5)
    ref = zonal_reference(raw, lab, bands=bands, start_label=1, n_labels=case["n_labels"])
    assert not ref["near_threshold"].any() and ref["count"][2] == 0 and (ref["count"][-5:] == 0).all()
    raw.setflags(write=False), lab.setflags(write=False)
    return case, ref, tolerances(ref)


def judge_zonal(got, w, moments):
    """count, min, max equal to the wrapper's; everything within the bars of the float64 reference (test_gpu_zonal_f64.py::check)"""
    case, ref, tol = w["_case"]
    st = {k: got[k] for k in ("count", "mean", "variance", "min", "max") if k in got}
    if moments:
        st.update(skewness=got["skewness"], kurtosis=got["kurtosis"])
        for k in ("count", "mean", "min", "max"):
            st.setdefault(k, w[k])
    bad = compare(st, ref, tol, moments=moments)
    assert not bad, bad
    for k in ("count", "min", "max"):
        if k in got:
            assert same(got[k], w[k]), f"`{k}` differs from the wrapper's"


def zonal_case(C, subset, moments, fresh_var=True, host=False):
    def want(oracle):
        from obia_amd.statistics import zonal_stats
        case, ref, tol = zonal_inputs(C, subset)
        st = to_host(zonal_stats(PA.dev(case["raw"]), PA.dev(case["lab"]), bands=case["bands"], start_label=1, n_labels=case["n_labels"], moments=moments))
        bad = compare(st, ref, tol, moments=moments)
        assert not bad, bad
        st["_case"] = (case, ref, tol)
        if moments:
            first = to_host(zonal_stats(PA.dev(case["raw"]), PA.dev(case["lab"]), bands=case["bands"], start_label=1, n_labels=case["n_labels"]))
            st["_first_var"], st["_first_mean"] = first["variance"], first["mean"]
        return st

    def call(run, w):
        _lib, lib, c = lib_ctx()
        case = w["_case"][0]
        raw, lab = case["raw"], case["lab"]
        H, W, _ = raw.shape
        bl = list(range(C)) if case["bands"] is None else case["bands"]
        B, N = len(bl), case["n_labels"]
        inp = run.host if host else run.dev
        rt, lt = inp("raw", raw), inp("labels", lab)
        bh = run.host("bands", np.ascontiguousarray(bl, I32))
        head = (c.handle, ptr(rt), ptr(lt), H, W, C, ptr(bh), B, N, 1)
        if not moments:
            g = [run.out("count", (N,), I64, host=host), run.out("mean", (N, B), F64, host=host), run.out("variance", (N, B), F64, host=host),
                 run.out("min", (N, B), F32, host=host), run.out("max", (N, B), F32, host=host)]
            ok((lib.obia_zonal_stats_f32 if host else lib.obia_zonal_stats_f32_dev)(*head, *(x.ptr for x in g)))
        elif host:
            g = [run.out("skewness", (N, B), F64, host=True), run.out("kurtosis", (N, B), F64, host=True), run.out("variance", (N, B), F64, host=True)]
            ok(lib.obia_zonal_moments_f32(*head, *(x.ptr for x in g)))
        else:
            mean = run.dev("mean", w["_first_mean"])
            g = [run.out("skewness", (N, B), F64), run.out("kurtosis", (N, B), F64)]
            if fresh_var:                                 # a fresh buffer: every entry, the empty labels' too, is this call's to write
                var = run.out("variance", (N, B), F64).ptr
            else:                                         # the first pass's table, as obia_amd.statistics passes it
                keep = PA.dev(w["_first_var"])
                var = keep.data_ptr()
            ok(lib.obia_zonal_moments_f32_dev(*head, ptr(mean), g[0].ptr, g[1].ptr, var))
            if not fresh_var:
                finish()
                return {"variance": keep.cpu().numpy()}
        finish()
        return {}
    return want, call


def _zj(moments):
    return lambda got, w: judge_zonal(got, w, moments)


for _C, _sub in [(3, False), (4, False), (9, False), (9, True), (4, True)]:
    _t = f"C{_C}{'_subset' if _sub else ''}"
    register(f"zonal_stats_{_t}", ["obia_zonal_stats_f32_dev"], *zonal_case(_C, _sub, False), judge=_zj(False), deterministic=False)
    register(f"zonal_moments_fresh_var_{_t}", ["obia_zonal_moments_f32_dev"], *zonal_case(_C, _sub, True), judge=_zj(True), deterministic=False)
register("zonal_moments_first_pass_var_C4", ["obia_zonal_moments_f32_dev"], *zonal_case(4, False, True, fresh_var=False), judge=_zj(True),
         deterministic=False)
register("zonal_stats_host_C4", ["obia_zonal_stats_f32"], *zonal_case(4, False, False, host=True), judge=_zj(False), deterministic=False)
register("zonal_moments_host_C4", ["obia_zonal_moments_f32"], *zonal_case(4, False, True, host=True), judge=_zj(True), deterministic=False)


def texture_case(C, subset):
    def want(oracle):
        from obia_amd.statistics import texture_stats
        from oracle.glcm import PROPS
        from tests.test_gpu_texture_cases import texture_reference
        case, _, _ = zonal_inputs(C, subset)
        kw = dict(bands=case["bands"], start_label=1, n_labels=case["n_labels"])
        ref = texture_reference(case["raw"], case["lab"], **kw)
        tx = texture_stats(PA.dev(case["raw"]), PA.dev(case["lab"]), **kw)
        out6 = np.stack([tx[p].cpu().numpy() for p in PROPS])
        for i, p in enumerate(PROPS):
            assert np.array_equal(np.isnan(out6[i]), np.isnan(ref[p])), p
            np.testing.assert_allclose(out6[i], ref[p], rtol=1e-9, atol=1e-12, equal_nan=True, err_msg=p)
        assert np.isnan(out6[:, 2]).all() and np.isnan(out6[:, -5:]).all()          # the empty labels
        return {"out6": out6}

    def call(run, w):
        _lib, lib, c = lib_ctx()
        case, _, _ = zonal_inputs(C, subset)
        raw, lab = case["raw"], case["lab"]
        H, W, _ = raw.shape
        bl = list(range(C)) if case["bands"] is None else case["bands"]
        rt, lt = run.dev("raw", raw), run.dev("labels", lab)
        bh = run.host("bands", np.ascontiguousarray(bl, I32))
        out = run.out("out6", (6, case["n_labels"], len(bl)), F64)
        ok(lib.obia_texture_stats_f32_dev(c.handle, ptr(rt), ptr(lt), H, W, C, ptr(bh), len(bl), case["n_labels"], 1, out.ptr))
        finish()
        return {}
    return want, call


for _C, _sub in [(3, False), (4, False), (9, True)]:
    register(f"texture_C{_C}{'_subset' if _sub else ''}", ["obia_texture_stats_f32_dev"], *texture_case(_C, _sub))


# ---- polygon rings and rasterize -------------------------------------------------------------------------------------------------
def polygon_case(name):
    def counts(lab, start):
        _lib, lib, c = lib_ctx()
        H, W = lab.shape
        n_r, n_v = ctypes.c_int64(0), ctypes.c_int64(0)
        ok(lib.obia_polygon_count_i32_dev(c.handle, ptr(PA.dev(lab)), H, W, start, ctypes.byref(n_r), ctypes.byref(n_v)))
        return int(n_r.value), int(n_v.value)

    def tuples(rl, rh, ro, xy):
        """the raw rings in the wrapper's order: by label, exterior before holes, then the library's order (stable)"""
        order = np.lexsort((rh.astype(bool), rl))
        return [(int(rl[r]), bool(rh[r]), [(int(x), int(y)) for x, y in xy[ro[r]:ro[r + 1]]]) for r in order]

    def want(oracle):
        from tests.test_gpu_polygons import oracle_grouped
        lab, start = PA.polygon_map(name)
        rings = PA.run_polygons(PA.dev(lab), start)
        assert rings == oracle_grouped(lab, start)
        R, V = counts(lab, start)
        assert R == len(rings) and V == sum(len(r[2]) for r in rings)
        return {"rings": rings, "R": R, "V": V}

    def call(run, w):
        _lib, lib, c = lib_ctx()
        lab, start = PA.polygon_map(name)
        H, W = lab.shape
        R, V = w["R"], w["V"]                               # the capacities are exactly the counts
        lt = run.dev("labels", lab)
        g = [run.out("ring_label", (R,), I32), run.out("ring_is_hole", (R,), U8), run.out("ring_offset", (R + 1,), I64), run.out("xy", (V, 2), I32)]
        n_r, n_v = ctypes.c_int64(-1), ctypes.c_int64(-1)
        ok(lib.obia_polygon_rings_i32_dev(c.handle, ptr(lt), H, W, start, R, V, *(x.ptr for x in g), ctypes.byref(n_r), ctypes.byref(n_v)))
        finish()
        assert (n_r.value, n_v.value) == (R, V)
        rl, rh, ro, xy = (x.host() for x in g)
        assert ro[0] == 0 and ro[-1] == V and set(np.unique(rh).tolist()) <= {0, 1}
        return {"rings": tuples(rl, rh, ro, xy), "R": R, "V": V, "ring_label": None, "ring_is_hole": None, "ring_offset": None, "xy": None}
    return want, call


for _name in ("donut", "salt"):
    register(f"polygon_rings_{_name}", ["obia_polygon_rings_i32_dev"], *polygon_case(_name))


@functools.lru_cache(maxsize=None)
def row_shapes():
    """a raster of one row: rectangles, a triangle and a ring wholly outside"""
    H, W = 1, 203
    shapes = [[RR.rect(3.2, -0.5, 40.7, 1.5)], [RR.rect(30.0, 0.0, 90.0, 1.0)], [np.array([[100.0, -3.0], [150.0, 4.0], [120.5, 0.2]])],
              [RR.rect(199.6, 0.1, 260.0, 0.9)], [RR.rect(-50.0, 5.0, -10.0, 9.0)]]
    values = np.array([5, 6, 7, 8, 9], I32)
    xy, ring_off, owner = RR.pack(shapes)
    want = RR.burn(xy, ring_off, owner, values, (H, W), fill=-7)
    assert len(np.unique(want)) >= 4 and (want == 8).any() and (want == -7).any()
    return (H, W), xy, ring_off, owner, values, want


def rasterize_case(builder):
    def want(oracle):
        from obia_amd.polygons import rasterize
        shape, xy, ring_off, owner, values, ref = builder()
        got = rasterize((xy, ring_off, owner), shape, values=values, fill=-7)
        assert np.array_equal(got, ref)
        return {"out": np.ascontiguousarray(got, I32)}

    def call(run, w):
        _lib, lib, c = lib_ctx()
        (H, W), xy, ring_off, owner, values, _ = builder()
        ts = [run.dev("xy_pix", xy), run.dev("ring_offset", ring_off), run.dev("ring_shape", owner), run.dev("shape_value", values)]
        out = run.out("out", (H, W), I32, labels=True)
        ok(lib.obia_rasterize_polygons_dev(c.handle, ptr(ts[0]), ptr(ts[1]), len(owner), ptr(ts[2]), ptr(ts[3]), len(values), H, W, -7, out.ptr))
        finish()
        return {}
    return want, call


register("rasterize_100x100", ["obia_rasterize_polygons_dev"], *rasterize_case(PA.raster_shapes), label_k3=True)
register("rasterize_1x203", ["obia_rasterize_polygons_dev"], *rasterize_case(row_shapes), label_k3=True)


# ---- consumers -------------------------------------------------------------------------------------------------------------------
def edges_case(lab_fn):
    def want(oracle):
        from oracle.consumers import edge_raster
        lab = lab_fn()
        ref = edge_raster(lab)
        e = PA.run_edges(PA.dev(lab))                       # the wrapper stretches the 0 / 1 raster by its percentiles
        n, z = lab.size, int(ref.sum())
        assert e.shape == lab.shape and np.array_equal(e != 0, ref != 0) if 0 < z else True
        return {"edge": np.ascontiguousarray(ref, U8), "n": z}

    def call(run, w):
        _lib, lib, c = lib_ctx()
        lab = lab_fn()
        H, W = lab.shape
        lt = run.dev("labels", lab)
        out = run.out("edge", (H, W), U8)
        n = ctypes.c_int64(-1)
        ok(lib.obia_label_edges_u8_dev(c.handle, ptr(lt), H, W, out.ptr, ctypes.byref(n)))
        finish()
        return {"n": n.value}
    return want, call


register("label_edges_9x1030", ["obia_label_edges_u8_dev"], *edges_case(PA.edge_labels))
register("label_edges_3x1", ["obia_label_edges_u8_dev"], *edges_case(lambda: np.array([[1], [1], [2]], I32)))


def sample_case():
    def want(oracle):
        from obia_amd.consumers import sample_labels
        lab, pts, _, _ = PA.sample_inputs()
        ref = PA.sample_restatement(lab, pts, -9)
        got = sample_labels(lab, PA.SHEAR, pts, outside=-9)
        assert np.array_equal(got, ref) and (ref == -9).sum() > 100
        return {"labels": got.astype(I32)}

    def call(run, w):
        from obia_amd.consumers import invert_affine
        _lib, lib, c = lib_ctx()
        lab, pts, _, _ = PA.sample_inputs()
        H, W = lab.shape
        lt, pt = run.dev("labels", lab), run.dev("points_xy", pts)
        inv = run.host("inverse_affine6", np.array(invert_affine(PA.SHEAR), F64))
        out = run.out("labels", (len(pts),), I32)
        ok(lib.obia_sample_labels_i32_dev(c.handle, ptr(lt), H, W, ptr(inv), ptr(pt), len(pts), -9, out.ptr))
        finish()
        return {}
    return want, call


register("sample_labels_1000", ["obia_sample_labels_i32_dev"], *sample_case())


# ---- cost surface ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cost_inputs(H, W):
    """the scene of tests/test_gpu_pointer_alignment.py::cost_scene cut to H x W"""
    wv3, chm, lab = PA.cost_scene()
    out = tuple(np.ascontiguousarray(a[:H, :W]) for a in (wv3, chm, lab))
    assert np.isnan(out[1]).any() or H * W < 100
    return out


def quiet(f, *a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return f(*a, **k)


def cost_case(op, H, W):
    """one layer kernel.  The wrapper's function of the same inputs is the expected plane; CR (tests/cost_restatement.py) judges it"""
    from tests.test_gpu_cost_surface import _same

    def planes():
        wv3, chm, lab = cost_inputs(H, W)
        return wv3, chm, lab, np.ascontiguousarray(wv3[:, :, 0]), np.ascontiguousarray(wv3[:, :, 4]), np.ascontiguousarray(wv3[:, :, 6])

    def want(oracle):
        from obia_amd import cost
        wv3, chm, lab, pan, red, nir = planes()
        if op == "bands":
            gap = (np.float32(1.0) - quiet(CR.ndvi, red, nir)).astype(F32)
            _lib, lib, c = lib_ctx()
            p, g = torch.empty((H, W), dtype=torch.float32, device="cuda"), torch.empty((H, W), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ok(lib.obia_cost_bands_f32_dev(c.handle, ptr(PA.dev(wv3)), H * W, ptr(p), ptr(g)))
            finish()
            _same(p.cpu().numpy(), pan), _same(g.cpu().numpy(), gap)
            return {"pan": pan, "gap": g.cpu().numpy()}
        if op == "ndvi":
            got = quiet(cost.ndvi, red, nir)
            _same(got, quiet(CR.ndvi, red, nir))
            return {"out": got}
        if op == "sobel":
            got = quiet(cost.chm_gradient, chm, _raw=True)
            _same(got, quiet(CR.hypot_plane, chm))
            return {"out": got}
        if op == "entropy":
            got = quiet(cost.texture_entropy, pan, _raw=True)
            full = quiet(cost.texture_entropy, pan)
            _same(full, quiet(CR.texture_entropy, pan))
            return {"out": got}
        if op in ("normalise32", "normalise64"):
            x = chm if op == "normalise32" else chm.astype(F64) * 1.25
            got = quiet(cost.normalise, x)
            _same(got, quiet(CR.normalise, x))
            return {"out": got}
        layers = {}
        got = quiet(cost.make_cost_surface, wv3, chm, slic=lab, weights=PA.COST_WEIGHTS, _layers=layers)
        _same(got, quiet(CR.make_cost_surface, wv3, chm, lab, PA.COST_WEIGHTS))
        return {"out": got, "_layers": layers}

    def call(run, w):
        from obia_amd import cost
        _lib, lib, c = lib_ctx()
        wv3, chm, lab, pan, red, nir = planes()
        if op == "bands":
            wt = run.dev("hwc8", wv3)
            p, g = run.out("pan", (H, W), F32), run.out("gap", (H, W), F32)
            ok(lib.obia_cost_bands_f32_dev(c.handle, ptr(wt), H * W, p.ptr, g.ptr))
        elif op == "ndvi":
            rt, nt = run.dev("red", red), run.dev("nir", nir)
            ok(lib.obia_cost_ndvi_f32_dev(c.handle, ptr(rt), ptr(nt), H * W, run.out("out", (H, W), F32).ptr))
        elif op == "sobel":
            ct = run.dev("chm", chm)
            ok(lib.obia_cost_sobel_f32_dev(c.handle, ptr(ct), H, W, run.out("out", (H, W), F32).ptr))
        elif op == "entropy":
            pt = run.dev("pan", pan)
            lo, hi, _ = cost._select(lib, c, pt)
            table = run.watch("table_30x32", cost._table_dev(0))
            ok(lib.obia_cost_entropy_f32_dev(c.handle, ptr(pt), H, W, lo, hi, ptr(table), run.out("out", (H, W), F64).ptr))
        elif op in ("normalise32", "normalise64"):
            x = chm if op == "normalise32" else chm.astype(F64) * 1.25
            xt = run.dev("plane", x)
            lo, hi, _ = cost._select(lib, c, xt)
            ok(lib.obia_cost_normalise_dev(c.handle, ptr(xt), int(op == "normalise64"), H * W, lo, hi, run.out("out", (H, W), F64).ptr))
        else:
            L = w["_layers"]
            pt, gt = torch.empty((H, W), dtype=torch.float32, device="cuda"), torch.empty((H, W), dtype=torch.float32, device="cuda")
            wt, ct = PA.dev(wv3), PA.dev(chm)
            ok(lib.obia_cost_bands_f32_dev(c.handle, ptr(wt), H * W, ptr(pt), ptr(gt)))
            tex = cost._entropy_dev(lib, c, pt, *L["pan"])
            grad = cost._sobel_dev(lib, c, ct)
            finish()
            grad, gap, tex = run.watch("grad", grad), run.watch("gap", gt), run.watch("tex", tex)
            lt = run.dev("labels", lab)
            lohi = [L["grad"], L["gap"], L["tex"], L["edge"]]
            lo4, hi4, w4 = run.host("lo4", np.array([p[0] for p in lohi], F64)), run.host("hi4", np.array([p[1] for p in lohi], F64)), \
                run.host("w4", np.array(L["weights"], F64))
            ok(lib.obia_cost_combine_dev(c.handle, ptr(grad), ptr(gap), ptr(tex), ptr(lt), H, W, ptr(lo4), ptr(hi4), ptr(w4),
                                         run.out("out", (H, W), F32).ptr))
        finish()
        return {}
    return want, call


_COST_SYM = {"bands": "obia_cost_bands_f32_dev", "ndvi": "obia_cost_ndvi_f32_dev", "sobel": "obia_cost_sobel_f32_dev",
             "entropy": "obia_cost_entropy_f32_dev", "normalise32": "obia_cost_normalise_dev", "normalise64": "obia_cost_normalise_dev",
             "combine": "obia_cost_combine_dev"}
for _op, _sym in _COST_SYM.items():
    register(f"cost_{_op}_33x41", [_sym], *cost_case(_op, 33, 41))
for _op in ("sobel", "entropy"):
    register(f"cost_{_op}_1x41", [_COST_SYM[_op]], *cost_case(_op, 1, 41))
    register(f"cost_{_op}_33x1", [_COST_SYM[_op]], *cost_case(_op, 33, 1))


def select_case():
    """obia_cost_select_dev: its outputs are host words (n_valid, four bit patterns)"""
    H, W = 33, 41

    def want(oracle):
        from tests.test_gpu_cost_surface import _select, _want_lohi
        _, chm, _ = cost_inputs(H, W)
        lo, hi, n = _select(chm)
        ref = _want_lohi(chm)
        assert (lo, hi) == (float(ref[0]), float(ref[1])) and n == int((~np.isnan(chm)).sum())
        return {"lohi": (lo, hi), "n": n}

    def call(run, w):
        from obia_amd import cost
        _lib, lib, c = lib_ctx()
        _, chm, _ = cost_inputs(H, W)
        ct = run.dev("plane", chm)
        n = run.out("n_valid", (1,), I64, host=True)
        bits = run.out("bits4", (4,), I64, host=True)
        ok(lib.obia_cost_select_dev(c.handle, ptr(ct), 0, H * W, float(cost._Q[0]), float(cost._Q[1]), n.ptr, bits.ptr))
        finish()
        vals = bits.host().view(np.uint64).astype(np.uint32).view(F32)
        lohi = cost._lerp(int(n.host()[0]), vals[[0, 2]], vals[[1, 3]], F32)
        return {"lohi": (float(lohi[0]), float(lohi[1])), "n": int(n.host()[0]), "n_valid": None, "bits4": None}
    return want, call


register("cost_select_33x41", ["obia_cost_select_dev"], *select_case())


# ---- seeds -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def peak_plane():
    from tests.test_gpu_seeds import surface
    a = surface(33 * 1000 + 37, 33, 37)
    a.setflags(write=False)
    return a


def peaks_case(sigma):
    """33 x 37 = 1221 pixels: the flag plane is one 4096-byte chunk, of which the library zeroes the padding -- all of it is payload.
    sigma == 0: smooth_out is "not written, may be NULL" (header) -- it is passed, and must stay wholly poison."""
    V_MIN, D = 12.0, 3

    def want(oracle):
        from obia_amd.seeds import detect_peaks
        a = peak_plane()
        rows, cols, gval, rval, sm = detect_peaks(a, V_MIN, D, sigma, _smooth=True)
        peaks = SR.peaks_scipy(a, V_MIN, D, sigma)
        wr, wc = np.where(peaks)
        ref_g = SR.smooth(a, sigma)
        assert 0 < len(wr) and np.array_equal(rows, wr) and np.array_equal(cols, wc)
        assert np.array_equal(sm, ref_g) and np.array_equal(gval, ref_g[wr, wc]) and np.array_equal(rval, a[wr, wc])
        flags = np.zeros(4096, U8)
        flags[:a.size] = peaks.reshape(-1)
        out = {"flags": flags, "offsets": np.array([0, len(wr)], I32), "n": len(wr), "rows": rows, "cols": cols, "smooth_val": gval, "raw_val": rval}
        if sigma > 0:
            out["smooth"] = sm
        return out

    def call(run, w):
        _lib, lib, c = lib_ctx()
        a = peak_plane()
        H, W = a.shape
        at = run.dev("plane", a)
        smooth = run.out("smooth", (H, W), F32, keep_poison=sigma == 0)
        flags = run.out("flags", (4096,), U8, aligned=True)
        offsets = run.out("offsets", (2,), I32)
        count = ctypes.c_int64(-1)
        ok(lib.obia_seeds_peaks_dev(c.handle, ptr(at), H, W, float(sigma), D, float(np.float32(V_MIN)), smooth.ptr, flags.ptr, offsets.ptr,
                                    ctypes.byref(count)))
        finish()
        k = int(count.value)
        assert k == w["n"]
        run.watch("flags (gather input)", flags.t), run.watch("offsets (gather input)", offsets.t)
        if sigma > 0:
            run.watch("smooth (gather input)", smooth.t)
        g = [run.out("rows", (k,), I32), run.out("cols", (k,), I32), run.out("smooth_val", (k,), F32), run.out("raw_val", (k,), F32)]
        ok(lib.obia_seeds_peaks_gather_dev(c.handle, ptr(at), smooth.ptr if sigma > 0 else ptr(at), flags.ptr, offsets.ptr, H, W, k, *(x.ptr for x in g)))
        finish()
        return {"n": k}
    return want, call


register("seeds_peaks_sigma0_33x37", ["obia_seeds_peaks_dev", "obia_seeds_peaks_gather_dev"], *peaks_case(0.0))
register("seeds_peaks_sigma1_33x37", ["obia_seeds_peaks_dev", "obia_seeds_peaks_gather_dev"], *peaks_case(1.0))


@functools.lru_cache(maxsize=None)
def pair_inputs():
    from tests.test_seeds_restatement_cpu import WEIGHT, XY_THRESH
    xs, ys, cost, aff = SR.pixel_centre_case(70, 70, 40, 50, 1.0)
    return np.ascontiguousarray(xs, F64), np.ascontiguousarray(ys, F64), cost, SR.inverse6(aff), WEIGHT, XY_THRESH


PAIR_SAMPLES = 12


def pair_case(op):
    def eps_of(D):
        v = np.sort(D[np.triu_indices(len(D), 1)])
        return float((v[len(v) // 20] + v[len(v) // 20 + 1]) / 2)      # links about a twentieth of the pairs

    def want(oracle):
        from obia_amd import seeds
        xs, ys, cost, inv, weight, thresh = pair_inputs()
        D = SR.distance_matrix(xs, ys, cost, inv, weight, thresh, PAIR_SAMPLES)
        if op == "matrix":
            got = seeds.pair_distances(xs, ys, cost, inv, weight, thresh, PAIR_SAMPLES)
            assert got.dtype == F32 and np.array_equal(got, D, equal_nan=True)
            return {"matrix": got}
        if op == "stats":
            lo, med, hi = seeds.pair_stats(xs, ys, cost, inv, weight, thresh, PAIR_SAMPLES)
            assert np.array_equal(np.array([lo, med, hi], F32), np.array(SR.triu_stats(D), F32))
            return {"stats": (lo, med, hi)}
        eps = eps_of(D)
        assert not SR.near_threshold(xs, ys, D, eps, thresh)
        got = seeds.merge_clusters(xs, ys, cost, inv, weight, thresh, eps, PAIR_SAMPLES)
        ref = SR.components(D, np.float32(eps))
        assert np.array_equal(got, ref) and 1 < len(np.unique(ref)) < len(xs)
        return {"cluster": got.astype(I32), "n": len(np.unique(ref)), "_eps": eps}

    def call(run, w):
        from obia_amd import seeds
        _lib, lib, c = lib_ctx()
        xs, ys, cost, inv, weight, thresh = pair_inputs()
        n = len(xs)
        H, W = cost.shape
        xt, yt, ct = run.dev("xs", xs), run.dev("ys", ys), run.dev("cost", cost)
        inv6 = run.host("inv6", np.array(inv, F64))
        ts = run.host("ts_host", np.ascontiguousarray(seeds.line_samples(PAIR_SAMPLES)))
        head = (c.handle, ptr(xt), ptr(yt), n, ptr(ct), H, W, ptr(inv6), float(weight), float(thresh), PAIR_SAMPLES, ptr(ts))
        if op == "matrix":
            ok(lib.obia_seeds_pair_matrix_dev(*head, run.out("matrix", (n, n), F32).ptr))
            finish()
            return {}
        if op == "stats":
            st, nn = run.out("stats4", (4,), F32, host=True), run.out("n_nan", (1,), I64, host=True)
            ok(lib.obia_seeds_pair_stats_dev(*head, st.ptr, nn.ptr))
            finish()
            v = st.host()
            assert nn.host()[0] == 0
            return {"stats": (v[0], np.mean(v[1:3]), v[3]), "stats4": None, "n_nan": None}
        ncl = ctypes.c_int(-1)
        ok(lib.obia_seeds_pair_link_dev(*head, float(w["_eps"]), int(bool((cost >= 0).all())), run.out("cluster", (n,), I32).ptr, ctypes.byref(ncl)))
        finish()
        return {"n": ncl.value}
    return want, call


register("seeds_pair_matrix_n70", ["obia_seeds_pair_matrix_dev"], *pair_case("matrix"))
register("seeds_pair_link_n70", ["obia_seeds_pair_link_dev"], *pair_case("link"))
register("seeds_pair_stats_n70", ["obia_seeds_pair_stats_dev"], *pair_case("stats"))


# ---- classification --------------------------------------------------------------------------------------------------------------
N_ROWS = 257


def scale_case(wide):
    def table():
        t = np.array(fr.load_case("a")["table"][:N_ROWS], order="C")
        t[:, 5] = np.nan                                   # an all-NaN column: NaN mean, NaN scale, NaN scaled values
        t[::17, 2] = np.nan
        return t

    def want(oracle):
        from tests.test_gpu_classify import exact_columns
        t = table()
        X, mean, scale = PA.run_scale(PA.dev(t), wide)
        n, m_ref, v_ref, mabs = exact_columns(t)
        empty = n == 0
        live = ~empty
        assert empty[5] and np.isnan(mean[empty]).all() and np.isnan(scale[empty]).all()
        assert (np.abs(mean[live] - m_ref[live]) <= n[live] * 2.0 ** -52 * mabs[live]).all()
        reg = live & (scale != 1.0)
        s_ref = np.sqrt(v_ref[reg])
        assert reg.sum() >= 10 and (np.abs(scale[reg] - s_ref) <= (n[reg] * 2.0 ** -51 + 2.0 ** -52) * s_ref).all()
        with np.errstate(invalid="ignore"):
            ref = ((t - mean) / scale).astype(X.dtype)
        assert same(X, ref)
        return {"mean": mean, "scale": scale, "scaled": X}

    def call(run, w):
        _lib, lib, c = lib_ctx()
        t = table()
        N, F = t.shape
        tt = run.dev("table", t)
        g = [run.out("mean", (F,), F64), run.out("scale", (F,), F64), run.out("scaled", (N, F), F64 if wide else F32)]
        ok((lib.obia_table_scale_f64_dev if wide else lib.obia_table_scale_dev)(c.handle, ptr(tt), N, F, *(x.ptr for x in g)))
        finish()
        return {}
    return want, call


register("table_scale_257", ["obia_table_scale_dev"], *scale_case(False))
register("table_scale_f64_257", ["obia_table_scale_f64_dev"], *scale_case(True))

NO_CLASS_ROW = 100      # a row without an acceptable class: pred -1 (header); its margin is written, its value unspecified


def acceptable(N, K):
    acc = np.array(PA.acceptable_rows(N, K))
    return acc


def forest_case():
    def inputs():
        c = fr.load_case("a")
        X32 = np.ascontiguousarray(c["transformed"][:N_ROWS].astype(F32))
        acc = acceptable(N_ROWS, c["proba"].shape[1])
        return c, X32, acc

    def want(oracle):
        c, X32, acc = inputs()
        pred, margin, proba = PA.run_forest(fr.forest_of(c), PA.dev(X32), PA.dev(acc))
        want_pred, want_margin = fr.choose(c["proba"][:N_ROWS], acc.astype(bool))
        assert PA.same_bits(proba, c["proba"][:N_ROWS]) and np.array_equal(pred, want_pred) and PA.same_bits(margin, want_margin)
        pred = pred.copy()
        pred[NO_CLASS_ROW] = -1
        return {"proba": proba, "pred": pred, "margin": margin}

    def call(run, w):
        _lib, lib, ctx = lib_ctx()
        c, X32, acc = inputs()
        acc[NO_CLASS_ROW] = 0
        N, F = X32.shape
        K = c["value"].shape[1]
        xt, at = run.dev("x", X32), run.dev("acceptable", acc)
        t = {n: run.dev(n, np.ascontiguousarray(c[n])) for n in fr.ARRAYS}
        toff = run.host("tree_offset_host", np.ascontiguousarray(c["tree_offset"], I64))
        fs = _lib.Forest(*(ptr(t[n]) for n in fr.ARRAYS[:6]), ptr(toff), ptr(t["value"]), len(c["threshold"]), len(toff), K)
        g = [run.out("proba", (N, K), F64), run.out("pred", (N,), I32), run.out("margin", (N,), F64)]
        ok(lib.obia_forest_predict_dev(ctx.handle, ptr(xt), N, F, ctypes.byref(fs), ptr(at), *(x.ptr for x in g)))
        finish()
        m = g[2].host()
        m[NO_CLASS_ROW] = w["margin"][NO_CLASS_ROW]         # (unspecified by the header; written: not exempt from `unwritten`)
        return {"margin": m}
    return want, call


register("forest_predict_257", ["obia_forest_predict_dev"], *forest_case())


def forest_shap_case():
    def want(oracle):
        c = SH.load_case("a")
        phi, base = PA.run_forest_shap(SH.forest_of(c), PA.dev(c["X32"]))
        e_ref = float(c["e_ref"])
        assert float(np.abs(phi - c["phi_exact"]).max()) <= 8 * e_ref and float(np.abs(base - c["base_exact"]).max()) <= 8 * e_ref
        return {"phi": phi, "base": base}

    def call(run, w):
        _lib, lib, ctx = lib_ctx()
        c = SH.load_case("a")
        X32 = c["X32"]
        N, F = X32.shape
        K = c["value"].shape[1]
        xt = run.dev("x", X32)
        t = {n: run.dev(n, np.ascontiguousarray(c[n])) for n in fr.ARRAYS}
        cover = run.dev("cover", np.ascontiguousarray(c["cover"], F64))
        toff = run.host("tree_offset_host", np.ascontiguousarray(c["tree_offset"], I64))
        fs = _lib.Forest(*(ptr(t[n]) for n in fr.ARRAYS[:6]), ptr(toff), ptr(t["value"]), len(c["threshold"]), len(toff), K)
        ok(lib.obia_forest_shap_dev(ctx.handle, ptr(xt), N, F, ctypes.byref(fs), ptr(cover), run.out("phi", (N, F, K), F64).ptr,
                                    run.out("base", (K,), F64).ptr))
        finish()
        return {}
    return want, call


register("forest_shap_48", ["obia_forest_shap_dev"], *forest_shap_case())


def mlp_struct(run, c):
    from obia_amd import _lib
    from obia_amd.classify import _HIDDEN_ACTIVATIONS, _OUT_ACTIVATIONS
    keep = [run.dev("weights", np.ascontiguousarray(c["weights"], F64)), run.dev("biases", np.ascontiguousarray(c["biases"], F64)),
            run.host("layer_sizes", np.ascontiguousarray(c["layer_sizes"], I32))]
    ms = _lib.Mlp(ptr(keep[0]), ptr(keep[1]), ptr(keep[2]), len(keep[2]) - 1, _HIDDEN_ACTIVATIONS.index(str(c["hidden_activation"])),
                  _OUT_ACTIVATIONS.index(str(c["out_activation"])), len(c["classes_"]))
    return ms, keep


def mlp_case():
    def inputs():
        c = mr.load_case("a")
        X = np.ascontiguousarray(c["transformed"][:N_ROWS])
        return c, X, acceptable(N_ROWS, c["proba"].shape[1])

    def want(oracle):
        c, X, acc = inputs()
        pred, margin, proba, logits = PA.run_mlp(mr.mlp_of(c), PA.dev(X), PA.dev(acc))
        assert PA.same_bits(logits, mr.logits(c, X))
        want_pred, want_margin = fr.choose(proba, acc.astype(bool))
        assert np.array_equal(pred, want_pred) and PA.same_bits(margin, want_margin)
        assert float(np.abs(proba - c["proba_ld"][:N_ROWS]).max()) <= 8 * mr.pooled_e_ref()
        pred = pred.copy()
        pred[NO_CLASS_ROW] = -1
        return {"proba": proba, "pred": pred, "margin": margin, "logits": logits}

    def call(run, w):
        _lib, lib, ctx = lib_ctx()
        c, X, acc = inputs()
        acc[NO_CLASS_ROW] = 0
        N, F = X.shape
        K = len(c["classes_"])
        xt, at = run.dev("x", X), run.dev("acceptable", acc)
        ms, keep = mlp_struct(run, c)
        g = [run.out("proba", (N, K), F64), run.out("pred", (N,), I32), run.out("margin", (N,), F64), run.out("logits", (N, int(keep[2][-1])), F64)]
        ok(lib.obia_mlp_predict_dev(ctx.handle, ptr(xt), N, F, ctypes.byref(ms), ptr(at), *(x.ptr for x in g)))
        finish()
        m = g[2].host()
        m[NO_CLASS_ROW] = w["margin"][NO_CLASS_ROW]
        return {"margin": m}
    return want, call


register("mlp_predict_257", ["obia_mlp_predict_dev"], *mlp_case())


def mlp_shap_case(op):
    def want(oracle):
        from obia_amd.classify import mlp_coalition_values, shapley_combine
        c = MS.load_case("author")
        mlp = mr.mlp_of(c)
        F = c["X"].shape[1]
        values = mlp_coalition_values(mlp, c["X"], c["background"], MS.all_masks(F))
        phi, base = PA.run_mlp_shap(mlp, PA.dev(c["X"]), PA.dev(c["background"]))
        E, e_comb = mr.pooled_e_ref(), float(c["e_comb"])
        assert float(np.abs(phi - c["phi_exact"]).max()) <= 16 * E + 8 * e_comb and float(np.abs(base - c["base_exact"]).max()) <= 8 * E
        assert PA.same_bits(values[0, 0], base) and float(np.abs(values - c["values_ld"]).max()) <= 8 * E
        assert same(shapley_combine(values), phi)
        return {"values": values} if op == "coalition" else {"phi": phi, "_values": values}

    def call(run, w):
        from obia_amd.classify import _size_weights
        _lib, lib, ctx = lib_ctx()
        c = MS.load_case("author")
        N, F = c["X"].shape
        K = len(c["classes_"])
        if op == "coalition":
            xt, bt = run.dev("x", c["X"]), run.dev("background", c["background"])
            ms, keep = mlp_struct(run, c)
            ok(lib.obia_mlp_coalition_dev(ctx.handle, ptr(xt), N, F, ctypes.byref(ms), ptr(bt), bt.shape[0], None, 1 << F,
                                          run.out("values", (N, 1 << F, K), F64).ptr))
        else:
            vt = run.dev("values", w["_values"])
            sw = run.host("size_weights", _size_weights(F))
            ok(lib.obia_shapley_combine_dev(ctx.handle, ptr(vt), N, F, K, ptr(sw), run.out("phi", (N, F, K), F64).ptr))
        finish()
        return {}
    return want, call


register("mlp_coalition_author", ["obia_mlp_coalition_dev"], *mlp_shap_case("coalition"))
register("shapley_combine_author", ["obia_shapley_combine_dev"], *mlp_shap_case("combine"))


# ---- the driver ------------------------------------------------------------------------------------------------------------------
def public(d):
    return {k: v for k, v in d.items() if not k.startswith("_")}


@pytest.mark.parametrize("name", list(REGISTRY))
def test_outputs_between_guards(oracle, name):
    case = REGISTRY[name]
    w = case.want(oracle)
    want = public(w)
    for k, v in want.items():                               # (on the host, before any guarded call) rule A cannot fire on a legitimate value
        if isinstance(v, np.ndarray):
            assert not holds_poison(v), f"the expected `{k}` holds an element that equals a poison"
    by_poison = {}
    for poison in POISONS:
        for k in case.ks:
            run = Run(poison, k)
            extra = case.call(run, w)
            tag = f"{name}, poison 0x{poison:02X}, k = {k}"
            found = run.findings()
            assert found == [], (tag, found)
            got = run.results()
            got.update(extra)
            got = {key: v for key, v in got.items() if v is not None}
            if case.judge is not None:
                case.judge(got, w)
            else:
                assert got.keys() == want.keys(), (tag, sorted(got), sorted(want))
                for key in want:
                    assert same(got[key], want[key]), f"{tag}: `{key}` differs from the wrapper's result"
            by_poison.setdefault(k, []).append(got)
    if case.deterministic:                                  # nothing of the previous contents reaches the result
        for k, (a, b) in by_poison.items():
            assert same(a, b), f"{name}, k = {k}: the runs at the two poisons differ"


# ---- after a refusal -------------------------------------------------------------------------------------------------------------
def test_a_refused_call_leaves_the_guards_and_the_context_intact(oracle):
    """Five refusals on ONE context, each with guarded outputs: the code is the header's, no guard byte changes, the polygon buffers stay
    wholly poison (the capacity check precedes the launch) and so do those of a call whose buffers are refused (a null output, an output
    one byte on, an output where an input starts: the text in full), and a SLIC call on the same context afterwards gives the labels of
    a fresh context."""
    from obia_amd import _lib
    from obia_amd.segmentation import make_params
    lib = _lib.load()
    H, W, C = 37, 53, 4
    img, mask, kw = slic_setup(H, W, C, True)
    used, fresh = _lib.Context(0), _lib.Context(0)

    def good(ctx, poison):
        run = Run(poison, 1)
        out = run.out("labels", (H, W), I32, labels=True)
        n = ctypes.c_int(-1)
        ok(lib.obia_slic_f32_dev(ctx.handle, ptr(run.dev("img", img)), H, W, C, ptr(run.dev("mask", mask)), ctypes.byref(make_params(normalize_bands=True, **kw)),
                                 out.ptr, ctypes.byref(n)))
        ok(lib.obia_synchronize(ctx.handle))
        assert run.findings() == []
        return out.host()

    def slic_refused(run, image, m):
        out = run.out("labels", (H, W), I32, labels=True)
        n = ctypes.c_int(-1)
        rc = lib.obia_slic_f32_dev(used.handle, ptr(run.dev("img", image)), H, W, C, ptr(run.dev("mask", m)), ctypes.byref(make_params(normalize_bands=True, **kw)),
                                   out.ptr, ctypes.byref(n))
        return rc

    def polygons_refused(run):
        lab, start = PA.polygon_map("salt")
        n_r, n_v = ctypes.c_int64(0), ctypes.c_int64(0)
        lt = run.dev("labels", lab)
        ok(lib.obia_polygon_count_i32_dev(used.handle, ptr(lt), *lab.shape, start, ctypes.byref(n_r), ctypes.byref(n_v)))
        R, V = int(n_r.value), int(n_v.value)
        g = [run.out("ring_label", (R - 1,), I32, keep_poison=True), run.out("ring_is_hole", (R - 1,), U8, keep_poison=True),
             run.out("ring_offset", (R,), I64, keep_poison=True), run.out("xy", (V, 2), I32, keep_poison=True)]
        return lib.obia_polygon_rings_i32_dev(used.handle, ptr(lt), *lab.shape, start, R - 1, V, *(x.ptr for x in g), ctypes.byref(n_r), ctypes.byref(n_v))

    def mlp_refused(run):
        c = mr.load_case("a")
        X = np.array(c["transformed"][:N_ROWS], order="C")
        X[N_ROWS - 1, 3] = np.nan
        N, F = X.shape
        K = len(c["classes_"])
        ms, keep = mlp_struct(run, c)
        g = [run.out("proba", (N, K), F64), run.out("pred", (N,), I32), run.out("margin", (N,), F64), run.out("logits", (N, int(keep[2][-1])), F64)]
        for name in ("proba", "pred", "margin", "logits"):       # header: "(outputs unspecified)" -- only the guards are judged
            run.exempt(name, np.ones(run.outs[name][0].shape, bool))
        return lib.obia_mlp_predict_dev(used.handle, ptr(run.dev("x", X)), N, F, ctypes.byref(ms), None, *(x.ptr for x in g))

    def buffers_refused(run):
        plane = ptr(run.dev("plane", np.ascontiguousarray(img[:, :, 0])))
        work, out = run.out("work", (H, W), F32, keep_poison=True), run.out("out", (H, W), F32, keep_poison=True)
        rcs = set()
        for w, o in ((work.ptr, None), (work.ptr, out.ptr + 1), (work.ptr, plane), (plane, out.ptr), (work.ptr, work.ptr)):
            rcs.add(lib.obia_sharp_box_dev(used.handle, plane, H, W, 3, w, o, None))
            assert _lib.last_error() == "sharp box: bad arguments", (w, o)
        assert len(rcs) == 1
        return rcs.pop()

    flat = img.copy()
    flat[:, :, 2] = 7.0                                      # a constant band: 0 / 0 in normalize_band
    refusals = [("all-zero mask", lambda r: slic_refused(r, img, np.zeros((H, W), U8)), _lib.E_EMPTY, True),
                ("constant band", lambda r: slic_refused(r, flat, mask), _lib.E_NONFINITE, True),
                ("cap_rings one short", polygons_refused, _lib.E_NOMEM, False),
                ("NaN in x", mlp_refused, _lib.E_INVALID, False),
                ("buffers of the box filter", buffers_refused, _lib.E_INVALID, False)]
    try:
        want = good(fresh, POISONS[0])
        judge_slic(oracle, want, img, mask, kw, "full")
        for i, (what, refuse, code, labels_unspecified) in enumerate(refusals):
            run = Run(POISONS[i % 2], 1)
            rc = refuse(run)
            ok(lib.obia_synchronize(used.handle))
            assert rc == code, f"{what}: returned {rc}, the header says {code} ({_lib.last_error()})"
            if labels_unspecified:                           # a refused SLIC call promises nothing about labels_out; the guards stay
                run.exempt("labels", np.ones((H, W), bool))
            assert run.findings() == [], (what, run.findings())
            got = good(used, POISONS[(i + 1) % 2])
            assert np.array_equal(got, want), f"after `{what}`: {(got != want).sum()} px differ from a fresh context"
    finally:
        used.close()
        fresh.close()


# ---- the checker itself, on device tensors -----------------------------------------------------------------------------------------
def test_the_checker_sees_planted_faults_on_the_device():
    """plain torch indexing into guarded CUDA tensors, no kernel of the library: each planted fault is reported"""
    H, W = 37, 53
    for poison in POISONS:
        for k in (0, 1, 3):
            def fresh():
                g = guarded((H, W), I32, poison, "cuda", k)
                assert g.t.is_cuda and g.t.data_ptr() % 16 == (4 * k) % 16
                g.t.copy_(torch.arange(H * W, dtype=torch.int32, device="cuda").view(H, W))
                assert g.findings() == []
                return g
            g = fresh()
            flat = g.buf[g.head:].view(torch.int32) if (g.head % 4 == 0) else None
            assert flat is not None
            first = g.front // 4                                # index of the payload's first element in `flat`
            flat[first + H * W] = 7                             # a stray element just past the payload
            assert g.stray().tolist() == [0, 1, 2, 3] and g.unwritten().tolist() == []
            g = fresh()
            flat = g.buf[g.head:].view(torch.int32)
            flat[first - W] = 7                                 # one row before the payload
            assert g.stray().tolist() == [-4 * W, -4 * W + 1, -4 * W + 2, -4 * W + 3]
            g = fresh()
            g.t[H - 1, W - 1] = int(np.frombuffer(bytes([poison]) * 4, I32)[0])       # an element the "kernel" never wrote
            assert g.unwritten().tolist() == [H * W - 1] and len(g.findings()) == 1
            x = torch.arange(100, dtype=torch.float32, device="cuda")
            snap = snapshot(x)
            assert unchanged(x, snap)
            x[99] += 1
            assert not unchanged(x, snap)
            run = Run(poison, k)
            t = run.dev("input", np.arange(10, dtype=F32))
            t[3] = -1
            assert run.findings() == ["input `input` was modified"]
