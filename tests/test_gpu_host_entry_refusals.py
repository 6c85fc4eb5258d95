"""Host-pointer entry points that fail AFTER their inputs were staged on the device, and the failure path of the call frame
(obia_amd/csrc/common.hpp: Staging, call_frame; DESIGN.md 3.8, "The entry layer").

tests/test_gpu_output_guards.py::test_a_refused_call_leaves_the_guards_and_the_context_intact refuses `_dev` calls; here the same two
refusals go through obia_slic_f32, whose temporary device buffers are freed on the way out while the refused inner call's kernels
were queued on them: the status and the message are the inner call's, no guard byte of the host output changes, and a good
obia_slic_f32 on the same context afterwards gives the labels of a fresh context.  Every refusal is an ordinary status code."""
import ctypes

import numpy as np
import pytest

from tests import test_gpu_output_guards as G

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H, W, C = 37, 53, 4


def slic_host(lib, ctx, run, image, mask, kw):
    from obia_amd.segmentation import make_params
    out = run.out("labels", (H, W), G.I32, labels=True, host=True)
    n = ctypes.c_int(-1)
    rc = lib.obia_slic_f32(ctx.handle, G.ptr(run.host("img", image)), H, W, C, G.ptr(run.host("mask", mask)),
                           ctypes.byref(make_params(normalize_bands=True, **kw)), out.ptr, ctypes.byref(n))
    return rc, out


def test_a_refused_host_call_keeps_its_message_the_guards_and_the_context(oracle):
    """ONE context (and a fresh one to compare with): two refused obia_slic_f32 calls, a good one after each, then obia_zonal_stats_f32
    with n_labels = 0"""
    from obia_amd import _lib
    lib = _lib.load()
    img, mask, kw = G.slic_setup(H, W, C, True)
    flat = img.copy()
    flat[:, :, 2] = 7.0                                      # a constant band: 0 / 0 in normalize_band
    used, fresh = _lib.Context(0), _lib.Context(0)

    def good(ctx, poison):
        run = G.Run(poison, 1)
        rc, out = slic_host(lib, ctx, run, img, mask, kw)
        G.ok(rc)
        assert run.findings() == []
        return out.host()

    refusals = [("all-zero mask", img, np.zeros((H, W), G.U8), _lib.E_EMPTY, "mask is empty"),
                ("constant band", flat, mask, _lib.E_NONFINITE, "band 2 is constant")]
    try:
        want = good(fresh, G.POISONS[0])
        G.judge_slic(oracle, want, img, mask, kw, "full")
        for i, (what, image, m, code, message) in enumerate(refusals):
            run = G.Run(G.POISONS[i % 2], 1)
            rc, out = slic_host(lib, used, run, image, m, kw)
            err = _lib.last_error()
            assert rc == code, f"{what}: returned {rc}, the header says {code} ({err})"
            assert message in err and "copy failed" not in err, f"{what}: the message is not the inner call's: {err!r}"
            run.exempt("labels", np.ones((H, W), bool))        # a refused SLIC call promises nothing about labels_out; the guards stay
            assert run.findings() == [], (what, run.findings())
            got = good(used, G.POISONS[(i + 1) % 2])
            assert np.array_equal(got, want), f"after `{what}`: {(got != want).sum()} px differ from a fresh context"
        # n_labels = 0 on the same context: OBIA_OK, nothing is copied back -- all five host outputs stay wholly poison
        for poison in G.POISONS:
            run = G.Run(poison, 1)
            raw, lab = run.host("raw", img), run.host("labels", mask.astype(G.I32))
            g = [run.out("count", (1,), G.I64, keep_poison=True, host=True), run.out("mean", (1, C), G.F64, keep_poison=True, host=True),
                 run.out("variance", (1, C), G.F64, keep_poison=True, host=True), run.out("min", (1, C), G.F32, keep_poison=True, host=True),
                 run.out("max", (1, C), G.F32, keep_poison=True, host=True)]
            G.ok(lib.obia_zonal_stats_f32(used.handle, G.ptr(raw), G.ptr(lab), H, W, C, None, 0, 0, 1, *(x.ptr for x in g)))
            assert run.findings() == []
    finally:
        used.close()
        fresh.close()
