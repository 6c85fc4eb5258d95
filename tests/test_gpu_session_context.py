"""A tiler session holds its context (include/obia_hip.h, "B3, sharded"): its persistent state lives in the context's workspace, which
the frame of any other call would reset -- and, once the arena has more than one block, free.  The library refuses every other call on
that context from obia_tiler_create to obia_tiler_destroy, before it touches anything, and HipTilerEngine(ctx=None) makes a context of
its own instead of taking the default one every wrapper shares.  40 x 40 x 2, four tiles of 20 with a buffer of 5, like
tests/test_gpu_tiling.py::test_corner_squares_that_cut_through_pixels_hip_vs_known_answers."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

HELD = "context is held by an open tiler session"
KW = dict(tile_size=20, buffer=5, crown_radius=2.0, pixel_size=(1.0, 1.0))


def inputs():
    from tests.test_gpu_tiling import synth
    img = synth(40, 40, 2, seed=4)
    return img, torch.as_tensor(img).cuda(), torch.ones((40, 40), dtype=torch.uint8, device="cuda")


def engine(it, mask, ctx=None):
    from obia_amd.distributed import HipTilerEngine
    return HipTilerEngine(it, mask, 40, 0, 20, 5, 2.0, (1.0, 1.0), {}, 8, ctx=ctx)


def oracle_session(img):
    """the oracle's tiler through the same passes: (G, alive flags of ids 1 .. next_id - 1)"""
    from oracle import tiler
    t = tiler.OracleTiler(img, None, 40, 0, **KW)
    t.run(False, 0, 2)
    t.run(True, 0, 2)
    return t.G, np.array([1 if t.alive.get(g) else 0 for g in range(1, t.next_id)], np.uint8)


def edge_labels():
    return np.random.RandomState(5).randint(0, 3, (9, 70)).astype(np.int32)


def test_other_calls_on_a_held_context_are_refused_and_the_session_runs_on(oracle):
    from obia_amd import _lib
    from obia_amd.consumers import slic_edge
    from obia_amd.statistics import zonal_stats
    from oracle.consumers import edge_raster
    img, it, mask = inputs()
    lab = torch.as_tensor(edge_labels()).cuda()
    ctx, other = _lib.Context(0), _lib.Context(0)
    e = u = None
    try:
        u = engine(it, mask, ctx=other)                                  # the uninterrupted session, on another context
        u.run(False, 0, 2)
        u.run(True, 0, 2)
        e = engine(it, mask, ctx=ctx)
        held = ctx.workspace_bytes()
        e.run(False, 0, 2)
        for call in (lambda: slic_edge(lab, ctx=ctx), lambda: zonal_stats(it, e.G, ctx=ctx), lambda: engine(it, mask, ctx=ctx)):
            with pytest.raises(ValueError, match=HELD):
                call()
        none = ctypes.c_int64(0)
        assert _lib.load().obia_test_poison_workspace_dev(ctx.handle, 0, 0xFF, ctypes.byref(none), None) == _lib.E_INVALID
        assert HELD in _lib.last_error() and ctx.workspace_bytes() == held
        h = ctx.handle
        _lib.load().obia_destroy(h)                                      # the header's rule: refused, nothing is freed
        assert HELD in _lib.last_error() and ctx.workspace_bytes() == held
        e.run(True, 0, 2)                                                # the session runs to its end ...
        n = e.next_id()
        assert n == u.next_id() > 1
        G, alive = e.G.cpu().numpy(), e.get_alive(n).cpu().numpy()
        assert np.array_equal(G, u.G.cpu().numpy()) and np.array_equal(alive, u.get_alive(n).cpu().numpy())   # ... as the uninterrupted one
        G_ref, alive_ref = oracle_session(img)
        assert np.array_equal(G, G_ref) and np.array_equal(alive[1:], alive_ref)
        e.close()
        e = None
        got = slic_edge(lab, ctx=ctx).cpu().numpy()                      # after close() the context serves other calls again
        assert np.array_equal(got, edge_raster(edge_labels()).astype(np.float32))
    finally:
        for s in (e, u):
            if s is not None:
                s.close()
        ctx.close()
        other.close()


def test_an_engine_without_a_context_makes_its_own(oracle):
    """engine.run, a wrapper on the default context, engine.run: nothing is refused, nothing is corrupted"""
    from obia_amd import _lib
    from obia_amd.consumers import slic_edge
    from oracle.consumers import edge_raster
    img, it, mask = inputs()
    lab = torch.as_tensor(edge_labels()).cuda()
    want_edges = edge_raster(edge_labels()).astype(np.float32)
    e = engine(it, mask)
    try:
        assert e.ctx is not _lib.default_context(0) and e.ctx.handle != _lib.default_context(0).handle
        assert np.array_equal(slic_edge(lab).cpu().numpy(), want_edges)
        e.run(False, 0, 2)
        assert np.array_equal(slic_edge(lab).cpu().numpy(), want_edges)
        e.run(True, 0, 2)
        assert np.array_equal(slic_edge(lab).cpu().numpy(), want_edges)
        G, alive = e.G.cpu().numpy(), e.get_alive(e.next_id()).cpu().numpy()
        own = e.ctx
    finally:
        e.close()
    assert own.handle is None                                            # close() closed the context the engine made
    G_ref, alive_ref = oracle_session(img)
    assert np.array_equal(G, G_ref) and np.array_equal(alive[1:], alive_ref)
