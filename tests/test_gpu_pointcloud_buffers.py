"""The entry points of include/obia_points.h through guarded states and outputs (tests/guarded.py, both poisons) with every input off a
16-byte boundary (tests/offset_views.py; z at a 4-byte, the intensity at a 2-byte residue): the results bit for bit, no stray write,
no element of the finish and column outputs left unwritten, the inputs unchanged, two runs equal; and what is refused writes
nothing.  Every entry point of the table is exercised here."""
import ctypes
import functools

import numpy as np
import pytest

from tests import pointcloud_restatement as R
from tests.guarded import POISONS, guarded, snapshot, unchanged
from tests.offset_views import offset_view, residue
from tests.refusal_text import refused_saying

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NZ, N = 106, R.NSEG
EXERCISED = ("obia_points_rasters_dev", "obia_points_rasters_finish_dev", "obia_points_segments_dev", "obia_points_segment_columns_dev")
U = {4: np.uint32, 8: np.uint64}


@functools.lru_cache(maxsize=None)
def case():
    c = R.base_case()
    st = R.segments_state(c["x"], c["y"], c["z"], c["intensity"], c["inv"], c["labels"], 1, N, NZ, R.DZ)
    zk, count = R.rasters_state(c["x"], c["y"], c["z"], c["inv"], R.H, R.W)
    chm, density = R.rasters_finish(zk, count, 0.25)
    col = R.columns(st, R.DZ, 1.0, 1.0, np.float64, pad=True)
    assert all(int(v) > 0 for v in st["counters"]) and (zk == 0).any() and np.isnan(col["ch"]).any()
    return dict(c=c, st=st, zkey=zk, count=count, chm=chm, density=density, col=col)


def dev_off(a, k):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "u":                                                  # the bits, in the signed type of the same width
        a = a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])
    return offset_view(torch.as_tensor(a).cuda(), k)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(U[a.dtype.itemsize])


def zeroed(shape, dt, poison, k):
    """a guarded STATE array: the payload all zero, everything around it poison"""
    g = guarded(shape, dt, poison, "cuda", k)
    g.t.zero_()
    torch.cuda.synchronize()
    return g


def test_every_entry_point_of_the_table_is_exercised():
    from obia_amd import _lib
    assert set(EXERCISED) == set(_lib._POINTS_SIGNATURES)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("poison", POISONS, ids=[f"{p:02X}" for p in POISONS])
def test_buffers_off_the_boundary_and_guarded_outputs(k, poison):
    """4-byte buffers 4, 8 and 12 bytes past a 16-byte boundary, 8-byte ones 8 bytes (k odd), the intensity 2, 4 and 6 bytes"""
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.default_context(0)
    r = case()
    c, st = r["c"], r["st"]
    n = len(c["x"])
    x, y, z, inten, labels = dev_off(c["x"], k), dev_off(c["y"], k), dev_off(c["z"], k), dev_off(c["intensity"], k), dev_off(c["labels"], k)
    zk_in, count_in = dev_off(r["zkey"], k), dev_off(r["count"], k)
    s_in = {name: dev_off(st[name], k) for name in ("profile", "top", "n_int", "s1", "s2")}
    assert residue(z) == 4 * k and residue(inten) == 2 * k and residue(x) == (8 * k) % 16 and residue(labels) == 4 * k
    ins = [x, y, z, inten, labels, zk_in, count_in] + list(s_in.values())
    snaps = [snapshot(t) for t in ins]
    inv = (ctypes.c_double * 6)(*c["inv"])
    X, Y, Z, I, L = x.data_ptr(), y.data_ptr(), z.data_ptr(), inten.data_ptr(), labels.data_ptr()
    runs = []
    for _ in range(2):
        s = {name: zeroed(shape, dt, poison, k) for name, shape, dt in (
            ("zkey", (R.H, R.W), np.int32), ("count", (R.H, R.W), np.int32), ("profile", (N, NZ), np.int32), ("top", (N,), np.int32),
            ("n_int", (N,), np.int32), ("s1", (N,), np.int64), ("s2", (N,), np.int64), ("counters", (4,), np.int64))}
        o = {name: guarded(shape, dt, poison, "cuda", k) for name, shape, dt in (
            ("chm", (R.H, R.W), np.float32), ("density", (R.H, R.W), np.float32), ("n_points", (N,), np.int64), ("ch", (N,), np.float64),
            ("pai", (N,), np.float64), ("fhd", (N,), np.float64), ("mean_intensity", (N,), np.float64),
            ("variance_intensity", (N,), np.float64), ("pad", (N, NZ), np.float64))}
        assert s["profile"].ptr % 16 == 4 * k and s["s1"].ptr % 16 == (8 * k) % 16 and o["chm"].ptr % 16 == 4 * k
        cut = 4099                                                           # the state is added to: two calls make the cloud
        calls = [lib.obia_points_rasters_dev(ctx.handle, X, Y, Z, cut, inv, R.H, R.W, s["zkey"].ptr, s["count"].ptr),
                 lib.obia_points_rasters_dev(ctx.handle, X + 8 * cut, Y + 8 * cut, Z + 4 * cut, n - cut, inv, R.H, R.W, s["zkey"].ptr, s["count"].ptr),
                 lib.obia_points_rasters_finish_dev(ctx.handle, zk_in.data_ptr(), count_in.data_ptr(), R.H, R.W, 0.25, o["chm"].ptr, o["density"].ptr),
                 lib.obia_points_segments_dev(ctx.handle, X, Y, Z, I, cut, inv, L, R.H, R.W, 1, N, NZ, R.DZ, s["profile"].ptr, s["top"].ptr,
                                              s["n_int"].ptr, s["s1"].ptr, s["s2"].ptr, s["counters"].ptr),
                 lib.obia_points_segments_dev(ctx.handle, X + 8 * cut, Y + 8 * cut, Z + 4 * cut, I + 2 * cut, n - cut, inv, L, R.H, R.W, 1, N, NZ,
                                              R.DZ, s["profile"].ptr, s["top"].ptr, s["n_int"].ptr, s["s1"].ptr, s["s2"].ptr, s["counters"].ptr),
                 lib.obia_points_segment_columns_dev(ctx.handle, *(s_in[name].data_ptr() for name in ("profile", "top", "n_int", "s1", "s2")), N,
                                                     NZ, R.DZ, 1.0, 1.0, *(o[name].ptr for name in R.COLUMNS), o["pad"].ptr)]
        assert calls == [0] * len(calls), (calls, _lib.last_error())
        want = dict(st, zkey=r["zkey"], count=r["count"])
        for name, g in s.items():
            assert np.array_equal(bits(g.host()), bits(want[name])), name
            assert g.stray().size == 0, name
        for name, w in (("chm", r["chm"]), ("density", r["density"]), ("n_points", r["col"]["n_points"]), ("ch", r["col"]["ch"]),
                        ("mean_intensity", r["col"]["mean_intensity"])):
            assert np.array_equal(bits(o[name].host()), bits(w)), name
        for name, g in o.items():
            assert g.findings(name=name) == []                               # (no expected value is all poison bytes: none is judged exempt)
            if name in ("pai", "fhd", "variance_intensity", "pad"):          # their values: tests/test_gpu_pointcloud.py
                assert np.array_equal(np.isnan(g.host()), np.isnan(r["col"][name])), name
        runs.append({name: g.host().tobytes() for name, g in list(s.items()) + list(o.items())})
    assert runs[0] == runs[1]
    assert all(unchanged(t, sn) for t, sn in zip(ins, snaps))

    # refused: nothing is written
    g = {name: guarded((N * NZ,), dt, poison, "cuda", k) for name, dt in (("a", np.int32), ("b", np.int32), ("c", np.int32), ("f", np.float32),
                                                                          ("e", np.float32), ("p", np.int64), ("q", np.int64), ("w", np.int64),
                                                                          ("d", np.float64), ("d2", np.float64), ("d3", np.float64),
                                                                          ("d4", np.float64), ("d5", np.float64), ("d6", np.float64))}
    a, b, c3, f, e, p, q, w, d, d2, d3, d4, d5, d6 = (g[name].ptr for name in ("a", "b", "c", "f", "e", "p", "q", "w", "d", "d2", "d3", "d4", "d5", "d6"))
    P, T, NI, S1, S2 = (s_in[name].data_ptr() for name in ("profile", "top", "n_int", "s1", "s2"))
    ZK, CN = zk_in.data_ptr(), count_in.data_ptr()
    h = ctx.handle
    nan = float("nan")

    def seg(x_=X, z_=Z, i_=I, n_=n, l_=L, H_=R.H, N_=N, nz_=NZ, dz_=R.DZ, pr=a, tp=b, ni=c3, s1=p, s2=q, cn=w):
        return lib.obia_points_segments_dev(h, x_, Y, z_, i_, n_, inv, l_, H_, R.W, 1, N_, nz_, dz_, pr, tp, ni, s1, s2, cn)

    def col(pr=P, N_=N, nz_=NZ, dz_=R.DZ, mh=1.0, k_=1.0, npo=p, ch=d, pad=d6):
        return lib.obia_points_segment_columns_dev(h, pr, T, NI, S1, S2, N_, nz_, dz_, mh, k_, npo, ch, d2, d3, d4, d5, pad)

    invalid = [lib.obia_points_rasters_dev(h, X, Y, Z, -1, inv, R.H, R.W, a, b), lib.obia_points_rasters_dev(h, None, Y, Z, n, inv, R.H, R.W, a, b),
               lib.obia_points_rasters_dev(h, X + 4, Y, Z, n, inv, R.H, R.W, a, b), lib.obia_points_rasters_dev(h, X, Y, Z + 2, n, inv, R.H, R.W, a, b),
               lib.obia_points_rasters_dev(h, X, Y, Z, n, None, R.H, R.W, a, b), lib.obia_points_rasters_dev(h, X, Y, Z, n, inv, 0, R.W, a, b),
               lib.obia_points_rasters_dev(h, X, Y, Z, n, inv, R.H, R.W, a, a), lib.obia_points_rasters_dev(h, X, Y, Z, n, inv, R.H, R.W, a + 2, b),
               lib.obia_points_rasters_dev(h, X, Y, Z, n, inv, R.H, R.W, None, b),
               lib.obia_points_rasters_finish_dev(h, ZK, CN, R.H, R.W, 0.0, f, e), lib.obia_points_rasters_finish_dev(h, ZK, CN, R.H, R.W, nan, f, e),
               lib.obia_points_rasters_finish_dev(h, ZK, CN, R.H, R.W, -0.25, f, e), lib.obia_points_rasters_finish_dev(h, ZK, CN, R.H, 0, 0.25, f, e),
               lib.obia_points_rasters_finish_dev(h, ZK, CN, R.H, R.W, 0.25, f, f), lib.obia_points_rasters_finish_dev(h, ZK, CN, R.H, R.W, 0.25, f + 1, e),
               lib.obia_points_rasters_finish_dev(h, None, CN, R.H, R.W, 0.25, f, e), lib.obia_points_rasters_finish_dev(h, ZK, CN, R.H, R.W, 0.25, ZK, e),
               seg(n_=-1), seg(x_=X + 4), seg(z_=Z + 1), seg(i_=I + 1), seg(l_=None), seg(l_=L + 2), seg(H_=0), seg(N_=-1), seg(nz_=0), seg(dz_=0.0),
               seg(dz_=-0.3), seg(dz_=nan), seg(dz_=float("inf")), seg(pr=None), seg(tp=b + 2), seg(s1=p + 4), seg(cn=None), seg(pr=a, tp=a),
               seg(s1=p, s2=p), seg(pr=L),
               col(N_=0), col(nz_=0), col(dz_=0.0), col(dz_=nan), col(mh=nan), col(mh=float("inf")), col(k_=0.0), col(k_=-1.0), col(k_=nan),
               col(pr=None), col(pr=P + 2), col(npo=None), col(npo=p + 4), col(ch=d + 4), col(pad=d6 + 4), col(ch=d2), col(pad=d), col(npo=S1)]
    assert invalid == [_lib.E_INVALID] * len(invalid), invalid
    # ... and says so in full: a null output, an output one byte on, an output where an input starts
    refused_saying("points: rasters: bad arguments (null, misaligned or overlapping buffers)", lib.obia_points_rasters_dev,
                   (h, X, Y, Z, n, inv, R.H, R.W, a, None), (h, X, Y, Z, n, inv, R.H, R.W, a, b + 1), (h, X, Y, Z, n, inv, R.H, R.W, Z, b))
    refused_saying("points: rasters finish: bad arguments (null, misaligned or overlapping buffers)", lib.obia_points_rasters_finish_dev,
                   (h, ZK, CN, R.H, R.W, 0.25, None, e), (h, ZK, CN, R.H, R.W, 0.25, f, e + 1), (h, ZK, CN, R.H, R.W, 0.25, f, CN))
    refused_saying("points: segments: bad arguments (null, misaligned or overlapping buffers)", seg,
                   dict(s2=None), dict(ni=c3 + 1), dict(cn=w + 1), dict(tp=L), dict(s1=X))
    refused_saying("points: segment columns: bad arguments (null, misaligned or overlapping buffers)", col,
                   dict(ch=None), dict(npo=p + 1), dict(pad=d6 + 1), dict(ch=S2), dict(pad=P))
    unsupported = [lib.obia_points_rasters_dev(h, X, Y, Z, 2 ** 31, inv, R.H, R.W, a, b), seg(n_=2 ** 31), seg(nz_=4097), seg(N_=2 ** 20, nz_=2048),
                   seg(N_=2 ** 31 - 1, nz_=2), col(nz_=4097), col(N_=2 ** 20, nz_=2048)]
    assert unsupported == [_lib.E_UNSUPPORTED] * len(unsupported), unsupported
    assert all(v.untouched() for v in g.values())
    assert all(unchanged(t, sn) for t, sn in zip(ins, snaps))


def test_an_empty_cloud_writes_nothing():
    """n = 0 is a valid call that does nothing: the state keeps whatever it held, and the cloud's pointers may be null"""
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.default_context(0)
    inv = (ctypes.c_double * 6)(*R.invert_affine(R.AFFINE))
    labels = torch.ones((4, 4), dtype=torch.int32).cuda()
    g = {name: guarded((8,), dt, 0xA5, "cuda", 1) for name, dt in (("a", np.int32), ("b", np.int32), ("c", np.int32), ("p", np.int64), ("q", np.int64),
                                                                   ("w", np.int64))}
    torch.cuda.synchronize()
    rc = [lib.obia_points_rasters_dev(ctx.handle, None, None, None, 0, inv, 4, 4, g["a"].ptr, g["b"].ptr),
          lib.obia_points_segments_dev(ctx.handle, None, None, None, None, 0, inv, labels.data_ptr(), 4, 4, 1, 1, 8, 0.5, g["a"].ptr, g["b"].ptr,
                                       g["c"].ptr, g["p"].ptr, g["q"].ptr, g["w"].ptr)]
    assert rc == [0, 0], (rc, _lib.last_error())
    assert all(v.untouched() and v.stray().size == 0 for v in g.values())
