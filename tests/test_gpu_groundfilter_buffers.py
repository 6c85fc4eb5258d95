"""The entry points of include/obia_groundfilter.h through guarded states, outputs and scratch planes (tests/guarded.py, both poisons)
with every input off a 16-byte boundary (tests/offset_views.py): the results bit for bit, no stray write, no element of an output left
unwritten (scratch planes are exempt), the inputs unchanged, two runs equal; what is refused writes nothing; and every entry point on
a context whose workspace was filled by obia_test_poison_workspace_dev equals the same call on a fresh context -- the case
"body:groundfilter" of the decision table of tests/workspace_history.py runs run_all / judge_all too.  Every entry point of the table
is exercised here."""
import ctypes
import functools

import numpy as np
import pytest

from tests import groundfilter_restatement as R
from tests import pointcloud_restatement as PR
from tests.guarded import POISONS, guarded, snapshot, unchanged
from tests.offset_views import offset_view, residue
from tests.refusal_text import refused_saying

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EXERCISED = ("obia_gf_cell_min_dev", "obia_gf_cell_min_finish_dev", "obia_morph_filter_dev", "obia_gf_threshold_dev", "obia_gf_classify_dev")
F32, F64, U8, I32, I64 = np.float32, np.float64, np.uint8, np.int32, np.int64
H, W = PR.H, PR.W                                                # the cloud's grid
PH, PW, RADIUS = 140, 1050, 5                                    # the plane of the filters: more than one tile on either axis
RADII, DH = [1, 3], [0.15, 1.0]
CUT = 4099


@functools.lru_cache(maxsize=None)
def case():
    c = PR.base_case()
    z = c["z"].astype(F64) * 2.0 - 10.0
    z[::29], z[1::31] = -0.0, 1e300
    keys = R.cell_keys(c["x"], c["y"], z, c["inv"], H, W)
    zmin = R.cell_min_finish(keys)
    rs = np.random.RandomState(17)
    plane = rs.normal(0, 10, (PH, PW)).astype(F32)
    plane[rs.uniform(size=plane.shape) < 0.3] = np.nan
    plane[50:70, 1000:1040] = np.nan
    S, T = R.threshold(plane, RADII, DH)
    thresh = np.where(np.isnan(zmin), F32(np.nan), zmin + F32(1.5)).astype(F32)
    flags, counters = R.classify(c["x"], c["y"], z, c["inv"], thresh)
    assert all(int(v) > 0 for v in counters) and np.isnan(zmin).any() and np.isnan(T).any()
    return dict(x=c["x"], y=c["y"], z=z, inv=c["inv"], keys=keys, zmin=zmin, plane=plane, erosion=R.erosion(plane, RADIUS),
                dilation=R.dilation(plane, RADIUS), surface=S, threshold=T, thresh=thresh, flags=flags, counters=counters)


def dev_off(a, k):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "u":                                                  # the bits, in the signed type of the same width
        a = a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])
    t = offset_view(torch.as_tensor(a).cuda(), k)
    torch.cuda.synchronize()
    return t


def zeroed(shape, dt, poison, k):
    g = guarded(shape, dt, poison, "cuda", k)
    g.t.zero_()
    torch.cuda.synchronize()
    return g


def run_all(ctx, k, poison):
    """every entry point once (the cell minimum twice: the state is added to) on guarded buffers k elements off a boundary; returns
    (states and outputs, scratch planes, inputs)"""
    from obia_amd import _lib
    lib = _lib.load()
    r = case()
    n = len(r["x"])
    ins = {name: dev_off(r[name], k) for name in ("x", "y", "z", "keys", "plane", "thresh")}
    X, Y, Z = (ins[name].data_ptr() for name in ("x", "y", "z"))
    inv = (ctypes.c_double * 6)(*r["inv"])
    s = {"keys": zeroed((H, W), I32, poison, k), "counters": zeroed((4,), I64, poison, k)}
    o = {name: guarded(shape, dt, poison, "cuda", k) for name, shape, dt in (
        ("zmin", (H, W), F32), ("erosion", (PH, PW), F32), ("dilation", (PH, PW), F32), ("surface", (PH, PW), F32), ("threshold", (PH, PW), F32),
        ("flags", (n,), U8))}
    scratch = {name: guarded((PH, PW), F32, poison, "cuda", k) for name in ("tmp_e", "tmp_d", "tmp0", "tmp1")}
    h = ctx.handle
    calls = [lib.obia_gf_cell_min_dev(h, X, Y, Z, CUT, inv, H, W, s["keys"].ptr),
             lib.obia_gf_cell_min_dev(h, X + 8 * CUT, Y + 8 * CUT, Z + 8 * CUT, n - CUT, inv, H, W, s["keys"].ptr),
             lib.obia_gf_cell_min_finish_dev(h, ins["keys"].data_ptr(), H, W, o["zmin"].ptr),
             lib.obia_morph_filter_dev(h, ins["plane"].data_ptr(), PH, PW, RADIUS, 0, scratch["tmp_e"].ptr, o["erosion"].ptr),
             lib.obia_morph_filter_dev(h, ins["plane"].data_ptr(), PH, PW, RADIUS, 1, scratch["tmp_d"].ptr, o["dilation"].ptr),
             lib.obia_gf_threshold_dev(h, ins["plane"].data_ptr(), PH, PW, (ctypes.c_int32 * 2)(*RADII), (ctypes.c_double * 2)(*DH), 2,
                                       scratch["tmp0"].ptr, scratch["tmp1"].ptr, o["surface"].ptr, o["threshold"].ptr),
             lib.obia_gf_classify_dev(h, X, Y, Z, n, inv, ins["thresh"].data_ptr(), H, W, o["flags"].ptr, s["counters"].ptr)]
    assert calls == [0] * len(calls), (calls, _lib.last_error())
    torch.cuda.synchronize()
    return s, o, scratch, ins


def judge_all(s, o, scratch):
    r = case()
    assert np.array_equal(s["keys"].host().view(np.uint32), r["keys"]) and s["counters"].host().view(np.uint64).tolist() == r["counters"].tolist()
    for name, g in s.items():
        assert g.stray().size == 0, name
    for name, g in o.items():
        want = r[name]
        assert R.same_bits(g.host(), want), name
        exempt = (want == g.poison) if want.dtype.itemsize == 1 else None
        assert g.findings(exempt=exempt, name=name) == []                    # no stray write, every element written
    for name, g in scratch.items():
        assert g.stray().size == 0, name                                     # what a scratch plane holds is not specified; around it: nothing


def test_every_entry_point_of_the_table_is_exercised():
    from obia_amd import _lib
    assert set(EXERCISED) == set(_lib._GROUNDFILTER_BINDINGS)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("poison", POISONS, ids=[f"{p:02X}" for p in POISONS])
def test_buffers_off_the_boundary_and_guarded_outputs(k, poison):
    """4-byte buffers 4, 8 and 12 bytes past a 16-byte boundary, 8-byte ones 8 bytes (k odd), the flags 1, 2 and 3 bytes"""
    from obia_amd import _lib
    ctx = _lib.default_context(0)
    runs = []
    for _ in range(2):
        s, o, scratch, ins = run_all(ctx, k, poison)
        assert residue(ins["plane"]) == 4 * k and residue(ins["x"]) == (8 * k) % 16 and o["flags"].ptr % 16 == k and o["zmin"].ptr % 16 == 4 * k
        snaps = {name: snapshot(t) for name, t in ins.items()}
        judge_all(s, o, scratch)
        r = case()
        assert all(unchanged(ins[name], snaps[name]) for name in ins) and R.same_bits(ins["plane"].cpu().numpy(), r["plane"])
        runs.append({name: g.host().tobytes() for name, g in list(s.items()) + list(o.items())})
    assert runs[0] == runs[1]


@pytest.mark.parametrize("poison", POISONS, ids=[f"{p:02X}" for p in POISONS])
def test_refusals_write_nothing(poison):
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.default_context(0)
    r = case()
    k, n = 1, len(r["x"])
    ins = {name: dev_off(r[name], k) for name in ("x", "y", "z", "keys", "plane", "thresh")}
    snaps = {name: snapshot(t) for name, t in ins.items()}
    X, Y, Z, KEYS, P, T = (ins[name].data_ptr() for name in ("x", "y", "z", "keys", "plane", "thresh"))
    inv = (ctypes.c_double * 6)(*r["inv"])
    g = {name: guarded((PH * PW,), dt, poison, "cuda", k) for name, dt in (("a", I32), ("f", F32), ("e", F32), ("t0", F32), ("t1", F32), ("b", U8),
                                                                           ("c", I64))}
    a, f, e, t0, t1, b, c = (g[name].ptr for name in ("a", "f", "e", "t0", "t1", "b", "c"))
    h = ctx.handle
    nan, inf = float("nan"), float("inf")
    I2, D2 = ctypes.c_int32 * 2, ctypes.c_double * 2

    def cmin(x_=X, z_=Z, n_=n, inv_=inv, H_=H, W_=W, k_=a):
        return lib.obia_gf_cell_min_dev(h, x_, Y, z_, n_, inv_, H_, W_, k_)

    def fin(k_=KEYS, H_=H, W_=W, o_=f):
        return lib.obia_gf_cell_min_finish_dev(h, k_, H_, W_, o_)

    def mf(s_=P, H_=PH, W_=PW, r_=RADIUS, op=0, t_=t0, d_=f):
        return lib.obia_morph_filter_dev(h, s_, H_, W_, r_, op, t_, d_)

    def th(s_=P, H_=PH, W_=PW, radii=(1, 3), dh=(0.15, 1.0), K=2, ta=t0, tb=t1, S=f, T_=e):
        return lib.obia_gf_threshold_dev(h, s_, H_, W_, None if radii is None else I2(*radii), None if dh is None else D2(*dh), K, ta, tb, S, T_)

    def cl(x_=X, z_=Z, n_=n, inv_=inv, t_=T, H_=H, W_=W, fl=b, cn=c):
        return lib.obia_gf_classify_dev(h, x_, Y, z_, n_, inv_, t_, H_, W_, fl, cn)

    invalid = [cmin(n_=-1), cmin(x_=None), cmin(x_=X + 4), cmin(z_=Z + 4), cmin(inv_=None), cmin(H_=0), cmin(W_=-3), cmin(k_=None), cmin(k_=a + 2),
               cmin(k_=X),
               fin(k_=None), fin(k_=KEYS + 2), fin(o_=None), fin(o_=f + 1), fin(H_=0), fin(o_=KEYS),
               mf(s_=None), mf(s_=P + 2), mf(t_=None), mf(d_=None), mf(d_=f + 2), mf(t_=t0 + 1), mf(H_=0), mf(W_=0), mf(r_=0), mf(r_=-1), mf(op=2),
               mf(op=-1), mf(t_=f), mf(d_=P), mf(t_=P),
               th(s_=None), th(radii=None), th(dh=None), th(ta=None), th(tb=None), th(S=None), th(T_=None), th(K=0), th(K=17), th(K=-1), th(H_=0),
               th(radii=(0, 3)), th(radii=(1, -2)), th(dh=(0.15, -1.0)), th(dh=(nan, 1.0)), th(dh=(0.15, inf)), th(S=f, T_=f), th(ta=t0, tb=t0),
               th(S=P), th(ta=f), th(T_=e + 2), th(s_=P + 1),
               cl(n_=-1), cl(x_=None), cl(z_=Z + 4), cl(inv_=None), cl(t_=None), cl(t_=T + 2), cl(H_=0), cl(fl=None), cl(cn=None), cl(cn=c + 4),
               cl(fl=X), cl(cn=Z)]
    assert invalid == [_lib.E_INVALID] * len(invalid), invalid
    # ... and says so in full: a null output, an output (the flags are bytes: the counters) one byte on, an output where an input starts
    why = "groundfilter: %s: bad arguments (null, misaligned or overlapping buffers)"
    assert why % "cell min" == "groundfilter: cell min: bad arguments (null, misaligned or overlapping buffers)"
    refused_saying(why % "cell min", cmin, dict(k_=None), dict(k_=a + 1), dict(k_=Z))
    refused_saying(why % "cell min finish", fin, dict(o_=None), dict(o_=f + 1), dict(o_=KEYS))
    refused_saying(why % "filter", mf, dict(d_=None), dict(t_=None), dict(d_=f + 1), dict(t_=t0 + 1), dict(d_=P), dict(t_=P), dict(t_=f))
    refused_saying(why % "threshold", th, dict(S=None), dict(T_=None), dict(S=f + 1), dict(tb=t1 + 1), dict(T_=P), dict(ta=P), dict(S=f, tb=f))
    refused_saying(why % "classify", cl, dict(fl=None), dict(cn=None), dict(cn=c + 1), dict(fl=T), dict(cn=X))
    unsupported = [cmin(n_=2 ** 31), cl(n_=2 ** 31), cmin(H_=65536, W_=32768), fin(H_=46341, W_=46341), mf(H_=65536, W_=32768), th(H_=2 ** 30, W_=2),
                   cl(H_=32768, W_=65536), mf(r_=128), mf(r_=2 ** 20), th(radii=(1, 128))]
    assert unsupported == [_lib.E_UNSUPPORTED] * len(unsupported), unsupported
    assert all(v.untouched() and v.stray().size == 0 for v in g.values())
    assert all(unchanged(ins[name], snaps[name]) for name in ins)
    # n = 0 is a valid call that does nothing, with null cloud pointers
    rc = [lib.obia_gf_cell_min_dev(h, None, None, None, 0, inv, H, W, a), lib.obia_gf_classify_dev(h, None, None, None, 0, inv, T, H, W, None, c)]
    assert rc == [0, 0] and all(v.untouched() and v.stray().size == 0 for v in g.values())


@pytest.mark.parametrize("byte", [0x01, 0xFF])
def test_a_used_context_gives_what_a_fresh_one_gives(byte):
    """each operator on a fresh context against the same call on a context whose workspace, one block of 64 MiB, holds `byte` in every
    byte: equal bit for bit, twice (the second run sees the first's leftovers), and the context holds what it held -- these entry
    points take nothing from the workspace"""
    from obia_amd import _lib
    lib = _lib.load()
    fresh, used = _lib.Context(0), _lib.Context(0)
    try:
        s, o, scratch, _ = run_all(fresh, 1, POISONS[0])
        judge_all(s, o, scratch)
        want = {name: g.host().tobytes() for name, g in list(s.items()) + list(o.items())}
        held, nz = ctypes.c_int64(-1), ctypes.c_int64(-1)
        torch.cuda.synchronize()
        _lib.check(lib.obia_test_poison_workspace_dev(used.handle, 64 << 20, byte, ctypes.byref(held), ctypes.byref(nz)))
        assert held.value >= 64 << 20 and used.workspace_bytes() == held.value
        for _ in range(2):
            s, o, scratch, _ = run_all(used, 1, POISONS[0])
            judge_all(s, o, scratch)
            assert {name: g.host().tobytes() for name, g in list(s.items()) + list(o.items())} == want
            assert used.workspace_bytes() == held.value
    finally:
        fresh.close()
        used.close()
