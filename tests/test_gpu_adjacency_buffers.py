"""The entry points of include/obia_adjacency.h through guarded outputs (tests/guarded.py, both poisons) with every input off a 16-byte
boundary (tests/offset_views.py): the results bit for bit, no stray write, no element of an output left unwritten (the write pass's
work words are scratch and exempt), the inputs unchanged, two runs equal; what is refused writes nothing; and every entry point on a
context whose workspace was filled by obia_test_poison_workspace_dev equals the same call on a fresh context -- the case
"body:adjacency" of the decision table of tests/workspace_history.py runs run_all / judge_all too.  Every entry point of the table is
exercised here."""
import ctypes
import functools

import numpy as np
import pytest

from tests import adjacency_restatement as R
from tests.guarded import POISONS, guarded, snapshot, unchanged
from tests.offset_views import offset_view, residue
from tests.refusal_text import refused_saying

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EXERCISED = ("obia_adj_tile_count_dev", "obia_adj_tile_write_dev", "obia_adj_edge_d2_dev", "obia_adj_neighbor_stats_dev",
             "obia_adj_class_border_dev", "obia_adj_best_neighbor_dev", "obia_adj_components_dev", "obia_adj_relabel_dev")
F64, U8, I32, I64 = np.float64, np.uint8, np.int32, np.int64
TH, TW = 16, 32
H, W, START, N, F, K = 2 * TH + 3, 2 * TW + 5, 1, 12, 3, 4
INPUTS = ("labels", "offset", "indptr", "neighbor", "border", "values", "classes", "dist", "link", "table")


@functools.lru_cache(maxsize=None)
def case():
    rs = np.random.RandomState(23)
    labels = np.kron(rs.randint(-1, N + 2, (-(-H // 3), -(-W // 4))), np.ones((3, 4), int))[:H, :W].astype(I32)
    tiles = R.tile_records(labels, START, N, TH, TW)
    count = np.array([len(k) for k, _ in tiles], I32)
    offset = (np.cumsum(count) - count).astype(I64)
    key, edges = np.concatenate([k for k, _ in tiles]), np.concatenate([e for _, e in tiles])
    indptr, neighbor, border = R.graph(labels, START, N)
    values = rs.choice([1e16, 1.0, -1e16, 0.25, -0.0, np.nan], (N, F), p=[.2, .2, .2, .2, .1, .1])
    classes = rs.randint(-1, K + 1, N).astype(I32)
    dist = R.d2(indptr, neighbor, N, values)
    stats = R.neighbor_stats(indptr, neighbor, border, N, values)
    best, best_d2 = R.best_neighbor(indptr, neighbor, N, dist)
    link = ((rs.uniform(size=len(neighbor)) < 0.04) * 201).astype(U8)
    root = R.components(indptr, neighbor, N, link)
    table = R.compact_roots(root, 7)
    assert len(neighbor) > 40 and np.isnan(dist).any() and (root != np.arange(N)).any() and count.min() > 0
    return dict(labels=labels, offset=offset, indptr=indptr, neighbor=neighbor, border=border, values=values, classes=classes, dist=dist,
                link=link, table=table, count=count, key=key, edges=edges, d2=dist, mean=stats["mean"], min=stats["min"], max=stats["max"],
                used=stats["used"], cls=R.class_border(indptr, neighbor, border, N, classes, K), best=best, best_d2=best_d2, root=root,
                relabelled=R.relabel(labels, table, START))


def dev_off(a, k):
    t = offset_view(torch.as_tensor(np.ascontiguousarray(a)).cuda(), k)
    torch.cuda.synchronize()
    return t


def run_all(ctx, k, poison):
    """every entry point once on guarded outputs, every input k elements off a boundary; returns (outputs, scratch, inputs)"""
    from obia_amd import _lib
    lib = _lib.load()
    r = case()
    nnz, total, nt = len(r["neighbor"]), int(r["count"].sum()), len(r["count"])
    ins = {name: dev_off(r[name], k) for name in INPUTS}
    p = {name: t.data_ptr() for name, t in ins.items()}
    o = {name: guarded(shape, dt, poison, "cuda", k) for name, shape, dt in (
        ("count", (nt,), I32), ("key", (total,), I64), ("edges", (total,), I32), ("d2", (nnz,), F64), ("mean", (N, F), F64), ("min", (N, F), F64),
        ("max", (N, F), F64), ("used", (N, F), I32), ("cls", (N, K), I64), ("best", (N,), I32), ("best_d2", (N,), F64), ("root", (N,), I32),
        ("relabelled", (H, W), I32))}
    scratch = {"work": guarded((_lib.ADJ_WORK,), I32, poison, "cuda", k)}
    h = ctx.handle
    calls = [lib.obia_adj_tile_count_dev(h, p["labels"], H, W, START, N, o["count"].ptr),
             lib.obia_adj_tile_write_dev(h, p["labels"], H, W, START, N, p["offset"], total, o["key"].ptr, o["edges"].ptr, scratch["work"].ptr),
             lib.obia_adj_edge_d2_dev(h, p["indptr"], p["neighbor"], N, nnz, p["values"], F, o["d2"].ptr),
             lib.obia_adj_neighbor_stats_dev(h, p["indptr"], p["neighbor"], p["border"], N, nnz, p["values"], F, o["mean"].ptr, o["min"].ptr,
                                             o["max"].ptr, o["used"].ptr),
             lib.obia_adj_class_border_dev(h, p["indptr"], p["neighbor"], p["border"], N, nnz, p["classes"], K, o["cls"].ptr),
             lib.obia_adj_best_neighbor_dev(h, p["indptr"], p["neighbor"], N, nnz, p["dist"], o["best"].ptr, o["best_d2"].ptr),
             lib.obia_adj_components_dev(h, p["indptr"], p["neighbor"], N, nnz, p["link"], o["root"].ptr),
             lib.obia_adj_relabel_dev(h, p["labels"], H * W, START, N, p["table"], o["relabelled"].ptr)]
    assert calls == [0] * len(calls), (calls, _lib.last_error())
    torch.cuda.synchronize()
    return o, scratch, ins


def sorted_inside_tiles(key, edges, count):
    """the records with every tile's rows in ascending key order: inside a tile the order is not specified"""
    key, edges = key.copy(), edges.copy()
    at = 0
    for n in count.tolist():
        order = np.argsort(key[at:at + n], kind="stable")
        key[at:at + n], edges[at:at + n] = key[at:at + n][order], edges[at:at + n][order]
        at += n
    return key, edges


def judge_all(o, scratch):
    r = case()
    got = {name: g.host() for name, g in o.items()}
    got["key"], got["edges"] = sorted_inside_tiles(got["key"], got["edges"], r["count"])
    for name, g in o.items():
        assert R.same_bits(got[name], r[name]), name
        assert g.findings(name=name) == []                                   # no stray write, every element written
    for name, g in scratch.items():
        assert g.stray().size == 0, name                                     # what the work words hold is not specified; around them: nothing
    return got


def test_every_entry_point_of_the_table_is_exercised():
    from obia_amd import _lib
    assert set(EXERCISED) == set(_lib._ADJACENCY_BINDINGS)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("poison", POISONS, ids=[f"{p:02X}" for p in POISONS])
def test_buffers_off_the_boundary_and_guarded_outputs(k, poison):
    """4-byte buffers 4, 8 and 12 bytes past a 16-byte boundary, 8-byte ones 8 bytes (k odd), the link bytes 1, 2 and 3 bytes"""
    from obia_amd import _lib
    ctx = _lib.default_context(0)
    runs = []
    for _ in range(2):
        o, scratch, ins = run_all(ctx, k, poison)
        assert residue(ins["labels"]) == 4 * k and residue(ins["indptr"]) == (8 * k) % 16 and residue(ins["link"]) == k
        assert o["root"].ptr % 16 == 4 * k and o["d2"].ptr % 16 == (8 * k) % 16
        snaps = {name: snapshot(t) for name, t in ins.items()}
        got = judge_all(o, scratch)
        r = case()
        assert all(unchanged(ins[name], snaps[name]) for name in ins) and np.array_equal(ins["labels"].cpu().numpy(), r["labels"])
        runs.append({name: a.tobytes() for name, a in got.items()})
    assert runs[0] == runs[1]


@pytest.mark.parametrize("poison", POISONS, ids=[f"{p:02X}" for p in POISONS])
def test_refusals_write_nothing(poison):
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.default_context(0)
    r = case()
    k, nnz, total = 1, len(r["neighbor"]), int(r["count"].sum())
    ins = {name: dev_off(r[name], k) for name in INPUTS}
    snaps = {name: snapshot(t) for name, t in ins.items()}
    L, OFF, IP, NB, BD, V, CL, D, LK, TB = (ins[name].data_ptr() for name in INPUTS)
    g = {name: guarded((H * W,), dt, poison, "cuda", k) for name, dt in (("a", I32), ("b", I32), ("w", I32), ("q", I64), ("x", F64), ("y", F64),
                                                                        ("z", F64))}
    a, b, w, q, x, y, z = (g[name].ptr for name in ("a", "b", "w", "q", "x", "y", "z"))
    h = ctx.handle

    def cnt(l_=L, H_=H, W_=W, n_=N, o_=a):
        return lib.obia_adj_tile_count_dev(h, l_, H_, W_, START, n_, o_)

    def wr(l_=L, H_=H, W_=W, n_=N, off=OFF, tot=total, k_=q, e_=a, w_=w):
        return lib.obia_adj_tile_write_dev(h, l_, H_, W_, START, n_, off, tot, k_, e_, w_)

    def d2(ip=IP, nb=NB, n_=N, nz=nnz, v_=V, F_=F, o_=x):
        return lib.obia_adj_edge_d2_dev(h, ip, nb, n_, nz, v_, F_, o_)

    def st(ip=IP, nb=NB, bd=BD, n_=N, nz=nnz, v_=V, F_=F, m_=x, lo=y, hi=z, u_=a):
        return lib.obia_adj_neighbor_stats_dev(h, ip, nb, bd, n_, nz, v_, F_, m_, lo, hi, u_)

    def cb(ip=IP, nb=NB, bd=BD, n_=N, nz=nnz, c_=CL, K_=K, o_=q):
        return lib.obia_adj_class_border_dev(h, ip, nb, bd, n_, nz, c_, K_, o_)

    def bn(ip=IP, nb=NB, n_=N, nz=nnz, d_=D, b_=a, bd_=x):
        return lib.obia_adj_best_neighbor_dev(h, ip, nb, n_, nz, d_, b_, bd_)

    def co(ip=IP, nb=NB, n_=N, nz=nnz, l_=LK, r_=a):
        return lib.obia_adj_components_dev(h, ip, nb, n_, nz, l_, r_)

    def rl(l_=L, n_=H * W, s_=N, t_=TB, o_=a):
        return lib.obia_adj_relabel_dev(h, l_, n_, START, s_, t_, o_)

    invalid = [cnt(l_=None), cnt(l_=L + 2), cnt(o_=None), cnt(o_=a + 1), cnt(H_=0), cnt(W_=-3), cnt(n_=-1), cnt(n_=2 ** 31 - 2), cnt(o_=L),
               wr(l_=None), wr(off=None), wr(off=OFF + 4), wr(k_=None), wr(e_=None), wr(w_=None), wr(k_=q + 4), wr(e_=a + 2), wr(w_=w + 1),
               wr(tot=-1), wr(H_=0), wr(n_=-1), wr(e_=w), wr(k_=OFF),
               d2(ip=None), d2(nb=None), d2(v_=None), d2(o_=None), d2(ip=IP + 4), d2(nb=NB + 2), d2(v_=V + 4), d2(o_=x + 4), d2(F_=0), d2(F_=-2),
               d2(nz=-1), d2(n_=-1), d2(o_=V),
               st(ip=None), st(bd=None), st(bd=BD + 4), st(v_=None), st(m_=None), st(lo=None), st(hi=None), st(u_=None), st(m_=x + 4),
               st(u_=a + 1), st(F_=0), st(n_=-1), st(nz=-1), st(m_=x, lo=x), st(hi=V),
               cb(ip=None), cb(bd=None), cb(c_=None), cb(c_=CL + 2), cb(o_=None), cb(o_=q + 4), cb(K_=0), cb(K_=-1), cb(n_=-1), cb(o_=BD),
               bn(ip=None), bn(nb=None), bn(d_=None), bn(d_=D + 4), bn(b_=None), bn(bd_=None), bn(b_=a + 2), bn(bd_=x + 4), bn(n_=-1), bn(nz=-1),
               bn(bd_=D),
               co(ip=None), co(nb=None), co(l_=None), co(r_=None), co(r_=a + 2), co(n_=-1), co(nz=-1), co(r_=NB),
               rl(l_=None), rl(t_=None), rl(o_=None), rl(l_=L + 1), rl(t_=TB + 2), rl(o_=a + 3), rl(n_=0), rl(n_=-5), rl(s_=-1), rl(o_=L), rl(o_=TB)]
    assert invalid == [_lib.E_INVALID] * len(invalid), invalid
    # ... and says so in full: a null output, an output one byte on, an output where an input starts
    why = "adjacency: %s: bad arguments (null, misaligned or overlapping buffers)"
    assert why % "tile count" == "adjacency: tile count: bad arguments (null, misaligned or overlapping buffers)"
    refused_saying(why % "tile count", cnt, dict(o_=None), dict(o_=a + 1), dict(o_=L))
    refused_saying(why % "tile write", wr, dict(k_=None), dict(w_=None), dict(e_=a + 1), dict(k_=q + 1), dict(e_=L), dict(w_=OFF))
    refused_saying(why % "edge d2", d2, dict(o_=None), dict(o_=x + 1), dict(o_=V), dict(o_=IP))
    refused_saying(why % "neighbor stats", st, dict(m_=None), dict(u_=None), dict(lo=y + 1), dict(hi=V), dict(u_=NB), dict(m_=x, hi=x))
    refused_saying(why % "class border", cb, dict(o_=None), dict(o_=q + 1), dict(o_=BD), dict(o_=IP))
    refused_saying(why % "best neighbor", bn, dict(b_=None), dict(bd_=None), dict(b_=a + 1), dict(bd_=x + 1), dict(bd_=D), dict(b_=NB))
    refused_saying(why % "components", co, dict(r_=None), dict(r_=a + 1), dict(r_=NB))
    refused_saying(why % "relabel", rl, dict(o_=None), dict(o_=a + 1), dict(o_=L), dict(o_=TB))
    unsupported = [cnt(H_=65536, W_=32768), wr(H_=46341, W_=46341), wr(tot=2 ** 31), d2(nz=2 ** 31), st(nz=2 ** 31), cb(nz=2 ** 31), bn(nz=2 ** 31),
                   co(nz=2 ** 31), rl(n_=2 ** 31), d2(n_=2 ** 30, F_=2), st(n_=2 ** 30, F_=2), cb(n_=2 ** 30, K_=2)]
    assert unsupported == [_lib.E_UNSUPPORTED] * len(unsupported), unsupported
    assert all(v.untouched() and v.stray().size == 0 for v in g.values())
    assert all(unchanged(ins[name], snaps[name]) for name in ins)
    # tables that are not those of the count: refused after the pass, rows inside key_out and edges_out may be written, nothing else
    bad = dev_off(r["offset"] + 1, k)
    assert wr(off=bad.data_ptr()) == _lib.E_INVALID and "not those of the count" in _lib.last_error()
    torch.cuda.synchronize()
    assert all(v.stray().size == 0 for v in g.values()) and all(g[name].untouched() for name in ("b", "x", "y", "z"))
    # calls that have nothing to do are valid and write nothing: no entries, no rows
    rc = [lib.obia_adj_edge_d2_dev(h, IP, None, N, 0, V, F, None), lib.obia_adj_edge_d2_dev(h, None, None, 0, 0, None, F, None),
          lib.obia_adj_neighbor_stats_dev(h, None, None, None, 0, 0, None, F, None, None, None, None),
          lib.obia_adj_class_border_dev(h, None, None, None, 0, 0, None, K, None), lib.obia_adj_best_neighbor_dev(h, None, None, 0, 0, None, None, None),
          lib.obia_adj_components_dev(h, None, None, 0, 0, None, None)]
    assert rc == [0] * len(rc), (rc, _lib.last_error())
    assert all(v.stray().size == 0 for v in g.values()) and all(g[name].untouched() for name in ("b", "x", "y", "z"))


@pytest.mark.parametrize("byte", [0x01, 0xFF])
def test_a_used_context_gives_what_a_fresh_one_gives(byte):
    """each entry point on a fresh context against the same call on a context whose workspace, one block of 64 MiB, holds `byte` in
    every byte: equal bit for bit, twice (the second run sees the first's leftovers), and the context holds what it held -- these
    entry points take nothing from the workspace"""
    from obia_amd import _lib
    lib = _lib.load()
    fresh, used = _lib.Context(0), _lib.Context(0)
    try:
        o, scratch, _ = run_all(fresh, 1, POISONS[0])
        want = {name: a.tobytes() for name, a in judge_all(o, scratch).items()}
        held, nz = ctypes.c_int64(-1), ctypes.c_int64(-1)
        torch.cuda.synchronize()
        _lib.check(lib.obia_test_poison_workspace_dev(used.handle, 64 << 20, byte, ctypes.byref(held), ctypes.byref(nz)))
        assert held.value >= 64 << 20 and used.workspace_bytes() == held.value
        for _ in range(2):
            o, scratch, _ = run_all(used, 1, POISONS[0])
            assert {name: a.tobytes() for name, a in judge_all(o, scratch).items()} == want
            assert used.workspace_bytes() == held.value
    finally:
        fresh.close()
        used.close()
