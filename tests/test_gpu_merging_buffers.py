"""The entry points of include/obia_merging.h through guarded outputs (tests/guarded.py, both poisons) with every buffer off a 16-byte
boundary (tests/offset_views.py): the results bit for bit against tests/merging_restatement.py, no stray write, no element left
unwritten, the inputs unchanged, two runs equal; what is refused writes nothing and leaves the context as it was.  Every entry point
of the table is exercised here.  (The calls on a poisoned workspace are the case `body:merging` of tests/test_gpu_workspace_history.py,
which runs run_all and judge_all below; the wrappers' stream order is the case `merge:cost_and_pairs` of tests/test_gpu_stream_order.py.)"""
import functools

import numpy as np
import pytest

from tests import adjacency_restatement as R
from tests import merging_restatement as M
from tests.guarded import POISONS, guarded, snapshot, unchanged
from tests.offset_views import offset_view
from tests.refusal_text import refused_saying

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

EXERCISED = ("obia_merge_cost_dev", "obia_merge_pairs_dev", "obia_merge_contract_rows_dev", "obia_merge_contract_count_dev",
             "obia_merge_contract_write_dev")
F64, I32, I64 = np.float64, np.int32, np.int64
TH, TW = 16, 32
H, W, START, N, F = 2 * TH + 3, 2 * TW + 5, 1, 40, 3
SHAPE, COMPACT = 0.3, 0.4
WEIGHTS = np.array([0.5, 1.0, 2.0], F64)


@functools.lru_cache(maxsize=None)
def case():
    rs = np.random.RandomState(29)
    labels = np.kron(rs.randint(-1, N + 2, (-(-H // 3), -(-W // 4))), np.ones((3, 4), int))[:H, :W].astype(I32)
    labels[labels == 5] = 4                                                    # label 5 occurs nowhere: an empty row that must be written
    raw = (rs.uniform(0, 50, (H, W, F)) + 20.0 * (labels[:, :, None] % 7)).astype(np.float32)
    st = M.state_of(raw, labels, START, n_labels=N)
    partner = M.round_partner(st, 1e9, WEIGHTS, SHAPE, COMPACT)[0]
    root = M.pair_root(partner, N)
    assert st.area[4] == 0 and (partner >= 0).sum() >= 10 and (root != np.arange(N)).sum() >= 5
    nnz = len(st.neighbor)
    lens = np.diff(st.indptr)
    raw_count = np.zeros(N, I64)
    np.add.at(raw_count, root, lens)
    raw_ptr = np.concatenate([[0], np.cumsum(raw_count)]).astype(I64)
    cptr, cnb, cbd = M.contract(*st.graph(), N, root)
    area, mean, m2, perimeter, box = M.merge_tables(st, partner)
    want = dict(cost=M.cost(st, WEIGHTS, SHAPE, COMPACT), area=area, mean=mean, m2=m2, perimeter=perimeter, box=box, raw_count=raw_count,
                count=np.diff(cptr).astype(I32), neighbor=cnb, border=cbd)
    ins = dict(indptr=st.indptr, neighbor=st.neighbor, border=st.border, area=st.area, mean=st.mean, m2=st.m2, perimeter=st.perimeter,
               box=st.box, weights=WEIGHTS, partner=partner, root=root, raw_ptr=raw_ptr, out_ptr=cptr)
    return dict(st=st, nnz=nnz, nnz_out=len(cnb), want=want, ins=ins)


def dev_off(a, k):
    t = offset_view(torch.as_tensor(np.ascontiguousarray(a)).cuda(), k)
    torch.cuda.synchronize()
    return t


def run_all(ctx, k, poison):
    """the five entry points on guarded outputs, every buffer k elements off a boundary; returns (outputs, scratch, inputs)"""
    from obia_amd import _lib
    lib = _lib.load()
    r = case()
    nnz, nnz_out = r["nnz"], r["nnz_out"]
    d = {name: dev_off(a, k) for name, a in r["ins"].items()}
    p = {name: t.data_ptr() for name, t in d.items()}
    o = {"cost": guarded(nnz, F64, poison, "cuda", k), "area": guarded(N, I64, poison, "cuda", k), "mean": guarded((N, F), F64, poison, "cuda", k),
         "m2": guarded((N, F), F64, poison, "cuda", k), "perimeter": guarded(N, I64, poison, "cuda", k), "box": guarded((N, 4), I32, poison, "cuda", k),
         "raw_count": guarded(N, I64, poison, "cuda", k), "count": guarded(N, I32, poison, "cuda", k),
         "neighbor": guarded(nnz_out, I32, poison, "cuda", k), "border": guarded(nnz_out, I64, poison, "cuda", k)}
    w = {"key_work": guarded(nnz, I32, poison, "cuda", k), "border_work": guarded(nnz, I64, poison, "cuda", k),
         "cursor_work": guarded(N, I32, poison, "cuda", k)}
    h = ctx.handle
    calls = [
        lib.obia_merge_cost_dev(h, p["indptr"], p["neighbor"], p["border"], N, nnz, p["area"], p["mean"], p["m2"], F, p["weights"], p["perimeter"],
                                p["box"], 1.0 - SHAPE, COMPACT, o["cost"].ptr),
        lib.obia_merge_pairs_dev(h, p["indptr"], p["neighbor"], p["border"], N, nnz, p["partner"], p["area"], p["mean"], p["m2"], F, p["perimeter"],
                                 p["box"], o["area"].ptr, o["mean"].ptr, o["m2"].ptr, o["perimeter"].ptr, o["box"].ptr),
        lib.obia_merge_contract_rows_dev(h, p["indptr"], N, nnz, p["root"], o["raw_count"].ptr),
        lib.obia_merge_contract_count_dev(h, p["indptr"], p["neighbor"], p["border"], N, nnz, p["root"], p["raw_ptr"], w["key_work"].ptr,
                                          w["border_work"].ptr, w["cursor_work"].ptr, o["count"].ptr),
    ]
    torch.cuda.synchronize()
    assert R.same_bits(o["count"].host(), r["want"]["count"])                  # the write pass is handed the count's own result
    calls.append(lib.obia_merge_contract_write_dev(h, N, nnz, p["raw_ptr"], o["count"].ptr, w["key_work"].ptr, w["border_work"].ptr, p["out_ptr"],
                                                   nnz_out, o["neighbor"].ptr, o["border"].ptr))
    assert calls == [0] * 5, (calls, _lib.last_error())
    torch.cuda.synchronize()
    return o, w, d


def judge_all(o, w):
    r = case()
    got = {name: g.host() for name, g in o.items()}
    for name, g in o.items():
        assert R.same_bits(got[name], r["want"][name]), name
        assert g.findings(name=name) == []                                   # no stray write, every element written
    for name, g in w.items():
        assert g.stray().size == 0, name                                     # scratch: what it holds is not specified, where it ends is
    return got


def test_every_entry_point_of_the_table_is_exercised():
    from obia_amd import _lib
    assert set(EXERCISED) == set(_lib._MERGE_ENTRIES)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("poison", POISONS, ids=[f"{p:02X}" for p in POISONS])
def test_buffers_off_the_boundary_and_guarded_outputs(k, poison):
    """every int32 buffer 4, 8 and 12 bytes past a 16-byte boundary, every 8-byte buffer 8 bytes (k odd)"""
    from obia_amd import _lib
    ctx = _lib.default_context(0)
    runs = []
    for _ in range(2):
        o, w, d = run_all(ctx, k, poison)
        assert d["neighbor"].data_ptr() % 16 == 4 * k and d["mean"].data_ptr() % 16 == (8 * k) % 16
        assert o["box"].ptr % 16 == 4 * k and o["cost"].ptr % 16 == (8 * k) % 16 and w["key_work"].ptr % 16 == 4 * k
        snaps = {name: snapshot(t) for name, t in d.items()}
        got = judge_all(o, w)
        assert all(unchanged(d[name], snaps[name]) for name in d)
        assert all(np.array_equal(d[name].cpu().numpy(), case()["ins"][name]) or name in ("mean", "m2") for name in d)
        assert all(R.same_bits(d[name].cpu().numpy(), case()["ins"][name]) for name in ("mean", "m2"))
        runs.append({name: a.tobytes() for name, a in got.items()})
    assert runs[0] == runs[1]


@pytest.mark.parametrize("poison", POISONS, ids=[f"{p:02X}" for p in POISONS])
def test_refusals_write_nothing_and_leave_the_context_intact(poison):
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.Context(0)
    try:
        r, k = case(), 1
        nnz, nnz_out = r["nnz"], r["nnz_out"]
        d = {name: dev_off(a, k) for name, a in r["ins"].items()}
        snaps = {name: snapshot(t) for name, t in d.items()}
        p = {name: t.data_ptr() for name, t in d.items()}
        g = {"cost": guarded(nnz, F64, poison, "cuda", k), "area": guarded(N, I64, poison, "cuda", k), "mean": guarded((N, F), F64, poison, "cuda", k),
             "m2": guarded((N, F), F64, poison, "cuda", k), "perimeter": guarded(N, I64, poison, "cuda", k), "box": guarded((N, 4), I32, poison, "cuda", k),
             "raw_count": guarded(N, I64, poison, "cuda", k), "count": guarded(N, I32, poison, "cuda", k), "key": guarded(nnz, I32, poison, "cuda", k),
             "bwork": guarded(nnz, I64, poison, "cuda", k), "cursor": guarded(N, I32, poison, "cuda", k),
             "neighbor": guarded(nnz_out, I32, poison, "cuda", k), "border": guarded(nnz_out, I64, poison, "cuda", k)}
        q = {name: v.ptr for name, v in g.items()}
        held = ctx.workspace_bytes()
        h = ctx.handle

        def cost(n_=N, nnz_=nnz, F_=F, out=q["cost"], **kw):
            a = dict(p, **kw)
            return lib.obia_merge_cost_dev(h, a["indptr"], a["neighbor"], a["border"], n_, nnz_, a["area"], a["mean"], a["m2"], F_, a["weights"],
                                           a["perimeter"], a["box"], 0.7, 0.4, out)

        def pairs(n_=N, nnz_=nnz, F_=F, area=q["area"], mean=q["mean"], m2=q["m2"], perimeter=q["perimeter"], box=q["box"], **kw):
            a = dict(p, **kw)
            return lib.obia_merge_pairs_dev(h, a["indptr"], a["neighbor"], a["border"], n_, nnz_, a["partner"], a["area"], a["mean"], a["m2"], F_,
                                            a["perimeter"], a["box"], area, mean, m2, perimeter, box)

        def rows(n_=N, nnz_=nnz, out=q["raw_count"], **kw):
            a = dict(p, **kw)
            return lib.obia_merge_contract_rows_dev(h, a["indptr"], n_, nnz_, a["root"], out)

        def count(n_=N, nnz_=nnz, key=q["key"], bwork=q["bwork"], cursor=q["cursor"], out=q["count"], **kw):
            a = dict(p, **kw)
            return lib.obia_merge_contract_count_dev(h, a["indptr"], a["neighbor"], a["border"], n_, nnz_, a["root"], a["raw_ptr"], key, bwork,
                                                     cursor, out)

        def write(n_=N, nnz_=nnz, nnz_out_=nnz_out, cnt=p["root"], key=p["neighbor"], bwork=p["border"], nb=q["neighbor"], bd=q["border"], **kw):
            a = dict(p, **kw)
            return lib.obia_merge_contract_write_dev(h, n_, nnz_, a["raw_ptr"], cnt, key, bwork, a["out_ptr"], nnz_out_, nb, bd)

        invalid = [cost(indptr=None), cost(neighbor=None), cost(border=None), cost(area=None), cost(mean=None), cost(m2=None), cost(weights=None),
                   cost(perimeter=None), cost(box=None), cost(out=None), cost(out=q["cost"] + 4), cost(mean=p["mean"] + 4), cost(box=p["box"] + 2),
                   cost(out=p["mean"]), cost(n_=-1), cost(n_=2 ** 31 - 2), cost(F_=0), cost(nnz_=-1),
                   pairs(partner=None), pairs(area=None), pairs(mean=None), pairs(box=None), pairs(area=q["area"] + 4), pairs(box=q["box"] + 2),
                   pairs(partner=p["partner"] + 2), pairs(area=q["perimeter"]), pairs(mean=p["mean"]), pairs(n_=-1), pairs(F_=-2), pairs(nnz_=-1),
                   rows(indptr=None), rows(root=None), rows(out=None), rows(out=q["raw_count"] + 4), rows(out=p["indptr"]), rows(n_=-1), rows(nnz_=-1),
                   count(root=None), count(raw_ptr=None), count(key=None), count(bwork=None), count(cursor=None), count(out=None),
                   count(key=q["key"] + 2), count(bwork=q["bwork"] + 4), count(out=q["cursor"]), count(key=p["neighbor"]), count(n_=-1), count(nnz_=-1),
                   write(raw_ptr=None), write(cnt=None), write(key=None), write(bwork=None), write(out_ptr=None), write(nb=None), write(bd=None),
                   write(nb=q["neighbor"] + 2), write(bd=q["border"] + 4), write(nb=p["neighbor"]), write(n_=-1), write(nnz_=-1), write(nnz_out_=-1)]
        assert invalid == [_lib.E_INVALID] * len(invalid), invalid
        # ... and says so in full: a null output, an output one byte on, an output where an input starts
        why = "merging: %s: bad arguments (null, misaligned or overlapping buffers)"
        assert why % "cost" == "merging: cost: bad arguments (null, misaligned or overlapping buffers)"
        refused_saying(why % "cost", cost, dict(out=None), dict(out=q["cost"] + 1), dict(out=p["weights"]), dict(out=p["border"]))
        refused_saying(why % "pairs", pairs, dict(area=None), dict(box=None), dict(mean=q["mean"] + 1), dict(box=q["box"] + 1), dict(m2=p["m2"]),
                       dict(box=p["partner"]), dict(perimeter=p["indptr"]), dict(area=q["perimeter"]))
        refused_saying(why % "contract rows", rows, dict(out=None), dict(out=q["raw_count"] + 1), dict(out=p["indptr"]))
        refused_saying(why % "contract count", count, dict(out=None), dict(cursor=None), dict(key=q["key"] + 1), dict(out=q["count"] + 1),
                       dict(bwork=p["raw_ptr"]), dict(cursor=p["root"]), dict(out=q["cursor"]))
        refused_saying(why % "contract write", write, dict(nb=None), dict(bd=None), dict(nb=q["neighbor"] + 1), dict(bd=q["border"] + 1),
                       dict(nb=p["root"]), dict(bd=p["out_ptr"]))
        unsupported = [cost(nnz_=2 ** 31), cost(n_=2 ** 30, F_=2), pairs(nnz_=2 ** 31), pairs(n_=2 ** 30, F_=2), rows(nnz_=2 ** 31), count(nnz_=2 ** 31),
                       write(nnz_=2 ** 31), write(nnz_out_=2 ** 31)]
        assert unsupported == [_lib.E_UNSUPPORTED] * len(unsupported), unsupported
        torch.cuda.synchronize()
        assert all(v.untouched() and v.stray().size == 0 for v in g.values()) and all(unchanged(d[name], snaps[name]) for name in d)
        # calls that have nothing to do are valid and write nothing
        assert [cost(n_=0, nnz_=0), pairs(n_=0, nnz_=0), rows(n_=0, nnz_=0), count(n_=0, nnz_=0), write(n_=0, nnz_=0, nnz_out_=0)] == [0] * 5
        torch.cuda.synchronize()
        assert all(v.untouched() and v.stray().size == 0 for v in g.values()) and ctx.workspace_bytes() == held
        # and the context serves the next call as a fresh one would
        assert cost(out=q["cost"]) == 0
        torch.cuda.synchronize()
        want = M.cost(r["st"], WEIGHTS, 1.0 - 0.7, 0.4)
        assert R.same_bits(g["cost"].host(), want) and g["cost"].findings(name="cost") == [] and ctx.workspace_bytes() == held
    finally:
        ctx.close()
