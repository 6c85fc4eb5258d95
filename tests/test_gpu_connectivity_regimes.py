"""Every regime of the connectivity stage by name (tests/cc_regimes.py): each case is bit-exact against the oracle AND the library's
record of the call (obia_test_cc_report) says the call took the branches the case was built for -- code[] or not, walks or pixel
lists, the side the settle rounds started on, the restart from above, more than 64 rounds, the size cut.  A closing test asserts that
the reports together cover every combination that exists.  Batches of several problems go through the stage-level batch entry
(obia_test_enforce_connectivity_batch_dev) between poisoned guards, against the oracle run per problem.

Round counts measured on an MI355X are in DESIGN.md 3.3; the assertions are the regimes' own conditions, not those counts."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests import cc_regimes as R                                             # noqa: E402
from tests.guarded import POISONS, guarded, snapshot, unchanged            # noqa: E402

RUNS = [(name, sl, wl) for name in R.CASES for sl, wl in R.runs(name)]
COUNTS = ("problems", "pixels", "surviving", "small", "small_px", "cut", "code", "evaluation", "side")


@functools.lru_cache(maxsize=None)
def run_case(name, start_label, worklist):
    """the stage on one case: (labels, count, report); OBIA_CC_WORKLIST set around the call when `worklist`"""
    from obia_amd.segmentation import enforce_connectivity
    lab, mn, mx = R.CASES[name].make()
    t = torch.as_tensor((lab - 1 + start_label).astype(np.int32)).cuda()
    old = os.environ.pop("OBIA_CC_WORKLIST", None)
    try:
        if worklist:
            os.environ["OBIA_CC_WORKLIST"] = "1"
        out, n = enforce_connectivity(t, mn, mx, start_label=start_label)
        rep = R.cc_report()
    finally:
        os.environ.pop("OBIA_CC_WORKLIST", None)
        if old is not None:
            os.environ["OBIA_CC_WORKLIST"] = old
    return out.cpu().numpy(), n, rep


@pytest.mark.parametrize("name,start_label,worklist", RUNS, ids=[f"{n}-sl{s}{'-worklist' if w else ''}" for n, s, w in RUNS])
def test_case_equals_the_oracle_and_reports_its_regime(oracle, name, start_label, worklist):
    case = R.CASES[name]
    lab, mn, mx = case.make()
    lab = lab - 1 + start_label
    ref = oracle.enforce_connectivity(lab, mn, mx, start_label=start_label)
    out, n, rep = run_case(name, start_label, worklist)
    print(name, start_label, worklist, rep)
    assert np.array_equal(out, ref), f"{(out != ref).sum()} px differ"
    want = R.predict(lab, mn, mx, start_label=start_label, worklist=worklist, oracle=oracle)
    assert n == want["surviving"]
    if start_label == 1:
        assert n == len(np.unique(ref[ref > 0]))
    assert {k: rep[k] for k in COUNTS} == {k: want[k] for k in COUNTS}
    if name != "none_small":
        assert (rep["code"], rep["side"], rep["cut"] > 0) == (case.code, case.side, case.cut)
    if start_label == 1:
        assert case.rounds(rep), f"{name}: {case.why}: {rep}"
    else:
        assert rep["evaluation"] == (R.NONE if name == "none_small" else R.WALKS)


def sequence(rep):
    if rep["side"] == R.ABOVE:
        return "above at once" if rep["rounds_below"] == 0 and rep["rounds_above"] >= 1 else "?"
    return "below and stayed" if rep["rounds_above"] == 0 else "below then above"


def test_the_reports_cover_every_regime():
    """{code[]} x {walks, lists} x {started below and stayed, below then above, above at once} x {cut, no cut}, as the DEVICE reports
    them.  Left out, because they cannot exist: the pixel lists without code[] (`dense = use_code && ...`: six combinations)."""
    seen = {}
    for name, sl, wl in RUNS:
        rep = run_case(name, sl, wl)[2]
        if rep["evaluation"] != R.NONE:
            seen.setdefault((rep["code"], rep["evaluation"], sequence(rep), rep["cut"] > 0), []).append((name, sl, wl))
    want = {(code, ev, seq, cut) for code in (0, 1) for ev in (R.WALKS, R.LISTS)
            for seq in ("below and stayed", "below then above", "above at once") for cut in (False, True)
            if not (ev == R.LISTS and code == 0)}
    assert len(want) == 18
    assert set(seen) == want, f"missing {sorted(want - set(seen))}, unexpected {sorted(set(seen) - want)}"


def test_the_ring_is_refilled():
    """`strips` and `strips_sparse` run more than 64 rounds in one call, on the lists and on both walks"""
    for name, sl, wl in (("strips", 1, False), ("strips", 1, True), ("strips_sparse", 1, False)):
        rep = run_case(name, sl, wl)[2]
        assert rep["rounds_below"] + rep["rounds_above"] > R.RING, (name, wl, rep)


# ---- batches -------------------------------------------------------------------------------------------------------------------
def run_batch(oracle, maps, probs, start_label, poison):
    maps = [np.asarray(m, np.int64) - 1 + start_label for m in maps]
    flat = torch.as_tensor(np.concatenate([m.ravel() for m in maps]).astype(np.int32)).cuda()
    snap = snapshot(flat)
    rows = [(m.shape[0], m.shape[1], mn, mx) for m, (mn, mx) in zip(maps, probs)]
    g = guarded((flat.numel(),), torch.int32, poison, "cuda", k=1)
    n = R.enforce_connectivity_batch(flat, rows, start_label, g.t)
    rep = R.cc_report()
    refs, n_ref = R.batch_reference(oracle, maps, probs, start_label)
    ref = np.concatenate([r.ravel() for r in refs])
    out = g.host()
    assert g.findings(name="labels_out") == [] and unchanged(flat, snap)
    bad = np.flatnonzero(out != ref)
    assert len(bad) == 0, f"{len(bad)} px differ, first at flat index {bad[:5].tolist()}: {out[bad[:5]].tolist()} != {ref[bad[:5]].tolist()}"
    assert n == n_ref
    want = R.predict_batch(maps, probs, start_label, oracle=oracle)
    assert {k: rep[k] for k in COUNTS} == {k: want[k] for k in COUNTS}
    return rep


@pytest.mark.parametrize("name", list(R.BATCHES))
def test_batch_equals_the_oracle_per_problem(oracle, name):
    """surviving components are numbered from start_label over the whole batch, in problem order and then raster order of the first
    pixel; problems do not see each other; an unresolved small component is 0"""
    maps, probs = R.BATCHES[name]()
    rep = run_batch(oracle, maps, probs, 1, POISONS[0])
    assert rep["problems"] == len(maps) > 1


def test_batch_with_start_label_0(oracle):
    """The rule for start_label 0: masked pixels are -1, surviving components are numbered from 0 over the whole batch -- and a small
    component that finds no labelled neighbour is the LITERAL 0 in every problem, which then counts as labelled from its first pixel
    (its small neighbours take 0 from it): in a problem after the first that is NOT the number of one of its own components.  The
    twin bars of `mixed`'s third problem are such components: 0 although the problem's survivors start at 29."""
    maps, probs = R.batch_mixed()
    rep = run_batch(oracle, maps, probs, 0, POISONS[1])
    assert rep["evaluation"] == R.WALKS
    refs, _ = R.batch_reference(oracle, [m - 1 for m in maps], probs, 0)
    assert (refs[2][1:25][maps[2][1:25] > 0] == 0).all() and refs[2].max() > refs[1].max() > refs[0].max() == 0
    maps, probs = R.batch_all_small_between()
    run_batch(oracle, maps, probs, 0, POISONS[0])


def test_batch_entry_refuses_before_any_device_work():
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.default_context(0)
    lab = torch.ones(16, dtype=torch.int32, device="cuda")
    g = guarded((16,), torch.int32, POISONS[0], "cuda")
    def call(rows, start_label=1, lab_ptr=lab.data_ptr(), out_ptr=g.t.data_ptr()):
        pr = np.ascontiguousarray(rows, np.int64).reshape(-1, 4)
        return lib.obia_test_enforce_connectivity_batch_dev(ctx.handle, lab_ptr, pr.ctypes.data, len(pr), start_label, out_ptr, None)
    assert call([(1, 1, 1, 1)] * 65536) == _lib.E_INVALID and "65535" in _lib.last_error()
    assert call([(32768, 32768, 1, 1), (32768, 32768, 1, 1)]) == _lib.E_INVALID and "2^31" in _lib.last_error()
    assert call([(46341, 46341, 1, 1)]) == _lib.E_INVALID and "2^31" in _lib.last_error()
    assert call([(4, 4, 1, 1), (0, 4, 1, 1)]) == _lib.E_INVALID
    assert call([(4, 4, 1, 1)], start_label=2) == _lib.E_INVALID
    assert call([(4, 4, 1, 1)], lab_ptr=None) == _lib.E_INVALID and call([(4, 4, 1, 1)], out_ptr=None) == _lib.E_INVALID
    assert lib.obia_test_enforce_connectivity_batch_dev(ctx.handle, lab.data_ptr(), None, 1, 1, g.t.data_ptr(), None) == _lib.E_INVALID
    buf = np.zeros(len(R.REPORT_FIELDS), np.int64)
    assert lib.obia_test_cc_report(ctx.handle, buf.ctypes.data, len(buf) - 1) == _lib.E_INVALID
    assert lib.obia_test_cc_report(ctx.handle, None, len(buf)) == _lib.E_INVALID
    assert g.untouched() and len(g.stray()) == 0
    assert call([(4, 4, 1, 100)]) == _lib.OBIA_OK and (g.host() == 1).all()


# ---- the visited map across calls ------------------------------------------------------------------------------------------------
def test_context_history_of_the_visited_map(oracle):
    """One context of its own: `strips_sparse`, then a larger map of the walk regime, then `strips_sparse` again.  The map of the
    component walks is allocated by the first call, grown by the second and reused by the third (n + n / 8 of the larger map); the
    third call's labels equal the first's and the oracle's."""
    from obia_amd import _lib
    from obia_amd.segmentation import enforce_connectivity
    ctx = _lib.Context(0)
    try:
        lab, mn, mx = R.CASES["strips_sparse"].make()
        big = np.concatenate([lab, np.full((100, lab.shape[1]), 4, np.int64)])
        assert big.size > lab.size + lab.size // 8 and R.predict(big, mn, big.size + 1)["code"] == 0
        outs, reps = [], []
        for m in (lab, big, lab):
            out, n = enforce_connectivity(torch.as_tensor(m.astype(np.int32)).cuda(), mn, m.size + 1, start_label=1, ctx=ctx)
            reps.append(R.cc_report(ctx))
            outs.append(out.cpu().numpy())
            assert n == 2 and np.array_equal(outs[-1], oracle.enforce_connectivity(m, mn, m.size + 1)), m.shape
        assert [r["visited_realloc"] for r in reps] == [1, 1, 0]
        assert [r["evaluation"] for r in reps] == [R.WALKS] * 3 and [r["code"] for r in reps] == [0] * 3
        assert np.array_equal(outs[0], outs[2]) and {k: reps[0][k] for k in COUNTS} == {k: reps[2][k] for k in COUNTS}
    finally:
        ctx.close()
