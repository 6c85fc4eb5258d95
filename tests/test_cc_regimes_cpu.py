"""tests/cc_regimes.py without a GPU: `predict` on hand-worked maps, every named case in the regime it was built for (a case that
drifts out of its regime fails HERE, not silently on the GPU), `batch_reference` on a hand-worked batch, the oracle's output for the
cases whose outcome is stated in their docstrings, and the report's field list against include/obia_testing.h."""
import os
import re

import numpy as np
import pytest

from tests import cc_regimes as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HAND = np.array([[1, 1, 2, 2],
                 [1, 0, 2, 3],
                 [3, 3, 0, 3]], np.int64)


def test_predict_on_a_hand_worked_map():
    """components (0 masked): label 1 {(0,0),(0,1),(1,0)}: 3 pixels; label 2 {(0,2),(0,3),(1,2)}: 3; label 3 twice, {(1,3),(2,3)} and
    {(2,0),(2,1)}: 2 pixels each.  min_size 3: 2 survive, 2 are small with 4 pixels; 2 x 64 >= 12: code[]; 2 <= 8 x 2: from below"""
    p = R.predict(HAND, 3, 100)
    assert p == {"problems": 1, "pixels": 12, "cut": 0, "surviving": 2, "small": 2, "small_px": 4, "code": 1, "evaluation": R.LISTS,
                 "side": R.BELOW}
    assert R.predict(HAND, 3, 100, worklist=True)["evaluation"] == R.WALKS
    # start_label 0: -1 is masked, the same components, and never the lists
    p0 = R.predict(HAND - 1, 3, 100, start_label=0)
    assert {k: p0[k] for k in ("surviving", "small", "small_px", "code", "evaluation")} == \
        {"surviving": 2, "small": 2, "small_px": 4, "code": 1, "evaluation": R.WALKS}
    # min_size 1: nothing is small, no evaluation; min_size 4: everything is, and 4 > 8 x 0 starts from above
    assert R.predict(HAND, 1, 100)["evaluation"] == R.NONE and R.predict(HAND, 1, 100)["surviving"] == 4
    p4 = R.predict(HAND, 4, 100)
    assert (p4["surviving"], p4["small"], p4["small_px"], p4["side"]) == (0, 4, 10, R.ABOVE)
    # max_size 3: the two components of 3 pixels reach it -- only the cut count is given
    assert R.predict(HAND, 3, 3) == {"problems": 1, "pixels": 12, "cut": 2}


def test_predict_at_the_thresholds():
    """one small pixel in 64 pixels: code[] (1 x 64 >= 64); in 65: none.  8 small beside 1 surviving: from below; 9: from above"""
    a = np.ones((8, 8), np.int64)
    a[4, 4] = 2
    assert R.predict(a, 2, 1000)["code"] == 1
    b = np.ones((5, 13), np.int64)
    b[2, 6] = 2
    pb = R.predict(b, 2, 1000)
    assert (pb["code"], pb["evaluation"], pb["small"], pb["surviving"]) == (0, R.WALKS, 1, 1)
    for k, side in ((8, R.BELOW), (9, R.ABOVE)):
        c = np.ones((3, 40), np.int64)
        c[1, 1:1 + 2 * k:2] = 2
        pc = R.predict(c, 2, 1000)
        assert (pc["small"], pc["surviving"], pc["side"]) == (k, 1, side)


def test_every_case_sits_in_its_regime(oracle):
    for name, c in R.CASES.items():
        lab, mn, mx = c.make()
        assert lab.size < 2e5 and lab.min() >= 0, name
        p = R.predict(lab, mn, mx, oracle=oracle)
        assert (p["cut"] > 0) == c.cut, (name, p)
        if name == "none_small":
            assert p["evaluation"] == R.NONE and p["small"] == 0, (name, p)
            continue
        assert (p["code"], p["side"]) == (c.code, c.side), (name, p)
        assert p["evaluation"] == (R.LISTS if c.code else R.WALKS), (name, p)
        # the other runs of the case: the switch and start_label 0 (on labels - 1) give the walks, nothing else moves
        pw = R.predict(lab, mn, mx, worklist=True, oracle=oracle)
        p0 = R.predict(lab - 1, mn, mx, start_label=0, oracle=oracle)
        for q in (pw, p0):
            assert q["evaluation"] == R.WALKS and {k: q[k] for k in q if k != "evaluation"} == {k: p[k] for k in p if k != "evaluation"}, name


def test_the_cases_cover_every_regime_by_prediction(oracle):
    """the set the GPU test must see on the device, here from the predictions: {code[]} x {walks, lists} x {side} x {cut}, lists only
    with code[] (the third axis' "below then above" is a matter of rounds: the device's to show)"""
    seen = set()
    for name, c in R.CASES.items():
        if name == "none_small":
            continue
        lab, mn, mx = c.make()
        for sl, wl in R.runs(name):
            p = R.predict(lab - 1 + sl, mn, mx, start_label=sl, worklist=wl, oracle=oracle)
            seen.add((p["code"], p["evaluation"], p["side"], p["cut"] > 0))
    want = {(code, ev, side, cut) for code in (0, 1) for ev in (R.WALKS, R.LISTS) for side in (R.BELOW, R.ABOVE) for cut in (False, True)
            if not (ev == R.LISTS and code == 0)}
    assert seen == want


def test_the_size_thresholds_inside_an_evaluation_are_crossed():
    """comb: a component above SETTLE_COOP pixels with more than BFS_PUSH small neighbours; mast: one of exactly SETTLE_COOP pixels
    (the per-lane path) with BFS_PUSH + 1 small neighbours that touch nothing else"""
    lab, _, _ = R.comb()
    assert (lab == 4).sum() == 60 > R.SETTLE_COOP and 60 > R.BFS_PUSH
    lab, _, _ = R.mast()
    assert (lab == 2).sum() == R.SETTLE_COOP and (lab == 3).sum() == R.BFS_PUSH + 1
    teeth = np.argwhere(lab == 3)
    for y, x in teeth:                     # a tooth's neighbours: the bar or masked
        nb = [lab[yy, xx] for yy, xx in ((y, x + 1), (y, x - 1), (y + 1, x), (y - 1, x)) if 0 <= yy < lab.shape[0] and 0 <= xx < lab.shape[1]]
        assert set(nb) <= {0, 2} and 2 in nb


def test_batch_reference_on_a_hand_worked_batch(oracle):
    """problem one: label 1 (4 pixels) survives as 1, label 2 (2 pixels, min_size 3) joins it; problem two: label 5 (3 pixels) is the
    batch's second survivor, label 7 (4 pixels) its third; problem three: an isolated pixel never finds a neighbour (0), label 4 is
    the fourth survivor"""
    maps = [np.array([[1, 1, 2], [1, 1, 2]]), np.array([[5, 5, 5, 7], [0, 7, 7, 7]]), np.array([[3, 0, 4, 4, 4]])]
    probs = [(3, 100)] * 3
    outs, n = R.batch_reference(oracle, maps, probs, 1)
    assert n == 4
    assert outs[0].tolist() == [[1, 1, 1], [1, 1, 1]]
    assert outs[1].tolist() == [[2, 2, 2, 3], [0, 3, 3, 3]]
    assert outs[2].tolist() == [[0, 0, 4, 4, 4]]
    # start_label 0 on labels - 1: survivors 0 .. 3, masked -1 -- and the isolated pixel the literal 0, not the third problem's first
    outs, n = R.batch_reference(oracle, [m - 1 for m in maps], probs, 0)
    assert n == 4
    assert outs[0].tolist() == [[0, 0, 0], [0, 0, 0]]
    assert outs[1].tolist() == [[1, 1, 1, 2], [-1, 2, 2, 2]]
    assert outs[2].tolist() == [[0, -1, 3, 3, 3]]
    tot = R.predict_batch(maps, probs, 1)
    assert (tot["problems"], tot["pixels"], tot["surviving"], tot["small"], tot["small_px"]) == (3, 19, 4, 2, 3)


def test_every_batch_is_what_its_docstring_says(oracle):
    maps, probs = R.batch_mixed()
    assert len({m.shape for m in maps}) == 3 and len(set(probs)) == 3
    maps, probs = R.batch_touching()
    assert maps[0].shape[1] == maps[1].shape[1] and (maps[0][-1] == maps[1][0]).all()
    outs, n = R.batch_reference(oracle, maps, probs, 1)
    assert n == 2 and (outs[0][-1] != outs[1][0]).all()          # the two halves of label 9 end on different survivors
    united = oracle.enforce_connectivity(np.concatenate(maps), 20, 1000)
    assert len(np.unique(united)) == 3                              # ... as one map the row pair (24 pixels) would survive
    maps, probs = R.batch_all_small_between()
    ps = [R.predict(m, *pr) for m, pr in zip(maps, probs)]
    assert [p["small"] for p in ps][0] == 0 and ps[2]["small"] == 0 and ps[1]["surviving"] == 0 and ps[1]["small"] > 100
    maps, probs = R.batch_tiny()
    assert maps[1].shape == (1, 1) and maps[2].shape[0] == 1 and maps[2].shape[1] > 1
    maps, probs = R.batch_cut()
    cuts = [R.predict(m, *pr)["cut"] for m, pr in zip(maps, probs)]
    assert cuts == [4, 0, 16] and len({mx for _, mx in probs}) == 3
    tot = R.predict_batch(maps, probs, 1, oracle=oracle)
    assert (tot["cut"], tot["surviving"], tot["small"]) == (20, 8 + 1 + 16, 32 + 300 + 16)


def test_the_oracle_on_the_cases_whose_outcome_is_stated(oracle):
    lab, mn, mx = R.CASES["strips"].make()
    assert lab.shape == (4, 302) and (oracle.enforce_connectivity(lab, mn, mx) == 1).all()
    lab, mn, mx = R.CASES["strips_sparse"].make()
    ref = oracle.enforce_connectivity(lab, mn, mx)
    assert lab.shape == (404, 302) and lab.size == 122008 and (ref[:4] == 1).all() and (ref[4:] == 2).all()
    lab, mn, mx = R.CASES["strips_reversed"].make()
    ref = oracle.enforce_connectivity(lab, mn, mx)
    assert (ref == 0).sum() == 1188 and (ref == 1).sum() == 20 and ref.max() == 1
    assert (ref[1:, 299] == 1).all() and (ref[2:, 298] == 1).all() and (ref[3:, 297] == 1).all()      # settled at rows 1, 2 and 3
    lab, mn, mx = R.CASES["twin_bars"].make()
    ref = oracle.enforce_connectivity(lab, mn, mx)
    assert lab.shape == (34, 49) and (ref[:26] == 0).all() and sorted(np.unique(ref[26:])) == [1, 2, 3, 4]
    lab, mn, mx = R.CASES["comb"].make()
    ref = oracle.enforce_connectivity(lab, mn, mx)
    assert lab.shape == (3, 64) and (ref[lab > 0] == 1).all() and (ref[lab == 0] == 0).all()
    # the variants of the comb: the bar settles on its tail and the teeth never; the teeth settle through the bar
    lab, mn, mx = R.CASES["comb_below"].make()
    ref = oracle.enforce_connectivity(lab, mn, mx)
    assert (ref[lab == 4] == 1).all() and (ref[0] == 0).all()
    for name in ("comb_fed", "mast"):
        lab, mn, mx = R.CASES[name].make()
        assert (oracle.enforce_connectivity(lab, mn, mx)[lab > 0] == 1).all(), name


def test_the_report_fields_are_the_header():
    txt = open(os.path.join(ROOT, "include", "obia_testing.h")).read()
    body = txt[txt.index("in this order:"):txt.index("int obia_test_cc_report")]
    rows = re.findall(r"^ \*\s+(\d+)  (.+)$", body, flags=re.M)
    assert [int(i) for i, _ in rows] == list(range(len(R.REPORT_FIELDS)))
    assert int(re.search(r"#define OBIA_TEST_CC_REPORT_FIELDS (\d+)", txt).group(1)) == len(R.REPORT_FIELDS)
    says = {"problems": "problems", "pixels": "pixels", "surviving": "surviving components", "small": "small components",
            "small_px": "pixels of the small components", "cut": "components cut at max_size", "code": "code[] used",
            "evaluation": "evaluation:", "side": "side the settle rounds started on", "rounds_below": "rounds run from below",
            "rounds_above": "rounds run from above", "visited_realloc": "visited map reallocated"}
    for (_, text), name in zip(rows, R.REPORT_FIELDS):
        assert text.startswith(says[name]), (name, text)
    for const, val in (("NONE", "0 none"), ("WALKS", "1 walks"), ("LISTS", "2 pixel lists")):
        assert val in body and getattr(R, const) == int(val[0])


def test_the_new_entries_refuse_a_null_context_and_a_short_buffer():
    from obia_amd import _lib
    lib = _lib.load()
    buf = np.zeros(len(R.REPORT_FIELDS), np.int64)
    assert lib.obia_test_cc_report(None, buf.ctypes.data, len(buf)) == _lib.E_INVALID and _lib.last_error() == "null context"
    assert lib.obia_test_enforce_connectivity_batch_dev(None, None, None, 1, 1, None, None) == _lib.E_INVALID
    assert _lib.last_error() == "null context"


def test_the_constants_are_the_sources():
    """the constants this module restates, against cc.hip as it stands"""
    src = open(os.path.join(ROOT, "obia_amd", "csrc", "cc.hip")).read()
    assert f"constexpr int RING = {R.RING};" in src
    assert f"constexpr int ROUNDS_FROM_BELOW = {R.ROUNDS_FROM_BELOW};" in src
    assert f"constexpr int SETTLE_COOP = {R.SETTLE_COOP};" in src
    assert f"constexpr int BFS_PUSH = {R.BFS_PUSH};" in src
    assert f'atoll(std::getenv("OBIA_CC_CODE_DIV")) : {R.CODE_DIV};' in src and "n_small * code_div >= n" in src
    assert src.count(f"first_side = n_small > {R.ABOVE_RATIO} * (long long)n_surv ? 1 : 0;") == 1 and src.count("int side = first_side;") == 2
    assert 'use_code && start_label == 1 && !std::getenv("OBIA_CC_WORKLIST")' in src
