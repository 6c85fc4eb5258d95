"""The entry points of include/obia_boxes.h through guarded outputs (tests/guarded.py, both poisons) with every input off a 16-byte
boundary (tests/offset_views.py): the results bit for bit, no stray write, no element left unwritten, the inputs unchanged, two runs
equal; and what is refused writes nothing.  Every entry point of the table is exercised here."""
import ctypes
import functools

import numpy as np
import pytest

from tests import boxes_restatement as R
from tests.guarded import POISONS, guarded, snapshot, unchanged
from tests.offset_views import offset_view, residue
from tests.refusal_text import refused_saying

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

H, W, NL = 21, 23, 14
N = 300                                                                      # two workgroups of the per-box kernels, the second ragged
THR = 0.2
EXERCISED = ("obia_boxes_assign_dev", "obia_boxes_pair_count_dev", "obia_boxes_pair_write_dev", "obia_boxes_dissolve_dev",
             "obia_boxes_iou_dev", "obia_boxes_nms_dev")


@functools.lru_cache(maxsize=None)
def case():
    rs = np.random.RandomState(99)
    labels = np.kron(rs.randint(0, NL + 3, (7, 8)), np.ones((3, 3), np.int64))[:H, :W].astype(np.int32)     # ids above NL: background
    labels[labels == NL] = 0
    labels[:, 20:] = NL                                                      # a segment no box reaches: the boxes end at column 19
    xy = rs.uniform(-2, [13, H], (N, 2))
    boxes = np.concatenate([xy, xy + rs.uniform(0, 6, (N, 2))], 1)
    boxes[::7] = np.round(boxes[::7])                                        # integer-aligned ones
    c = dict(labels=labels, boxes=boxes)
    c["table"] = R.pair_table(labels, boxes, NL)
    c["assigned"], c["area"] = R.assign(labels, boxes, NL)
    count = np.bincount(c["table"]["box"], minlength=N).astype(np.int64)
    c["count"], c["offset"], c["total"] = count, np.cumsum(count) - count, int(count.sum())
    c["dissolved"] = R.dissolve(labels, c["assigned"])
    c["b2"] = boxes[:37] + rs.uniform(-1, 1, (37, 4)) * [1, 1, 0, 0]
    c["iou"] = R.iou_matrix(boxes[:29], c["b2"])
    # the grid by the rule of include/obia_seed_table.h on (x0, y0), cell side >= the largest box side
    scores = rs.uniform(0, 1, N)
    groups = rs.randint(0, 2, N).astype(np.int32)
    side = float(max((boxes[:, 2] - boxes[:, 0]).max(), (boxes[:, 3] - boxes[:, 1]).max())) * (1.0 + 2.0 ** -20)
    cx, cy = np.floor(boxes[:, 0] / side).astype(np.int64), np.floor(boxes[:, 1] / side).astype(np.int64)
    ncx = int(cx.max() - cx.min()) + 3
    key = (cy - cy.min() + 1) * ncx + (cx - cx.min() + 1)
    order = np.argsort(key, kind="stable")
    pos = np.empty(N, np.int32)
    pos[np.argsort(-scores, kind="stable")] = np.arange(N, dtype=np.int32)
    keep = R.nms(boxes, scores, THR, groups)[0]
    assert 0 < keep.sum() < N and (c["assigned"] >= 0).any() and (c["assigned"][1:] < 0).any() and (c["area"] > 0).any()
    c.update(order=order, skey=key[order], ncx=ncx, pos=pos, groups=groups, keep=keep[order].astype(np.uint8))
    return c


def dev_off(a, k):
    return offset_view(torch.as_tensor(np.ascontiguousarray(a)).cuda(), k)


def judge(g, want, name):
    """the guarded output holds `want` bit for bit, nothing around it changed, nothing in it was left as it was"""
    got = g.host()
    b = {1: np.uint8, 4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    want = np.ascontiguousarray(want)
    assert np.array_equal(got.view(b), want.view(b)), f"{name}: {int((got.view(b) != want.view(b)).sum())} differ"
    poison = np.frombuffer(bytes([g.poison]) * want.dtype.itemsize, b)[0]
    assert g.findings(exempt=want.view(b) == poison, name=name) == []


def test_every_entry_point_of_the_table_is_exercised():
    from obia_amd import _lib
    assert set(EXERCISED) == set(_lib._BOXES_SIGNATURES)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("poison", POISONS, ids=[f"{p:02X}" for p in POISONS])
def test_buffers_off_the_boundary_and_guarded_outputs(k, poison):
    """int32 buffers 4, 8 and 12 bytes past a 16-byte boundary, float64 / int64 ones 8 bytes (k odd), byte outputs k bytes"""
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.default_context(0)
    c = case()
    o, T = c["order"], c["total"]
    labels, boxes, boxes_s = dev_off(c["labels"], k), dev_off(c["boxes"], k), dev_off(c["boxes"][o], k)
    pos_s, grp_s, skey, offset = dev_off(c["pos"][o], k), dev_off(c["groups"][o], k), dev_off(c["skey"], k), dev_off(c["offset"], k)
    a29, b37, assigned_in = dev_off(c["boxes"][:29], k), dev_off(c["b2"], k), dev_off(c["assigned"], k)
    assert residue(labels) == 4 * k and residue(boxes) == (8 * k) % 16 and residue(skey) == (8 * k) % 16
    ins = [labels, boxes, boxes_s, pos_s, grp_s, skey, offset, a29, b37, assigned_in]
    snaps = [snapshot(t) for t in ins]
    runs = []
    for _ in range(2):
        g = {n: guarded(shape, dt, poison, "cuda", k) for n, shape, dt in (
            ("assigned", (NL + 1,), np.int32), ("area", (NL + 1,), np.float64), ("count", (N,), np.int64), ("passes", (N,), np.int32),
            ("box", (T,), np.int32), ("seg", (T,), np.int32), ("parea", (T,), np.float64), ("meets", (T,), np.int32),
            ("dissolved", (H, W), np.int32), ("iou", (29, 37), np.float64), ("keep", (N,), np.uint8))}
        assert g["assigned"].ptr % 16 == 4 * k and g["area"].ptr % 16 == (8 * k) % 16 and g["keep"].ptr % 16 == k
        rounds = ctypes.c_int32(-1)
        torch.cuda.synchronize()
        L, B = labels.data_ptr(), boxes.data_ptr()
        calls = [lib.obia_boxes_assign_dev(ctx.handle, L, H, W, B, N, NL, g["assigned"].ptr, g["area"].ptr),
                 lib.obia_boxes_pair_count_dev(ctx.handle, L, H, W, B, N, NL, g["count"].ptr, g["passes"].ptr),
                 lib.obia_boxes_pair_write_dev(ctx.handle, L, H, W, B, N, NL, offset.data_ptr(), g["passes"].ptr, T, g["box"].ptr, g["seg"].ptr,
                                               g["parea"].ptr, g["meets"].ptr),
                 lib.obia_boxes_dissolve_dev(ctx.handle, L, H * W, assigned_in.data_ptr(), NL, g["dissolved"].ptr),
                 lib.obia_boxes_iou_dev(ctx.handle, a29.data_ptr(), 29, b37.data_ptr(), 37, g["iou"].ptr),
                 lib.obia_boxes_nms_dev(ctx.handle, boxes_s.data_ptr(), pos_s.data_ptr(), grp_s.data_ptr(), skey.data_ptr(), N, c["ncx"], THR,
                                        g["keep"].ptr, ctypes.byref(rounds))]
        assert calls == [0] * 6, (calls, _lib.last_error())
        # the pairs of a box are written in no particular order: sorted by (box, segment) they are the table
        box, seg = g["box"].host(), g["seg"].host()
        srt = np.lexsort((seg, box))
        t = c["table"]
        assert np.array_equal(box[srt], t["box"]) and np.array_equal(seg[srt], t["segment"]) and np.array_equal(g["meets"].host()[srt], t["meets"])
        assert np.array_equal(g["parea"].host()[srt].view(np.uint64), t["area"].view(np.uint64))
        for n in ("box", "seg", "parea", "meets"):
            assert g[n].findings(name=n) == []
        want = dict(assigned=c["assigned"], area=c["area"], count=c["count"], passes=np.ones(N, np.int32), dissolved=c["dissolved"],
                    iou=c["iou"], keep=c["keep"])
        for n, w in want.items():
            judge(g[n], w, n)
        assert 1 <= rounds.value <= N
        runs.append({n: g[n].host().tobytes() for n in want})
    assert runs[0] == runs[1]
    assert all(unchanged(t, s) for t, s in zip(ins, snaps))

    # refused: nothing is written
    g = {n: guarded((max(N, c["total"]),), dt, poison, "cuda", k) for n, dt in (("a", np.int32), ("b", np.int32), ("c", np.int32), ("d", np.float64),
                                                                               ("q", np.int64), ("u", np.uint8))}
    a, b, c4, d, q, u = (g[n].ptr for n in ("a", "b", "c", "d", "q", "u"))
    L, B, O, P, K = labels.data_ptr(), boxes.data_ptr(), offset.data_ptr(), pos_s.data_ptr(), skey.data_ptr()
    nonfinite, reversed_ = c["boxes"].copy(), c["boxes"].copy()
    nonfinite[N - 1, 2] = np.inf
    reversed_[N - 1, [1, 3]] = [5.0, 4.0]
    BN, BR = dev_off(nonfinite, k), dev_off(reversed_, k)
    invalid = [lib.obia_boxes_assign_dev(ctx.handle, L, H, W, B, 0, NL, a, d), lib.obia_boxes_assign_dev(ctx.handle, L, H, W, B, 2 ** 31, NL, a, d),
               lib.obia_boxes_assign_dev(ctx.handle, None, H, W, B, N, NL, a, d), lib.obia_boxes_assign_dev(ctx.handle, L, H, W, B + 4, N, NL, a, d),
               lib.obia_boxes_assign_dev(ctx.handle, L + 2, H, W, B, N, NL, a, d), lib.obia_boxes_assign_dev(ctx.handle, L, H, W, B, N, NL, a + 1, d),
               lib.obia_boxes_assign_dev(ctx.handle, L, H, W, B, N, NL, a, d + 4), lib.obia_boxes_assign_dev(ctx.handle, L, 0, W, B, N, NL, a, d),
               lib.obia_boxes_assign_dev(ctx.handle, L, H, W, B, N, -1, a, d), lib.obia_boxes_assign_dev(ctx.handle, L, H, W, BR.data_ptr(), N, NL, a, d),
               lib.obia_boxes_pair_count_dev(ctx.handle, L, H, W, B, 0, NL, q, a), lib.obia_boxes_pair_count_dev(ctx.handle, L, H, W, B, N, NL, q + 4, a),
               lib.obia_boxes_pair_count_dev(ctx.handle, L, H, W, B, N, NL, None, a), lib.obia_boxes_pair_count_dev(ctx.handle, L, H, W, BR.data_ptr(), N, NL, q, a),
               lib.obia_boxes_pair_write_dev(ctx.handle, L, H, W, B, N, NL, O, P, 0, a, b, d, c4),
               lib.obia_boxes_pair_write_dev(ctx.handle, L, H, W, B, N, NL, O, P, T, a, a, d, c4),
               lib.obia_boxes_pair_write_dev(ctx.handle, L, H, W, B, N, NL, O + 4, P, T, a, b, d, c4),
               lib.obia_boxes_pair_write_dev(ctx.handle, L, H, W, B, N, NL, O, None, T, a, b, d, c4),
               lib.obia_boxes_pair_write_dev(ctx.handle, L, H, W, BR.data_ptr(), N, NL, O, P, T, a, b, d, c4),
               lib.obia_boxes_dissolve_dev(ctx.handle, L, 0, assigned_in.data_ptr(), NL, a), lib.obia_boxes_dissolve_dev(ctx.handle, L, H * W, None, NL, a),
               lib.obia_boxes_dissolve_dev(ctx.handle, L, H * W, assigned_in.data_ptr(), NL, a + 3),
               lib.obia_boxes_iou_dev(ctx.handle, B, 0, B, 3, d), lib.obia_boxes_iou_dev(ctx.handle, B, 3, B + 2, 3, d),
               lib.obia_boxes_iou_dev(ctx.handle, B, 3, B, 3, None),
               lib.obia_boxes_nms_dev(ctx.handle, B, P, None, K, 0, c["ncx"], THR, u, None), lib.obia_boxes_nms_dev(ctx.handle, B, P, None, K, N, 2, THR, u, None),
               lib.obia_boxes_nms_dev(ctx.handle, B, P, None, K, N, c["ncx"], -0.5, u, None),
               lib.obia_boxes_nms_dev(ctx.handle, B, P, None, K, N, c["ncx"], float("nan"), u, None),
               lib.obia_boxes_nms_dev(ctx.handle, B, P + 1, None, K, N, c["ncx"], THR, u, None),
               lib.obia_boxes_nms_dev(ctx.handle, B, P, None, K + 4, N, c["ncx"], THR, u, None),
               lib.obia_boxes_nms_dev(ctx.handle, B, None, None, K, N, c["ncx"], THR, u, None),
               lib.obia_boxes_nms_dev(ctx.handle, BR.data_ptr(), P, None, K, N, c["ncx"], THR, u, None),
               # an output that starts where an input starts
               lib.obia_boxes_nms_dev(ctx.handle, B, P, None, K, N, c["ncx"], THR, P, None),
               lib.obia_boxes_nms_dev(ctx.handle, B, P, None, K, N, c["ncx"], THR, K, None),
               lib.obia_boxes_nms_dev(ctx.handle, B, P, grp_s.data_ptr(), K, N, c["ncx"], THR, grp_s.data_ptr(), None),
               lib.obia_boxes_pair_write_dev(ctx.handle, L, H, W, B, N, NL, O, P, T, a, b, B, c4),
               lib.obia_boxes_pair_write_dev(ctx.handle, L, H, W, B, N, NL, O, P, T, a, b, O, c4),
               lib.obia_boxes_pair_write_dev(ctx.handle, L, H, W, B, N, NL, O, P, T, a, P, d, c4),
               lib.obia_boxes_assign_dev(ctx.handle, L, H, W, B, N, NL, a, B), lib.obia_boxes_assign_dev(ctx.handle, L, H, W, B, N, NL, L, d),
               lib.obia_boxes_pair_count_dev(ctx.handle, L, H, W, B, N, NL, B, a)]
    assert invalid == [_lib.E_INVALID] * len(invalid), invalid
    # ... and says so in full: a null output, an output (the keep flags are bytes: an input) one byte on, an output where an input starts
    h, AI = ctx.handle, assigned_in.data_ptr()
    refused_saying("boxes: assign: bad arguments (null, misaligned or overlapping buffers)", lib.obia_boxes_assign_dev,
                   (h, L, H, W, B, N, NL, None, d), (h, L, H, W, B, N, NL, a + 1, d), (h, L, H, W, B, N, NL, a, B))
    refused_saying("boxes: pair count: bad arguments (null, misaligned or overlapping buffers)", lib.obia_boxes_pair_count_dev,
                   (h, L, H, W, B, N, NL, None, a), (h, L, H, W, B, N, NL, q + 1, a), (h, L, H, W, B, N, NL, q, L))
    refused_saying("boxes: pair write: bad arguments (null, misaligned or overlapping buffers)", lib.obia_boxes_pair_write_dev,
                   (h, L, H, W, B, N, NL, O, P, T, None, b, d, c4), (h, L, H, W, B, N, NL, O, P, T, a, b, d + 1, c4),
                   (h, L, H, W, B, N, NL, O, P, T, a, b, d, L))
    refused_saying("boxes: dissolve: bad arguments (null, misaligned or overlapping buffers)", lib.obia_boxes_dissolve_dev,
                   (h, L, H * W, AI, NL, None), (h, L, H * W, AI, NL, a + 1), (h, L, H * W, AI, NL, L), (h, L, H * W, AI, NL, AI))
    refused_saying("boxes: iou: bad arguments (null, misaligned or overlapping buffers)", lib.obia_boxes_iou_dev,
                   (h, B, 3, B, 3, None), (h, B, 3, B, 3, d + 1), (h, B, 3, BR.data_ptr(), 3, B), (h, BR.data_ptr(), 3, B, 3, B))
    refused_saying("boxes: nms: bad arguments (null, misaligned or overlapping buffers)", lib.obia_boxes_nms_dev,
                   (h, B, P, None, K, N, c["ncx"], THR, None, None), (h, B, P + 1, None, K, N, c["ncx"], THR, u, None),
                   (h, B, P, None, K, N, c["ncx"], THR, B, None))
    nonfin = [lib.obia_boxes_assign_dev(ctx.handle, L, H, W, BN.data_ptr(), N, NL, a, d),
              lib.obia_boxes_pair_count_dev(ctx.handle, L, H, W, BN.data_ptr(), N, NL, q, a),
              lib.obia_boxes_pair_write_dev(ctx.handle, L, H, W, BN.data_ptr(), N, NL, O, P, T, a, b, d, c4),
              lib.obia_boxes_nms_dev(ctx.handle, BN.data_ptr(), P, None, K, N, c["ncx"], THR, u, None)]
    assert nonfin == [_lib.E_NONFINITE] * len(nonfin), nonfin
    assert all(v.untouched() for v in g.values())
    assert all(unchanged(t, s) for t, s in zip(ins, snaps))


def test_tables_that_are_not_those_of_the_count_are_refused_without_a_write_out_of_bounds():
    """offsets that lead past `total`: OBIA_E_INVALID, and nothing outside the outputs changes"""
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.default_context(0)
    c = case()
    labels, boxes = torch.as_tensor(c["labels"]).cuda(), torch.as_tensor(c["boxes"]).cuda()
    offset = torch.as_tensor(c["offset"] + 7).cuda()
    passes = torch.ones(N, dtype=torch.int32).cuda()
    T = c["total"]
    g = {n: guarded((T,), dt, 0xA5, "cuda", 1) for n, dt in (("box", np.int32), ("seg", np.int32), ("area", np.float64), ("meets", np.int32))}
    torch.cuda.synchronize()
    rc = lib.obia_boxes_pair_write_dev(ctx.handle, labels.data_ptr(), H, W, boxes.data_ptr(), N, NL, offset.data_ptr(), passes.data_ptr(), T,
                                       g["box"].ptr, g["seg"].ptr, g["area"].ptr, g["meets"].ptr)
    assert rc == _lib.E_INVALID and "not those of the count" in _lib.last_error()
    assert all(len(v.stray()) == 0 for v in g.values())


def test_a_footprint_of_2_31_pixels_is_unsupported():
    """the check reads only the box table: the raster is claimed, not allocated, and nothing is launched over it"""
    from obia_amd import _lib
    lib, ctx = _lib.load(), _lib.default_context(0)
    labels = torch.zeros(16, dtype=torch.int32).cuda()
    boxes = torch.as_tensor(np.array([[0.0, 0.0, 1.0, 1.0], [0.5, 0.5, 65536.5, 32768.5]])).cuda()
    g = {n: guarded((4,), dt, 0x5A, "cuda", 1) for n, dt in (("assigned", np.int32), ("area", np.float64))}
    torch.cuda.synchronize()
    rc = lib.obia_boxes_assign_dev(ctx.handle, labels.data_ptr(), 70000, 70000, boxes.data_ptr(), 2, 3, g["assigned"].ptr, g["area"].ptr)
    assert rc == _lib.E_UNSUPPORTED and "2^31" in _lib.last_error()
    assert all(v.untouched() for v in g.values())
