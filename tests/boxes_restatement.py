"""NumPy / plain-Python restatement of include/obia_boxes.h (test helper, not a conftest): the overlap rule as loops over pixels, the
winner of a segment, sequential greedy NMS, ``calculate_iou`` on Python floats, and an exact oracle for the overlap with
``fractions.Fraction``.  Nothing here is clever on purpose: every function follows the header sentence by sentence."""
import math
from fractions import Fraction

import numpy as np


# ------------------------------------------------------------------------------------------------------------ the overlap rule
def footprint(lo, hi, n):
    """first and last footprint index on an axis of n pixels (first > last: empty)"""
    return max(0, math.ceil(lo) - 1), min(n - 1, math.floor(hi))


def axis_class(c, lo, hi):
    """(class, weight) of the footprint index c: 'Z' 0, 'L' fl(min(hi, c + 1) - lo), 'R' fl(hi - c), 'I' 1"""
    if float(c + 1) == lo or float(c) == hi:
        return "Z", 0.0
    if c < lo:
        return "L", min(hi, float(c + 1)) - lo
    if c + 1 > hi:
        return "R", hi - float(c)
    return "I", 1.0


def pairs_of_box(labels, box, n_labels):
    """{segment: (area, meets)} of one box by the header's rule"""
    H, W = labels.shape
    x0, y0, x1, y1 = (float(v) for v in box)
    c0, c1 = footprint(x0, x1, W)
    r0, r1 = footprint(y0, y1, H)
    counts, meets, wx, wy = {}, {}, {"I": 1.0}, {"I": 1.0}
    for r in range(r0, r1 + 1):
        kb, wb = axis_class(r, y0, y1)
        for c in range(c0, c1 + 1):
            lab = int(labels[r, c])
            if lab < 1 or lab > n_labels:
                continue
            ka, wa = axis_class(c, x0, x1)
            meets[lab] = meets.get(lab, 0) + 1
            if ka == "Z" or kb == "Z":
                continue
            assert wx.setdefault(ka, wa) == wa and wy.setdefault(kb, wb) == wb      # one weight per class
            key = (lab, ka, kb)
            counts[key] = counts.get(key, 0) + 1
    out = {}
    for lab in meets:
        area = 0.0
        for kb in ("L", "I", "R"):                  # the row classes T, I, B carry the column classes' names here
            for ka in ("L", "I", "R"):
                nab = counts.get((lab, ka, kb), 0)
                if nab:
                    area = area + (wx[ka] * wy[kb]) * float(nab)
        out[lab] = (area, meets[lab])
    return out


def pair_table(labels, boxes, n_labels=None):
    """dict of box, segment (int32), area (float64), meets (int32), sorted by (box, segment)"""
    labels = np.asarray(labels)
    n_labels = max(0, int(labels.max())) if n_labels is None else int(n_labels)
    rows = []
    for b, box in enumerate(np.asarray(boxes, dtype=np.float64)):
        for seg, (area, meets) in sorted(pairs_of_box(labels, box, n_labels).items()):
            rows.append((b, seg, area, meets))
    return {"box": np.array([r[0] for r in rows], np.int32), "segment": np.array([r[1] for r in rows], np.int32),
            "area": np.array([r[2] for r in rows], np.float64), "meets": np.array([r[3] for r in rows], np.int32)}


def assign(labels, boxes, n_labels=None):
    """(assigned (n_labels + 1,) int32, area (n_labels + 1,) float64): argmax of the area per segment, ties to the lowest box"""
    labels = np.asarray(labels)
    n_labels = max(0, int(labels.max())) if n_labels is None else int(n_labels)
    t = pair_table(labels, boxes, n_labels)
    assigned = np.full(n_labels + 1, -1, np.int32)
    area = np.zeros(n_labels + 1, np.float64)
    for b, seg, a in zip(t["box"], t["segment"], t["area"]):                    # ascending box: only a larger area replaces
        if assigned[seg] < 0 or a > area[seg]:
            assigned[seg], area[seg] = b, a
    return assigned, area


def dissolve(labels, assigned):
    labels = np.asarray(labels)
    out = np.zeros(labels.shape, np.int32)
    ok = (labels >= 1) & (labels < len(assigned))
    a = np.asarray(assigned)[np.where(ok, labels, 0)]
    out[ok & (a >= 0)] = a[ok & (a >= 0)] + 1
    return out


# ------------------------------------------------------------------------------------------------------------ the exact oracle
def exact_areas(labels, box, n_labels):
    """{segment: Fraction} the exact area every segment shares with the box, from the doubles as they are; segments that meet the
    box are all present, with 0 where they only touch"""
    H, W = labels.shape
    x0, y0, x1, y1 = (Fraction(float(v)) for v in box)
    out = {}
    for r in range(H):
        oy = min(y1, Fraction(r + 1)) - max(y0, Fraction(r))
        if oy < 0:
            continue
        for c in range(W):
            ox = min(x1, Fraction(c + 1)) - max(x0, Fraction(c))
            lab = int(labels[r, c])
            if ox < 0 or lab < 1 or lab > n_labels:
                continue
            out[lab] = out.get(lab, Fraction(0)) + ox * oy
    return out


# ------------------------------------------------------------------------------------------------------------------ IoU, NMS
def calculate_iou(box1, box2):
    """obia/detection/utils.py:63-81, statement by statement, on Python floats"""
    box1, box2 = [float(v) for v in box1], [float(v) for v in box2]
    x1 = max(box1[0], box2[0])
    y1 = max(box1[1], box2[1])
    x2 = min(box1[2], box2[2])
    y2 = min(box1[3], box2[3])
    inter_width = max(0, x2 - x1)
    inter_height = max(0, y2 - y1)
    inter_area = inter_width * inter_height
    box1_area = (box1[2] - box1[0]) * (box1[3] - box1[1])
    box2_area = (box2[2] - box2[0]) * (box2[3] - box2[1])
    return inter_area / float(box1_area + box2_area - inter_area + 1e-6)


def iou_matrix(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.array([[calculate_iou(p, q) for q in b] for p in a], np.float64).reshape(len(a), len(b))


def nms(boxes, scores, iou_threshold, groups=None):
    """(keep (n,) bool, kept indices by descending score): sequential greedy suppression, stable order"""
    boxes = np.asarray(boxes, dtype=np.float64)
    order = np.argsort(-np.asarray(scores, dtype=np.float64), kind="stable")
    keep = np.zeros(len(boxes), bool)
    kept = []
    for i in order:
        bi = boxes[i]
        ok = True
        for j in kept:
            bj = boxes[j]
            if bj[2] <= bi[0] or bi[2] <= bj[0] or bj[3] <= bi[1] or bi[3] <= bj[1]:
                continue                                   # no positive overlap: iou == 0, and 0 > threshold >= 0 is false
            if groups is not None and groups[j] != groups[i]:
                continue
            if calculate_iou(bj, bi) > iou_threshold:
                ok = False
                break
        if ok:
            keep[i] = True
            kept.append(int(i))
    return keep, np.array(kept, np.int64)
