"""The regimes of the connectivity stage by name (test helper, not a conftest).

`enforce_connectivity_batch` (obia_amd/csrc/cc.hip) lets the data of a call choose its branches: whether the dense `code[]` pass
runs, whether the settle times come from BFS walks or from pixel lists, on which side the settle rounds start and whether they
restart, whether a size cut runs first.  The library records what it chose (`obia_test_cc_report`, include/obia_testing.h); this
module says what it MUST choose for a given map -- `predict`, NumPy and scipy.ndimage.label only -- and holds maps built to sit in
one regime each (`CASES`), so that tests/test_cc_regimes_cpu.py can tell, without a GPU, when a case has drifted out of its regime
and tests/test_gpu_connectivity_regimes.py can compare the device's record with the prediction.

Every map is below 2e5 pixels.  A case is a function returning `(labels, min_size, max_size)` with labels >= 1 and 0 = masked (the
layout of start_label 1; a start_label 0 run takes `labels - 1`)."""
import ctypes
import functools

import numpy as np
from scipy import ndimage

# ---- the three rules, stated once, each with the line of cc.hip it restates -----------------------------------------------------
CODE_DIV = 64          # `use_code = n_small * code_div >= n` (code_div = 64 unless OBIA_CC_CODE_DIV is set)
ABOVE_RATIO = 8        # `first_side = n_small > 8 * n_surv ? 1 : 0`: the rounds start from above at once
ROUNDS_FROM_BELOW = 5  # `max_rounds = side == 0 ? ROUNDS_FROM_BELOW : ...` with `round <= max_rounds`: at most 6 rounds run from below
RING = 64              # `constexpr int RING = 64`: the "moved" counters; the 65th round of a call is the first to refill them
SETTLE_COOP = 12       # `constexpr int SETTLE_COOP = 12`: components above it are evaluated by the whole wave (pixel lists)
BFS_PUSH = 12          # `constexpr int BFS_PUSH = 12`: new small neighbours a lane keeps before the re-walk / the direct append
NONE, WALKS, LISTS = 0, 1, 2          # field 7 of the report
BELOW, ABOVE = 0, 1                   # field 8

# include/obia_testing.h, obia_test_cc_report: the fields in the header's order
REPORT_FIELDS = ("problems", "pixels", "surviving", "small", "small_px", "cut", "code", "evaluation", "side", "rounds_below",
                 "rounds_above", "visited_realloc")


def evaluation_rule(code, start_label, worklist):
    """`dense = use_code && start_label == 1 && !getenv("OBIA_CC_WORKLIST")`: lists need code[], start_label 1 and no switch"""
    return LISTS if (code and start_label == 1 and not worklist) else WALKS


def regime(pixels, surviving, small, start_label=1, worklist=False):
    """(code[] used, evaluation, starting side) from the counts, by the three rules; (0, NONE, BELOW) without small components"""
    if small == 0:
        return 0, NONE, BELOW
    code = int(small * CODE_DIV >= pixels)
    return code, evaluation_rule(code, start_label, worklist), (ABOVE if small > ABOVE_RATIO * surviving else BELOW)


def component_sizes(lab, mask_label):
    """sizes of the 4-connected components of equal label, masked pixels left out (scipy.ndimage.label per label value, inside the
    value's bounding box)"""
    lab = np.asarray(lab, np.int64)
    shifted = lab - lab.min() + 1
    sizes = []
    for i, sl in enumerate(ndimage.find_objects(shifted.astype(np.int32))):
        v = i + 1 + lab.min() - 1
        if sl is None or v == mask_label:
            continue
        cl, k = ndimage.label(lab[sl] == v)
        sizes.extend(np.bincount(cl.ravel())[1:].tolist())
    return np.array(sizes, np.int64)


def predict(lab, min_size, max_size, start_label=1, worklist=False, oracle=None):
    """What the report of a single-problem call on `lab` must say: a dict of pixels, surviving, small, small_px, cut (components of
    at least max_size pixels) and -- derived by the three rules -- code, evaluation, side.  When a component reaches max_size the cut
    changes the counts: then only `pixels` and `cut` are given, unless `oracle` is passed: the pieces are then read off the oracle's
    output for min_size 1 (every piece keeps a label of its own there) and counted against min_size."""
    lab = np.asarray(lab)
    cap = max(int(max_size), 1)
    sizes = component_sizes(lab, start_label - 1)
    out = {"problems": 1, "pixels": int(lab.size), "cut": int((sizes >= cap).sum())}
    if out["cut"]:
        if oracle is None:
            return out
        pieces = oracle.enforce_connectivity(lab, 1, max_size, start_label=start_label)
        sizes = np.bincount(pieces[pieces >= start_label] - start_label)
    small = sizes < min_size
    out.update(surviving=int((~small).sum()), small=int(small.sum()), small_px=int(sizes[small].sum()))
    out["code"], out["evaluation"], out["side"] = regime(out["pixels"], out["surviving"], out["small"], start_label, worklist)
    return out


def predict_batch(maps, problems, start_label=1, oracle=None):
    """the sums of `predict` over the problems of a batch, and the regime of the sums: the batch is ONE call"""
    tot = {"problems": len(maps), "pixels": 0, "surviving": 0, "small": 0, "small_px": 0, "cut": 0}
    for lab, (mn, mx) in zip(maps, problems):
        p = predict(lab, mn, mx, start_label, oracle=oracle)
        for k in ("pixels", "surviving", "small", "small_px", "cut"):
            tot[k] += p[k]
    tot["code"], tot["evaluation"], tot["side"] = regime(tot["pixels"], tot["surviving"], tot["small"], start_label)
    return tot


def batch_reference(oracle, maps, problems, start_label=1):
    """The oracle per problem, every label at or above start_label shifted by the surviving components of the problems before it:
    the numbering over the whole batch of obia_test_enforce_connectivity_batch_dev.  Returns (list of label maps, survivors).

    start_label 0: a small component that never meets a labelled neighbour is the literal 0 and stays it, while the first surviving
    component of its problem -- 0 as well in a run of the problem alone -- is shifted.  To tell the two apart, a problem after the
    first runs below a pad that survives on its own (rows of a label the map does not use, then a masked row: nothing of the problem
    touches it, the raster order of the problem's pixels is unchanged): labels below the pad's count are then the literal 0."""
    outs, offset = [], 0
    for lab, (mn, mx) in zip(maps, problems):
        lab = np.asarray(lab, np.int64)
        H, W = lab.shape
        if start_label == 1 or offset == 0:
            ref = oracle.enforce_connectivity(lab, mn, mx, start_label=start_label)
            n = int(ref.max()) - start_label + 1 if (ref >= start_label).any() else 0
            if start_label == 0 and not predict(lab, mn, mx, 0, oracle=oracle)["surviving"]:
                n = 0                   # (nothing survives: every 0 is the literal one)
            out = np.where(ref >= start_label, ref + offset, ref) if start_label == 1 else ref   # (offset 0: nothing to shift)
        else:
            rows = -(-max(int(mn), 1) // W)
            pad = np.full((rows + 1, W), -1, np.int64)
            pad[:rows] = lab.max() + 1
            ref = oracle.enforce_connectivity(np.concatenate([pad, lab]), mn, mx, start_label=0)
            n_pad = int(ref[:rows].max()) + 1
            ref = ref[rows + 1:]
            n = max(int(ref.max()) + 1 - n_pad, 0)
            out = np.where(ref >= n_pad, ref - n_pad + offset, np.where(ref >= 0, 0, ref))
        outs.append(out)
        offset += n
    return outs, offset


# ---- the named cases -------------------------------------------------------------------------------------------------------------
def _never(lab):
    return lab.size + 1


def pad_sparse(lab, small):
    """`lab` with rows of one more surviving label below it until 64 x small < pixels: the same map without code[]"""
    H, W = lab.shape
    rows = (CODE_DIV * small) // W + 1 - H
    assert rows > 0
    return np.concatenate([lab, np.full((rows, W), lab.max() + 1, lab.dtype)])


def strips(n=300, H=4):
    """A horizontal chain: a surviving H x 2 block, to its right `n` H x 1 strips of alternating labels.  Every strip ends on the
    survivor's label; from above one strip settles per round."""
    lab = np.empty((H, n + 2), np.int64)
    lab[:, :2] = 3
    lab[:, 2:] = 1 + (np.arange(n) % 2)
    return lab, H + 1, _never(lab)


def strips_sparse():
    lab, mn, _ = strips()
    lab = np.concatenate([lab, np.full((400, lab.shape[1]), 4, np.int64)])
    return lab, mn, _never(lab)


def strips_reversed():
    """`strips` mirrored: the strip next to the survivor starts before it, settles at its second row, the next at its third, the
    next at its fourth -- and the rest never: 297 strips end as 0"""
    lab, mn, mx = strips()
    return lab[:, ::-1].copy(), mn, mx


def strips_cut():
    """`strips` with a 4 x 4 surviving block cut at 8 pixels into two surviving pieces"""
    lab, mn, _ = strips()
    lab = np.concatenate([np.full((4, 2), 3, np.int64), lab], 1)
    return lab, mn, 8


def strips_sparse_cut():
    """`strips_sparse` whose lower survivor (400 x W) is cut into pieces of 20 000 pixels"""
    lab, mn, _ = strips_sparse()
    return lab, mn, 20000


def twin_bars(units=16, bar=24, surv_rows=4):
    """`units` pairs of vertical bar x 1 bars side by side (labels 1 | 2), each pair in a moat of masked pixels, above `surv_rows`
    surviving rows of 2 x W: the two bars of a pair see only each other -- from below they leapfrog one pixel per round, from above
    nothing moves: the reference leaves every bar 0"""
    W = 3 * units + 1
    lab = np.zeros((1 + bar + 1 + 2 * surv_rows, W), np.int64)
    lab[1:1 + bar, 1::3] = 1
    lab[1:1 + bar, 2::3] = 2
    for r in range(surv_rows):
        lab[bar + 2 + 2 * r: bar + 4 + 2 * r] = 3 + r
    return lab, 30, _never(lab)


def twin_bars_sparse():
    """eight surviving rows of 2 x W: 2058 pixels > 64 x 32"""
    return twin_bars(surv_rows=8)


def twin_bars_cut():
    """the surviving rows (98 pixels) cut at 60 into 60 + 38, both surviving"""
    lab, mn, _ = twin_bars()
    return lab, mn, 60


def twin_bars_sparse_cut():
    lab, mn, _ = twin_bars_sparse()
    return lab, mn, 60


def comb(surv_rows=1):
    """A surviving first row above a row of 60 one-pixel teeth of alternating labels above a 1 x 60 bar of a third label: the bar has
    60 distinct small neighbours (> BFS_PUSH) and 60 pixels (> SETTLE_COOP)"""
    lab = np.zeros((surv_rows + 2, 64), np.int64)
    lab[:surv_rows] = 1
    lab[surv_rows, :60] = 2 + (np.arange(60) % 2)
    lab[surv_rows + 1, :60] = 4
    return lab, 61, _never(lab)


def comb_sparse():
    lab, mn, _ = comb()
    lab = pad_sparse(lab, 61)
    return lab, mn, _never(lab)


def comb_cut():
    """two surviving rows (128 pixels) cut at 64 into two surviving pieces"""
    lab, mn, _ = comb(surv_rows=2)
    return lab, mn, 64


def comb_below():
    """The surviving rows LAST: teeth, then the bar, then three surviving rows of 62; the bar has a tail down the last column, so that
    it has pixels after the survivor's first one.  The bar (67 pixels, first pixel 64) settles at pixel 191, the first of its tail --
    a time that is NOT its first pixel and, in the pixel lists, not the first entry of its slice; the teeth never settle (0)."""
    lab = np.zeros((5, 64), np.int64)
    lab[0, :60] = 2 + (np.arange(60) % 2)
    lab[1, :] = 4
    lab[2:, :62] = 1
    lab[2:, 63] = 4
    return lab, 100, _never(lab)


def comb_fed():
    """The bar BETWEEN the survivor and the teeth: two surviving rows, the 1 x 60 bar, then 60 one-pixel teeth that touch nothing but
    the bar and each other.  From above the bar settles in the first round, in which the teeth of its wave still read "never": they
    settle only because the bar enqueues its 60 neighbours (the `nbrs.overflow` re-walk of the BFS walks)."""
    lab = np.zeros((4, 64), np.int64)
    lab[:2] = 1
    lab[2, :60] = 4
    lab[3, :60] = 2 + (np.arange(60) % 2)
    return lab, 100, _never(lab)


def comb_fed_sparse():
    lab, mn, _ = comb_fed()
    lab = pad_sparse(lab, 61)
    return lab, mn, _never(lab)


def mast(top=1):
    """A vertical 12 x 1 bar (<= SETTLE_COOP: one lane evaluates it) below a surviving row, with 13 one-pixel teeth that touch
    nothing but the bar: six left, six right, one below (> BFS_PUSH: the 13th goes through the direct append of the pixel lists, or
    the re-walk of the BFS walks).  All of them settle after the bar, on its label."""
    lab = np.zeros((top + 13, 15), np.int64)
    lab[:top] = 1
    lab[top:top + 12, 7] = 2
    lab[top + 1:top + 12:2, 6] = 3
    lab[top + 1:top + 12:2, 8] = 3
    lab[top + 12, 7] = 3
    return lab, 13, _never(lab)


def mast_sparse():
    return mast(top=48)


def slic_like(H=96, W=130, seed=5, noise=0.8, cell=12):
    """grid cells with noisy borders, what a SLIC sweep leaves: small components between surviving ones -- a few rounds from below
    converge"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    lab = ((yy + noise * rs.randn(H, W)) // cell).astype(np.int64) * 1000 + ((xx + noise * rs.randn(H, W)) // cell).astype(np.int64) + 2000
    lab -= lab.min() - 1
    return lab, 9, _never(lab)


def slic_like_sparse():
    """the same grid with little noise: one small component per 150 pixels"""
    return slic_like(noise=0.25)


def slic_like_cut():
    """every cell (144 pixels) cut at 100"""
    lab, mn, _ = slic_like()
    return lab, mn, 100


def slic_like_sparse_cut():
    lab, mn, _ = slic_like_sparse()
    return lab, mn, 100


def cut_to_small():
    """5 x 5 blocks of labels of their own, cut at 20 pixels: every block leaves a piece of 5, below min_size 8 -- a cut piece that
    becomes a small component itself"""
    yy, xx = np.mgrid[0:20, 0:20]
    return (yy // 5) * 4 + xx // 5 + 1, 8, 20


def none_small():
    lab, _, mx = slic_like()
    return lab, 1, mx


class Case:
    """fn: the map; regime: (code[], side) it was built for; cut: whether a size cut runs; rounds: the case's own condition on the
    report (a function of the report dict -> bool) with its text; worklist: also run with OBIA_CC_WORKLIST set"""

    def __init__(self, fn, code, side, cut=False, rounds=None, why="", worklist=False, starred=False):
        self.fn, self.code, self.side, self.cut, self.rounds, self.why, self.worklist = fn, code, side, cut, rounds, why, worklist
        self.starred = starred

    @functools.lru_cache(maxsize=None)
    def make(self):
        lab, mn, mx = self.fn()
        lab = np.ascontiguousarray(lab, np.int64)
        lab.setflags(write=False)
        return lab, int(mn), int(mx)


def _ring(r):
    return r["rounds_below"] == 0 and r["rounds_above"] > RING


def _restart(r):
    return r["rounds_below"] >= ROUNDS_FROM_BELOW and r["rounds_above"] >= 1


def _stayed(r):
    return r["rounds_below"] >= 1 and r["rounds_above"] == 0


def _above(r):
    return r["rounds_below"] == 0 and r["rounds_above"] >= 1


RING_WHY = "more than 64 rounds, all from above: the ring of counters is refilled"
RESTART_WHY = "at least five rounds from below, then a restart from above"
STAYED_WHY = "converged from below: no round from above"
ABOVE_WHY = "every round from above"

CASES = {
    "strips": Case(strips, 1, ABOVE, rounds=_ring, why=RING_WHY, worklist=True, starred=True),
    "strips_sparse": Case(strips_sparse, 0, ABOVE, rounds=_ring, why=RING_WHY, starred=True),
    "strips_reversed": Case(strips_reversed, 1, ABOVE, rounds=_above, why=ABOVE_WHY, worklist=True, starred=True),
    "strips_cut": Case(strips_cut, 1, ABOVE, cut=True, rounds=_ring, why=RING_WHY, worklist=True),
    "strips_sparse_cut": Case(strips_sparse_cut, 0, ABOVE, cut=True, rounds=_ring, why=RING_WHY),
    "twin_bars": Case(twin_bars, 1, BELOW, rounds=_restart, why=RESTART_WHY, worklist=True, starred=True),
    "twin_bars_sparse": Case(twin_bars_sparse, 0, BELOW, rounds=_restart, why=RESTART_WHY),
    "twin_bars_cut": Case(twin_bars_cut, 1, BELOW, cut=True, rounds=_restart, why=RESTART_WHY, worklist=True),
    "twin_bars_sparse_cut": Case(twin_bars_sparse_cut, 0, BELOW, cut=True, rounds=_restart, why=RESTART_WHY),
    "comb": Case(comb, 1, ABOVE, rounds=_above, why=ABOVE_WHY, worklist=True, starred=True),
    "comb_sparse": Case(comb_sparse, 0, ABOVE, rounds=_above, why=ABOVE_WHY),
    "comb_cut": Case(comb_cut, 1, ABOVE, cut=True, rounds=_above, why=ABOVE_WHY, worklist=True),
    "comb_below": Case(comb_below, 1, ABOVE, rounds=_above, why=ABOVE_WHY, worklist=True),
    "comb_fed": Case(comb_fed, 1, ABOVE, rounds=_above, why=ABOVE_WHY, worklist=True),
    "comb_fed_sparse": Case(comb_fed_sparse, 0, ABOVE, rounds=_above, why=ABOVE_WHY),
    "mast": Case(mast, 1, ABOVE, rounds=_above, why=ABOVE_WHY, worklist=True),
    "mast_sparse": Case(mast_sparse, 0, ABOVE, rounds=_above, why=ABOVE_WHY),
    "slic_like": Case(slic_like, 1, BELOW, rounds=_stayed, why=STAYED_WHY, worklist=True),
    "slic_like_sparse": Case(slic_like_sparse, 0, BELOW, rounds=_stayed, why=STAYED_WHY),
    "slic_like_cut": Case(slic_like_cut, 1, BELOW, cut=True, rounds=_stayed, why=STAYED_WHY, worklist=True),
    "slic_like_sparse_cut": Case(slic_like_sparse_cut, 0, BELOW, cut=True, rounds=_stayed, why=STAYED_WHY),
    "cut_to_small": Case(cut_to_small, 1, BELOW, cut=True, rounds=_stayed, why=STAYED_WHY, worklist=True),
    "none_small": Case(none_small, 0, BELOW, rounds=lambda r: r["rounds_below"] == 0 and r["rounds_above"] == 0,
                       why="no small component: no round at all"),
}


def runs(name):
    """the runs of a case: (start_label, worklist switch)"""
    out = [(1, False)]
    if CASES[name].worklist:
        out.append((1, True))
    out.append((0, False))
    return out


# ---- batches: (maps, [(min_size, max_size)]) -----------------------------------------------------------------------------------
def batch_mixed():
    """strips | slic_like | twin_bars with their own min_size / max_size, three shapes under one maxh"""
    cs = [strips(), slic_like(H=40, W=70), twin_bars()]
    return [c[0] for c in cs], [(c[1], c[2]) for c in cs]


def batch_touching():
    """two problems of equal W whose touching rows -- the last of the first, the first of the second -- carry the same labels: they
    must not unite.  Alone in their problems the halves are small (12 pixels each, min_size 20); united they would survive."""
    a = np.ones((6, 12), np.int64) * 5
    a[4:] = 7                            # last two rows: label 7, 24 pixels: survives in problem one
    a[5, :] = 9                          # last row: label 9, 12 pixels
    b = np.ones((6, 12), np.int64) * 5
    b[0, :] = 9                          # first row: label 9 again, 12 pixels
    return [a, b], [(20, 1000), (20, 1000)]


def batch_all_small_between():
    """an all-small problem (salt and pepper, min_size above everything) between two all-surviving ones"""
    rs = np.random.RandomState(3)
    a = np.repeat(np.repeat(np.arange(1, 13).reshape(3, 4), 8, 0), 8, 1)
    b = rs.randint(1, 4, (20, 33)).astype(np.int64)
    c = np.repeat(np.repeat(np.arange(1, 7).reshape(2, 3), 10, 0), 9, 1)
    return [a, b, c], [(5, 10000), (5000, 10000), (5, 10000)]


def batch_tiny():
    """a 1 x 1 and a 1 x W problem among larger ones"""
    a, mn, mx = slic_like(H=30, W=41)
    b = np.array([[4]], np.int64)
    c = np.array([[1, 1, 1, 2, 2, 0, 3, 3, 3, 3, 1]], np.int64)
    d, mn2, mx2 = comb()
    return [a, b, c, d], [(mn, mx), (1, 5), (3, 100), (mn2, mx2)]


def batch_cut():
    """a size cut in two of three problems, each at its own max_size: twin_bars_cut (60) | strips (never) | cut_to_small (20)"""
    cs = [twin_bars_cut(), strips(), cut_to_small()]
    return [c[0] for c in cs], [(c[1], c[2]) for c in cs]


BATCHES = {"mixed": batch_mixed, "touching": batch_touching, "all_small_between": batch_all_small_between, "tiny": batch_tiny,
           "cut": batch_cut}


# ---- the two entries of include/obia_testing.h (private wrappers: no public name of obia_amd) ----------------------------------
def cc_report(ctx=None, dev=0):
    """the record of the last connectivity call of `ctx` (default: the default context of device `dev`) as a dict of REPORT_FIELDS"""
    from obia_amd import _lib
    c = ctx or _lib.default_context(dev)
    out = np.zeros(len(REPORT_FIELDS), np.int64)
    _lib.check(_lib.load().obia_test_cc_report(c.handle, out.ctypes.data, len(out)))
    return dict(zip(REPORT_FIELDS, (int(v) for v in out)))


def enforce_connectivity_batch(labels_in, problems, start_label, labels_out, ctx=None):
    """obia_test_enforce_connectivity_batch_dev: `labels_in` / `labels_out` flat int32 CUDA tensors (the maps back to back),
    `problems` rows of (H, W, min_size, max_size); returns the number of surviving components"""
    from obia_amd import _device, _lib
    lib, c = _device.begin(labels_in.device.index or 0, ctx)
    pr = np.ascontiguousarray(problems, np.int64).reshape(-1, 4)
    n = ctypes.c_int(0)
    _lib.check(lib.obia_test_enforce_connectivity_batch_dev(c.handle, labels_in.data_ptr(), pr.ctypes.data, len(pr), int(start_label),
                                                            labels_out.data_ptr(), ctypes.byref(n)))
    return n.value
