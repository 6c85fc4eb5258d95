"""Stage-level references of SLIC (obia_slic_stages_f32_dev): what the features, one sweep and the centroid update must be, in
plain NumPy and the oracle's pinned functions.  Shared by tests/test_slic_stages_cpu.py (which validates these references on the
oracle's own chain, without a GPU) and tests/test_gpu_slic_stages.py (which judges the kernels with them).

  Stage A  features      features_ref32 (bit for bit without Lab) / features_ref64 (Lab: the oracle's own float32 error is the yardstick)
  Stage B  one sweep     sweep_ref32 = oracle.slic_core(max_iter=1) on the DEVICE's features and centroids, every pixel, no tolerance;
                         sweep_ref64 = independent float64 assignment, decides wherever the runner-up is further than gap_threshold(C)
  Stage C  the update    centroid_ref64 with the derived bound of centroid_bounds
"""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden")
SPACING = [1.0, 0.5, 1.75]
SPECIALS = np.array([0.0, 1.0, 0.04045, 0.0031], np.float32)   # sRGB: the ends, the knee of the gamma curve, a value below it
NEAR_TIE_CAP = 0.01                                            # of the valid pixels of a colour-pass sweep


# ---- cases ------------------------------------------------------------------------------------------------------------------
def _case(name, H, W, C, per_seg, comp, lab=False, norm=True, sigma=0, mask=None, spacing=None, zero=False, grouped=False,
          start_label=1, iters=4, seeds=None):
    return dict(name=name, H=H, W=W, C=C, per_seg=per_seg, compactness=comp, lab=lab, normalize=norm, sigma=sigma, mask=mask,
                spacing=spacing, slic_zero=zero, grouped=grouped, start_label=start_label, iters=iters, seeds=seeds)


# The smallest shapes that cross the sweep tile (64 x 64), the footprint (16 x 16), the quad row (4) and the 16-column block; band counts on
# both sides of every record class (CP 4 / 8 / 12 / 16; 16 against 32 accumulator qwords); H * W / 9 centroids (tiles with more candidates
# than slots: no list) down to H * W / 500; compactness on both sides of the colour bound (non-Lab: ratio >= 2; Lab: ratio * 100 >= 2).
FIXED_CASES = [
    _case("tiny_c1", 7, 9, 1, 9, 1.0),
    _case("tiny_c4_label0", 7, 9, 4, 9, 0.25, start_label=0),
    _case("s33_c3_nolab", 33, 31, 3, 30, 0.05),
    _case("s33_c5_raw_dense", 33, 31, 5, 9, 1.0, norm=False),
    _case("t64_c4", 64, 64, 4, 80, 0.25),
    _case("t64_c8_dense", 64, 64, 8, 9, 10.0),
    _case("t64_c9_raw", 64, 64, 9, 200, 0.05, norm=False),
    _case("m65_c12", 65, 130, 12, 30, 1.0),
    _case("m65_c13", 65, 130, 13, 80, 0.25),
    _case("m65_c16_raw_sparse", 65, 130, 16, 500, 10.0, norm=False),
    _case("b129_c8", 129, 257, 8, 80, 0.25, iters=10),
    _case("b129_c5_dense", 129, 257, 5, 9, 0.05),
    _case("b129_c1_raw_sparse", 129, 257, 1, 500, 1.0, norm=False),
    _case("b129_c4_raw", 129, 257, 4, 200, 10.0, norm=False),
    _case("sigma_c4", 65, 130, 4, 30, 0.25, sigma=1.3),
    _case("sigma_list_c8_raw", 33, 31, 8, 30, 1.0, norm=False, sigma=[0, 2.0, 0.6]),
    _case("sigma_c13", 64, 64, 13, 80, 0.05, sigma=1.3),
    _case("mask_disc_c4", 65, 130, 4, 30, 0.25, mask="disc"),
    _case("mask_stripes_c8", 129, 257, 8, 80, 1.0, mask="stripes"),
    _case("mask_rects_c5_raw", 64, 64, 5, 30, 0.05, norm=False, mask="rects"),
    _case("mask_disc_c12_sigma", 33, 31, 12, 9, 10.0, mask="disc", sigma=1.3),
    _case("spacing_c4", 65, 130, 4, 80, 0.25, spacing=SPACING),
    _case("spacing_stripes_c3_nolab", 33, 31, 3, 30, 1.0, mask="stripes", spacing=SPACING),
    _case("seeds_golden_sigma_mask", 96, 128, 4, None, 0.4, sigma=1.5, mask="golden", seeds="sigma_mask_96x128x4"),
    _case("zero_c4", 64, 64, 4, 80, 0.25, zero=True),
    _case("zero_lab", 33, 31, 3, 30, 10.0, lab=True, zero=True),
    _case("grouped_c8", 65, 130, 8, 30, 0.25, grouped=True),
    _case("grouped_c16_disc", 64, 64, 16, 30, 1.0, mask="disc", grouped=True),
    _case("lab_c01_unit", 129, 257, 3, 80, 0.1, lab=True, norm=False),
    _case("lab_c10", 65, 130, 3, 30, 10.0, lab=True),
    _case("lab_c100_unit_nobound", 64, 64, 3, 80, 100.0, lab=True, norm=False),
    _case("lab_sigma", 33, 31, 3, 9, 10.0, lab=True, sigma=1.3),
    _case("lab_disc_c01", 65, 130, 3, 200, 0.1, lab=True, mask="disc"),
    _case("lab_tiny_unit", 7, 9, 3, 9, 10.0, lab=True, norm=False),
]


def random_case(seed):
    """A seeded draw over the same axes."""
    rs = np.random.RandomState(7000 + seed)
    H, W = [(7, 9), (33, 31), (64, 64), (65, 130), (129, 257)][rs.randint(5)]
    lab = rs.rand() < 0.3
    C = 3 if lab else int(rs.choice([1, 3, 4, 5, 8, 9, 12, 13, 16]))
    comp = float(rs.choice([0.1, 10.0, 100.0] if lab else [0.05, 0.25, 1.0, 10.0]))
    sigma = [0, 0, 1.3, [0, 2.0, 0.6]][rs.randint(4)]
    mask = [None, None, "disc", "stripes", "rects"][rs.randint(5)]
    return _case(f"random{seed}", H, W, C, int(rs.choice([9, 30, 80, 200, 500])), comp, lab=lab, norm=bool(rs.rand() < 0.6), sigma=sigma,
                 mask=mask, spacing=SPACING if rs.rand() < 0.15 else None, start_label=int(rs.randint(2)), iters=int(rs.choice([3, 4])))


def make_mask(kind, H, W, rs):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind == "disc":      # disc with a hole
        m = ((yy - H / 2) ** 2 + (xx - W / 2) ** 2 < (0.45 * max(H, W)) ** 2) & ~((abs(yy - H / 3) < H / 10) & (abs(xx - W / 2) < W / 8))
    elif kind == "stripes":  # thin diagonal stripes: centroids drift, pixels get orphaned
        m = ((xx + 2 * yy).astype(np.int64) % 17) < 5
    else:                   # a few scattered rectangles
        m = np.zeros((H, W), bool)
        for _ in range(4):
            y0, x0 = rs.randint(0, max(1, H - 4)), rs.randint(0, max(1, W - 4))
            m[y0:y0 + rs.randint(3, max(4, H // 2)), x0:x0 + rs.randint(3, max(4, W // 2))] = True
    return m.astype(np.uint8)


def make_inputs(case):
    """(image float32 (H, W, C), mask uint8 or None, seeds (yx, steps) or None).  Textured noise, as tests/test_gpu_random_parity.make_case
    draws it: raw values around 800 +- 300, or -- Lab on un-normalised input -- the same texture inside [0, 1]; the special sRGB values
    are planted in every channel."""
    if case["seeds"]:
        z = np.load(os.path.join(GOLD, case["seeds"] + ".npz"))
        return z["raw"].astype(np.float32), z["mask"].astype(np.uint8), (z["seeds_yx"], z["seed_steps_all"])
    H, W, C = case["H"], case["W"], case["C"]
    rs = np.random.RandomState(abs(hash_name(case["name"])) % (2 ** 31))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    img = np.stack([300 * np.sin(xx / (5 + 2 * c)) * np.cos(yy / (6 + c)) + 800 + 40 * c + rs.normal(0, 25, (H, W)) for c in range(C)], -1)
    if case["lab"] and not case["normalize"]:
        img = np.clip((img - 400.0) / 900.0, 0.0, 1.0)
    img = img.astype(np.float32)
    if case["lab"] and not case["normalize"]:
        for c in range(C):
            for j, v in enumerate(SPECIALS):
                img[(3 * c + j) % H, (5 * j + c + 1) % W, c] = v
    mask = make_mask(case["mask"], H, W, rs) if case["mask"] else None
    return img, mask, None


def hash_name(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % 1000003
    return h


def n_segments(case, mask):
    if case["per_seg"] is None:
        return 40
    n = case["H"] * case["W"] if mask is None else int(mask.sum())
    return max(2, n // case["per_seg"])


def slic_kwargs(case, mask, seeds):
    """Arguments of obia_amd.segmentation._slic_stages / slic for the case."""
    kw = dict(n_segments=n_segments(case, mask), compactness=case["compactness"], convert2lab=bool(case["lab"]), sigma=case["sigma"],
              slic_zero=case["slic_zero"], start_label=case["start_label"], _normalize_bands=case["normalize"], mask=mask)
    if case["spacing"]:
        kw["spacing"] = case["spacing"]
    if seeds is not None:
        kw["seeds"] = seeds
    return kw


# ---- Stage A: features -------------------------------------------------------------------------------------------------------
def features_ref32(oracle, img, case):
    """normalise -> sRGB to Lab -> Gaussian -> * float32(1 / compactness): the float32 restatement pinned on scikit-image's and scipy's
    output (tests/test_oracle_golden.py, tests/golden/sigma*.npz)."""
    x = oracle.normalize(img) if case["normalize"] else np.ascontiguousarray(img, np.float32).copy()
    if case["lab"]:
        x = oracle.rgb2lab(x)
    if any(s > 0 for s in oracle.sigma_zyx(case["sigma"], case["spacing"])):
        x = oracle.gaussian_filter_zyx(x, case["sigma"], case["spacing"])
    return x * np.float32(1.0 / case["compactness"])


def features_ref64(oracle, img, case):
    """The same chain with every operation in float64 (the input and the two given constants -- the Gaussian weights and
    float32(1 / compactness) -- are the same numbers)."""
    x = np.asarray(img, np.float32).astype(np.float64)
    if case["normalize"]:
        mn, mx = x.min(axis=(0, 1)), x.max(axis=(0, 1))
        x = (x - mn) / (mx - mn)
    if case["lab"]:
        x = oracle.rgb2lab_f64(x)
    x = x[None]
    for ax, s in enumerate(oracle.sigma_zyx(case["sigma"], case["spacing"])):
        if s > 1e-15:
            w, lw = oracle.gaussian_weights(s)
            x = oracle._correlate1d_reflect(x, w, lw, ax)   # float64 in, float64 out
    assert x.dtype == np.float64
    return x[0] * float(np.float32(1.0 / case["compactness"]))


def expected_fscale(features):
    """2^s, the largest power of two with max|feature| * 2^s < 2^29 (s clamped to [-90, 100] as the library does)."""
    m = float(np.abs(features).max())
    if not m > 0.0:
        return 1.0
    e = int(np.frexp(m)[1])        # m = f * 2^e, f in [0.5, 1)
    return float(np.ldexp(1.0, min(100, max(-90, 29 - e))))


# ---- Stage B: one sweep --------------------------------------------------------------------------------------------------------
def sweep_ref32(oracle, features, centroids, step, mask=None, ignore_color=False, slic_zero=False, start_label=1, spacing=None):
    """The reference's assignment sweep (_slic_cython through oracle.slic_core, max_iter=1) from the given centroids.  Pixels no
    window reaches (and masked ones) keep start_label - 1.  `centroids` is not changed."""
    seg = np.ascontiguousarray(centroids, np.float32).copy()
    sp = None if spacing is None else (spacing[1], spacing[2])
    return oracle.slic_core(np.ascontiguousarray(features, np.float32), seg, np.float32(step), max_iter=1, mask=mask, slic_zero=slic_zero,
                            ignore_color=ignore_color, start_label=start_label, spacing_yx=sp)


def window_steps(oracle, H, W, K):
    g = oracle.regular_grid(H, W, K)
    return (g[1] or 1), (g[3] or 1)


def sweep_ref64(oracle, features, centroids, step, mask=None, ignore_color=False, start_label=1, spacing=None):
    """An assignment sweep in float64, written independently of the oracle's C code: the window of a centroid is the reference's
    (float32 bounds cast to integers, obia_oracle.c:253-260; a NaN centroid has none), the distance is
    ((sy (cy - y))^2 + (sx (cx - x))^2) * float32(1 / step^2) + sum_c (f_c - c_c)^2 with float64 operations on the float32 inputs,
    the lowest k wins an exact tie.  Returns (labels int64, start_label - 1 where no window reaches; gap float64: (d2 - d1) / d2 with d1
    the winning distance and d2 the smallest distance ABOVE it -- candidates that tie the winner exactly are decided by their index,
    the gap says how far the first candidate that is not one of them lies; 1 where there is none)."""
    f = np.asarray(features, np.float32).astype(np.float64)
    H, W, C = f.shape
    cen = np.asarray(centroids, np.float32)
    K = cen.shape[0]
    sy_step, sx_step = window_steps(oracle, H, W, K)
    sw = float(np.float32(1.0 / (float(np.float32(step)) ** 2)))
    sp_y, sp_x = (1.0, 1.0) if spacing is None else (float(np.float32(spacing[1])), float(np.float32(spacing[2])))
    d1 = np.full((H, W), np.inf)
    d2 = np.full((H, W), np.inf)
    lab = np.full((H, W), start_label - 1, np.int64)
    valid = np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0
    f32 = np.float32
    for k in range(K):
        cy, cx = cen[k, 0], cen[k, 1]
        if np.isnan(cy) or np.isnan(cx):
            continue
        y0 = int(max(cy - f32(2 * sy_step), f32(0)))
        y1 = int(min(cy + f32(2 * sy_step) + f32(1), f32(H)))
        x0 = int(max(cx - f32(2 * sx_step), f32(0)))
        x1 = int(min(cx + f32(2 * sx_step) + f32(1), f32(W)))
        if y1 <= y0 or x1 <= x0:
            continue
        ys = np.arange(y0, y1, dtype=np.float64)[:, None]
        xs = np.arange(x0, x1, dtype=np.float64)[None, :]
        d = ((sp_y * (float(cy) - ys)) ** 2 + (sp_x * (float(cx) - xs)) ** 2) * sw
        if not ignore_color:
            d = d + ((f[y0:y1, x0:x1] - cen[k, 2:].astype(np.float64)) ** 2).sum(-1)
        a1, a2, al = d1[y0:y1, x0:x1], d2[y0:y1, x0:x1], lab[y0:y1, x0:x1]
        v = valid[y0:y1, x0:x1]
        win = v & (d < a1)                       # strictly closer: an equal distance leaves the lower k in place
        nxt = v & (d > a1) & (d < a2)
        a2[...] = np.where(win, a1, np.where(nxt, d, a2))
        a1[...] = np.where(win, d, a1)
        al[...] = np.where(win, k + start_label, al)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(np.isinf(d2), 1.0, (d2 - d1) / d2)
    gap[lab == start_label - 1] = 1.0
    return lab, gap


def gap_threshold(C):
    """A float32 distance is a sum of C + 2 non-negative squares, each of a rounded difference, times / plus: C + 4 roundings of relative
    size 2^-24 at the most; two distances are compared, so a float64 gap above (C + 4) * 2^-24 * 2 decides the float32 comparison too."""
    return (C + 6) * 2.0 ** -23


def judge_sweep64(labels, ref64, gap, C, valid):
    """(pixels where the float64 winner is binding but `labels` disagrees, fraction of valid pixels that are near ties).  Binding: the
    gap exceeds the threshold -- the winner is then the lowest k of the candidates at exactly the smallest distance.  Near tie: the rest."""
    thr = gap_threshold(C)
    binding = valid & (gap > thr)
    near = valid & ~binding
    wrong = binding & (np.asarray(labels, np.int64) != ref64)
    return int(wrong.sum()), float(near.sum()) / max(1, int(valid.sum()))


def cap_applies(case, mask, n, features, step):
    """Is the near-tie cap a condition this colour sweep's input can meet?  Always, but for sweep 1 of an unmasked case: its centroids
    still carry the initial colours, zero, so every candidate of a pixel has the SAME colour term S = sum_c f_c^2 and only the spatial
    terms tell the candidates apart.  The seeds sit on integer positions, so two squared distances are equal or at least one unit u
    apart (u = 1; 1 / 16 with the spacing (0.5, 1.75), whose squares are sixteenths), and a window reaches 2 * step each way: two
    candidates that do not tie exactly differ by at least u / step^2 in a distance of S + 8 * 3.0625 at the most.  Where that ratio
    exceeds the threshold for the largest S of the image, no pixel can be a near tie and the cap is asserted; where it does not -- raw
    bands, Lab at low compactness: S of 1e6 and more -- no input of the kind can meet it, and the sweep is judged by the float32
    reference at every pixel and by float64 wherever that is binding.  With a mask the colour pass starts from the centroids the
    pre-pass left, which have colours."""
    if mask is not None or n > 1:
        return True
    u = 1.0 if case["spacing"] is None else 1.0 / 16.0
    s_max = float((np.asarray(features, np.float64) ** 2).sum(-1).max())
    return u / float(step) ** 2 / (s_max + 8.0 * 3.0625) > gap_threshold(case["C"])


# ---- Stage C: the centroid update ------------------------------------------------------------------------------------------------
def centroid_ref64(features, labels, mask, K, start_label=1):
    """float64 means of y, x and every channel over the valid pixels of each label, and the pixel counts.  A label without a pixel
    is 0 / 0 = NaN in every column, as in the reference."""
    f = np.asarray(features, np.float32).astype(np.float64)
    H, W, C = f.shape
    k = np.asarray(labels, np.int64).ravel() - start_label
    keep = k >= 0
    if mask is not None:
        keep &= np.asarray(mask).ravel() != 0
    k = k[keep]
    yy, xx = np.mgrid[0:H, 0:W]
    cols = [yy.ravel()[keep].astype(np.float64), xx.ravel()[keep].astype(np.float64)] + [f[..., c].ravel()[keep] for c in range(C)]
    n = np.bincount(k, minlength=K).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.stack([np.bincount(k, weights=col, minlength=K) / n for col in cols], -1)
    return mean, n.astype(np.int64)


def centroid_bounds(mean64, fscale):
    """How far the library's float32 centroid may lie from the float64 mean (the one documented deviation of the port: integer sums).
    eps = 2^-23, one float32 ulp relative to the value.

    Positions.  sum(y) and n are integers, exact in the 64-bit accumulators.  cy = float(sum) / float(n): float(n) is exact (n < 2^24),
    float(sum) rounds once (relative 2^-24), the division rounds once more: |cy - mean| <= ((1 + 2^-24)^2 - 1) |mean| = 1 ulp.
    Colours.  A pixel adds trunc(f * 2^s) with 2^s = fscale; the product is exact, the truncation drops less than one unit, towards
    zero: the integer sum over a cluster is within n units of sum(f) * 2^s, so sum / 2^s / n within 2^-s of the mean.  The sum (below
    2^53) times 2^-s is exact in double; then the same two roundings, float(.) and the division, on a value within 2^-s of the mean:
        |c - mean| <= 2^-s + ((1 + 2^-24)^2 - 1) * (|mean| + 2^-s).
    The float64 reference's own summation error (up to 2^16 terms, 2^-53 each) is four thousand times below one float32 ulp and
    is covered by the 2^-36 added to eps."""
    eps = (1.0 + 2.0 ** -24) ** 2 - 1.0 + 2.0 ** -36
    b = np.empty_like(mean64)
    b[:, :2] = eps * np.abs(mean64[:, :2])
    t = 1.0 / fscale
    b[:, 2:] = t + eps * (np.abs(mean64[:, 2:]) + t)
    return b


def initial_segments(seeds_yx, C):
    """slic_superpixels.py: segments = [centroid positions | zeros(C)] -- the colours of the initial centroids are zero."""
    s = np.zeros((len(seeds_yx), 2 + C), np.float32)
    s[:, :2] = np.asarray(seeds_yx, np.float32)
    return s


def reference_seeds(oracle, case, mask, seeds):
    """(yx (K, 2) float32, step): the library's seeding rule restated by the oracle, or the caller's seeds."""
    if seeds is not None:
        st = [float(v) for v in np.ravel(seeds[1])]
        return np.asarray(seeds[0], np.float32), np.float32(max(1.0, max(st)))
    H, W = case["H"], case["W"]
    n = n_segments(case, mask)
    yx, steps = oracle.grid_centroids(H, W, n) if mask is None else oracle.masked_grid_centroids(mask, n)
    return yx.astype(np.float32), np.float32(max(1.0, float(steps.max())))
