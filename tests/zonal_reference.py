"""Float64 reference of the per-segment zonal statistics (TEST INFRASTRUCTURE ONLY): count, NaN-excluded count, mean,
variance, min, max, skewness and kurtosis per (label, band), the quantities zonal.hip computes.

Vectorised with ``np.bincount`` over float64 weights, so an 8192^2 raster stays in seconds:
  * count = pixels carrying the label; ``n`` = its non-NaN pixels per band (NaN pixels are dropped per band);
  * min / max over the non-NaN pixels;
  * mean = sum / n, refined once by the mean of the residuals (x - mean), so the sum's rounding does not stay in it;
  * the central sums m2, m3, m4 from a second pass over d = x - mean[label]; variance = m2 (ddof 0);
  * skewness = m3 / m2^1.5, kurtosis = m4 / m2^2 - 3, NaN where m2 <= (float32_eps * mean)^2 -- the kernel's rule
    (SciPy's "nearly constant" test, eps of the float32 raster).
``near_threshold`` flags the (label, band) pairs whose m2 lies within 1e-6 relative of that threshold: there the NaN
pattern is decided by the last bits of m2, so pattern comparisons exclude them (like the near-tie flags of qs_stages).

``abs_d3`` / ``d4`` (means of |d|^3 and d^4) feed the error bounds of the GPU tests (test_gpu_zonal_f64.py)."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
U64 = 2.0 ** -53            # unit roundoff of float64
NEAR_THRESHOLD_REL = 1e-6


def zonal_reference(raw, labels, bands=None, start_label=1, n_labels=None):
    raw = np.asarray(raw)
    H, W, C = raw.shape
    bands = list(range(C)) if bands is None else [int(b) for b in bands]
    lab = np.asarray(labels).reshape(-1).astype(np.int64) - int(start_label)
    if n_labels is None:
        n_labels = int(lab.max()) + 1 if lab.size else 0
    N, B = max(int(n_labels), 0), len(bands)
    inr = (lab >= 0) & (lab < N)
    li = lab[inr]
    flat = raw.reshape(-1, C)
    out = {"count": np.bincount(li, minlength=N).astype(np.int64)[:N]}
    for k in ("n",):
        out[k] = np.zeros((N, B), np.int64)
    for k in ("mean", "variance", "skewness", "kurtosis", "m2", "m3", "m4", "abs_d3", "d4"):
        out[k] = np.full((N, B), np.nan, np.float64)
    for k in ("min", "max"):
        out[k] = np.full((N, B), np.nan, np.float32)
    out["near_threshold"] = np.zeros((N, B), bool)
    for j, b in enumerate(bands):
        x = flat[inr, b]
        ok = ~np.isnan(x)
        lv, xv = li[ok], x[ok].astype(np.float64)
        n = np.bincount(lv, minlength=N)[:N]
        has = n > 0
        nn = np.where(has, n, 1).astype(np.float64)
        mean = np.bincount(lv, xv, minlength=N)[:N] / nn
        mean = mean + np.bincount(lv, xv - mean[lv], minlength=N)[:N] / nn
        d = xv - mean[lv]
        d2 = d * d
        m2 = np.bincount(lv, d2, minlength=N)[:N] / nn
        m3 = np.bincount(lv, d2 * d, minlength=N)[:N] / nn
        m4 = np.bincount(lv, d2 * d2, minlength=N)[:N] / nn
        a3 = np.bincount(lv, d2 * np.abs(d), minlength=N)[:N] / nn
        mn = np.full(N, np.inf, np.float32)
        mx = np.full(N, -np.inf, np.float32)
        np.minimum.at(mn, lv, x[ok])
        np.maximum.at(mx, lv, x[ok])
        t = (EPS32 * mean) ** 2
        with np.errstate(divide="ignore", invalid="ignore"):
            defined = has & ~(m2 <= t)
            sk = np.where(defined, m3 / (m2 * np.sqrt(m2)), np.nan)
            ku = np.where(defined, m4 / (m2 * m2) - 3.0, np.nan)
            near = has & (t > 0) & (np.abs(m2 / np.where(t > 0, t, 1.0) - 1.0) < NEAR_THRESHOLD_REL)
        out["n"][:, j] = n
        for k, v in (("mean", mean), ("variance", m2), ("m2", m2), ("m3", m3), ("m4", m4), ("abs_d3", a3), ("d4", m4)):
            out[k][:, j] = np.where(has, v, np.nan)
        out["skewness"][:, j], out["kurtosis"][:, j] = sk, ku
        out["min"][:, j] = np.where(has, mn, np.nan)
        out["max"][:, j] = np.where(has, mx, np.nan)
        out["near_threshold"][:, j] = near
    out["bands"] = bands
    return out


def segment_stats(v):
    """The same quantities for ONE (label, band) from its float64 pixel values (NaN already dropped): a direct restatement
    used to perturb a reference entry (one pixel removed or doubled)."""
    v = np.asarray(v, np.float64)
    n = v.size
    mean = v.sum() / n
    mean = mean + (v - mean).sum() / n
    d = v - mean
    m2, m3, m4 = (d ** 2).mean(), (d ** 3).mean(), (d ** 4).mean()
    if m2 <= (EPS32 * mean) ** 2:
        sk = ku = np.nan
    else:
        sk, ku = m3 / m2 ** 1.5, m4 / m2 ** 2 - 3.0
    return {"n": n, "mean": mean, "variance": m2, "m2": m2, "m3": m3, "m4": m4, "abs_d3": (np.abs(d) ** 3).mean(),
            "d4": m4, "skewness": sk, "kurtosis": ku, "min": np.float32(v.min()), "max": np.float32(v.max())}


# ---- error bounds of the kernels and the comparison --------------------------------------------------------------------
BOUND_C = 8.0     # rounding steps per term (difference, product, fma, the pivot conversions) and the reference's own share


def tolerances(ref):
    """Absolute bars per (label, band) from the error bound of the HIP arithmetic (float64 throughout).

    Notation: n non-NaN pixels, u = 2^-53, R = max - min, M2 / A3 / M4 the central moments m2, mean|d|^3, m4.
      * mean: the kernel sums x - P about a pixel P of the segment (|x - P| <= R), n terms in any order:
        |err| <= n u n R / n + u |mean|  ->  tol = C (n u R + u |mean|).
      * variance = S2/n - (S1/n)^2 with S2 = sum (x - P)^2 = n (M2 + (mean - P)^2) <= n (M2 + R^2) and |S1/n| <= R:
        |err| <= C n u (M2 + 3 R^2).  (A pixel dropped or doubled moves it by about (d^2 - M2)/n.)
      * skewness / kurtosis from the second pass about the first pass's mean (error e = tol_mean):
        |dm2| <= C n u M2 + e^2,  |dm3| <= 3 e M2 + C n u A3,  |dm4| <= 4 e A3 + C n u M4,
        |dskew| <= |dm3| / M2^1.5 + 1.5 |skew| |dm2| / M2,  |dkurt| <= |dm4| / M2^2 + 2 (M4 / M2^2) |dm2| / M2.
    C = BOUND_C covers the handful of roundings per term and the reference's own (sequential float64) sums."""
    n = ref["n"].astype(np.float64)
    c = BOUND_C
    R = ref["max"].astype(np.float64) - ref["min"].astype(np.float64)
    mean, M2, A3, M4 = ref["mean"], ref["m2"], ref["abs_d3"], ref["m4"]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        t_mean = c * (n * U64 * R + U64 * np.abs(mean))
        t_var = c * n * U64 * (M2 + 3.0 * R * R)
        dm2 = c * n * U64 * M2 + t_mean ** 2
        dm3 = 3.0 * t_mean * M2 + c * n * U64 * A3
        dm4 = 4.0 * t_mean * A3 + c * n * U64 * M4
        t_skew = dm3 / M2 ** 1.5 + 1.5 * np.abs(ref["skewness"]) * dm2 / M2
        t_kurt = dm4 / M2 ** 2 + 2.0 * (M4 / M2 ** 2) * dm2 / M2
    return {"mean": t_mean, "variance": t_var, "skewness": t_skew, "kurtosis": t_kurt}


def compare(got, ref, tol, keys=("mean", "variance", "min", "max"), moments=False):
    """-> list of failure messages (empty = within the bars).  count, min and max must be equal; mean / variance /
    skewness / kurtosis within ``tol``; NaN patterns identical, except skewness / kurtosis at near-threshold pairs."""
    bad = []
    if not np.array_equal(np.asarray(got["count"]), ref["count"]):
        bad.append(f"count: {int(np.sum(np.asarray(got['count']) != ref['count']))} labels differ")
    keys = list(keys) + (["skewness", "kurtosis"] if moments else [])
    for k in keys:
        g, r = np.asarray(got[k]), ref[k]
        if g.shape != r.shape:
            bad.append(f"{k}: shape {g.shape} != {r.shape}")
            continue
        gn, rn = np.isnan(g), np.isnan(r)
        pat = gn != rn
        if k in ("skewness", "kurtosis"):
            pat &= ~ref["near_threshold"]
        if pat.any():
            bad.append(f"{k}: NaN pattern differs at {np.argwhere(pat)[:4].tolist()}")
        both = ~gn & ~rn
        if k in ("min", "max"):
            neq = both & (g.astype(np.float32) != r)
        else:
            with np.errstate(invalid="ignore"):
                neq = both & ~(np.abs(g.astype(np.float64) - r) <= tol[k])
        if neq.any():
            i = tuple(np.argwhere(neq)[0])
            extra = f" (tol {tol[k][i]:.3g})" if k in tol else ""
            bad.append(f"{k}: {int(neq.sum())} entries off, first {i}: got {g[i]!r} ref {r[i]!r}{extra}")
    return bad


def perturbations(raw, labels, ref, start_label=1, bands=None):
    """For the largest segment that is not constant, every band: the reference entry recomputed with its most distant
    pixel (from the mean) removed, and with it doubled.  -> list of (label index, band index, what, stats dict)."""
    C = raw.shape[2]
    bands = list(range(C)) if bands is None else list(bands)
    lab = np.asarray(labels).reshape(-1).astype(np.int64) - start_label
    flat = np.asarray(raw).reshape(-1, C)
    order = np.argsort(-ref["count"], kind="stable")
    for L in order[:64]:
        if ref["count"][L] < 2:
            break
        idx = np.nonzero(lab == L)[0]
        out = []
        for j, b in enumerate(bands):
            v = flat[idx, b].astype(np.float64)
            v = v[~np.isnan(v)]
            if v.size < 2 or v.min() == v.max():
                continue
            far = int(np.argmax(np.abs(v - ref["mean"][L, j])))
            out.append((int(L), j, "removed", segment_stats(np.delete(v, far))))
            out.append((int(L), j, "doubled", segment_stats(np.append(v, v[far]))))
        if out:
            return out
    return []


def assert_bars_detect_one_pixel(raw, labels, ref, tol, start_label=1, bands=None, moments=False):
    """The bars must reject a result that dropped or doubled one pixel in one band of the largest non-constant segment."""
    cases = perturbations(raw, labels, ref, start_label, bands)
    assert cases, "no non-constant segment to perturb"
    for L, j, what, st in cases:
        got = {k: (np.array(ref[k], copy=True) if isinstance(ref[k], np.ndarray) else ref[k]) for k in ref}
        for k in ("mean", "variance", "skewness", "kurtosis", "min", "max"):
            got[k][L, j] = st[k]
        assert compare(got, ref, tol, moments=moments), f"one pixel {what} in label {L} band {j} passes the bars"
