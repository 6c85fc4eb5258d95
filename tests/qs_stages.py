"""Stage-level comparison of quickshift (obia_quickshift_stages_f32_dev) with the oracle's float64 restatement
(oracle.quickshift_stages).  Shared by the GPU quickshift tests.

Both sides are float64, built without FMA contraction, and sum in the same order, so:
  Tier A (no Lab, sigma 0): the staged image is float64(normalised float32) * ratio on both sides, bit for bit; squared distances
         are then bitwise equal and densities differ only by device exp against glibc's (~1e-13 relative).  A parent can differ
         only where two densities tie to within that: the oracle's density-tie flag (bit 0) is the only one that counts.
  Tier B (Lab and / or sigma > 0): the staged image differs in the last bits (device pow / cbrt, the smoothing sums); every
         flag counts (bit 1 distance tie, bit 2 cut tie as well).
Where no pixel carries a counting flag the labels must be IDENTICAL.  Otherwise every pixel whose label differs must have a
flagged pixel on its path to the root, in the oracle's forest or the GPU's.
"""
import numpy as np

TAU = 1e-12
DENS_RTOL = 1e-12
STAGED_RTOL_B = 1e-13      # Tier B staged image: max |diff| relative to max |image|
COUNTING = {"A": 1, "B": 7}


def run_gpu(image, **kw):
    """obia_amd.segmentation._quickshift_stages on `image`, every output copied to the host (image as (H, W, C))."""
    from obia_amd.segmentation import _quickshift_stages
    g = _quickshift_stages(image, **kw)
    out = {k: v.cpu().numpy() for k, v in g.items() if k != "n_labels"}
    out["image"] = np.ascontiguousarray(np.moveaxis(out["image"], 0, -1))
    out["n_labels"] = g["n_labels"]
    return out


def oracle_image(oracle, img_f32, ratio, sigma, lab, normalize=False):
    """The image the reference's window kernel reads: normalise (float32), widen, Lab, smooth, `* ratio`."""
    x = oracle.normalize(img_f32) if normalize else np.asarray(img_f32, np.float32)
    x = x.astype(np.float64)
    if x.ndim == 2:
        x = x[..., None]
    if lab:
        x = oracle.rgb2lab_f64(x)
    return oracle.quickshift_smooth(x, sigma) * ratio


def cut(parent, dist_parent, max_dist):
    idx = np.arange(parent.size, dtype=np.int64).reshape(parent.shape)
    return np.where(dist_parent > max_dist, idx, parent.astype(np.int64))


def flatten(par):
    """Root of every pixel of a forest given as a flat parent array (pointer jumping)."""
    r = par.reshape(-1).copy()
    while True:
        nxt = r[r]
        if np.array_equal(nxt, r):
            return r.reshape(par.shape)
        r = nxt


def flagged_on_path(par, flagged):
    """For every pixel: does some pixel on its path to the root (itself and the root included) carry a flag?"""
    p = par.reshape(-1).copy()
    f = flagged.reshape(-1).copy()
    while True:
        f2 = f | f[p]
        p2 = p[p]
        if np.array_equal(p2, p) and np.array_equal(f2, f):
            return f.reshape(par.shape)
        p, f = p2, f2


def rank_labels(roots):
    idx = np.arange(roots.size).reshape(roots.shape)
    is_root = roots == idx
    rank = np.cumsum(is_root.reshape(-1)) - 1
    return rank[roots.reshape(-1)].reshape(roots.shape), int(is_root.sum())


def check(g, o, max_dist, tier, expect_flags=0, staged_ref=None, name=""):
    """Compare the GPU stages `g` (run_gpu) with the oracle's `o` (oracle.quickshift_stages on the same noise).
    staged_ref: the oracle-side staged image (H, W, C); Tier A demands bitwise equality, Tier B STAGED_RTOL_B.
    expect_flags: counting flag bits this case provokes on purpose; any other counting flag fails the test.
    Returns the number of pixels whose root differs (0 unless a counting flag is present; each one traced to a flag)."""
    count = COUNTING[tier]
    flags = o["flags"] & count
    stray = flags & np.uint8(~expect_flags & 0xff)
    assert not stray.any(), f"{name}: {int((stray != 0).sum())} pixels carry a near-tie flag this input should not have " \
                            f"(bits {sorted(set(np.unique(stray).tolist()) - {0})})"
    if staged_ref is not None:
        assert g["image"].shape == staged_ref.shape
        if tier == "A":
            nd = int((g["image"] != staged_ref).sum())
            assert nd == 0, f"{name}: staged image differs at {nd} values"
        else:
            err = np.abs(g["image"] - staged_ref).max() / max(np.abs(staged_ref).max(), 1e-300)
            assert err <= STAGED_RTOL_B, f"{name}: staged image off by {err:.3g} of its max"
    np.testing.assert_allclose(g["dens"], o["dens"], rtol=DENS_RTOL, atol=0, err_msg=f"{name}: density")
    tie = (o["flags"] & (1 if tier == "A" else 3)) != 0
    bad = (g["parent"] != o["parent"]) & ~tie
    assert not bad.any(), f"{name}: parent differs at {int(bad.sum())} untied pixels, first {np.argwhere(bad)[0].tolist()}"
    same = g["parent"] == o["parent"]
    if tier == "A":
        nd = int((g["dist_parent"][same] != o["dist_parent"][same]).sum())
        assert nd == 0, f"{name}: dist_parent differs bitwise at {nd} pixels with the same parent"
    else:
        np.testing.assert_allclose(g["dist_parent"][same], o["dist_parent"][same], rtol=DENS_RTOL, atol=0,
                                   err_msg=f"{name}: dist_parent")
    # the GPU's own forest: roots are the flattening of its cut parents, labels the rank of the root among the roots
    gcut = cut(g["parent"], g["dist_parent"], max_dist)
    assert np.array_equal(g["roots"], flatten(gcut)), f"{name}: roots are not the flattened forest of the parents"
    lab, n = rank_labels(g["roots"])
    assert np.array_equal(g["labels"], lab) and g["n_labels"] == n, f"{name}: labels are not the rank of the root"
    if not flags.any():
        nd = int((g["labels"] != o["labels"]).sum())
        assert nd == 0 and np.array_equal(g["roots"], o["roots"]), f"{name}: {nd} labels differ with no counting near-tie"
        return 0
    # a root more or less renumbers every later segment: compare the partitions through the roots
    diff = g["roots"] != o["roots"]
    nd = int(diff.sum())
    ocut = cut(o["parent"], o["dist_parent"], max_dist)
    excused = flagged_on_path(ocut, flags != 0) | flagged_on_path(gcut, flags != 0)
    unexplained = diff & ~excused
    assert not unexplained.any(), f"{name}: {int(unexplained.sum())} of {nd} differing labels trace to no near-tie"
    return nd
