"""Goldens of the box filter: ``scipy.ndimage.uniform_filter(plane, size=win)`` on float32 planes, SciPy 1.15.3 (recorded in every
file).  Run once where SciPy is installed; the tests only read the files.

    python tests/golden/gen_goldens_sharpness.py

tests/golden/sharpness/<data>_<H>x<W>.npz holds ``plane`` (float32), ``wins`` and one ``out_<win>`` per window.  Data sets:
  n50   standard_normal * 50: every summation order gives the same bits (the double sums are exact);
  wide  standard_normal * 10.0 ** randint(-12, 13): the running sum's bits depend on SciPy's serial order -- summing every window
        directly in double on both axes differs from SciPy at 206 of 8710 pixels for win = 3 and at 60 for win = 4 on the 67 x 130 plane.
The largest plane (130 x 517: more rows than a workgroup's band of 64, more columns than two LDS chunks of 64) would be 270 kB per
output, so its files hold SHA-256 digests instead: ``sha_plane`` of the plane, which tests/sharpness_restatement.golden_plane makes
again from its seed, and ``sha_<win>`` of each output's bytes."""
import hashlib
import os
import sys

import numpy as np
import scipy
from scipy.ndimage import uniform_filter

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sharpness")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.sharpness_restatement import golden_plane as plane_of  # noqa: E402

SMALL = [(1, 1), (1, 9), (9, 1), (2, 2), (7, 13), (9, 4), (33, 17)]
WINS = [1, 2, 3, 4, 15]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def save(data, shape, wins, digest_only=False):
    plane = plane_of(data, shape)
    rec = {"sha_plane": sha(plane), "wins": np.array(wins, np.int64), "scipy_version": scipy.__version__, "numpy_version": np.__version__}
    if not digest_only:
        rec["plane"] = plane
    for w in wins:
        out = uniform_filter(plane, size=w)
        assert out.dtype == np.float32 and out.shape == plane.shape
        if digest_only:
            rec[f"sha_{w}"] = sha(out)
        else:
            rec[f"out_{w}"] = out
    np.savez_compressed(os.path.join(HERE, f"{data}_{shape[0]}x{shape[1]}.npz"), **rec)


def main():
    os.makedirs(HERE, exist_ok=True)
    for shape in SMALL:
        save("n50", shape, WINS + [2 * max(shape) + 12])            # the last window: longer than twice the longer side
    save("wide", (7, 13), [3, 4])
    save("wide", (33, 17), [2, 3, 4, 15, 80])
    save("n50", (67, 130), [2, 15, 300])
    save("wide", (67, 130), [3, 4])
    save("n50", (130, 517), [4, 15], digest_only=True)
    save("wide", (130, 517), [3], digest_only=True)


if __name__ == "__main__":
    main()
