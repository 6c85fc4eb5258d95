#!/usr/bin/env python3
"""Golden vectors for the shape columns from scikit-image itself.

Run with the interpreter that holds scikit-image 0.18.3 (the conda python 3.9 of the build container), like the other generators:
    python3.9 tests/golden/gen_goldens_shapes.py
It reads the `labels` of three existing fixtures (SLIC label maps scikit-image produced) and records what
`skimage.measure.regionprops` says about every label present: area, bbox, centroid, inertia_tensor, inertia_tensor_eigvals,
eccentricity, orientation, major_axis_length, minor_axis_length and extent, one row per label in ascending label order, into
tests/golden/shapes/<fixture>.npz.  Data only; nothing of scikit-image is copied.  It also prints what was checked for those maps:
the smallest segment and whether any segment has equal eigenvalues (its orientation would be the isotropic +-pi/4).
"""
import os

import numpy as np
import skimage
from skimage.measure import regionprops

HERE = os.path.dirname(os.path.abspath(__file__))
MAPS = ("c2s_256x256x4_c025", "quickstart_128x128x3", "mask_128x160x4_c025")


def main():
    os.makedirs(os.path.join(HERE, "shapes"), exist_ok=True)
    for name in MAPS:
        labels = np.load(os.path.join(HERE, name + ".npz"))["labels"]
        props = regionprops(labels)
        out = {"label": np.array([p.label for p in props], np.int32),
               "area": np.array([p.area for p in props], np.int64),
               "bbox": np.array([p.bbox for p in props], np.int64),
               "centroid": np.array([p.centroid for p in props], np.float64),
               "inertia_tensor": np.array([p.inertia_tensor for p in props], np.float64),
               "inertia_tensor_eigvals": np.array([p.inertia_tensor_eigvals for p in props], np.float64),
               "eccentricity": np.array([p.eccentricity for p in props], np.float64),
               "orientation": np.array([p.orientation for p in props], np.float64),
               "major_axis_length": np.array([p.major_axis_length for p in props], np.float64),
               "minor_axis_length": np.array([p.minor_axis_length for p in props], np.float64),
               "extent": np.array([p.extent for p in props], np.float64)}
        np.savez_compressed(os.path.join(HERE, "shapes", name + ".npz"), skimage_version=skimage.__version__, numpy_version=np.__version__, **out)
        ev = out["inertia_tensor_eigvals"]
        print(f"wrote shapes/{name}.npz: {len(props)} segments, smallest {int(out['area'].min())} px, "
              f"equal eigenvalues: {int((ev[:, 0] == ev[:, 1]).sum())}, skimage {skimage.__version__}")


if __name__ == "__main__":
    main()
