#!/opt/conda/bin/python3.9
"""Golden vectors for the boundary overlay from scikit-image 0.18.3.

Run ONLY in the build container:   /opt/conda/bin/python3.9 tests/golden/gen_goldens_boundaries.py
It calls skimage.segmentation.find_boundaries(mode="outer") and mark_boundaries -- what
obia.segmentation.segment.Segments.to_segmented_image calls (segment.py:49-53) -- and writes small .npz fixtures under
tests/golden/boundaries/: the int32 label map, the uint8 image (RGB or grey), the boundary raster and
(mark_boundaries(image, labels) * 255).astype(uint8).  Data only; nothing of scikit-image or the reference is copied.
"""
import os

import numpy as np
import skimage
from skimage.segmentation import find_boundaries, mark_boundaries

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "boundaries")


def blocks(H, W, rs):
    """jagged blocks 1.., a background (0) lake and strip, a masked (-1) corner and hole, one-pixel regions, diagonal contacts"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    lab = ((yy // 6) * 7 + (xx + 2 * np.sin(yy / 2.0)) // 5 + 1).astype(np.int32)
    lab[3:9, 4:11] = 0
    lab[H - 2:, :] = 0                      # background along the bottom border
    lab[:5, W - 6:] = -1                    # masked corner touching two borders
    lab[12:15, 15:19] = -1                  # masked hole next to background
    lab[12:15, 19:22] = 0
    lab[0, 0] = 900                         # one-pixel regions: a corner, the interior, inside background, inside the mask
    lab[10, 13] = 901
    lab[5, 7] = 902
    lab[13, 16] = 903
    for i in range(5):                      # a diagonal line of one-pixel contacts
        lab[16 + i, 3 + i] = 950
    lab[17, 3] = 0                          # background touching the diagonal only across a corner
    return lab


def checker(H, W):
    """every pixel its own neighbour's opposite: labels 0 / 5 / -1 in a diagonal pattern"""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.choose((yy + xx) % 3, [0, 5, -1]).astype(np.int32)


def cases():
    rs = np.random.RandomState(7)
    out = {}
    lab = blocks(24, 31, rs)
    out["blocks_rgb_24x31"] = (lab, rs.randint(0, 256, (24, 31, 3)).astype(np.uint8))
    out["blocks_grey_24x31"] = (lab, rs.randint(0, 256, (24, 31)).astype(np.uint8))
    out["checker_grey_9x13"] = (checker(9, 13), rs.randint(0, 256, (9, 13)).astype(np.uint8))
    # an image holding all 256 values in every channel, over two regions and background
    allv = np.arange(256, dtype=np.uint8).reshape(16, 16)
    lab = np.ones((16, 16), np.int32)
    lab[:, 9:] = 2
    lab[6:9, 6:12] = 0
    out["allvalues_rgb_16x16"] = (lab, np.stack([allv, allv[::-1], allv.T], axis=-1).copy())
    out["allvalues_grey_16x16"] = (lab, allv.copy())
    out["row_rgb_1x7"] = (np.array([[1, 1, 0, 2, 2, -1, 3]], np.int32), rs.randint(0, 256, (1, 7, 3)).astype(np.uint8))
    out["column_grey_6x1"] = (np.array([[4], [4], [-1], [0], [0], [7]], np.int32), rs.randint(0, 256, (6, 1)).astype(np.uint8))
    out["single_rgb_1x1"] = (np.array([[3]], np.int32), rs.randint(0, 256, (1, 1, 3)).astype(np.uint8))
    out["flat_rgb_5x6"] = (np.full((5, 6), 2, np.int32), rs.randint(0, 256, (5, 6, 3)).astype(np.uint8))
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, (lab, img) in cases().items():
        bnd = find_boundaries(lab, mode="outer").astype(np.uint8)
        marked = (mark_boundaries(img, lab) * 255).astype(np.uint8)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), labels=lab, image=img, boundaries=bnd, marked=marked,
                            skimage_version=skimage.__version__)
        print("wrote", name, lab.shape, "boundary pixels", int(bnd.sum()), "skimage", skimage.__version__)


if __name__ == "__main__":
    main()
