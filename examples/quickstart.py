#!/usr/bin/env python3
"""End-to-end walk through the replaced path on one small raster, with the reference's function names:

    segment()                -> label raster + per-segment objects table      (obia.segmentation.segment, segment.py:63-93)
    Segments.polygons()      -> polygons in map coordinates                   (create_segments back half, :59-77)
    create_tiled_segments()  -> the same for a raster that is processed in tiles (obia.utils.tiling, :62-291)
    slic_edge(), label_segments() -> the consumers of the label raster       (utils/cost.py:44-48, utils/utils.py:12-34)
    make_chm_seeds() ... grow_crowns() -> seeds, cost surface, one crown per canonical cluster (utils/seeds.py, utils/cost.py; the
                                crowns are this package's own: the reference has no consumer of the two)
    box_nms(), assign_boxes(), dissolve_by_box() -> superpixels joined with tree boxes (notebooks/deepfor2.ipynb, assign_fid)
    points_to_rasters(), create_objects(pointcloud=) -> CHM and density from points, the point-cloud columns (segment_statistics.py:332-389)
    normalize_heights()      -> heights above ground from raw elevations     (main.py:26, read_lidar(..., hag=True))
    classify_ground()        -> the ground class of an unclassified cloud     (the host run of PDAL before main.py)
    classify()               -> class and margin per segment, class raster    (obia.classification.classify, classify.py:68-175)

Needs an MI355X (there is no CPU path).  Writes quickstart_objects.csv, quickstart_segments.geojson and segments.gpkg next to itself.
    python examples/quickstart.py
"""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from obia_amd import segment, create_objects                       # noqa: E402
from obia_amd.tiling import create_tiled_segments                  # noqa: E402
from obia_amd.consumers import slic_edge, label_segments           # noqa: E402
from obia_amd.polygons import polygonize                           # noqa: E402
from obia_amd.cost import rasterise_slic_gpkg                      # noqa: E402
from obia_amd.classify import classify                             # noqa: E402
from obia_amd.cost import chm_gradient                             # noqa: E402
from obia_amd import make_chm_seeds, make_density_seeds, make_canonical_seeds, canonical_seeds, grow_crowns   # noqa: E402
from obia_amd import box_nms, assign_boxes, dissolve_by_box        # noqa: E402
from obia_amd import points_to_rasters                             # noqa: E402
from obia_amd.pointcloud import classify_ground, normalize_heights  # noqa: E402


class Image:
    """The two attributes of obia.handlers.geotif.Image that the path reads."""

    def __init__(self, img_data, affine_transformation):
        self.img_data = img_data
        self.affine_transformation = affine_transformation       # [a, b, d, e, xoff, yoff], shapely order


def main():
    rs = np.random.RandomState(0)
    H, W, C = 600, 800, 4
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    data = np.stack([400 * np.sin(xx / (11 + 3 * c)) * np.cos(yy / (13 + 2 * c)) + 1000 + 50 * c + rs.normal(0, 20, (H, W))
                     for c in range(C)], -1).astype(np.float32)
    image = Image(data, [0.5, 0.0, 0.0, -0.5, 300000.0, 2200000.0])           # 0.5 m pixels, north up

    # 1. one raster: SLIC + connectivity + statistics (mean / variance / min / max / skewness / kurtosis per band)
    seg = segment(image, segmentation_bands=[0, 1, 2, 3], statistics_bands=[0, 1, 2, 3], method="slic",
                  n_segments=1500, compactness=0.25)
    print(f"segment(): {int(seg._segments.max())} segments, objects table {seg.segments.shape}")
    seg.segments.to_csv(os.path.join(os.path.dirname(__file__), "quickstart_objects.csv"), index=False)

    # 2. polygons in map coordinates, ids 1..N like the reference's GeoDataFrame
    polys = seg.polygons(image.affine_transformation)
    with open(os.path.join(os.path.dirname(__file__), "quickstart_segments.geojson"), "w") as f:
        json.dump({"type": "FeatureCollection", "features": polys.geojson_features()}, f)
    print(f"polygons(): {len(polys)} polygons, {len(polys.xy)} vertices")

    # 3. the tiled driver (checkerboard tiles with overlap), then texture columns for one band
    mask = np.ones((H, W), np.uint8)
    mask[:40, :60] = 0
    here = os.path.dirname(os.path.abspath(__file__))
    labels, n = create_tiled_segments(data, output_dir=here, input_mask=mask, tile_size=256, buffer=32, crown_radius=5,
                                      pixel_size=(0.5, 0.5), affine_transformation=image.affine_transformation, compactness=0.25)
    # ... which wrote segments.gpkg like the reference; the way back to the label raster (what make_cost_surface(slic=...) takes)
    profile = {"height": H, "width": W, "transform": (0.5, 0.0, 300000.0, 0.0, -0.5, 2200000.0)}      # rasterio order
    assert np.array_equal(rasterise_slic_gpkg(os.path.join(here, "segments.gpkg"), profile), labels)
    table = create_objects(labels, image, spectral_bands=[0], textural_bands=[0], calculate_textural=True)
    print(f"create_tiled_segments(): {n} segments; create_objects(): columns {list(table.columns)[:5]} ...")

    # 4. consumers of the label raster
    edges = slic_edge(labels)
    pts = [(300000.0 + 0.5 * 400.5, 2200000.0 - 0.5 * 300.5), (300000.0 + 0.5 * 10.5, 2200000.0 - 0.5 * 10.5)]
    labelled, mixed = label_segments(labels, image.affine_transformation, pts, ["canopy", "masked corner"])
    print(f"slic_edge(): {100 * float(edges.mean()):.1f} % edge pixels; label_segments(): {labelled}, mixed {mixed}")
    assert len(polygonize(labels, start_label=1)) == n

    # 5. crowns: tree tops of a canopy height model and of a point density, the cost surface, the cost-aware merge of the seeds, and
    #    then every canopy pixel to the cluster it is cheapest to reach.  Crown ids are 1..N; the raster goes where `labels` went.
    chm = np.zeros((H, W))
    for cy in range(12, H, 24):
        for cx in range(12, W, 24):
            chm = np.maximum(chm, rs.uniform(6, 20) * np.exp(-((yy - cy - rs.uniform(-4, 4)) ** 2 + (xx - cx - rs.uniform(-4, 4)) ** 2)
                                                               / (2 * rs.uniform(3, 6) ** 2)))
    chm = chm.astype(np.float32)
    chm_seeds = make_chm_seeds(chm, affine_transformation=image.affine_transformation)
    den_seeds = make_density_seeds(1.5 * chm, affine_transformation=image.affine_transformation)
    cost = chm_gradient(chm).astype(np.float32)                              # one layer of make_cost_surface; the whole surface works alike
    seeds = make_canonical_seeds(chm_seeds, den_seeds, cost, cost_affine=image.affine_transformation, debug_dist=False)
    crowns = grow_crowns(cost, seeds, mask=chm > 2.0, cost_affine=image.affine_transformation, max_dist=10.0)      # at most 10 m from a seed
    crown_table = create_objects(crowns, image, calculate_textural=False, geometry=False)
    print(f"grow_crowns(): {len(seeds['x'])} seeds in {int(crowns.max())} crowns over {100 * float((crowns > 0).mean()):.0f} % of the raster; "
          f"{len(polygonize(crowns, image.affine_transformation, start_label=1))} polygons, objects table {crown_table.shape}")
    # the table options make_canonical_seeds refuses: a cluster whose heights spread more than 3 m is split at its median, and a seed
    # within 1.5 m of a later (lower) one of its cluster is dropped
    split = canonical_seeds(chm_seeds, den_seeds, cost, cost_affine=image.affine_transformation, debug_dist=False, dz_merge=3.0, nms_base=1.5)
    more = grow_crowns(cost, split, mask=chm > 2.0, cost_affine=image.affine_transformation, max_dist=10.0)
    print(f"canonical_seeds(dz_merge=3, nms_base=1.5): {len(split['x'])} seeds in {len(np.unique(split['cluster']))} clusters, "
          f"{int(more.max())} crowns")

    # 5b. the other way to crowns, the reference author's: tree boxes (here 6 m squares around the tree tops, in place of a detector's
    #     predictions), the copies suppressed, every superpixel to the box it shares the most area with, one crown per box
    sx, sy = np.asarray(chm_seeds["x"]), np.asarray(chm_seeds["y"])
    tree_boxes = np.stack([sx - 3.0, sy - 3.0, sx + 3.0, sy + 3.0], 1)                 # map bounds (minx, miny, maxx, maxy)
    _, kept = box_nms(tree_boxes, np.asarray(chm_seeds["ch_max"]), 0.15)
    fid = assign_boxes(labels, image.affine_transformation, tree_boxes[kept], n_labels=n)
    box_crowns = dissolve_by_box(labels, fid.assigned)
    print(f"assign_boxes(): {len(kept)} of {len(tree_boxes)} boxes after box_nms, {int((fid.assigned >= 0).sum())} of {n} segments in a box, "
          f"{len(polygonize(box_crowns, image.affine_transformation, start_label=1))} crowns")

    # 5c. the LiDAR leg: a synthetic cloud (ten returns per square metre under the canopy surface above) -> the CHM and the density
    #     raster the seeds start from, and the five point-cloud columns of the objects table, one height profile per crown
    n_pts = 10 * (H // 2) * (W // 2)
    pc, pr = rs.uniform(0, W, n_pts), rs.uniform(0, H, n_pts)
    cloud = {"X": 300000.0 + 0.5 * pc, "Y": 2200000.0 - 0.5 * pr,
             "HeightAboveGround": (chm[pr.astype(int), pc.astype(int)] * rs.beta(2.0, 1.0, n_pts)).astype(np.float32),
             "Intensity": rs.randint(0, 4096, n_pts).astype(np.uint16)}
    rasters = points_to_rasters(cloud, image.affine_transformation, (H, W))
    lidar_seeds = make_chm_seeds(rasters["chm"], affine_transformation=image.affine_transformation)
    lidar_table = create_objects(crowns, image, voxel_resolution=(0.5, 0.5, 0.5), calculate_textural=False, calculate_structural=True,
                                 calculate_radiometric=True, pointcloud=cloud, geometry=False)
    print(f"points_to_rasters(): {n_pts} points, {int(np.isfinite(rasters['chm']).sum())} CHM pixels, {len(lidar_seeds['id'])} tree tops; "
          f"create_objects(pointcloud=): median ch {float(lidar_table['ch'].median()):.1f} m, pai {float(lidar_table['pai'].median()):.2f}, "
          f"fhd {float(lidar_table['fhd'].median()):.2f}, mean intensity {float(lidar_table['mean_intensity'].median()):.0f}")

    # 5d. the same cloud as a LAS tile delivers it -- elevations and a ground class, no heights: normalize_heights() finds the ground
    #     under every point (main.py:26, read_lidar(..., hag=True)) and hands on the cloud that points_to_rasters() takes
    terrain = 120.0 + 0.02 * (cloud["X"] - 300000.0) + 3.0 * np.sin((cloud["Y"] - 2200000.0) / 40.0)
    is_ground = cloud["HeightAboveGround"] < 0.3
    raw = {"X": cloud["X"], "Y": cloud["Y"], "Z": terrain + np.where(is_ground, 0.0, cloud["HeightAboveGround"]),
           "Classification": np.where(is_ground, 2, 5).astype(np.uint8), "Intensity": cloud["Intensity"]}
    normalized = normalize_heights(raw, count=3, max_distance=10.0)
    raw_rasters = points_to_rasters(normalized, image.affine_transformation, (H, W))
    print(f"normalize_heights(): {int(is_ground.sum())} ground points, median height {float(np.nanmedian(normalized['HeightAboveGround'])):.1f} m, "
          f"{int(np.isfinite(raw_rasters['chm']).sum())} CHM pixels")

    # 5e. ... and as a drone delivers it -- no ground class at all: classify_ground() finds the ground points with a progressive
    #     morphological filter, and normalize_heights() goes on from there
    unclassified = {k: v for k, v in raw.items() if k != "Classification"}
    found = classify_ground(unclassified, cell_size=1.0)
    renormalized = normalize_heights(found, count=3, max_distance=10.0)
    agree = float(((found["Classification"] == 2) == is_ground).mean())
    print(f"classify_ground(): {int((found['Classification'] == 2).sum())} ground points found, {100 * agree:.1f} % of the points as labelled above, "
          f"median height {float(np.nanmedian(renormalized['HeightAboveGround'])):.1f} m")

    # 6. classification (needs scikit-learn for the training): label segments from points, train on them, predict every segment
    try:
        import sklearn  # noqa: F401
    except ImportError:
        print("classify(): skipped, scikit-learn is not installed")
        return
    py, px = np.mgrid[5:H:20, 5:W:20]
    pts = np.stack([300000.0 + 0.5 * (px.ravel() + 0.5), 2200000.0 - 0.5 * (py.ravel() + 0.5)], 1)
    classes = np.digitize(data[py.ravel(), px.ravel(), 0], [900, 1100]) + 1            # three classes from band 0
    labelled, _ = label_segments(labels, image.affine_transformation, pts, classes)
    objects = create_objects(labels, image, calculate_textural=False, geometry=False)
    training = objects[objects["segment_id"].isin(list(labelled))].copy()
    training["feature_class"] = [labelled[int(s)] for s in training["segment_id"]]
    result = classify(objects, training, n_estimators=50, random_state=0)
    class_raster = result.to_raster(labels)
    print(f"classify(): {len(training)} training segments, classes {sorted(set(result.classified['predicted_class']))}, "
          f"mean margin {float(result.classified['prediction_margin'].mean()):.2f}, class raster {class_raster.shape}")


if __name__ == "__main__":
    main()
