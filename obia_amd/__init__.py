"""obia_amd -- MI355X-native tiled SLIC + per-segment zonal statistics, a drop-in for the hot path of
iosefa/obia (segment(method="slic"), create_tiled_segments).  See DESIGN.md / INTEGRATION.md."""
from .segmentation import slic, quickshift, create_segments, segments_table, segment, Segments, normalize_band  # noqa: F401
from .statistics import zonal_stats, create_objects, stats_columns  # noqa: F401
from .polygons import polygonize, rasterize, PolygonTable  # noqa: F401
from .cost import rasterise_slic_gpkg  # noqa: F401
from .geopackage import write_geopackage, read_geopackage  # noqa: F401
from .seeds import make_chm_seeds, make_density_seeds, make_canonical_seeds  # noqa: F401
from .seeds import canonical_seeds, sample_heights, stage1_clusters, stage1_rounds, reduce_stage1  # noqa: F401
from .seeds import split_clusters_by_height, trim_clusters, nms_per_crown  # noqa: F401
from .classify import classify, ClassifiedImage, Forest, standard_scale, forest_predict, acceptable_mask  # noqa: F401
from .classify import MLP, mlp_predict, predict_segments, forest_shap  # noqa: F401
from .classify import mlp_shap, mlp_coalition_values, shapley_combine  # noqa: F401
from . import training  # noqa: F401
from .training import tile_and_process, process_tile, TrainingTiles, gaussian_blur_u8, chamfer_distance  # noqa: F401
from . import crowns  # noqa: F401
from .crowns import cost_allocation, grow_crowns  # noqa: F401
from . import boxes  # noqa: F401
from .boxes import box_overlaps, assign_boxes, dissolve_by_box, box_iou, box_nms, BoxAssignment, BoxTable  # noqa: F401
from .boxes import predictions_to_map, save_predictions_to_gpkg, mosaic_predictions  # noqa: F401
from . import pointcloud  # noqa: F401
from .pointcloud import as_points, PointRasters, points_to_rasters, SegmentPoints, segment_point_stats  # noqa: F401
from .pointcloud import GroundIndex, height_above_ground, height_above_dtm, normalize_heights  # noqa: F401
from .pointcloud import grey_erosion, grey_dilation, grey_opening, pmf_schedule, GroundFilter, ground_filter, classify_ground  # noqa: F401
from . import adjacency  # noqa: F401
from .adjacency import SegmentGraph, segment_graph, compact_roots, relabel, merge_by_threshold, dissolve_by_class  # noqa: F401
from .adjacency import merge_similar, context_columns  # noqa: F401
from . import shapes  # noqa: F401
from .shapes import ShapeTable, segment_shapes, pair_shapes, shape_columns  # noqa: F401
from . import merging  # noqa: F401
from .merging import RegionState, fusion_cost, merge_pairs, merge_regions, multiresolution_merge  # noqa: F401

__version__ = "0.1.0"
