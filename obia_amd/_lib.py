"""ctypes binding of libobia_hip.so.  The C ABI is the headers of include/; BINDINGS below holds one table of entry points per header,
and load() binds them all.

There is NO CPU fallback: if the HIP library is missing or no GPU is present the operators raise.
"""
import ctypes
import os
import subprocess

import numpy as np

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# OBIA_HIP_LIB: developer override used by kernel experiments (tools/build_variant.sh); still a HIP build of this library
LIB_PATH = os.environ.get("OBIA_HIP_LIB") or os.path.join(_CSRC, "libobia_hip.so")

OBIA_OK = 0
MASK_SEEDS_CHUNK = 1024   # OBIA_MASK_SEEDS_CHUNK (include/obia_hip.h): centroids the seeding kernels stage in LDS at a time
E_INVALID, E_HIP, E_NOMEM, E_UNSUPPORTED, E_EMPTY, E_NONFINITE = -1, -2, -3, -4, -5, -6
E_INTERNAL = -7           # OBIA_E_INTERNAL (include/obia_crowns.h): a proven bound was exceeded; check() raises RuntimeError


class SlicParams(ctypes.Structure):
    """obia_slic_params (include/obia_hip.h)."""
    _fields_ = [("compactness", ctypes.c_double), ("min_size_factor", ctypes.c_double),
                ("max_size_factor", ctypes.c_double), ("n_segments", ctypes.c_int32),
                ("max_num_iter", ctypes.c_int32), ("convert2lab", ctypes.c_int32),
                ("enforce_connectivity", ctypes.c_int32), ("slic_zero", ctypes.c_int32),
                ("start_label", ctypes.c_int32), ("normalize_bands", ctypes.c_int32),
                ("exit_on_fixed_point", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("sigma_zyx", ctypes.c_double * 3), ("spacing_zyx", ctypes.c_double * 3)]


class SlicSeeds(ctypes.Structure):
    """obia_slic_seeds (include/obia_hip.h): caller-supplied initial centroids."""
    _fields_ = [("yx", ctypes.c_void_p), ("steps_zyx", ctypes.c_double * 3), ("n", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class SlicStages(ctypes.Structure):
    """obia_slic_stages (include/obia_hip.h): stage outputs of obia_slic_stages_f32_dev."""
    _fields_ = [("features", ctypes.c_void_p), ("seeds_yx", ctypes.c_void_p), ("centroids", ctypes.c_void_p),
                ("labels_pre", ctypes.c_void_p), ("centroid_capacity", ctypes.c_int32), ("prepass_only", ctypes.c_int32),
                ("prepass_iters", ctypes.c_int32), ("K", ctypes.c_int32), ("step", ctypes.c_double), ("prescale", ctypes.c_double),
                ("fscale", ctypes.c_double)]


class TilingParams(ctypes.Structure):
    """obia_tiling_params (include/obia_hip.h)."""
    _fields_ = [("crown_radius", ctypes.c_double), ("pixel_width", ctypes.c_double),
                ("pixel_height", ctypes.c_double), ("tile_size", ctypes.c_int32), ("buffer", ctypes.c_int32),
                ("white_order", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Forest(ctypes.Structure):
    """obia_forest (include/obia_hip.h): the flat node arrays of a tree ensemble."""
    _fields_ = [("threshold", ctypes.c_void_p), ("feature", ctypes.c_void_p), ("left", ctypes.c_void_p), ("right", ctypes.c_void_p),
                ("missing_go_to_left", ctypes.c_void_p), ("tree_offset", ctypes.c_void_p), ("tree_offset_host", ctypes.c_void_p),
                ("value", ctypes.c_void_p), ("n_nodes", ctypes.c_int64), ("n_trees", ctypes.c_int32), ("n_classes", ctypes.c_int32)]


class Mlp(ctypes.Structure):
    """obia_mlp (include/obia_hip.h): the flat weights and biases of a multi-layer perceptron."""
    _fields_ = [("weights", ctypes.c_void_p), ("biases", ctypes.c_void_p), ("layer_sizes", ctypes.c_void_p), ("n_layers", ctypes.c_int32),
                ("hidden_activation", ctypes.c_int32), ("out_activation", ctypes.c_int32), ("n_classes", ctypes.c_int32)]


_P = ctypes.c_void_p
_I = ctypes.c_int
SEEDING_GRID, SEEDING_SKIMAGE = 0, 1   # OBIA_SEEDING_* (include/obia_hip.h)
# obia_pick_fn: (user, n_valid, n_segments, &idx, &n_idx, &dense, &n_dense) -> 0
PickFn = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p),
                          ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64))
_SIGNATURES = {
    "obia_abi_version": (ctypes.c_int, []),
    "obia_last_error": (ctypes.c_char_p, []),
    "obia_create": (_P, [_I]),
    "obia_create_on_stream": (_P, [_I, _P]),
    "obia_destroy": (None, [_P]),
    "obia_synchronize": (_I, [_P]),
    "obia_workspace_bytes": (ctypes.c_int64, [_P]),
    "obia_slic_default_params": (None, [ctypes.POINTER(SlicParams)]),
    "obia_slic_f32": (_I, [_P, _P, _I, _I, _I, _P, ctypes.POINTER(SlicParams), _P, ctypes.POINTER(_I)]),
    "obia_slic_f32_dev": (_I, [_P, _P, _I, _I, _I, _P, ctypes.POINTER(SlicParams), _P, ctypes.POINTER(_I)]),
    "obia_slic_assign_only_f32_dev": (_I, [_P, _P, _I, _I, _I, _P, ctypes.POINTER(SlicParams), _P, ctypes.POINTER(_I)]),
    "obia_slic_seeded_f32_dev": (_I, [_P, _P, _I, _I, _I, _P, ctypes.POINTER(SlicParams), ctypes.POINTER(SlicSeeds), _I, _P,
                                      ctypes.POINTER(_I)]),
    "obia_mask_centroids_dev": (_I, [_P, _P, _I, _I, _P, ctypes.c_int32, _P, ctypes.c_int64, _I, _P, _P]),
    "obia_slic_stages_f32_dev": (_I, [_P, _P, _I, _I, _I, _P, ctypes.POINTER(SlicParams), ctypes.POINTER(SlicSeeds),
                                      ctypes.POINTER(SlicStages)]),
    "obia_enforce_connectivity_i32_dev": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, ctypes.POINTER(_I)]),
    "obia_zonal_stats_f32": (_I, [_P, _P, _P, _I, _I, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "obia_zonal_stats_f32_dev": (_I, [_P, _P, _P, _I, _I, _I, _P, _I, _I, _I, _P, _P, _P, _P, _P]),
    "obia_zonal_moments_f32_dev": (_I, [_P, _P, _P, _I, _I, _I, _P, _I, _I, _I, _P, _P, _P, _P]),
    "obia_zonal_moments_f32": (_I, [_P, _P, _P, _I, _I, _I, _P, _I, _I, _I, _P, _P, _P]),
    "obia_texture_stats_f32_dev": (_I, [_P, _P, _P, _I, _I, _I, _P, _I, _I, _I, _P]),
    "obia_label_edges_u8_dev": (_I, [_P, _P, _I, _I, _P, _P]),
    "obia_sample_labels_i32_dev": (_I, [_P, _P, _I, _I, _P, _P, ctypes.c_int64, _I, _P]),
    "obia_cost_bands_f32_dev": (_I, [_P, _P, ctypes.c_int64, _P, _P]),
    "obia_cost_ndvi_f32_dev": (_I, [_P, _P, _P, ctypes.c_int64, _P]),
    "obia_cost_sobel_f32_dev": (_I, [_P, _P, _I, _I, _P]),
    "obia_cost_select_dev": (_I, [_P, _P, _I, ctypes.c_int64, ctypes.c_double, ctypes.c_double, _P, _P]),
    "obia_cost_entropy_f32_dev": (_I, [_P, _P, _I, _I, ctypes.c_double, ctypes.c_double, _P, _P]),
    "obia_cost_normalise_dev": (_I, [_P, _P, _I, ctypes.c_int64, ctypes.c_double, ctypes.c_double, _P]),
    "obia_cost_edge_count_dev": (_I, [_P, _P, _I, _I, _P]),
    "obia_cost_combine_dev": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "obia_seeds_peaks_dev": (_I, [_P, _P, _I, _I, ctypes.c_double, _I, ctypes.c_float, _P, _P, _P, _P]),
    "obia_seeds_peaks_gather_dev": (_I, [_P, _P, _P, _P, _P, _I, _I, ctypes.c_int64, _P, _P, _P, _P]),
    "obia_seeds_pair_link_dev": (_I, [_P, _P, _P, _I, _P, _I, _I, _P, ctypes.c_double, ctypes.c_double, _I, _P, ctypes.c_double, _I, _P,
                                      ctypes.POINTER(_I)]),
    "obia_seeds_pair_stats_dev": (_I, [_P, _P, _P, _I, _P, _I, _I, _P, ctypes.c_double, ctypes.c_double, _I, _P, _P, _P]),
    "obia_seeds_pair_matrix_dev": (_I, [_P, _P, _P, _I, _P, _I, _I, _P, ctypes.c_double, ctypes.c_double, _I, _P, _P]),
    "obia_polygon_count_i32_dev": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "obia_polygon_rings_i32_dev": (_I, [_P, _P, _I, _I, _I, ctypes.c_int64, ctypes.c_int64, _P, _P, _P, _P, _P, _P]),
    "obia_rasterize_polygons_dev": (_I, [_P, _P, _P, ctypes.c_int64, _P, _P, ctypes.c_int64, _I, _I, ctypes.c_int32, _P]),
    "obia_rasterize_info": (_I, [ctypes.POINTER(ctypes.c_int64)]),
    "obia_quickshift_f32": (_I, [_P, _P, _I, _I, _I, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _I, _P, _I, _P, ctypes.POINTER(_I)]),
    "obia_quickshift_f32_dev": (_I, [_P, _P, _I, _I, _I, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _I, _P, _I, _P, ctypes.POINTER(_I)]),
    "obia_quickshift_stages_f32_dev": (_I, [_P, _P, _I, _I, _I, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double, _I, _P, _I, _P,
                                            ctypes.POINTER(_I), _P, _P, _P, _P, _P, _P]),
    "obia_tiled_slic_f32_dev": (_I, [_P, _P, _P, _I, _I, _I, ctypes.POINTER(TilingParams), ctypes.POINTER(SlicParams), _P,
                                     ctypes.POINTER(ctypes.c_int64)]),
    "obia_tiled_slic_f32": (_I, [_P, _P, _P, _I, _I, _I, ctypes.POINTER(TilingParams), ctypes.POINTER(SlicParams), _P,
                                 ctypes.POINTER(ctypes.c_int64)]),
    "obia_tiled_slic_seeded_f32_dev": (_I, [_P, _P, _P, _I, _I, _I, ctypes.POINTER(TilingParams), ctypes.POINTER(SlicParams), _I, PickFn, _P,
                                            _P, ctypes.POINTER(ctypes.c_int64)]),
    "obia_tiled_slic_seeded_f32": (_I, [_P, _P, _P, _I, _I, _I, ctypes.POINTER(TilingParams), ctypes.POINTER(SlicParams), _I, PickFn, _P,
                                        _P, ctypes.POINTER(ctypes.c_int64)]),
    "obia_tiler_set_seeding": (_I, [_P, _I, PickFn, _P]),
    "obia_tiler_create": (_P, [_P, _P, _P, _I, _I, _I, _I, _I, ctypes.POINTER(TilingParams), ctypes.POINTER(SlicParams), _P, _I]),
    "obia_tiler_destroy": (None, [_P]),
    "obia_tiler_run": (_I, [_P, _I, _I, _I, _I]),
    "obia_tiler_next_id": (_I, [_P]),
    "obia_tiler_set_segments": (_I, [_P, _I, _I, _P]),
    "obia_tiler_get_alive": (_I, [_P, _P, _I]),
    "obia_tiler_set_alive": (_I, [_P, _P, _I]),
    "obia_tiler_finalize": (_I, [_P, ctypes.POINTER(ctypes.c_int64)]),
    "obia_tiler_import_seam": (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                    ctypes.POINTER(ctypes.c_int)]),
    "obia_table_scale_dev": (_I, [_P, _P, ctypes.c_int64, _I, _P, _P, _P]),
    "obia_forest_predict_dev": (_I, [_P, _P, ctypes.c_int64, _I, ctypes.POINTER(Forest), _P, _P, _P, _P]),
    "obia_mlp_predict_dev": (_I, [_P, _P, ctypes.c_int64, _I, ctypes.POINTER(Mlp), _P, _P, _P, _P, _P]),
    "obia_table_scale_f64_dev": (_I, [_P, _P, ctypes.c_int64, _I, _P, _P, _P]),
    "obia_forest_shap_dev": (_I, [_P, _P, ctypes.c_int64, _I, ctypes.POINTER(Forest), _P, _P, _P]),
    "obia_mlp_coalition_dev": (_I, [_P, _P, ctypes.c_int64, _I, ctypes.POINTER(Mlp), _P, ctypes.c_int64, _P, ctypes.c_int64, _P]),
    "obia_shapley_combine_dev": (_I, [_P, _P, ctypes.c_int64, _I, _I, _P, _P]),
    "obia_set_profiling": (_I, [_P, _I]),
    "obia_last_timing": (ctypes.c_double, [_P, _I]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)   # the names of include/obia_hip.h
# include/obia_image.h: the image previews
_IMAGE_SIGNATURES = {
    "obia_image_stretch_u8_dev": (_I, [_P, _P, _I, ctypes.c_int64, ctypes.c_double, ctypes.c_double, _P]),
    "obia_image_gray_hist_dev": (_I, [_P, _P, _I, ctypes.c_int64, _P, _P]),
    "obia_image_lut_u8_dev": (_I, [_P, _P, ctypes.c_int64, _P, _I, _P]),
    "obia_image_clahe_u8_dev": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "obia_image_boundaries_dev": (_I, [_P, _P, _I, _I, _P]),
    "obia_image_mark_u8_dev": (_I, [_P, _P, _I, _P, _I, _I, _P, _P, _P]),
}
# include/obia_sharpness.h: the sharpness raster
SHARP_MAX_WIN = 65536     # OBIA_SHARP_MAX_WIN: the largest `win`
_SHARPNESS_SIGNATURES = {
    "obia_sharp_gray_lap_dev": (_I, [_P, _P, _I, _I, _I, ctypes.POINTER(ctypes.c_int32), _P, _P]),
    "obia_sharp_laplacian_dev": (_I, [_P, _P, _I, _I, _P, _P]),
    "obia_sharp_box_dev": (_I, [_P, _P, _I, _I, _I, _P, _P, _P]),
    "obia_sharp_variance_dev": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "obia_sharp_stretch_f32_dev": (_I, [_P, _P, ctypes.c_int64, ctypes.c_double, ctypes.c_double, _P]),
}
# include/obia_training.h: the training-tile passes
TRAIN_MAX_KSIZE = 31      # OBIA_TRAIN_MAX_KSIZE: the largest side of a blur kernel
TRAIN_MAX_SIDE = 4096     # OBIA_TRAIN_MAX_SIDE: the largest H or W of the distance pass
TRAIN_MINMAX_WORK = 512   # OBIA_TRAIN_MINMAX_WORK: floats of the min-max pass's work buffer
_TRAINING_SIGNATURES = {
    "obia_train_blur_u8_dev": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P, _P]),
    "obia_train_distance_dev": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "obia_train_compose_u8_dev": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, ctypes.c_double, _P, _P]),
    "obia_train_minmax_u8_dev": (_I, [_P, _P, ctypes.c_int64, _P, _P, _P]),
}
# include/obia_crowns.h: crowns from seeds
CROWNS_TILE = 32          # OBIA_CROWNS_TILE: side of the tile one workgroup relaxes
_D = ctypes.c_double
_CROWNS_SIGNATURES = {
    "obia_crowns_allocate_dev": (_I, [_P, _P, _P, _I, _I, _P, _P, _I, _D, _D, _D, _D, _I, _D, _P, _P, _P]),
    "obia_crowns_last_work": (_I, [_P, _P]),
}
# include/obia_seed_table.h: the table options of the canonical seeds
_L = ctypes.c_int64
_F = ctypes.c_float
_SEED_TABLE_SIGNATURES = {
    "obia_seedtab_cells_dev": (_I, [_P, _P, _P, _L, _D, _P, _P]),
    "obia_seedtab_sample_dev": (_I, [_P, _P, _P, _L, _P, _I, _I, _P, _P, _P]),
    "obia_seedtab_stage1_dev": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _F, _F, _F, _F, _I, _P, _P, _P]),
    "obia_seedtab_last_work": (_I, [_P, _P]),
    "obia_seedtab_segments_dev": (_I, [_P, _P, _P, _L, _F, _P, _P, _P]),
    "obia_seedtab_nms_dev": (_I, [_P, _P, _P, _P, _P, _P, _P, _L, _L, _D, _D, _P]),
}
# include/obia_boxes.h: segments and detection boxes
BOXES_TABLE = 256         # OBIA_BOXES_TABLE: labels of the LDS table one workgroup counts a box's footprint into
_I32 = ctypes.c_int32
_BOXES_SIGNATURES = {
    "obia_boxes_assign_dev": (_I, [_P, _P, _I, _I, _P, _L, _I32, _P, _P]),
    "obia_boxes_pair_count_dev": (_I, [_P, _P, _I, _I, _P, _L, _I32, _P, _P]),
    "obia_boxes_pair_write_dev": (_I, [_P, _P, _I, _I, _P, _L, _I32, _P, _P, _L, _P, _P, _P, _P]),
    "obia_boxes_dissolve_dev": (_I, [_P, _P, _L, _P, _I32, _P]),
    "obia_boxes_iou_dev": (_I, [_P, _P, _L, _P, _L, _P]),
    "obia_boxes_nms_dev": (_I, [_P, _P, _P, _P, _P, _L, _L, _D, _P, ctypes.POINTER(_I32)]),
}
# include/obia_points.h: point clouds
POINTS_MAX_NZ = 4096      # OBIA_POINTS_MAX_NZ: height bins of a segment's profile
POINTS_CHUNK = 2048       # OBIA_POINTS_CHUNK: consecutive points one workgroup sums in LDS before it touches global memory
_POINTS_SIGNATURES = {
    "obia_points_rasters_dev": (_I, [_P, _P, _P, _P, _L, ctypes.POINTER(_D), _I, _I, _P, _P]),
    "obia_points_rasters_finish_dev": (_I, [_P, _P, _P, _I, _I, _D, _P, _P]),
    "obia_points_segments_dev": (_I, [_P, _P, _P, _P, _P, _L, ctypes.POINTER(_D), _P, _I, _I, _I32, _I32, _I32, _D, _P, _P, _P, _P, _P, _P]),
    "obia_points_segment_columns_dev": (_I, [_P, _P, _P, _P, _P, _P, _I32, _I32, _D, _D, _D, _P, _P, _P, _P, _P, _P, _P]),
}
# include/obia_ground.h: height above ground
GROUND_MAX_COUNT = 8      # OBIA_GROUND_MAX_COUNT: the most neighbours a query averages
_GROUND_SIGNATURES = {
    "obia_ground_query_dev": (_I, [_P, _P, _P, _P, _P, _L, _P, _L, _L, _L, _L, _D, _P, _P, _P, _L, _I32, _D, _P, _P, _P]),
    "obia_ground_dtm_dev": (_I, [_P, _P, _P, _P, _L, ctypes.POINTER(_D), _P, _I, _I, _P, _P]),
}
# include/obia_groundfilter.h: the ground filter
MORPH_MAX_RADIUS = 127    # OBIA_MORPH_MAX_RADIUS: the largest half-width of a grey filter's window
GF_MAX_STEPS = 16         # OBIA_GF_MAX_STEPS: the most steps of a schedule
MORPH_ROW_TILE, MORPH_COL_TILE, MORPH_COL_LANES = 1024, 128, 32   # OBIA_MORPH_ROW_TILE, OBIA_MORPH_COL_TILE, OBIA_MORPH_COL_LANES: a line pass's run
_GROUNDFILTER_BINDINGS = {
    "obia_gf_cell_min_dev": (_I, [_P, _P, _P, _P, _L, ctypes.POINTER(_D), _I, _I, _P]),
    "obia_gf_cell_min_finish_dev": (_I, [_P, _P, _I, _I, _P]),
    "obia_morph_filter_dev": (_I, [_P, _P, _I, _I, _I, _I, _P, _P]),
    "obia_gf_threshold_dev": (_I, [_P, _P, _I, _I, ctypes.POINTER(_I32), ctypes.POINTER(_D), _I, _P, _P, _P, _P]),
    "obia_gf_classify_dev": (_I, [_P, _P, _P, _P, _L, ctypes.POINTER(_D), _P, _I, _I, _P, _P]),
}
# include/obia_adjacency.h: the segment adjacency graph
ADJ_TILE_H, ADJ_TILE_W = 16, 32   # OBIA_ADJ_TILE_H, OBIA_ADJ_TILE_W: the tile one workgroup counts into its LDS table
ADJ_TABLE = 2048          # OBIA_ADJ_TABLE: slots of that table
ADJ_WORK = 4              # OBIA_ADJ_WORK: int32 of scratch the write pass asks for
_ADJACENCY_BINDINGS = {
    "obia_adj_tile_count_dev": (_I, [_P, _P, _I, _I, _I32, _I32, _P]),
    "obia_adj_tile_write_dev": (_I, [_P, _P, _I, _I, _I32, _I32, _P, _L, _P, _P, _P]),
    "obia_adj_edge_d2_dev": (_I, [_P, _P, _P, _I32, _L, _P, _I, _P]),
    "obia_adj_neighbor_stats_dev": (_I, [_P, _P, _P, _P, _I32, _L, _P, _I, _P, _P, _P, _P]),
    "obia_adj_class_border_dev": (_I, [_P, _P, _P, _P, _I32, _L, _P, _I, _P]),
    "obia_adj_best_neighbor_dev": (_I, [_P, _P, _P, _I32, _L, _P, _P, _P]),
    "obia_adj_components_dev": (_I, [_P, _P, _P, _I32, _L, _P, _P]),
    "obia_adj_relabel_dev": (_I, [_P, _P, _L, _I32, _I32, _P, _P]),
}
# include/obia_shapes.h: the raster pass of the shape columns
SHAPE_SUMS = 7            # OBIA_SHAPE_SUMS: columns of the sums table (n, sum r, sum c, sum r^2, sum c^2, sum r c, perimeter)
SHAPE_TABLE = 1024        # OBIA_SHAPE_TABLE: slots of the LDS table of one workgroup
_SHAPE_ENTRIES = {
    "obia_shape_sums_dev": (_I, [_P, _P, _I, _I, _I32, _I32, _P, _P]),
}
# include/obia_merging.h: region merging on the graph alone (fusion cost, pair merge, contraction of the CSR)
MERGE_ROW_CAP = 2048      # OBIA_MERGE_ROW_CAP: gathered entries of a row one workgroup sorts in LDS; a longer row is sorted in the scratch
_MERGE_ENTRIES = {
    "obia_merge_cost_dev": (_I, [_P, _P, _P, _P, _I32, _L, _P, _P, _P, _I, _P, _P, _P, _D, _D, _P]),
    "obia_merge_pairs_dev": (_I, [_P, _P, _P, _P, _I32, _L, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "obia_merge_contract_rows_dev": (_I, [_P, _P, _I32, _L, _P, _P]),
    "obia_merge_contract_count_dev": (_I, [_P, _P, _P, _P, _I32, _L, _P, _P, _P, _P, _P, _P]),
    "obia_merge_contract_write_dev": (_I, [_P, _I32, _L, _P, _P, _P, _P, _P, _L, _P, _P]),
}
# include/obia_testing.h: internal pieces driven directly by the test suite
_TEST_SIGNATURES = {
    "obia_test_clear_ranges_dev": (_I, [_P, _P, _P, _P, _I]),
    # the plan of a batch's sweeps as text: pure host code, no context (tests/test_sweep_plan_cpu.py)
    "obia_test_sweep_plan": (_I, [_P, _I, _P, _I, _P, _P, _P, ctypes.c_int64]),
    # the grid of a clamped launch by name, and the names: pure host code, no context (tests/test_launch_grids_cpu.py)
    "obia_test_launch_grid": (_I, [ctypes.c_char_p, _P, _I, _P]),
    "obia_test_launch_grid_names": (_I, [_P, ctypes.c_int64]),
    # the most new ids a seam import ranks by its LDS sort; above it the counting kernel (tests/test_gpu_seam_import.py)
    "obia_test_seam_sort_limit": (_I, []),
    # the connectivity stage on a batch of problems, and what its last call decided (tests/cc_regimes.py)
    "obia_test_enforce_connectivity_batch_dev": (_I, [_P, _P, _P, _I, _I, _P, ctypes.POINTER(_I)]),
    "obia_test_cc_report": (_I, [_P, _P, _I]),
    # a used context with known contents: the workspace filled with one byte, the visited map's non-zero words counted
    # (tests/test_gpu_workspace_history.py)
    "obia_test_poison_workspace_dev": (_I, [_P, ctypes.c_int64, _I, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]),
    "obia_test_visited_nonzero": (_I, [_P, ctypes.POINTER(ctypes.c_int64)]),
    # the wave and workgroup primitives of obia_amd/csrc/wave_ops.hpp, one at a time (tests/test_gpu_wave_ops.py)
    "obia_test_wave_ops_dev": (_I, [_P, _I, _I, _P, ctypes.c_int64, _P, _P]),
}

# The registry: one table per header of include/, in the order load() binds them.  Everything that enumerates the entry points -- load(),
# the decision tables of the test suite -- reads this mapping; the names above are for code that wants one table.
BINDINGS = {
    "obia_hip.h": _SIGNATURES,
    "obia_image.h": _IMAGE_SIGNATURES,
    "obia_sharpness.h": _SHARPNESS_SIGNATURES,
    "obia_training.h": _TRAINING_SIGNATURES,
    "obia_crowns.h": _CROWNS_SIGNATURES,
    "obia_seed_table.h": _SEED_TABLE_SIGNATURES,
    "obia_boxes.h": _BOXES_SIGNATURES,
    "obia_points.h": _POINTS_SIGNATURES,
    "obia_ground.h": _GROUND_SIGNATURES,
    "obia_groundfilter.h": _GROUNDFILTER_BINDINGS,
    "obia_adjacency.h": _ADJACENCY_BINDINGS,
    "obia_shapes.h": _SHAPE_ENTRIES,
    "obia_merging.h": _MERGE_ENTRIES,
    "obia_testing.h": _TEST_SIGNATURES,
}


def bound_entry_points():
    """every entry point load() binds, in registry order"""
    return [name for table in BINDINGS.values() for name in table]


_lib = None


def build(force=False):
    """Compile libobia_hip.so for gfx950 with hipcc (obia_amd/csrc/Makefile)."""
    args = ["make", "-C", _CSRC, "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


def load():
    """Load the HIP library; raise ImportError loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc, gfx950). obia_amd has no CPU fallback.")
        lib = ctypes.CDLL(LIB_PATH)
        for table in BINDINGS.values():
            for name, (res, args) in table.items():
                try:
                    fn = getattr(lib, name)
                except AttributeError:
                    # an OLDER build of this library shipped for an A/B timing (OBIA_HIP_LIB, tools/ab.sh) may lack the newest entry
                    # points; the regular library must export every one of them (tests/test_binding_tables_cpu.py checks the list)
                    if os.environ.get("OBIA_HIP_LIB"):
                        continue
                    raise
                fn.restype = res
                fn.argtypes = args
        _lib = lib
    return _lib


def last_error():
    return load().obia_last_error().decode("utf-8", "replace")


def check(rc):
    """Map ABI status codes to the exceptions the reference's callers see."""
    if rc == OBIA_OK:
        return
    msg = last_error()
    if rc in (E_INVALID, E_EMPTY, E_NONFINITE):
        raise ValueError(msg)          # the tiler catches ValueError per tile (tiling.py:149-150)
    if rc == E_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == E_NOMEM:
        raise MemoryError(msg)
    raise RuntimeError(f"obia_hip error {rc}: {msg}")


class Context:
    """One obia_ctx: a (device, stream) pair plus its reusable device workspace."""

    def __init__(self, device=0, stream=None):
        lib = load()
        if stream is None:
            self._h = lib.obia_create(int(device))
        else:
            self._h = lib.obia_create_on_stream(int(device), ctypes.c_void_p(int(stream)))
        if not self._h:
            raise RuntimeError(f"obia_create failed: {last_error()} (obia_amd needs an AMD GPU; there is no CPU path)")
        self.device = int(device)

    @property
    def handle(self):
        return self._h

    def close(self):
        if getattr(self, "_h", None):
            load().obia_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_profiling(self, on):
        """False / 0: off; True / 1: event pairs around every kernel class; 2: around the SLIC colour sweeps only."""
        check(load().obia_set_profiling(self._h, int(on)))

    def timing(self):
        lib = load()
        names = ["assign_ms", "sweeps", "features_ms", "connectivity_ms", "zonal_ms", "total_ms", "prepass_ms", "assign_px",
                 "prepass_px", "assign_store_px", "assign_busy_ms", "prepass_busy_ms", "batch_repeats",
                 "prepass_shared_px", "feature_fused_px", "prepass_group_launches", "fills", "uploads", "readbacks",
                 "assign_group_launches", "assign_launch_sum_ms"]
        return {n: lib.obia_last_timing(self._h, i) for i, n in enumerate(names)}

    def workspace_bytes(self):
        return int(load().obia_workspace_bytes(self._h))


_default_ctx = {}


def default_context(device=0):
    ctx = _default_ctx.get(device)
    if ctx is None:
        ctx = _default_ctx[device] = Context(device)
    return ctx


def np_ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def mask_bytes(mask, device=None):
    """Device mask as one byte per pixel, any non-zero byte = valid (what every kernel tests).  uint8 and bool tensors
    are passed through without a copy; other dtypes are compared with zero once."""
    import torch
    m = torch.as_tensor(mask, device=device)
    if m.dtype == torch.bool:
        m = m.contiguous().view(torch.uint8)
    elif m.dtype != torch.uint8:
        m = (m != 0).view(torch.uint8)
    return m.contiguous()
