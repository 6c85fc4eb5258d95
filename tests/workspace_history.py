"""The decision table of tests/test_gpu_workspace_history.py: one row per entry point that obia_amd/_lib.py binds.

Every operator takes its scratch memory from the context's bump allocator (Arena, obia_amd/csrc/common.hpp), which keeps the memory
between calls: a buffer that is read before it is written holds what the call before left there.  A row says either which cases of the
GPU test's OPS run the entry point on a poisoned context -- with one line on what initialises each of its workspace buffers before the
first read, found by reading the entry point -- or why no case is needed.  A new entry point fails tests/test_workspace_history_cpu.py
until somebody reads it and adds its row.

Case names: "pa:NAME" is OPS[NAME] of tests/test_gpu_pointer_alignment.py (the wrapper's call); "guards:NAME" is the case NAME of the
registry of tests/test_gpu_output_guards.py (the entry point through ctypes, judged there against the wrapper and its reference);
"body:NAME" runs the body of an existing test of a *_buffers file on the context; the others are built in the GPU test itself."""


class Row:
    def __init__(self, cases=(), init=None, exempt=None):
        self.cases = (cases,) if isinstance(cases, str) else tuple(cases)
        self.init, self.exempt = init, exempt


def run(cases, init):
    return Row(cases=cases, init=init)


def exempt(reason):
    return Row(exempt=reason)


NO_CONTEXT = "takes no context: pure host code"
BOOKKEEPING = "host only: reads or sets a field of the context, opens no frame and takes no workspace"
ONE_KERNEL = "takes no workspace: queues kernels (or one fill) on the caller's buffers only, no arena.get in the entry point or below it"
SESSION = ("session", "session_refusals")
SLIC_INIT = ("slic.hip / slic_sweep.hip / api.cpp: features, keys, seeds, centroid records and labels are written whole by their kernels; "
             "bin heads, accumulators, tile-list meta, the 513 pixel counters and the orphan flag by the batch's ClearSet / fill_async; "
             "cc.hip: counters, ring and tile-root bits by ONE fill_async, parent / size by cc_tile_kernel, root bits by cc_roots_kernel, "
             "block sums by the blocksum kernels, tag / ccur by fill_async, the lists by the kernels that count them")
CC_INIT = ("cc.hip: counters + ring + tile-root bits by one fill_async (again before the recount after a size cut and every 64 rounds), "
           "parent / size by cc_tile_kernel, rootbits by cc_roots_kernel, block_sums by cc_rank_blocksum*, newlab / small_list / "
           "small_qoff by cc_rank_apply*, settle by cc_settle_init_kernel, tag and ccur by fill_async, code[] by cc_code_kernel, "
           "px_g / px_cn by cc_small_pixels_kernel, work lists up to the count read back; the visited map is the context's, all zero "
           "between calls")
TILED_INIT = SLIC_INIT + ("; tiling.hip: seg_size / alive by fill_async at create, inside per batch by the ClearSet, newid / d_total by "
                          "ids_scan_kernel, tile masks and d_tile_any by the batch's clear and tile_mask_kernel; mask_seeds.hip (seeding "
                          "\"skimage\"): see obia_mask_centroids_dev")
ZONAL_INIT = "zonal.hip: every accumulator by zonal_init_kernel (statistics) or one ClearSet of four ranges (moments)"
QS_INIT = ("quickshift.hip: features, float64 image, density, parents and ranks are written whole by their kernels, the tie noise by "
           "the caller's copy or a memset, d_flags by hipMemsetAsync before every pass that counts, block sums by the scan")

ROWS = {
    # ---- include/obia_hip.h -------------------------------------------------------------------------------------------------------
    "obia_abi_version": exempt(NO_CONTEXT),
    "obia_last_error": exempt(NO_CONTEXT),
    "obia_create": exempt(NO_CONTEXT + " (makes the context)"),
    "obia_create_on_stream": exempt(NO_CONTEXT + " (makes the context)"),
    "obia_slic_default_params": exempt(NO_CONTEXT),
    "obia_rasterize_info": exempt(NO_CONTEXT),
    "obia_destroy": exempt("frees the context; refused while a session holds it: case `session_refusals`"),
    "obia_synchronize": exempt(BOOKKEEPING),
    "obia_workspace_bytes": exempt(BOOKKEEPING),
    "obia_set_profiling": exempt(BOOKKEEPING),
    "obia_last_timing": exempt(BOOKKEEPING),
    "obia_slic_f32": run("guards:slic_host_37x53x4_masked", "Staging buffers are plain allocations filled by its uploads; then obia_slic_f32_dev"),
    "obia_slic_f32_dev": run(("pa:slic_full_c8_masked", "pa:slic_full_c3_masked", "guards:slic_37x53x4_masked"), SLIC_INIT),
    "obia_slic_assign_only_f32_dev": run(("pa:slic_pre_c4", "guards:assign_37x53x3_masked"), SLIC_INIT),
    "obia_slic_seeded_f32_dev": run(("guards:seeded0_37x53x4_masked", "guards:seeded1_37x53x4_masked"),
                                    SLIC_INIT + "; seeding \"skimage\" (seeded1): mask_seeds.hip as obia_mask_centroids_dev"),
    "obia_mask_centroids_dev": run("guards:mask_centroids_37x53",
                                   "mask_seeds.hip: rowcnt / rowoff by ms_row_count / ms_row_scan, picks by upload, acc by hipMemsetAsync (and "
                                   "cleared again by ms_finalise_kernel), seeds and pts by ms_gather_kernel (strictly ascending picks below "
                                   "n_valid: one pixel each), book by ms_init_book_kernel, closest by ms_nearest_kernel"),
    "obia_slic_stages_f32_dev": run(("pa:slic_stages", "guards:slic_stages_s33_c3_nolab_capHW"), SLIC_INIT),
    "obia_enforce_connectivity_i32_dev": run(("pa:enforce_connectivity", "cc_walks", "cc_lists", "cc_code_walks", "cc_cut"), CC_INIT),
    "obia_zonal_stats_f32": run("guards:zonal_stats_host_C4", "Staging; then obia_zonal_stats_f32_dev"),
    "obia_zonal_stats_f32_dev": run(("pa:zonal_stats", "guards:zonal_stats_C9_subset"), ZONAL_INIT),
    "obia_zonal_moments_f32_dev": run(("pa:zonal_moments", "guards:zonal_moments_fresh_var_C3"), ZONAL_INIT),
    "obia_zonal_moments_f32": run("guards:zonal_moments_host_C4", "Staging; then the two _dev calls"),
    "obia_texture_stats_f32_dev": run(("pa:texture_thin_strips", "pa:texture_dense"),
                                      "texture.hip: bbox by bbox_init_kernel, d_nbig by hipMemsetAsync, big_list up to the count read back, the "
                                      "dense path's scratch cleared by the workgroup that uses it"),
    "obia_label_edges_u8_dev": run("pa:slic_edge", "consumers.hip: the one counter d_n by hipMemsetAsync"),
    "obia_sample_labels_i32_dev": run("pa:sample_labels", ONE_KERNEL),
    "obia_cost_bands_f32_dev": run("guards:cost_bands_33x41", ONE_KERNEL),
    "obia_cost_ndvi_f32_dev": run("guards:cost_ndvi_33x41", ONE_KERNEL),
    "obia_cost_sobel_f32_dev": run("guards:cost_sobel_33x41", ONE_KERNEL),
    "obia_cost_select_dev": run(("guards:cost_select_33x41", "pa:cost_layers"), "cost.hip: SelState and the histograms by sel_init_kernel, the histograms again by every resolve"),
    "obia_cost_entropy_f32_dev": run("guards:cost_entropy_33x41", ONE_KERNEL + " (the term table is the caller's)"),
    "obia_cost_normalise_dev": run(("guards:cost_normalise32_33x41", "guards:cost_normalise64_33x41"), ONE_KERNEL),
    "obia_cost_edge_count_dev": run("pa:cost_layers", "cost.hip: the one counter d_n by hipMemsetAsync"),
    "obia_cost_combine_dev": run("guards:cost_combine_33x41", ONE_KERNEL),
    "obia_seeds_peaks_dev": run(("pa:seed_peaks", "guards:seeds_peaks_sigma1_33x37"),
                                "seeds.hip: Gaussian weights by upload, tmp by the row pass, counts by seeds_count_kernel (every chunk), the flag "
                                "bytes past the last pixel by hipMemsetAsync"),
    "obia_seeds_peaks_gather_dev": run(("pa:seed_peaks", "guards:seeds_peaks_sigma1_33x37"), ONE_KERNEL),
    "obia_seeds_pair_link_dev": run("guards:seeds_pair_link_n70", "seeds.hip: sample table by upload, parent by seeds_iota_kernel, root / is_root by seeds_flatten_kernel, rank by seeds_scan_kernel"),
    "obia_seeds_pair_stats_dev": run("guards:seeds_pair_stats_n70", "seeds.hip: sample table by upload, PairStats by hipMemsetAsync before every pass (and the first pass's extremes by upload)"),
    "obia_seeds_pair_matrix_dev": run(("pa:seed_pair_matrix", "guards:seeds_pair_matrix_n70"), "seeds.hip: the sample table by upload, nothing else"),
    "obia_polygon_count_i32_dev": run("pa:polygon_rings", "polygons.hip: cnt by the count kernel, d_totals by hipMemsetAsync, block sums by the scan"),
    "obia_polygon_rings_i32_dev": run(("pa:polygon_rings", "guards:polygon_rings_donut"), "polygons.hip: as the count, then cand / nverts / ring_idx / vert_off by the kernels that list the rings"),
    "obia_rasterize_polygons_dev": run(("pa:rasterize", "guards:rasterize_1x203"),
                                       "rasterize.hip: out by hipMemsetAsync(0xff), counters and band_n by hipMemsetAsync, start / large / band tables by their kernels"),
    "obia_quickshift_f32": run("guards:quickshift_host_lds_23x31x3", "Staging; then obia_quickshift_f32_dev"),
    "obia_quickshift_f32_dev": run(("pa:quickshift_lds", "pa:quickshift_global"), QS_INIT),
    "obia_quickshift_stages_f32_dev": run(("guards:quickshift_stages_lds_23x31x3", "guards:quickshift_stages_global_17x19x5"), QS_INIT),
    "obia_tiled_slic_f32_dev": run(("pa:tiled", "guards:tiled_129x131x4", "tiled_orphan_repeat"), TILED_INIT),
    "obia_tiled_slic_f32": run("guards:tiled_host_129x131x4", "Staging; then the _dev call"),
    "obia_tiled_slic_seeded_f32_dev": run(("guards:tiled_seeded_grid_129x131x4", "tiled_skimage"), TILED_INIT),
    "obia_tiled_slic_seeded_f32": run("guards:tiled_seeded_grid_host_129x131x4", "Staging; then the _dev call"),
    "obia_tiler_create": run(SESSION, TILED_INIT),
    "obia_tiler_destroy": run(SESSION, "frees the seam scratch, clears the context's session record"),
    "obia_tiler_run": run(SESSION, TILED_INIT),
    "obia_tiler_next_id": run(SESSION, "a host integer of the session"),
    "obia_tiler_set_seeding": run("tiled_skimage", "host fields of the session (the one-shot call sets the same fields)"),
    "obia_tiler_set_segments": run("session", "copies into seg_size, fills alive: session state that create cleared"),
    "obia_tiler_get_alive": run(SESSION, "one device-to-device copy out of the session's alive flags, no workspace"),
    "obia_tiler_set_alive": exempt("one device-to-device copy into the session's alive flags, no workspace; the sharded driver's tests call it"),
    "obia_tiler_finalize": run(SESSION, "tiling.hip: d_partial and newid by ids_scan_kernel, d_total by its last workgroup"),
    "obia_tiler_import_seam": run("session", "tiling.hip: scratch outside the arena (hipMalloc kept by the session): the two counters by fill_async, "
                                             "the list of new ids by seam_mark_kernel up to the count read back"),
    "obia_table_scale_dev": run(("pa:table_scale", "guards:table_scale_257"), "classify.hip: partial sums and counts written whole by the first pass"),
    "obia_table_scale_f64_dev": run(("pa:table_scale_f64", "guards:table_scale_f64_257"), "classify.hip: as obia_table_scale_dev"),
    "obia_forest_predict_dev": run(("pa:forest_predict", "guards:forest_predict_257"), "classify.hip: node records and feature map by the check kernel, `bad` by hipMemsetAsync"),
    "obia_forest_shap_dev": run(("pa:forest_shap", "guards:forest_shap_48"), "shap.hip: `bad` and parent (0xff) by hipMemsetAsync, the other node tables, paths and elements by their kernels"),
    "obia_mlp_predict_dev": run(("pa:mlp_predict", "guards:mlp_predict_257"), "mlp.hip: `bad` by hipMemsetAsync"),
    "obia_mlp_coalition_dev": run(("pa:mlp_shap", "guards:mlp_coalition_author"), "mlp_shap.hip: the two flags by hipMemsetAsync"),
    "obia_shapley_combine_dev": run(("pa:mlp_shap", "guards:shapley_combine_author"), ONE_KERNEL),
    # ---- include/obia_image.h -----------------------------------------------------------------------------------------------------
    "obia_image_stretch_u8_dev": exempt(ONE_KERNEL),
    "obia_image_gray_hist_dev": exempt(ONE_KERNEL + " (the histogram is the caller's, cleared by hipMemsetAsync)"),
    "obia_image_lut_u8_dev": exempt(ONE_KERNEL),
    "obia_image_clahe_u8_dev": run("body:image_clahe", "image.hip: the 64 tile histograms by hipMemsetAsync, the 64 LUTs written whole by clahe_lut_kernel"),
    "obia_image_boundaries_dev": exempt(ONE_KERNEL),
    "obia_image_mark_u8_dev": exempt(ONE_KERNEL),
    # ---- include/obia_sharpness.h -------------------------------------------------------------------------------------------------
    "obia_sharp_gray_lap_dev": run("body:sharp_gray_lap", "sharpness.hip: a partial record per workgroup by band_minmax_kernel (band_stats_kernel reads that many), "
                                                          "stats by band_stats_kernel, the scratch counter by hipMemsetAsync"),
    "obia_sharp_laplacian_dev": exempt(ONE_KERNEL),
    "obia_sharp_box_dev": exempt(ONE_KERNEL + " (`work` is the caller's)"),
    "obia_sharp_variance_dev": exempt(ONE_KERNEL + " (`work` is the caller's)"),
    "obia_sharp_stretch_f32_dev": exempt(ONE_KERNEL),
    # ---- include/obia_training.h --------------------------------------------------------------------------------------------------
    "obia_train_blur_u8_dev": exempt(ONE_KERNEL + " (training.hip names the arena nowhere)"),
    "obia_train_distance_dev": exempt(ONE_KERNEL + " (training.hip names the arena nowhere)"),
    "obia_train_compose_u8_dev": exempt(ONE_KERNEL + " (training.hip names the arena nowhere)"),
    "obia_train_minmax_u8_dev": exempt(ONE_KERNEL + " (its work buffer is the caller's)"),
    # ---- include/obia_crowns.h ----------------------------------------------------------------------------------------------------
    "obia_crowns_allocate_dev": run("crowns_mask", "crowns.hip: Counters by fill_async, `changed` again before every round"),
    "obia_crowns_last_work": exempt("host only: four integers kept by the last call"),
    # ---- include/obia_seed_table.h ------------------------------------------------------------------------------------------------
    "obia_seedtab_cells_dev": run("body:seed_table", ONE_KERNEL),
    "obia_seedtab_sample_dev": run("body:seed_table", ONE_KERNEL),
    "obia_seedtab_stage1_dev": run("body:seed_table", "seed_table.hip: eps and the first state plane written whole by seedtab_eligible_kernel, the other plane "
                                                      "by every round, `remaining` by fill_async before every round"),
    "obia_seedtab_last_work": exempt("host only: two integers kept by the last call"),
    "obia_seedtab_segments_dev": run("body:seed_table", ONE_KERNEL),
    "obia_seedtab_nms_dev": run("body:seed_table", ONE_KERNEL),
    # ---- include/obia_boxes.h -----------------------------------------------------------------------------------------------------
    "obia_boxes_assign_dev": run(("boxes_table", "boxes_passes", "body:boxes"),
                                 "boxes.hip: flags by fill_async (check_boxes, and after every attempt), passes by boxes_fill_i32_kernel, pending "
                                 "written for every box by the first walk (which does not read it), best by fill_async"),
    "obia_boxes_pair_count_dev": run(("boxes_table", "boxes_passes", "body:boxes"), "boxes.hip: flags and pending as obia_boxes_assign_dev"),
    "obia_boxes_pair_write_dev": run(("boxes_table", "boxes_passes", "body:boxes"), "boxes.hip: flags by fill_async"),
    "obia_boxes_dissolve_dev": run("body:boxes", ONE_KERNEL),
    "obia_boxes_iou_dev": run("body:boxes", ONE_KERNEL),
    "obia_boxes_nms_dev": run("body:boxes", "boxes.hip: flags, `remaining` (before every round) and the first state plane by fill_async, the other plane by every round"),
    # ---- include/obia_points.h, include/obia_ground.h -----------------------------------------------------------------------------
    "obia_points_rasters_dev": exempt(ONE_KERNEL + " (points.hip names the arena nowhere: accumulators are the caller's)"),
    "obia_points_rasters_finish_dev": exempt(ONE_KERNEL + " (points.hip names the arena nowhere)"),
    "obia_points_segments_dev": exempt(ONE_KERNEL + " (points.hip names the arena nowhere)"),
    "obia_points_segment_columns_dev": exempt(ONE_KERNEL + " (points.hip names the arena nowhere)"),
    "obia_ground_query_dev": exempt(ONE_KERNEL + " (ground.hip names the arena nowhere)"),
    "obia_ground_dtm_dev": exempt(ONE_KERNEL + " (ground.hip names the arena nowhere)"),
    # ---- include/obia_groundfilter.h: groundfilter.hip names the arena nowhere, every state, scratch plane and counter is the caller's ----
    "obia_gf_cell_min_dev": run("body:groundfilter", ONE_KERNEL + " (the key plane is the caller's state, cleared by the caller and added to)"),
    "obia_gf_cell_min_finish_dev": run("body:groundfilter", ONE_KERNEL),
    "obia_morph_filter_dev": run("body:groundfilter", ONE_KERNEL + " (`tmp` is the caller's, written whole by the row pass before the column pass reads it)"),
    "obia_gf_threshold_dev": run("body:groundfilter", ONE_KERNEL + " (`tmp0` / `tmp1` are the caller's, each written whole by the pass before the one that reads it)"),
    "obia_gf_classify_dev": run("body:groundfilter", ONE_KERNEL + " (the four counters are the caller's state, cleared by the caller and added to)"),
    # ---- include/obia_adjacency.h: adjacency.hip names the arena nowhere, every buffer is the caller's ------------------------------------
    "obia_adj_tile_count_dev": run("body:adjacency", ONE_KERNEL + " (the tile's table lives in LDS, cleared by its workgroup)"),
    "obia_adj_tile_write_dev": run("body:adjacency", ONE_KERNEL + " (`work`, the caller's four words, by one fill before the pass; read back after it)"),
    "obia_adj_edge_d2_dev": run("body:adjacency", ONE_KERNEL),
    "obia_adj_neighbor_stats_dev": run("body:adjacency", ONE_KERNEL),
    "obia_adj_class_border_dev": run("body:adjacency", ONE_KERNEL),
    "obia_adj_best_neighbor_dev": run("body:adjacency", ONE_KERNEL),
    "obia_adj_components_dev": run("body:adjacency", ONE_KERNEL + " (root_out is written whole by adj_iota_kernel before the link kernel reads it)"),
    "obia_adj_relabel_dev": run("body:adjacency", ONE_KERNEL),
    # ---- include/obia_shapes.h: shapes.hip names the arena nowhere, both tables are the caller's --------------------------------------
    "obia_shape_sums_dev": run("body:shapes", ONE_KERNEL + " (sums_out and box_out by two fill_async before the tile kernel adds to them; the tile's "
                                              "keys, accumulators and slot count live in LDS, cleared by their workgroup before its first tile and "
                                              "again, slot by slot, as it flushes one)"),
    # ---- include/obia_merging.h: merging.hip names the arena nowhere, every table, scratch row and cursor is the caller's -------------
    "obia_merge_cost_dev": run("body:merging", ONE_KERNEL + " (a value per entry, written whole; nothing is accumulated)"),
    "obia_merge_pairs_dev": run("body:merging", ONE_KERNEL + " (a row per segment, written whole; nothing is accumulated)"),
    "obia_merge_contract_rows_dev": run("body:merging", ONE_KERNEL + " (raw_count_out by fill_async before contract_rows_kernel adds the row lengths to it)"),
    "obia_merge_contract_count_dev": run("body:merging", ONE_KERNEL + " (`cursor_work`, the caller's, by fill_async before the gather takes its tickets; the "
                                                         "gather writes every stretch of `key_work` / `border_work` whole before a sort kernel reads it; "
                                                         "the block sort loads its LDS row, chunk keys and sums before it reads them; count_out is written "
                                                         "for every row by the one sort kernel whose length class the row falls in)"),
    "obia_merge_contract_write_dev": run("body:merging", ONE_KERNEL + " (reads the count pass's scratch, writes every entry of neighbor_out / border_out)"),
    # ---- include/obia_testing.h ---------------------------------------------------------------------------------------------------
    "obia_test_clear_ranges_dev": exempt("takes no workspace: the table of ranges is the clear kernel's argument, passed by value"),
    "obia_test_sweep_plan": exempt(NO_CONTEXT),
    "obia_test_launch_grid": exempt(NO_CONTEXT),
    "obia_test_launch_grid_names": exempt(NO_CONTEXT),
    "obia_test_seam_sort_limit": exempt(NO_CONTEXT),
    "obia_test_enforce_connectivity_batch_dev": run("cc_batch", CC_INIT),
    "obia_test_cc_report": exempt("host only: copies the record of the last connectivity call"),
    "obia_test_poison_workspace_dev": exempt("the instrument itself: every case of the GPU test calls it"),
    "obia_test_visited_nonzero": exempt("the instrument itself: reads the visited map, writes nothing"),
    "obia_test_wave_ops_dev": exempt("takes no workspace: one kernel on the caller's buffers (the int32 scans run on the first half of out)"),
}

# Source files of obia_amd/csrc that take memory from the arena, and a case that runs each: tests/test_workspace_history_cpu.py looks
# for `arena.get` / `A.get` / `arena.alloc` in every file of the directory and fails on one that is not listed.
ARENA_FILES = {
    "api.cpp": "pa:slic_full_c8_masked", "slic.hip": "pa:slic_full_c8_masked", "slic_sweep.hip": "pa:slic_full_c8_masked", "cc.hip": "cc_lists",
    "zonal.hip": "pa:zonal_stats", "tiling.hip": "pa:tiled", "quickshift.hip": "pa:quickshift_lds", "polygons.hip": "pa:polygon_rings",
    "rasterize.hip": "pa:rasterize", "consumers.hip": "pa:slic_edge", "texture.hip": "pa:texture_dense", "cost.hip": "pa:cost_layers",
    "seeds.hip": "guards:seeds_pair_link_n70", "classify.hip": "pa:forest_predict", "mlp.hip": "pa:mlp_predict", "mask_seeds.hip": "tiled_skimage",
    "shap.hip": "pa:forest_shap", "mlp_shap.hip": "pa:mlp_shap", "image.hip": "body:image_clahe", "sharpness.hip": "body:sharp_gray_lap",
    "crowns.hip": "crowns_mask", "seed_table.hip": "body:seed_table", "boxes.hip": "boxes_table",
    "context.cpp": "pa:tiled",       # (PlanBlob: the device side of a batch's tables)
}


def bound_entry_points():
    """every name of the registry of obia_amd/_lib.py, in its order"""
    from obia_amd import _lib
    return _lib.bound_entry_points()


def cases():
    """every case a row names, in table order"""
    out = []
    for row in ROWS.values():
        out += [c for c in row.cases if c not in out]
    return out
