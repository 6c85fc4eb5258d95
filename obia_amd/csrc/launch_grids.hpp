// launch_grids.hpp -- the grid of every launch whose workgroup count is clamped, as data.  Pure host arithmetic: no pointer is
// dereferenced, nothing is launched, no HIP type appears.
//
// A clamped launch gives an axis min(units, cap) workgroups and lets every workgroup walk the remaining units in a stride loop
// (unit += gridDim).  `units` is what ONE workgroup takes in ONE trip of that loop: 256 elements, 256 four-byte chunks, a row, a
// tile row of 16 rows, a box.  An Axis holds the workgroup count and the trips of the workgroup with the most work, so a test
// reads off whether a shape reaches the second trip -- the code no small shape runs -- without knowing the clamp (DESIGN.md,
// "Launch clamps").  An axis that is not clamped (whole()) grows with the input; its device limit is 2^31 - 1 in x.
//
// Every launch site calls its function here; table() (at the end) names each one for obia_test_launch_grid (include/obia_testing.h).
// A new clamped launch gets a function AND a row of that table: the row is what makes its threshold visible to tests/test_launch_grids_cpu.py.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/obia_adjacency.h"
#include "../../include/obia_groundfilter.h"
#include "../../include/obia_points.h"
#include "../../include/obia_training.h"

namespace obia {
namespace grids {

constexpr long long GRID_X_MAX = 0x7fffffffLL, GRID_Y_MAX = 65535;

// tile shapes and chunk sizes the grids below are made of; the kernels take them from here
constexpr int COST_SOBEL_TW = 64, COST_SOBEL_TH = 16;
constexpr int COST_ENTROPY_TW = 64, COST_ENTROPY_TH = 16;
constexpr int COST_SELECT_THREADS = 1024;
constexpr int SEEDS_FLAG_TW = 64, SEEDS_FLAG_TH = 16;
constexpr int SEEDS_PAIR_TILE = 64;        // a pair tile is 64 x 64 seeds
constexpr int CLAHE_ROWS = 32;             // rows of one interpolation workgroup (256 columns wide)
constexpr int QS_TILE = 16;                // side of a quickshift tile
constexpr int RAST_LARGE_TILE_W = 2048;    // columns of one workgroup's bit plane
constexpr int SHARPNESS_MINMAX_PARTS = 2048;
constexpr int TILER_IDS_PER_WG = 256 * 16;

inline long long cdivl(long long a, long long b) { return (a + b - 1) / b; }

struct Axis { long long n, trips; };       // workgroups; loop trips of the workgroup with the most work
struct Grid { Axis x, y; };

inline Axis strided(long long units, long long cap) {
    const long long g = std::max(1LL, std::min(units, std::max(1LL, cap)));
    return Axis{g, std::max(1LL, cdivl(units, g))};
}
inline Axis whole(long long units) { return Axis{std::max(1LL, units), 1}; }
inline Grid one_axis(Axis x) { return Grid{x, Axis{1, 1}}; }

// ---- flat arrays -------------------------------------------------------------------------------------------------------------------
// n work items (elements, or 4- / 12-byte chunks), 256 per workgroup and trip, 8192 workgroups at the most
inline Grid flat(long long n) { return one_axis(strided(cdivl(n, 256), 8192)); }
inline Grid image_stretch(long long n) { return flat(n / 4 + 2); }                    // 4-byte chunks of the output, head and tail
inline Grid image_lut(long long n, long long rep) { return flat(n * rep / 4 + 2); }
inline Grid image_gray_hist(long long n) { return one_axis(strided(cdivl(n / 4 + 2, 256), 2048)); }
inline Grid training_compose(long long npx) { return flat((3 * npx + 6) / 4); }
inline Grid training_minmax_scale(long long n) { return flat((n + 6) / 4); }
inline Grid training_minmax_reduce(long long n) { return one_axis(strided(cdivl(n, 256), OBIA_TRAIN_MINMAX_WORK / 2)); }
inline Grid sharpness_minmax(long long npx) { return one_axis(strided(cdivl(npx, 256), SHARPNESS_MINMAX_PARTS)); }
inline Grid scale_transform(long long n_rows, long long F) { return one_axis(strided(cdivl(n_rows * F, 256), 2048)); }
inline Grid cost_select(long long nv) { return one_axis(strided(cdivl(nv, COST_SELECT_THREADS), 512)); }   // nv: 16-byte vectors
inline Grid seeds_gauss(long long npx) { return one_axis(strided(cdivl(npx, 256), 16384)); }
inline Grid seeds_pairs(long long n) {                                                  // pair tiles of the upper triangle
    const long long nt = cdivl(n, SEEDS_PAIR_TILE);
    return one_axis(strided(nt * (nt + 1) / 2, 256 * 16));
}
inline Grid points_segments(long long n) { return one_axis(strided(cdivl(n, OBIA_POINTS_CHUNK), 1280)); }
inline Grid ground_query(long long n) { return one_axis(strided(cdivl(n, 256), 4096)); }   // a query per lane; its ring walk is long: 16 workgroups per CU of 256
inline Grid boxes_walk(long long n) { return one_axis(strided(n, 4096)); }              // a box per workgroup and trip
inline Grid quickshift_flat(long long npx) { return one_axis(strided(cdivl(npx, 256 * 4), 65535)); }
inline Grid quickshift_gauss(long long n) { return one_axis(strided(cdivl(n, 256), 65535)); }   // n = pixels x bands
inline Grid polygons_candidates(long long npx) { return one_axis(strided(cdivl(npx, 256 * 4), 262144)); }
inline Grid rast_value(long long npx) { return one_axis(strided(cdivl(npx, 256 * 4), 16384)); }
inline Grid zonal_labels(long long nlb) { return one_axis(strided(cdivl(nlb, 256), 4096)); }   // labels x bands
inline Grid texture_segments(long long n_labels) { return one_axis(strided(n_labels, 65536)); }
inline Grid texture_big_segments(long long n_big) { return one_axis(strided(n_big, 256)); }
inline Grid label_edges(long long H) { return one_axis(strided(H, 8192)); }             // a row per workgroup and trip

// ---- rasters: columns in x, rows in y ----------------------------------------------------------------------------------------------
// rows of 4-byte (boundaries) or 12-byte (mark) output chunks: W / 4 + 2 chunks cover a row with its head and tail
inline Grid image_rows(long long H, long long W) { return Grid{strided(cdivl(W / 4 + 2, 256), 64), strided(H, GRID_Y_MAX)}; }
inline Grid image_clahe_interp(long long H, long long W) { return Grid{whole(cdivl(W, 256)), strided(cdivl(H, CLAHE_ROWS), GRID_Y_MAX)}; }
// histogram of the 8 x 8 CLAHE tiles of th x tw pixels: the rows of a workgroup grow so that grid.y stays within its limit
inline long long image_clahe_hist_rows(long long th, long long tw) {
    return std::max(std::max(1LL, 16384 / std::max(1LL, tw)), cdivl(th, GRID_Y_MAX));
}
inline Grid image_clahe_hist(long long th, long long tw) { return Grid{whole(64), whole(cdivl(th, image_clahe_hist_rows(th, tw)))}; }
inline Grid cost_rows(long long H, long long W) { return Grid{whole(cdivl(W, 256)), strided(H, GRID_Y_MAX)}; }
inline Grid tiles(long long H, long long W, long long tw, long long th) { return Grid{whole(cdivl(W, tw)), strided(cdivl(H, th), GRID_Y_MAX)}; }
inline Grid cost_sobel(long long H, long long W) { return tiles(H, W, COST_SOBEL_TW, COST_SOBEL_TH); }
inline Grid cost_entropy(long long H, long long W) { return tiles(H, W, COST_ENTROPY_TW, COST_ENTROPY_TH); }
inline Grid seeds_flag(long long H, long long W) { return tiles(H, W, SEEDS_FLAG_TW, SEEDS_FLAG_TH); }
inline Grid quickshift_density(long long H, long long W) { return tiles(H, W, QS_TILE, QS_TILE); }
// a few thousand workgroups striding over the rows: gx <= 16 columns of 256 pixels, gx * gy <= 4096
inline Grid cost_edge_count(long long H, long long W) {
    const Axis x = strided(cdivl(W, 256), 16);
    return Grid{x, strided(H, std::max(1LL, 4096 / x.n))};
}
// line passes of the grey filters (groundfilter.hip): a run of OBIA_MORPH_ROW_TILE cells of a row in x and a row per trip in y; a
// band of OBIA_MORPH_COL_LANES columns in x and a run of OBIA_MORPH_COL_TILE rows per trip in y
inline Grid morph_rows(long long H, long long W) { return Grid{whole(cdivl(W, OBIA_MORPH_ROW_TILE)), strided(H, GRID_Y_MAX)}; }
inline Grid morph_cols(long long H, long long W) { return Grid{whole(cdivl(W, OBIA_MORPH_COL_LANES)), strided(cdivl(H, OBIA_MORPH_COL_TILE), 8192)}; }
// the tile passes of the segment graph (adjacency.hip): a workgroup keeps its LDS table over the tiles it walks on both axes, so a
// few thousand workgroups clear a table once each
inline Grid adj_tiles(long long H, long long W) { return Grid{strided(cdivl(W, OBIA_ADJ_TILE_W), 64), strided(cdivl(H, OBIA_ADJ_TILE_H), 128)}; }
// IoU matrix: 256 boxes of b per workgroup and trip in x, a box of a in y
inline Grid boxes_iou(long long na, long long nb) { return Grid{strided(cdivl(nb, 256), 4096), strided(na, 4096)}; }
// large shapes of the rasteriser: a shape (bin) or a row band (large) in x, its vertices / columns in y
inline Grid rast_band_bin(long long n_large, long long max_nv) { return Grid{whole(n_large), strided(cdivl(max_nv, 256), 64)}; }
inline Grid rast_large(long long n_bands, long long max_w) { return Grid{whole(n_bands), strided(cdivl(max_w, RAST_LARGE_TILE_W), 1024)}; }

// ---- SLIC, connectivity and the tiler: x walks rows (or flat chunks), y is the problem of the batch ---------------------------------
// np, the problems of one batch, is 65535 at the most (slic_batch_layout refuses a larger batch)
inline Grid slic_band_minmax(long long maxh, long long np) { return Grid{strided(maxh, 2048), whole(np)}; }
inline Grid slic_feature_rows(long long rows, long long np) { return Grid{strided(rows, 4096), whole(np)}; }   // rows, bands of 4 or of 16 rows
inline Grid slic_gauss(long long n, long long np) { return Grid{strided(cdivl(n, 256), 65535), whole(np)}; }   // n = pixels x padded bands
inline Grid slic_stage_features(long long n) { return one_axis(strided(cdivl(n, 256), 65535)); }
inline Grid slic_fill_labels(long long npx) { return one_axis(strided(cdivl(npx, 256 * 8), 65535)); }
inline Grid slic_mask_pack(long long maxh, long long np) { return Grid{strided((maxh + 3) / 4, 16384), whole(np)}; }
inline Grid slic_maxdist(long long maxh, long long np) { return Grid{strided(maxh, 4096), whole(np)}; }
inline Grid cc_flat(long long npx) { return one_axis(strided(cdivl(npx, 256 * 4), 65535 * 4)); }
inline Grid cc_seam(long long max_seam, long long np) { return Grid{strided(cdivl(max_seam, 256), 65535), whole(np)}; }
inline Grid tiler_rows(long long maxh, long long np) { return Grid{strided(maxh, 8192), whole(np)}; }
inline Grid tiler_ids_apply(long long npx) { return one_axis(strided(cdivl(npx, TILER_IDS_PER_WG), 65535)); }
inline Grid tiler_seam(long long n) { return one_axis(strided(cdivl(n, 256), 2048)); }

// ---- the names ---------------------------------------------------------------------------------------------------------------------
// `sizes`: what the function takes, in its order.  Every size may go up to 2^31 - 1 (a raster side, a row count, a flat count below
// 2^31 elements) but `np`, a batch's problems: 65535.  Products are formed in 64 bits.  A unit may be more than one step of the
// kernel's own loop (quickshift_flat: 1024 pixels, which 256 lanes take in four): the trips count units.
struct Named {
    const char *name;
    int n_sizes;
    const char *sizes;
    Grid (*fn)(const long long *s);
};

#define OBIA_GRID1(f, doc) {#f, 1, doc, [](const long long *s) { return f(s[0]); }}
#define OBIA_GRID2(f, doc) {#f, 2, doc, [](const long long *s) { return f(s[0], s[1]); }}
#define OBIA_GRID4(f, doc) {#f, 4, doc, [](const long long *s) { return f(s[0], s[1], s[2], s[3]); }}
inline const Named *table(int *count) {
    static const Named TABLE[] = {
    OBIA_GRID1(flat, "n"),
    OBIA_GRID1(image_stretch, "n"),
    OBIA_GRID2(image_lut, "n rep"),
    OBIA_GRID1(image_gray_hist, "n"),
    OBIA_GRID1(training_compose, "npx"),
    OBIA_GRID1(training_minmax_scale, "n"),
    OBIA_GRID1(training_minmax_reduce, "n"),
    OBIA_GRID1(sharpness_minmax, "npx"),
    OBIA_GRID2(scale_transform, "n_rows F"),
    OBIA_GRID1(cost_select, "nv"),
    OBIA_GRID1(seeds_gauss, "npx"),
    OBIA_GRID1(seeds_pairs, "n"),
    OBIA_GRID1(points_segments, "n"),
    OBIA_GRID1(ground_query, "n"),
    OBIA_GRID1(boxes_walk, "n"),
    OBIA_GRID1(quickshift_flat, "npx"),
    OBIA_GRID1(quickshift_gauss, "n"),
    OBIA_GRID1(polygons_candidates, "npx"),
    OBIA_GRID1(rast_value, "npx"),
    OBIA_GRID1(zonal_labels, "nlb"),
    OBIA_GRID1(texture_segments, "n_labels"),
    OBIA_GRID1(texture_big_segments, "n_big"),
    OBIA_GRID1(label_edges, "H"),
    OBIA_GRID2(image_rows, "H W"),
    OBIA_GRID2(image_clahe_interp, "H W"),
    OBIA_GRID2(image_clahe_hist, "th tw"),
    OBIA_GRID2(cost_rows, "H W"),
    OBIA_GRID4(tiles, "H W tw th"),
    OBIA_GRID2(cost_sobel, "H W"),
    OBIA_GRID2(cost_entropy, "H W"),
    OBIA_GRID2(seeds_flag, "H W"),
    OBIA_GRID2(quickshift_density, "H W"),
    OBIA_GRID2(cost_edge_count, "H W"),
    OBIA_GRID2(morph_rows, "H W"),
    OBIA_GRID2(morph_cols, "H W"),
    OBIA_GRID2(adj_tiles, "H W"),
    OBIA_GRID2(boxes_iou, "na nb"),
    OBIA_GRID2(rast_band_bin, "n_large max_nv"),
    OBIA_GRID2(rast_large, "n_bands max_w"),
    OBIA_GRID2(slic_band_minmax, "maxh np"),
    OBIA_GRID2(slic_feature_rows, "rows np"),
    OBIA_GRID2(slic_gauss, "n np"),
    OBIA_GRID1(slic_stage_features, "n"),
    OBIA_GRID1(slic_fill_labels, "npx"),
    OBIA_GRID2(slic_mask_pack, "maxh np"),
    OBIA_GRID2(slic_maxdist, "maxh np"),
    OBIA_GRID1(cc_flat, "npx"),
    OBIA_GRID2(cc_seam, "max_seam np"),
    OBIA_GRID2(tiler_rows, "maxh np"),
    OBIA_GRID1(tiler_ids_apply, "npx"),
    OBIA_GRID1(tiler_seam, "n"),
    };
    *count = (int)(sizeof(TABLE) / sizeof(TABLE[0]));
    return TABLE;
}
#undef OBIA_GRID1
#undef OBIA_GRID2
#undef OBIA_GRID4

}  // namespace grids
}  // namespace obia
