// tiling.hip -- B3: the tiled driver on label rasters.
//
// Restates the two tile loops of obia.utils.tiling.create_tiled_segments (tiling.py:103-291), where the
// reference keeps two growing GeoDataFrames and tests every accumulated polygon against every white tile
// with shapely predicates (tiling.py:205-231).  Here the state is one global label raster G (0 = no
// segment) plus a per-segment pixel count, and the predicates are pixel counts:
//   within(tile_polygon)   <=>  every pixel of the segment lies inside the grown window minus the two
//                               bottom corner squares           (count inside == segment size)
//   overlaps(tile_polygon) <=>  some but not all of its pixels do
// (segments are 4-connected pixel sets and rasterize() uses the pixel-centre rule; the window is pixel-aligned, the two corner
// squares are when buffer/2 is a whole number of pixels -- otherwise the cut passes THROUGH pixels, and "inside" means three
// different things for the three uses of the squares: see TileWin).
//   pass 1  "black" tiles ((i/T + j/T) even), exact windows          tiling.py:103-153
//   pass 2  "white" tiles, windows grown by `buffer` and clamped      tiling.py:156-172
//           segments within the polygon are dropped and re-segmented  tiling.py:220-231
//           segments overlapping it are kept and masked out, together with the corner squares
//                                                                    tiling.py:213-260
//           ... but only when at least one existing segment is within / overlaps the polygon (tiling.py:212); otherwise
//           the mask is left as read and the corner squares ARE segmented (tiling.py:261-262): tile_any[]
//           n_segments = round(mask.sum() * pixel_area / (pi * crown_radius^2))   tiling.py:126-135
//   ids 1..N in the order black (survivors), then white              tiling.py:289-290
// All tiles of a pass (or of one white tile-row) are ONE batch for the SLIC engine and for the
// connectivity kernels: no per-tile launches, two host read-backs per batch.
#include "slic.hpp"
#include "wave_ops.hpp"
#include "../../include/obia_testing.h"

#include <cmath>
#include <cstdlib>

namespace obia {

// window, dense offset, corner squares in pixels.  The squares have side buffer/2 in MAP units (tiling.py:189), i.e. a = buffer/2/pixel
// pixels, which need not be whole; three pixel counts follow from the reference's three uses of the square (per axis):
//   cl*     pixels whose CENTRE lies inside: what rasterize() burns into the mask (all_touched=False)        tiling.py:245-255
//   cl*_in  pixels that lie WHOLLY inside: a segment made of such pixels only has no area in tile_polygon,
//           it is neither `within` nor `overlaps` (not selected)                                             tiling.py:205-210
//   cl*_any pixels that meet the square's interior at all: a segment with such a pixel is not `within`       tiling.py:220-231
// (equal when a is a whole number -- even buffer, pixel size 1 or 0.5 -- which is every case rounds 1-3 tested)
struct TileWin { int y0, x0, h, w; long long pix_off; int cly, clx; int cly_in, clx_in, cly_any, clx_any; int m4_off; };   // pix_off, m4_off: copied from SlicProblem

// wave-aggregated histogram add: lanes of a wave that hold the same key add once
__device__ __forceinline__ void wave_hist_add(unsigned *hist, int key, bool active) {
    bool todo = active;
    while (true) {
        const unsigned long long act = __ballot(todo);
        if (!act) break;
        const int leader = __ffsll((long long)act) - 1;
        const int kk = __shfl(key, leader);
        const unsigned long long same = __ballot(todo && key == kk);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[kk], (unsigned)__popcll(same));
        if (key == kk) todo = false;
    }
}

__device__ __forceinline__ bool in_corner(const TileWin &t, int y, int x) {
    return (y >= t.h - t.cly) && (x < t.clx || x >= t.w - t.clx);
}
__device__ __forceinline__ bool wholly_in_corner(const TileWin &t, int y, int x) {
    return (y >= t.h - t.cly_in) && (x < t.clx_in || x >= t.w - t.clx_in);
}
__device__ __forceinline__ bool meets_corner(const TileWin &t, int y, int x) {
    return (y >= t.h - t.cly_any) && (x < t.clx_any || x >= t.w - t.clx_any);
}

// Occupancy map of the label raster (TileState::occ): one bit per 64 x 64 block, in the raster's own coordinates, row-major over
// occ_bw = cdiv(W, 64) blocks a row.  A block whose bit is clear holds only zeros, so its labels need not be read.  A null map (a
// session, OBIA_G_OCCUPANCY=0) says nothing: every block counts as occupied.  Windows are not aligned to the blocks in general.
constexpr int OCC_SHIFT = 6;
__device__ __forceinline__ bool occ_test(const unsigned *__restrict__ occ, int occ_bw, int gy, int gx) {
    if (!occ) return true;
    const int b = (gy >> OCC_SHIFT) * occ_bw + (gx >> OCC_SHIFT);
    return (occ[b >> 5] >> (b & 31)) & 1u;
}

// white tiles, step 1: inside[g] = pixels of every existing segment that lie in the window and do not meet a corner square
// (inside[g] == seg_size[g]  <=>  the segment is `within` tile_polygon)
// tile_any[tile] = 1 when some existing segment has area inside the polygon -- a pixel in the window that is not wholly inside a
// corner square: `not intersecting_black_segments.empty or not intersecting_white_segments.empty` (tiling.py:205-212)
// The kernel walks the window by the blocks of the occupancy map (raster coordinates): a workgroup per 64 x 64 block the window
// meets, a wave per sixteen of its rows, a lane per column -- so the bit is tested once per workgroup, a workgroup in a clear block
// ends at once (its labels are zero: they add to neither inside[] nor tile_any), and the rows of an occupied block are read as
// aligned 256-byte stretches, eight in flight.  Without a map every block is walked.
constexpr int COUNT_ROWS_PER_WAVE = (1 << OCC_SHIFT) / 4;
__global__ __launch_bounds__(256) void tile_count_inside_kernel(const TileWin *__restrict__ wins, const int32_t *__restrict__ G,
                                                                int Wr, unsigned *__restrict__ inside, int *__restrict__ tile_any,
                                                                const unsigned *__restrict__ occ, int occ_bw) {
    const TileWin t = wins[blockIdx.y];
    const int cb0 = t.x0 >> OCC_SHIFT, rb0 = t.y0 >> OCC_SHIFT;                      // the first block column / row the window meets
    const int nbx = ((t.x0 + t.w - 1) >> OCC_SHIFT) - cb0 + 1, nby = ((t.y0 + t.h - 1) >> OCC_SHIFT) - rb0 + 1;
    if ((int)blockIdx.x >= nbx * nby) return;   // whole workgroup (the grid is sized for the batch's largest window)
    const int rb = rb0 + (int)blockIdx.x / nbx, cb = cb0 + (int)blockIdx.x % nbx;
    if (!occ_test(occ, occ_bw, rb << OCC_SHIFT, cb << OCC_SHIFT)) return;            // whole workgroup
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int x = (cb << OCC_SHIFT) + (int)(threadIdx.x & 63) - t.x0;                // the lane's column in the window
    const bool col_ok = x >= 0 && x < t.w;
    const int y_first = (rb << OCC_SHIFT) + wv * COUNT_ROWS_PER_WAVE - t.y0;         // the wave's first row in the window (wave-uniform)
    bool seen = false;
#pragma unroll 1
    for (int yb = y_first; yb < y_first + COUNT_ROWS_PER_WAVE; yb += 8) {            // eight loads in flight
        int g[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int y = yb + j;
            g[j] = 0;
            if (y < 0 || y >= t.h) continue;                                         // wave-uniform
            const bool low = y >= t.h - t.cly_any;   // a row the corner squares reach (wave-uniform: the others test no pixel)
            if (col_ok && !(low && wholly_in_corner(t, y, x))) {
                g[j] = G[(long long)(t.y0 + y) * Wr + t.x0 + x];
                seen |= g[j] > 0;
                if (low && meets_corner(t, y, x)) g[j] = 0;   // (a pixel the cut passes through: selected, but not counted as inside)
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (yb + j >= 0 && yb + j < t.h) wave_hist_add(inside, g[j], g[j] > 0);   // wave-uniform condition
    }
    if (__ballot(seen) && (threadIdx.x & 63) == 0) tile_any[blockIdx.y] = 1;   // (every writer stores the same value)
}

// step 2: dense tile mask.  black: the input mask.  white: input mask minus kept (overlapping) segments
// minus the corner squares; segments within the polygon are erased from G (they will be re-segmented).
template <bool VEC4>
__global__ __launch_bounds__(256) void tile_mask_kernel(const TileWin *__restrict__ wins, const uint8_t *__restrict__ inmask,
                                                        int32_t *__restrict__ G, int Wr, int white,
                                                        const unsigned *__restrict__ inside, const unsigned *__restrict__ seg_size,
                                                        uint8_t *__restrict__ alive, uint8_t *__restrict__ dmask,
                                                        const int *__restrict__ tile_any, unsigned *__restrict__ dmask4,
                                                        const unsigned *__restrict__ occ, int occ_bw, int *__restrict__ parts) {
    const TileWin t = wins[blockIdx.y];
    // parts[tile * gridDim.x + workgroup] = the non-zero mask bytes this workgroup wrote (every byte is 0 or 1): partial sums of the
    // tile's valid count, mask.sum() (tiling.py:133), which the host adds up after the read-back it makes anyway.  Plain stores, every
    // slot written: atomics on the tiles' counters serialise, about 8 ns each, and cost more than the counting kernel they replace.
    int nz = 0;
    auto store_count = [&]() {
        nz = block_sum<256>(nz);
        if (threadIdx.x == 0) parts[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = nz;
    };
    // a white tile whose polygon no existing segment intersects keeps the mask it read: neither kept segments (there are none
    // inside the polygon) nor the corner squares are masked out (tiling.py:212, 261-262)
    if (white && tile_any[blockIdx.y] == 0) white = 0;
    // one pixel of the tile: its mask byte given the input mask byte and the global label under it
    auto decide = [&](int y, int x, long long gp, uint8_t m, int g) -> uint8_t {
        if (!white) return m;
        if (in_corner(t, y, x)) return 0;
        if (g > 0) {
            if (inside[g] == seg_size[g]) { G[gp] = 0; alive[g] = 0; }   // within: dropped
            else m = 0;                                                    // overlaps: kept, masked out
        }
        return m;
    };
    if (VEC4) {
        // four consecutive pixels per lane: one dword of mask bytes, one int4 of labels, one dword stored (the host checks that
        // every window's x0, w and pix_off and the row pitch are multiples of four and the base pointers aligned)
        // A thread owns a 4 x 4 block: the four rows of one quad row (the eight loads in flight together), so that it can also
        // write the block TRANSPOSED -- the packed mask of the sweeps (SlicBatch::d_mask4: dword (q, x) = the bytes of the rows
        // 4q .. 4q+3 at column x), which used to be a pass of its own over the batch's mask (round 4).
        const int w4 = t.w >> 2, nq = (t.h + 3) >> 2;
        for (int q = blockIdx.x; q < nq; q += gridDim.x)
            for (int x4 = threadIdx.x; x4 < w4; x4 += 256) {
                const int x = 4 * x4;
                unsigned mw[4];
                int4 g[4];
                // the block's four pixels of a row lie in one block of the occupancy map (x0 + x is a multiple of four), its four
                // rows in at most two: when both are clear the labels are not loaded, g stays 0 and `decide` takes its path for no
                // segment.  (One test for the four loads, so that they are issued together as before; rows of a clear block that
                // are loaded beside an occupied one hold zeros.)
                const bool load_g = white && (occ_test(occ, occ_bw, t.y0 + 4 * q, t.x0 + x) || occ_test(occ, occ_bw, t.y0 + min(4 * q + 3, t.h - 1), t.x0 + x));
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int y = 4 * q + j;
                    const int gy = t.y0 + (y < t.h ? y : t.h - 1);
                    const long long gp = (long long)gy * Wr + t.x0 + x;
                    mw[j] = inmask ? *reinterpret_cast<const unsigned *>(inmask + gp) : 0x01010101u;
                    g[j] = make_int4(0, 0, 0, 0);
                    if (load_g) g[j] = *reinterpret_cast<const int4 *>(G + gp);
                }
                unsigned out[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int y = 4 * q + j;
                    if (y >= t.h) continue;   // (rows past the window: zero bytes in the packed mask, nothing in the row-major one)
                    const long long gp = (long long)(t.y0 + y) * Wr + t.x0 + x;
                    const int gv[4] = {g[j].x, g[j].y, g[j].z, g[j].w};
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const uint8_t m = ((mw[j] >> (8 * u)) & 0xffu) != 0;
                        out[j] |= (unsigned)decide(y, x + u, gp + u, m, gv[u]) << (8 * u);
                    }
                    *reinterpret_cast<unsigned *>(dmask + t.pix_off + (long long)y * t.w + x) = out[j];
                    nz += __popc(out[j]);
                }
                uint4 o;   // column c of the block: byte c of every row
                unsigned *ov = &o.x;
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    ov[c] = ((out[0] >> (8 * c)) & 0xffu) | (((out[1] >> (8 * c)) & 0xffu) << 8) | (((out[2] >> (8 * c)) & 0xffu) << 16) |
                            (((out[3] >> (8 * c)) & 0xffu) << 24);
                *reinterpret_cast<uint4 *>(dmask4 + (long long)t.m4_off + (long long)q * t.w + x) = o;
            }
        store_count();
        return;
    }
    for (int y = blockIdx.x; y < t.h; y += gridDim.x)
    for (int x0 = threadIdx.x; x0 < t.w; x0 += 4 * 256) {   // four pixels in flight per lane
        uint8_t mv[4];
        int gv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int x = x0 + 256 * u;
            mv[u] = 0; gv[u] = 0;
            if (x < t.w) {
                const long long gp = (long long)(t.y0 + y) * Wr + t.x0 + x;
                mv[u] = inmask ? (inmask[gp] != 0) : 1;
                // (outside the burned square => not wholly inside it: the segment is selected; a pixel in a clear block has g = 0)
                if (white && !in_corner(t, y, x) && occ_test(occ, occ_bw, t.y0 + y, t.x0 + x)) gv[u] = G[gp];
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int x = x0 + 256 * u;
            if (x >= t.w) continue;
            const long long gp = (long long)(t.y0 + y) * Wr + t.x0 + x;
            const uint8_t m = decide(y, x, gp, mv[u], gv[u]);
            dmask[t.pix_off + (long long)y * t.w + x] = m;
            nz += m;
        }
    }
    store_count();
}

// step 3: write the new segments of the batch into G with their provisional global ids + size histogram.
// Global atomics run at ~2e10 per second device-wide, so the histogram is built per 64x64 block of the window first:
// a lane walks one column (runs of equal label down the column are counted in a register), run totals go to a 128-slot
// LDS table keyed by label, and the table is flushed with one global atomic per (block, label).
constexpr int TS_SLOTS = 128;
__global__ __launch_bounds__(64) void tile_scatter_kernel(const TileWin *__restrict__ wins, const CcResolve R,
                                                          int32_t *__restrict__ G, int Wr, int id_base,
                                                          unsigned *__restrict__ seg_size, unsigned *__restrict__ occ, int occ_bw) {
    __shared__ int s_key[TS_SLOTS];
    __shared__ unsigned s_cnt[TS_SLOTS];
    const TileWin t = wins[blockIdx.y];
    const int bw = (t.w + 63) / 64;
    const int by = blockIdx.x / bw, bx = blockIdx.x % bw;
    if (by * 64 >= t.h) return;   // whole workgroup
    const int lane = threadIdx.x;
    for (int i = lane; i < TS_SLOTS; i += 64) { s_key[i] = 0; s_cnt[i] = 0; }
    __syncthreads();
    const int x = bx * 64 + lane;
    const bool col_ok = x < t.w;
    const int y_lo = by * 64, y_hi = min(y_lo + 64, t.h);
    int rid = 0;
    unsigned rn = 0;
    auto close_run = [&]() {
        if (rid <= 0) return;
        const unsigned h = ((unsigned)rid * 2654435761u) >> 25;
        int slot = -1;
#pragma unroll 1
        for (int probe = 0; probe < TS_SLOTS; ++probe) {
            const int sidx = (h + probe) & (TS_SLOTS - 1);
            const int old = atomicCAS(&s_key[sidx], 0, rid);
            if (old == 0 || old == rid) { slot = sidx; break; }
        }
        if (slot >= 0) atomicAdd(&s_cnt[slot], rn);
        else atomicAdd(&seg_size[rid], rn);          // table full: straight to global memory
    };
    // the workgroup's 64 x 64 pixels meet at most 2 x 2 blocks of the occupancy map: y_split is the window row where the second
    // block row starts, wrote0 / wrote1 say that this lane stored an id in the first / second block row
    const int rb0 = (t.y0 + y_lo) >> OCC_SHIFT;
    const int y_split = ((rb0 + 1) << OCC_SHIFT) - t.y0;
    bool wrote0 = false, wrote1 = false;
    // The label of the pixel's component is resolved here (the connectivity pass hands over its tables instead of a label map), and
    // it depends on the pixel's parent alone: the parents of the eight rows are loaded (coalesced), the two or three gathers behind
    // them are made only where the parent differs from the one above in the column, every other pixel takes the label above.
    int p_above = -1, l_above = R.mask_label;   // (every negative parent is a masked pixel: mask_label)
#pragma unroll 1
    for (int y0 = y_lo; y0 < y_hi; y0 += 8) {       // eight rows in flight
        int par[8], l[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int y = y0 + j;
            par[j] = (col_ok && y < y_hi) ? R.parent[t.pix_off + (long long)y * t.w + x] : -1;
        }
        unsigned fresh = 0;   // bit j: row j starts a run of parents
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            l[j] = R.mask_label;
            if (par[j] >= 0 && par[j] != (j ? par[j - 1] : p_above)) { l[j] = cc_resolve_parent(R, par[j]); fresh |= 1u << j; }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (par[j] >= 0 && !((fresh >> j) & 1u)) l[j] = j ? l[j - 1] : l_above;
        p_above = par[7]; l_above = l[7];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int y = y0 + j;
            const int id = (col_ok && y < y_hi && l[j] > 0) ? id_base + l[j] : 0;
            if (id > 0) {
                G[(long long)(t.y0 + y) * Wr + t.x0 + x] = id;
                if (y >= y_split) wrote1 = true; else wrote0 = true;
            }
            if (id != rid) { close_run(); rid = id; rn = 0; }
            rn += 1;
        }
    }
    close_run();
    // the invariant of the occupancy map: a block's bit is set in the kernel that first stores a non-zero label into it (the readers
    // are later kernels of the stream).  One atomic per workgroup and block, none when the bit is there already.
    if (occ) {
        const int cb0 = (t.x0 + bx * 64) >> OCC_SHIFT;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const bool mine = (r ? wrote1 : wrote0) && ((t.x0 + x) >> OCC_SHIFT) == cb0 + c;
                if (__ballot(mine) && lane == 0) {
                    const int b = (rb0 + r) * occ_bw + cb0 + c;
                    if (!((occ[b >> 5] >> (b & 31)) & 1u)) atomicOr(&occ[b >> 5], 1u << (b & 31));
                }
            }
    }
    __syncthreads();
    for (int i = lane; i < TS_SLOTS; i += 64)
        if (s_key[i] > 0 && s_cnt[i]) atomicAdd(&seg_size[s_key[i]], s_cnt[i]);
}

// final ids 1..N: exclusive scan over the alive flags of the provisional ids (the table has ~1e6 entries).
// Two launches: per-chunk counts, then every workgroup adds up the counts of the chunks before its own and scans its
// chunk of 1024 x 16 flags (coalesced 16-byte reads).
constexpr int IDS_CHUNK = 1024 * 16;

__global__ __launch_bounds__(1024) void ids_count_kernel(const uint8_t *__restrict__ alive, int n_ids, int *__restrict__ partial) {
    const int tid = threadIdx.x;
    const int i0 = blockIdx.x * IDS_CHUNK + tid * 16;
    int c = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) c += (i0 + q < n_ids) ? (alive[i0 + q] != 0) : 0;
    c = block_sum<1024>(c);
    if (tid == 0) partial[blockIdx.x] = c;
}

__global__ __launch_bounds__(1024) void ids_scan_kernel(const uint8_t *__restrict__ alive, int n_ids, const int *__restrict__ partial,
                                                        int *__restrict__ newid, long long *__restrict__ total) {
    const int tid = threadIdx.x;
    // alive ids in the chunks before this one
    int pre = 0;
    for (int j = tid; j < (int)blockIdx.x; j += 1024) pre += partial[j];
    const int i0 = blockIdx.x * IDS_CHUNK + tid * 16;
    unsigned char f[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) f[q] = (i0 + q < n_ids) ? alive[i0 + q] : 0;
    pre = block_sum<1024>(pre);   // (behind the loads: they are in flight before its barriers)
    int c = 0;
#pragma unroll
    for (int q = 0; q < 16; ++q) c += f[q] != 0;
    int chunk_total;
    int run = pre + block_exclusive_scan<1024>(c, chunk_total);
#pragma unroll
    for (int q = 0; q < 16; ++q)
        if (i0 + q < n_ids) { if (f[q]) { run += 1; newid[i0 + q] = run; } else newid[i0 + q] = 0; }
    if (blockIdx.x == gridDim.x - 1 && tid == 1023) *total = pre + chunk_total;
}

// G[i] = newid[G[i]]: four pixels per lane and step (one 16-byte access, four gathers in flight)
__global__ __launch_bounds__(256) void ids_apply_kernel(int32_t *__restrict__ G, long long n, const int *__restrict__ newid) {
    const long long n4 = ((reinterpret_cast<uintptr_t>(G) & 15) == 0) ? n / 4 : 0;
    int4 *G4 = reinterpret_cast<int4 *>(G);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        int4 g = G4[i];
        g.x = g.x > 0 ? newid[g.x] : 0;
        g.y = g.y > 0 ? newid[g.y] : 0;
        g.z = g.z > 0 ? newid[g.z] : 0;
        g.w = g.w > 0 ? newid[g.w] : 0;
        G4[i] = g;
    }
    for (long long i = n4 * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const int g = G[i];
        G[i] = g > 0 ? newid[g] : 0;
    }
}

struct TileState {
    int H, W, C;            // local raster: rows [row0, row0 + H) of a (Hg, W) raster
    int Hg, row0;
    const float *img;
    const uint8_t *inmask;
    int32_t *G;
    // Occupancy map of G (occ_test): one bit per 64 x 64 block, clear = the block holds only zeros.  tile_scatter_kernel sets a
    // block's bit in the launch that first stores an id into it; tile_mask_kernel only ever stores zeros, so a bit stays set once
    // it is (conservative).  Only a one-call run (tiled_slic_dev) has the map: there the library zero-fills G and is its only
    // writer.  A session (obia_tiler_*) runs on a raster the caller owns and writes between calls -- the sharded driver puts imported
    // seam rows there -- so its map is null, every block counts as occupied and the kernels read all of G.
    unsigned *occ = nullptr;
    int occ_bw = 0;        // blocks per row of the map: cdiv(W, 64)
    unsigned *seg_size, *inside;
    uint8_t *alive;
    int *newid;
    long long *d_total;
    int id_cap, next_id;   // provisional ids 1..next_id-1
    int clx, cly, clx_in, cly_in, clx_any, cly_any;   // corner squares in pixels (see TileWin)
    obia_tiling_params tp;
    obia_slic_params sp;
    SlicBatch settings;    // slic_batch_settings of (sp, C): every batch of the tiler, and the white prefetch, starts as a copy
    int seeding = OBIA_SEEDING_GRID;       // OBIA_SEEDING_*: how every tile is seeded (obia_tiler_set_seeding)
    obia_pick_fn pick_fn = nullptr;        // OBIA_SEEDING_SKIMAGE: the caller's source of the random picks
    void *pick_user = nullptr;
    // features of ALL white tiles, prepared in one batch (they depend on the raster only): windows in processing order,
    // one dense buffer, keys read back once before the white pass
    // Batches that take the fused feature pass (slic.hpp: slic_fuse_features) need the min / max keys only: the prefetch is then the
    // min / max pass of all white windows with its one read-back, no planes are allocated for the set (4.85 GB at the headline
    // size), and every white batch takes its planes from its own scope of the arena, where its last pre-pass sweep writes them.
    struct PreFeat {
        bool ready = false;
        bool planned = false;            // there is a prefetch (windows, keys; planes unless fused)
        bool fused = false;              // keys only: the white batches fuse their feature pass into their sweeps
        SlicBatch b;                     // windows, layout and feature buffers of the whole set
        std::vector<unsigned> host;      // keys | nonfinite | max|feature| of all windows
        unsigned *d_keys = nullptr;
        bool launched = false;
        bool on_side = false;            // the pass was queued on a side stream (beside the black sweeps): join before it is read
        size_t cursor = 0;               // next window to be consumed by a white batch
    } pf;
};

// The feature pass of the white tiles (bound by HBM, few vector instructions) ran on a side stream beside the black batch's
// sweeps while their first nine launches -- the spatial pre-pass, bound by vector issue, no data moved -- covered the whole batch:
// 46.62 / 46.48 -> 46.10 / 46.00 ms per step then.  Since the black tiles of a class share one pre-pass (slic_sweep.hip) there is little
// left to run beside, and the pass is queued on the context's stream in front of the black sweeps: 37.8 - 38.1 ms per step against
// 38.1 - 38.5 beside (five alternating runs each, profiles/prepass_share_notes.md).  Batches that never share -- exit_on_fixed_point,
// SLIC-zero: every sweep stores its labels -- keep the side stream; OBIA_PREFETCH_BESIDE=1 builds that form for every batch.

static int grid_rows(const std::vector<TileWin> &wins) {   // row-walking kernels: one block per row (capped)
    int g = 1;
    for (auto &t : wins) if (t.h > g) g = t.h;
    return (int)grids::tiler_rows(g, 1).x.n;
}

// One batch of tiles: mask -> features -> plan -> sweeps -> connectivity -> scatter.
#ifndef OBIA_PREFETCH_BESIDE
#define OBIA_PREFETCH_BESIDE 0   /* developer builds: 1 = the white feature pass runs on a side stream beside the black sweeps */
#endif
static int prefetch_white_launch(obia_ctx *ctx, TileState &S, bool beside = false);

// OBIA_SEEDING_SKIMAGE: every tile of the batch is seeded as scikit-image seeds maskSLIC, from its own window of the batch's mask
// (b.d_mask + pix_off: dense (h, w), for a white tile what tile_mask_kernel left of the input mask).  A tile with n < 2 or fewer
// than two valid pixels is skipped (nseg[p] = 0): scikit-image ends with a zero step there and raises, the reference's tile loop
// prints "empty tile" (tiling.py:149-150).  The tiles are queued one after the other on the context's stream with no host
// synchronisation in between -- the host fetches and checks the picks of tile p + 1 while the kernels of tile p run -- and the steps
// of all tiles come back in ONE read-back; the centroids never leave the device (ext[p].d_yx).
static int seed_tiles_skimage(obia_ctx *ctx, TileState &S, const SlicBatch &b, const std::vector<int> &nvalid, std::vector<int> &nseg,
                              std::vector<ExternalSeeds> &ext) {
    const int np = b.nprob;
    if (!S.pick_fn) { set_error("seeding = skimage needs a pick function"); return OBIA_E_INVALID; }
    Arena &A = ctx->arena;
    ext.assign(np, ExternalSeeds{nullptr, 0, 1.0, nullptr});
    std::vector<long long> off(np, 0);
    long long total = 0;
    for (int p = 0; p < np; ++p) {
        if (nseg[p] < 2 || nvalid[p] < 2) { nseg[p] = 0; continue; }
        off[p] = total;
        total += std::min(nseg[p], nvalid[p]);   // K = min(n, n_valid) exactly
    }
    if (total == 0) return OBIA_OK;
    if (total > 0x7fff0000LL) { set_error("too many centroids in one batch"); return OBIA_E_INVALID; }
    float *d_seeds = A.get<float>(2 * (size_t)total);
    double *d_steps = A.get<double>(2 * (size_t)np);
    if (!d_seeds || !d_steps) return OBIA_E_NOMEM;
    OBIA_TRY(fill_async(ctx, d_steps, 0, sizeof(double) * 2 * (size_t)np));
    auto ascending_below = [](const int64_t *v, long long n, long long bound) {
        if (v[0] < 0 || v[n - 1] >= bound) return false;
        for (long long i = 1; i < n; ++i) if (v[i] <= v[i - 1]) return false;
        return true;
    };
    for (int p = 0; p < np; ++p) {
        if (nseg[p] == 0) continue;
        const int K = std::min(nseg[p], nvalid[p]);
        const int64_t *idx = nullptr, *dense = nullptr;
        int32_t n_idx = 0;
        int64_t n_dense = 0;
        if (S.pick_fn(S.pick_user, (int64_t)nvalid[p], (int32_t)nseg[p], &idx, &n_idx, &dense, &n_dense) != 0) {
            set_error("the pick function failed for a tile with %d valid pixels and n_segments = %d", nvalid[p], nseg[p]);
            return OBIA_E_INVALID;
        }
        if (!idx || n_idx != K || !ascending_below(idx, K, nvalid[p]) ||
            (dense && (n_dense < 1 || n_dense > nvalid[p] || !ascending_below(dense, n_dense, nvalid[p])))) {
            set_error("the pick function returned bad picks for a tile with %d valid pixels and n_segments = %d: %d strictly ascending ranks below the "
                      "valid count are needed", nvalid[p], nseg[p], K);
            return OBIA_E_INVALID;
        }
        const SlicProblem &P = b.probs[p];
        OBIA_TRY(mask_centroids_queue(ctx, b.d_mask + P.pix_off, P.H, P.W, nvalid[p], idx, K, dense, dense ? (long long)n_dense : 0, 5,
                                      d_seeds + 2 * off[p], d_steps + 2 * (size_t)p));
        ext[p].n = K;
        ext[p].d_yx = d_seeds + 2 * off[p];
    }
    std::vector<double> steps(2 * (size_t)np);
    OBIA_TRY(read_back(ctx, steps.data(), d_steps, sizeof(double) * steps.size()));
    for (int p = 0; p < np; ++p) {
        if (ext[p].n == 0) continue;
        const double st = std::max(steps[2 * (size_t)p], steps[2 * (size_t)p + 1]);   // step = max(steps); the depth axis contributes 0
        if (!(st >= 0.0) || !(st < 1e9)) { set_error("tile seeding: steps are not finite"); return OBIA_E_INVALID; }
        ext[p].step = st;
    }
    return OBIA_OK;
}

static int run_tile_batch(obia_ctx *ctx, TileState &S, std::vector<TileWin> &wins, bool white) {
    const int np = (int)wins.size();
    if (np == 0) return OBIA_OK;
    Arena &A = ctx->arena;
    const Arena::Mark mk = A.mark();
    SlicBatch b = S.settings;
    for (auto &t : wins) b.windows.push_back(SrcWindow{t.y0, t.x0, t.h, t.w, 0, 0, 0});
    OBIA_TRY(slic_batch_layout(b));
    for (int p = 0; p < np; ++p) { wins[p].pix_off = b.probs[p].pix_off; wins[p].m4_off = b.probs[p].m4_off; }
    b.d_mask = A.get<uint8_t>((size_t)b.total_pix);
    unsigned *d_mask4 = A.get<unsigned>((size_t)b.total_m4);   // the packed mask of the sweeps, written by tile_mask_kernel<true>
    if (!d_mask4) return OBIA_E_NOMEM;
    const bool pre = white && S.pf.ready;
    if (pre) {
        // this batch is the next np windows of the prefetched set (same order, same sizes: checked)
        const SlicBatch &pb = S.pf.b;
        if (S.pf.cursor + np > pb.windows.size()) { set_error("white batch beyond the prefetched windows"); return OBIA_E_INVALID; }
        const SrcWindow *a = &pb.windows[S.pf.cursor];
        for (int p = 0; p < np; ++p)
            if (a[p].y0 != wins[p].y0 || a[p].x0 != wins[p].x0 || a[p].h != wins[p].h || a[p].w != wins[p].w) { set_error("white batch does not match the prefetched windows"); return OBIA_E_INVALID; }
        if (S.pf.fused) {
            // keys only: the planes come from this batch's scope of the arena, its last pre-pass sweep writes them
            b.d_feat = A.get<float>(4 * (size_t)b.total_feat_f4);
            b.fuse_features = true;
            b.raw_src = S.img; b.raw_ws = S.W;
            b.d_keys = S.pf.d_keys + S.pf.cursor * (size_t)S.C * 2;
        } else {
            // (the batch's feat_off / fb_off values start at 0: offsets from the first window's block in the prefetched set)
            b.d_feat = pb.d_feat + 4 * (size_t)a[0].feat_off;
            if (b.col_lb) b.d_fbox = pb.d_fbox + (size_t)a[0].fb_off * 2 * b.CP;
        }
    } else {
        b.d_feat = A.get<float>(4 * (size_t)b.total_feat_f4);
        if (b.col_lb) {
            b.d_fbox = A.get<float>((size_t)b.total_boxes * 2 * b.CP);
            if (!b.d_fbox) return OBIA_E_NOMEM;
        }
    }
    b.d_labels = A.get<int32_t>((size_t)b.total_pix);
    if (!b.d_mask || !b.d_feat || !b.d_labels) return OBIA_E_NOMEM;
    // first planning phase, up to the read-back of the valid counts: everything that depends on the window shapes alone is ONE upload,
    // queued here so that it travels while the mask and count kernels run -- the windows in both forms, the layout version of the
    // problems and the tile -> problem table (slic_plan_layout) -- and the phase's fills are ONE clear
    TileWin *d_wins = ctx->plan.add(ctx, wins.data(), (size_t)np);
    b.d_windows = ctx->plan.add(ctx, b.windows.data(), (size_t)np);
    if (!d_wins || !b.d_windows) return OBIA_E_NOMEM;
    OBIA_TRY(slic_plan_layout(ctx, b));
    OBIA_TRY(ctx->plan.flush(ctx));
    // the mask kernel's form and grid: its workgroups leave partial sums of the tiles' valid counts, one slot each (all written)
    bool vec4 = (S.W % 4 == 0) && (reinterpret_cast<uintptr_t>(S.inmask) % 4 == 0) && (reinterpret_cast<uintptr_t>(S.G) % 16 == 0) &&
                (reinterpret_cast<uintptr_t>(b.d_mask) % 4 == 0) && (reinterpret_cast<uintptr_t>(d_mask4) % 16 == 0);
    for (auto &t : wins) vec4 = vec4 && (t.x0 % 4 == 0) && (t.w % 4 == 0) && (t.pix_off % 4 == 0);
    const int mask_grid = vec4 ? (grid_rows(wins) + 3) / 4 : grid_rows(wins);
    int *d_tile_any = A.get<int>(np), *d_cnt = A.get<int>((size_t)np * mask_grid);
    if (!d_tile_any || !d_cnt) return OBIA_E_NOMEM;
    if (white) {
        ClearSet clr(ctx);
        OBIA_TRY(clr.add(S.inside, 0, sizeof(unsigned) * (size_t)S.next_id));
        OBIA_TRY(clr.add(d_tile_any, 0, sizeof(int) * (size_t)np));
        OBIA_TRY(clr.flush());
        int cblocks = 1;   // the blocks of the occupancy map a window can meet: one more than its own per axis when it is unaligned
        for (auto &t : wins) cblocks = std::max(cblocks, (cdiv(t.w, 1 << OCC_SHIFT) + 1) * (cdiv(t.h, 1 << OCC_SHIFT) + 1));
        hipLaunchKernelGGL(tile_count_inside_kernel, dim3(cblocks, np), dim3(256), 0, ctx->stream, d_wins, S.G, S.W, S.inside, d_tile_any, S.occ,
                           S.occ_bw);
    }
    if (vec4) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(tile_mask_kernel<true>), dim3(mask_grid, np), dim3(256), 0, ctx->stream, d_wins, S.inmask,
                           S.G, S.W, white ? 1 : 0, S.inside, S.seg_size, S.alive, b.d_mask, d_tile_any, d_mask4, S.occ, S.occ_bw, d_cnt);
        b.d_mask4 = d_mask4;   // (slic_run_sweeps packs the mask itself when nobody did)
    } else {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(tile_mask_kernel<false>), dim3(mask_grid, np), dim3(256), 0, ctx->stream, d_wins, S.inmask,
                           S.G, S.W, white ? 1 : 0, S.inside, S.seg_size, S.alive, b.d_mask, d_tile_any, d_mask4, S.occ, S.occ_bw, d_cnt);
    }
    // per-tile normalisation of every band (create_segments normalises the tile it is given, :32-33)
    std::vector<int> skip;
    if (pre) {
        const size_t NP = S.pf.b.windows.size(), nkeys = NP * (size_t)S.C * 2;
        const unsigned *h = S.pf.host.data();
        OBIA_TRY(slic_features_finish(b, h + S.pf.cursor * (size_t)S.C * 2, h + nkeys + S.pf.cursor, h + nkeys + NP + S.pf.cursor, &skip));
        S.pf.cursor += np;
    } else {
        OBIA_TRY(slic_prepare_features(ctx, b, S.img, S.W, &skip));
    }
    std::vector<int> nvalid;
    debug_sync(ctx, "tiler: mask + features");
    OBIA_TRY(slic_count_valid(ctx, b, nvalid, d_cnt, mask_grid));   // (the mask kernel counted what it wrote: the read-back and the partial sums' sum)
    debug_sync(ctx, "tiler: count_valid");
    std::vector<int> nseg(np);
    const double pixel_area = S.tp.pixel_width * S.tp.pixel_height;
    const double crown_area = M_PI * S.tp.crown_radius * S.tp.crown_radius;
    for (int p = 0; p < np; ++p) {
        double n;
        if (S.sp.n_segments > 0)   // extension: explicit n_segments per full tile, scaled by the valid area
            n = std::nearbyint((double)S.sp.n_segments * (double)nvalid[p] / ((double)S.tp.tile_size * S.tp.tile_size));
        else
            n = std::nearbyint((double)nvalid[p] * pixel_area / crown_area);   // Python round(): half to even
        nseg[p] = (skip[p] || n < 1.0) ? 0 : (n > 2.0e9 ? 2000000000 : (int)n);   // empty tile -> skipped (tiling.py:149-150)
    }
    std::vector<ExternalSeeds> ext;
    if (S.seeding == OBIA_SEEDING_SKIMAGE) OBIA_TRY(seed_tiles_skimage(ctx, S, b, nvalid, nseg, ext));
    OBIA_TRY(slic_plan_and_seed(ctx, b, nseg, &nvalid, ext.empty() ? nullptr : ext.data()));
    debug_sync(ctx, "tiler: plan_and_seed");
    // the connectivity stage's table joins the upload of the sweeps' descriptors (slic_plan_and_seed left it open; the sweeps flush)
    std::vector<CcProblem> cps(np);
    for (int p = 0; p < np; ++p) {
        const SlicProblem &P = b.probs[p];
        const auto [min_size, max_size] = slic_cc_sizes(S.sp.min_size_factor, S.sp.max_size_factor, P.n_valid, P.K);
        cps[p] = CcProblem{P.H, P.W, P.pix_off, min_size, max_size};
    }
    const CcProblem *d_cps = S.sp.enforce_connectivity ? ctx->plan.add(ctx, cps.data(), (size_t)np) : nullptr;
    if (S.sp.enforce_connectivity && !d_cps) return OBIA_E_NOMEM;
    // (a batch whose sweeps all store their labels never shares its pre-pass: the whole black pre-pass is there to run beside, as before)
    if (!white && S.pf.planned && !S.pf.launched)
        OBIA_TRY(prefetch_white_launch(ctx, S, OBIA_PREFETCH_BESIDE != 0 || b.exit_on_fixed_point || b.slic_zero));
    const Arena::Mark sweeps_mk = A.mark();   // a repeat of the sweeps reuses their workspace
    unsigned *const mask4 = b.d_mask4;        // (null: the sweeps pack the mask above the mark)
    OBIA_TRY(slic_run_sweeps(ctx, b));   // (the orphan flag is looked at after the connectivity stage's own synchronisation)
    debug_sync(ctx, "tiler: sweeps");
    int n_new = 0;
    CcResolve resolve{};
    if (S.sp.enforce_connectivity) {
        OBIA_TRY(enforce_connectivity_batch(ctx, cps, b.d_labels, b.total_pix, 1, nullptr, &n_new, &resolve, d_cps));
        bool repeat = false;
        OBIA_TRY(slic_sweeps_settle(ctx, &repeat));
        if (repeat) {   // rare: a valid pixel no window reached kept a label that was not stored -- sweeps with stored labels, stage again
            A.rewind(sweeps_mk);
            b.d_mask4 = mask4;
            OBIA_TRY(slic_rerun_storing(ctx, b));
            OBIA_TRY(enforce_connectivity_batch(ctx, cps, b.d_labels, b.total_pix, 1, nullptr, &n_new, &resolve, d_cps));
            OBIA_TRY(slic_sweeps_settle(ctx, nullptr));   // (the repeat's counters came back beside the connectivity stage's)
        }
        debug_sync(ctx, "tiler: connectivity");
    } else {
        set_error("the tiled driver needs enforce_connectivity=True (segments must be connected pixel sets)");
        return OBIA_E_UNSUPPORTED;
    }
    if (S.next_id + n_new > S.id_cap) { set_error("segment id capacity exceeded (%d + %d > %d)", S.next_id, n_new, S.id_cap); return OBIA_E_NOMEM; }
    if (n_new > 0) {
        int sblocks = 1;
        for (auto &t : wins) sblocks = std::max(sblocks, cdiv(t.w, 64) * cdiv(t.h, 64));
        hipLaunchKernelGGL(tile_scatter_kernel, dim3(sblocks, np), dim3(64), 0, ctx->stream, d_wins, resolve, S.G, S.W,
                           S.next_id - 1, S.seg_size, S.occ, S.occ_bw);
        OBIA_TRY(fill_async(ctx, S.alive + S.next_id, 1, (size_t)n_new));
        S.next_id += n_new;
    }
    OBIA_HIP_TRY(hipGetLastError());
    // (no synchronisation here: every host table of the batch went through the pinned ring, and the arena is reused in stream order)
    OBIA_TRY(ctx->plan.flush(ctx));   // (nothing is open on any path that gets here; a table must not outlive its arena scope)
    A.rewind(mk);
    return OBIA_OK;
}

// ---- seam import (sharded driver): wire codes -> local ids -------------------------------------------------------------------
// 1. every code is translated where it can be (my own ids, ids of `owner` that are in the map); a code of `owner` whose id is not in
//    the map yet claims its map entry (0 -> -1: one claimant per id) and joins the list of new ids; the largest owner id on the
//    seam goes to ctr[1].  An import that meets no new id -- the write-back imports, half of all -- is complete after this kernel.
__global__ __launch_bounds__(256) void seam_mark_kernel(const int32_t *__restrict__ codes, int n, int me, int owner, int32_t *__restrict__ fmap,
                                                        int cap, int *__restrict__ new_list, int *__restrict__ ctr, int32_t *__restrict__ ids) {
    int tmax = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int c = codes[i];
        int id = 0;
        if (c > 0) {
            const int o = (c >> 24) - 1, t = c & 0xffffff;
            if (o == me) id = t;
            else if (o == owner) {
                tmax = max(tmax, t);
                if (t > 0 && t < cap) {
                    const int f = fmap[t];
                    if (f > 0) id = f;
                    else if (f == 0 && atomicCAS(&fmap[t], 0, -1) == 0) new_list[atomicAdd(&ctr[0], 1)] = t;
                }
            }
        }
        ids[i] = id;      // (0 for a new id: seam_translate_kernel fills it in)
    }
    for (int off = 32; off > 0; off >>= 1) tmax = max(tmax, __shfl_xor(tmax, off));
    if ((threadIdx.x & 63) == 0 && tmax > 0) atomicMax(&ctr[1], tmax);
}
// 2. a new id's local id = first + its rank among the new ids (ascending ids of the owner); its wire code is noted.  One workgroup sorts
//    the list in LDS (bitonic, up to SEAM_SORT entries: a seam of BASELINE configs[3] brings ~7 000 new ids); longer lists are ranked
//    by counting (seam_assign_count_kernel).
constexpr int SEAM_SORT = 16384;
__global__ __launch_bounds__(1024) void seam_assign_sort_kernel(int *__restrict__ new_list, int m, int first, int owner,
                                                                int32_t *__restrict__ fmap, int32_t *__restrict__ code_of) {
    __shared__ int s[SEAM_SORT];
    int np2 = 1;
    while (np2 < m) np2 <<= 1;
    for (int i = threadIdx.x; i < np2; i += 1024) s[i] = i < m ? new_list[i] : 0x7fffffff;
    __syncthreads();
    for (int k = 2; k <= np2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < np2; i += 1024) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const int a = s[i], b = s[ixj];
                    if (((i & k) == 0) ? (a > b) : (a < b)) { s[i] = b; s[ixj] = a; }
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < m; i += 1024) {
        const int t = s[i];
        fmap[t] = first + i;
        code_of[first + i] = t | ((owner + 1) << 24);
    }
}
__global__ __launch_bounds__(256) void seam_assign_count_kernel(const int *__restrict__ new_list, int m, int first, int owner,
                                                                int32_t *__restrict__ fmap, int32_t *__restrict__ code_of) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
        const int t = new_list[i];
        int rank = 0;
        for (int j = 0; j < m; ++j) rank += new_list[j] < t;
        fmap[t] = first + rank;
        code_of[first + rank] = t | ((owner + 1) << 24);
    }
}
// 3. the codes of the new ids, translated (only launched when there are new ids)
__global__ __launch_bounds__(256) void seam_translate_kernel(const int32_t *__restrict__ codes, int n, int owner,
                                                             const int32_t *__restrict__ fmap, int cap, int32_t *__restrict__ ids) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (ids[i] != 0) continue;
        const int c = codes[i];
        if (c <= 0 || (c >> 24) - 1 != owner) continue;
        const int t = c & 0xffffff;
        if (t > 0 && t < cap) ids[i] = fmap[t];
    }
}
// a refused import (no room for its new ids) takes its claims back: -1 -> 0, so a later import on the same map meets these ids as new
__global__ __launch_bounds__(256) void seam_unclaim_kernel(const int *__restrict__ new_list, int m, int32_t *__restrict__ fmap) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) fmap[new_list[i]] = 0;
}
__global__ void seam_register_kernel(unsigned *__restrict__ seg_size, uint8_t *__restrict__ alive, int first, int count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) { seg_size[first + i] = 0xffffffffu; alive[first + i] = 1; }
}

static int tiler_check(const float *img, int H, int W, int C, int Hg, int row0, const obia_tiling_params *tp,
                       const obia_slic_params *sp, const int32_t *labels) {
    if (!img || !tp || !sp || !labels) { set_error("null argument"); return OBIA_E_INVALID; }
    if (H <= 0 || W <= 0 || C <= 0 || C > 16) { set_error("bad raster shape (%d,%d,%d)", H, W, C); return OBIA_E_INVALID; }
    if (row0 < 0 || row0 + H > Hg) { set_error("local rows [%d,%d) outside the global raster of %d rows", row0, row0 + H, Hg); return OBIA_E_INVALID; }
    if ((long long)H * W > 0x7fffffffLL) { set_error("raster above 2^31 pixels: shard it across GPUs"); return OBIA_E_INVALID; }
    if (tp->tile_size <= 0 || tp->buffer < 0) { set_error("tile_size must be positive and buffer non-negative"); return OBIA_E_INVALID; }
    if (!(sp->compactness > 0.0) || sp->max_num_iter < 0) { set_error("bad SLIC parameters"); return OBIA_E_INVALID; }
    for (int i = 0; i < 3; ++i) {
        if (!(sp->sigma_zyx[i] >= 0.0)) { set_error("sigma must be >= 0"); return OBIA_E_INVALID; }
        if (!(sp->spacing_zyx[i] > 0.0) || !(sp->spacing_zyx[i] < 1.0e30)) { set_error("spacing must be positive and finite"); return OBIA_E_INVALID; }
    }
    if (!sp->enforce_connectivity) { set_error("the tiled driver needs enforce_connectivity=True (segments must be connected pixel sets)"); return OBIA_E_UNSUPPORTED; }
    if (sp->n_segments <= 0 && !(tp->crown_radius > 0.0 && tp->pixel_width > 0.0 && tp->pixel_height > 0.0)) {
        set_error("crown_radius and pixel size must be positive when n_segments is not given");
        return OBIA_E_INVALID;
    }
    return OBIA_OK;
}

static int tiler_init(obia_ctx *ctx, TileState &S, const float *img, const uint8_t *mask, int H, int W, int C, int Hg,
                      int row0, const obia_tiling_params *tp, const obia_slic_params *sp, int32_t *labels, int extra_ids,
                      bool occupancy = false) {   // occupancy: the caller zero-fills `labels` and nobody else writes it (TileState::occ)
    OBIA_TRY(tiler_check(img, H, W, C, Hg, row0, tp, sp, labels));
    const int T = tp->tile_size, B = tp->buffer;
    Arena &A = ctx->arena;
    // capacity for provisional ids: every tile can create at most its grid of seeds
    const int ntx = cdiv(W, T), nty = cdiv(H, T) + 2;
    const double pixel_area = tp->pixel_width * tp->pixel_height;
    const double crown_area = M_PI * tp->crown_radius * tp->crown_radius;
    const long long wh = (long long)(T + 2 * B) * (T + 2 * B);
    double n = sp->n_segments > 0 ? (double)sp->n_segments * (double)wh / ((double)T * T) : (double)wh * pixel_area / crown_area;
    if (n < 1) n = 1;
    // masked seeding lays a grid for n_eff ~ n over the window; rounding of the step can add ~(1 + 1/S)^2.  (OBIA_SEEDING_SKIMAGE: a tile
    // has K = min(n, n_valid) <= n + 1/2 centroids, n_valid at most the grown window's pixels: inside the same bound.)
    long long cap = (long long)(n * 1.5 + 64.0) * (long long)ntx * nty + 16 + extra_ids;
    if (cap > 0x7ffffff0LL) { set_error("too many segments for int32 ids"); return OBIA_E_INVALID; }
    S.H = H; S.W = W; S.C = C; S.Hg = Hg; S.row0 = row0; S.img = img; S.inmask = mask; S.G = labels; S.tp = *tp; S.sp = *sp;
    S.id_cap = (int)cap; S.next_id = 1;
    slic_batch_settings(S.settings, *sp, C, 1, true);   // the tiler always hands a mask to slic (tiling.py:137-143): maskSLIC structure
    S.settings.start_label = 1;                         // (labels local to a tile; the raster's ids are the tiler's own)
    S.seg_size = A.get<unsigned>((size_t)cap);
    S.inside = A.get<unsigned>((size_t)cap);
    S.alive = A.get<uint8_t>((size_t)cap);
    S.newid = A.get<int>((size_t)cap);
    S.d_total = A.get<long long>(1);
    if (!S.seg_size || !S.inside || !S.alive || !S.newid || !S.d_total) return OBIA_E_NOMEM;
    OBIA_TRY(fill_async(ctx, S.seg_size, 0, sizeof(unsigned) * (size_t)cap));
    OBIA_TRY(fill_async(ctx, S.alive, 0, (size_t)cap));
    S.occ = nullptr;
    S.occ_bw = cdiv(W, 1 << OCC_SHIFT);
    if (occupancy) {
        const size_t words = ((size_t)S.occ_bw * (size_t)cdiv(H, 1 << OCC_SHIFT) + 31) / 32;
        S.occ = A.get<unsigned>(words);
        if (!S.occ) return OBIA_E_NOMEM;
        OBIA_TRY(fill_async(ctx, S.occ, 0, sizeof(unsigned) * words));
    }
    // corner squares: side buffer/2 in MAP units (tiling.py:189), i.e. buffer/2/pixel_size pixels; a pixel is
    // inside when its centre is (rasterize default all_touched=False)
    S.clx = S.cly = S.clx_in = S.cly_in = S.clx_any = S.cly_any = 0;
    if (B > 0) {
        const double cl = (double)B / 2.0;
        // pixel k of an axis (counted from the square's outer edge) spans [k * px, (k + 1) * px) map units; the three counts are the
        // numbers of k with  centre (k + 0.5) * px < cl,  far edge (k + 1) * px <= cl,  near edge k * px < cl  -- evaluated as written,
        // in doubles, so that a quotient like 3.5 / 0.7 landing a hair beside a whole number cannot move a count
        auto count = [](double px, double cl, int kind) {
            if (!(px > 0.0)) px = 1.0;
            long long k = (long long)std::floor(cl / px) + 2;
            if (k < 0) k = 0;
            auto holds = [&](long long i) { return kind == 0 ? (i + 0.5) * px < cl : (kind == 1 ? (i + 1.0) * px <= cl : i * px < cl); };
            while (k > 0 && !holds(k - 1)) --k;     // k = number of pixels 0 .. k-1 for which the statement holds (it is monotone in k)
            return (int)std::min<long long>(k, 0x3fffffff);
        };
        S.clx = count(tp->pixel_width, cl, 0);  S.cly = count(tp->pixel_height, cl, 0);
        S.clx_in = count(tp->pixel_width, cl, 1);  S.cly_in = count(tp->pixel_height, cl, 1);
        S.clx_any = count(tp->pixel_width, cl, 2);  S.cly_any = count(tp->pixel_height, cl, 2);
    }
    return OBIA_OK;
}

// window of the white tile (tj, ti): grown by `buffer`, clamped to the GLOBAL raster, in local rows
static TileWin white_window(const TileState &S, int tj, int ti) {
    const int T = S.tp.tile_size, B = S.tp.buffer;
    const int y0 = std::max(0, tj * T - B), y1 = std::min(S.Hg, tj * T + T + B);
    const int x0 = std::max(0, ti * T - B), x1 = std::min(S.W, ti * T + T + B);
    const int h = y1 - y0, w = x1 - x0;
    return TileWin{y0 - S.row0, x0, h, w, 0, std::min(S.cly, h), std::min(S.clx, w), std::min(S.cly_in, h), std::min(S.clx_in, w),
                   std::min(S.cly_any, h), std::min(S.clx_any, w), 0};
}

// The feature pass of ALL white tiles runs as ONE batch before the white rows (it depends on the raster only), in the
// order in which the white batches will consume the windows: one large launch instead of one per tile row, one read-back
// instead of eight.  plan: windows and buffers (allocated before any batch scope of the arena); launch; fetch: the keys.
// (Running it on a second stream beside the black sweeps was measured: the HBM-bound pass and the VALU-bound sweeps slow
// each other down by more than the overlap gains -- 66.5 vs 63.2 ms per step -- so it stays on the main stream.)
static int prefetch_white_plan(obia_ctx *ctx, TileState &S, int white_order) {
    const int T = S.tp.tile_size;
    const int ntx = cdiv(S.W, T), nty = cdiv(S.Hg, T);
    TileState::PreFeat &pf = S.pf;
    pf = TileState::PreFeat();
    if (S.sp.sigma_zyx[0] > 0.0 || S.sp.sigma_zyx[1] > 0.0 || S.sp.sigma_zyx[2] > 0.0) return OBIA_OK;   // Gaussian pre-smoothing: per-batch features (slic_prepare_features holds the smoothing passes)
    SlicBatch b = S.settings;
    for (int cls = 0; cls < (white_order == 1 ? 2 : 1); ++cls)
        for (int tj = 0; tj < nty; ++tj) {
            if (white_order == 1 && (tj & 1) != cls) continue;
            for (int ti = 0; ti < ntx; ++ti) {
                if ((ti + tj) % 2 == 0) continue;
                const TileWin t = white_window(S, tj, ti);
                if (t.h <= 0 || t.w <= 0) continue;
                if (t.y0 < 0 || t.y0 + t.h > S.H) return OBIA_OK;   // the batches report the halo error
                b.windows.push_back(SrcWindow{t.y0, t.x0, t.h, t.w, 0, 0, 0});
            }
        }
    const size_t NP = b.windows.size();
    if (NP == 0) return OBIA_OK;
    // too big to hold: per-batch features
    if (slic_batch_layout(b) != OBIA_OK) return OBIA_OK;
    pf.fused = slic_fuse_features(b, S.img, S.W);
    if (!pf.fused && (double)b.total_feat_f4 * 16.0 > 32.0 * 1024 * 1024 * 1024) return OBIA_OK;
    Arena &A = ctx->arena;
    const size_t ntot = NP * (size_t)S.C * 2 + 2 * NP;
    b.d_windows = A.get<SrcWindow>(NP);
    pf.d_keys = A.get<unsigned>(ntot);
    if (!pf.fused) b.d_feat = A.get<float>(4 * (size_t)b.total_feat_f4);
    if (!b.d_windows || !pf.d_keys || (!pf.fused && !b.d_feat)) return OBIA_E_NOMEM;
    if (b.col_lb) {
        b.d_fbox = A.get<float>((size_t)b.total_boxes * 2 * b.CP);
        if (!b.d_fbox) return OBIA_E_NOMEM;
    }
    pf.host.resize(ntot);
    pf.b = std::move(b);
    pf.planned = true;
    return OBIA_OK;
}

static int prefetch_white_launch(obia_ctx *ctx, TileState &S, bool beside) {
    TileState::PreFeat &pf = S.pf;
    if (pf.launched || !pf.planned) return OBIA_OK;
    pf.launched = true;
    if (pf.fused) beside = false;   // (the side stream stays for the unfused batches that have it: exit_on_fixed_point, SLIC-zero)
    OBIA_TRY(upload_async(ctx, pf.b.d_windows, pf.b.windows.data(), sizeof(SrcWindow) * pf.b.windows.size()));
    if (beside) {
        // `beside`: on a side stream, forked here and joined in prefetch_white_fetch -- the caller queues the black batch's
        // spatial pre-pass next, a kernel that is bound by vector issue and moves no data, beside this pass, which is bound by HBM
        OBIA_TRY(side_stream(ctx));
        hipStream_t side = ctx->side;
        OBIA_HIP_TRY(hipEventRecord(ctx->aux_fork, ctx->stream));
        OBIA_HIP_TRY(hipStreamWaitEvent(side, ctx->aux_fork, 0));
        OBIA_TRY(slic_features_launch(side, pf.b, S.img, S.W, pf.d_keys, nullptr, false));
        OBIA_HIP_TRY(hipEventRecord(ctx->aux_join, side));
        pf.on_side = true;
        return OBIA_OK;
    }
    ScopedSpan span(ctx, T_FEAT);
    OBIA_TRY(slic_features_launch(ctx->stream, pf.b, S.img, S.W, pf.d_keys, nullptr, pf.fused));
    return OBIA_OK;
}

static int prefetch_white_fetch(obia_ctx *ctx, TileState &S) {
    if (!S.pf.planned) return OBIA_OK;
    OBIA_TRY(prefetch_white_launch(ctx, S));
    if (S.pf.on_side) { OBIA_HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->aux_join, 0)); S.pf.on_side = false; }
    OBIA_TRY(read_back(ctx, S.pf.host.data(), S.pf.d_keys, S.pf.host.size() * sizeof(unsigned)));
    S.pf.ready = true;
    S.pf.cursor = 0;
    return OBIA_OK;
}

// Tiles of GLOBAL tile rows [tr_lo, tr_hi) with (tr % 2 == parity) when parity is 0 or 1.  Black tiles: exact
// windows, one batch for the whole range.  White tiles: windows grown by `buffer` and clamped to the GLOBAL
// raster, one batch per tile-row (windows of one tile-row never overlap; those of adjacent rows overlap at
// corners).  Every window must lie inside the local rows.
static int tiler_run(obia_ctx *ctx, TileState &S, bool white, int tr_lo, int tr_hi, int parity) {
    const int T = S.tp.tile_size, B = S.tp.buffer;
    const int ntx = cdiv(S.W, T), nty = cdiv(S.Hg, T);
    if (tr_lo < 0) tr_lo = 0;
    if (tr_hi > nty) tr_hi = nty;
    // white tile rows of ONE parity class do not see each other (their windows are T - 2B rows apart): the whole class is
    // one batch; in raster order every row sees the corner overlaps of the row before it: one batch per row
    const bool per_row = !(parity >= 0 && T > 2 * B);
    // tile_size <= 2 * buffer: the grown windows of two white tiles of ONE tile row overlap (they are T - 2B columns apart), so
    // even a row cannot be one batch -- every white tile runs on its own, in the reference's order (tiling.py:156-287)
    const bool per_tile = white && T <= 2 * B;
    std::vector<TileWin> wins;
    auto flush = [&]() -> int {
        for (auto &t : wins)
            if (t.y0 < 0 || t.y0 + t.h > S.H) { set_error("tile window rows [%d,%d) (local) outside the %d local rows: halo too small", t.y0, t.y0 + t.h, S.H); return OBIA_E_INVALID; }
        int rc = run_tile_batch(ctx, S, wins, white);
        wins.clear();
        return rc;
    };
    for (int tj = tr_lo; tj < tr_hi; ++tj) {
        if (parity >= 0 && (tj & 1) != parity) continue;
        for (int ti = 0; ti < ntx; ++ti) {
            const bool is_white = (ti + tj) % 2 != 0;
            if (is_white != white) continue;
            if (!white) {
                TileWin t{tj * T - S.row0, ti * T, std::min(T, S.Hg - tj * T), std::min(T, S.W - ti * T), 0, 0, 0, 0, 0, 0, 0, 0};
                if (t.h > 0 && t.w > 0) wins.push_back(t);
            } else {
                const TileWin t = white_window(S, tj, ti);
                if (t.h > 0 && t.w > 0) wins.push_back(t);
                if (per_tile && !wins.empty()) OBIA_TRY(flush());
            }
        }
        if (white && per_row) OBIA_TRY(flush());
    }
    if (!wins.empty()) OBIA_TRY(flush());
    return OBIA_OK;
}

// ids 1..N: black survivors first, then white, each in creation order (tiling.py:289-290)
static int tiler_finalize(obia_ctx *ctx, TileState &S, int64_t *n_segments_out) {
    const int nchunks = cdiv(S.next_id, IDS_CHUNK);
    int *d_partial = ctx->arena.get<int>((size_t)nchunks);
    if (!d_partial) return OBIA_E_NOMEM;
    hipLaunchKernelGGL(ids_count_kernel, dim3(nchunks), dim3(1024), 0, ctx->stream, S.alive, S.next_id, d_partial);
    hipLaunchKernelGGL(ids_scan_kernel, dim3(nchunks), dim3(1024), 0, ctx->stream, S.alive, S.next_id, d_partial, S.newid, S.d_total);
    const int g = (int)grids::tiler_ids_apply((long long)S.H * S.W).x.n;
    hipLaunchKernelGGL(ids_apply_kernel, dim3(g), dim3(256), 0, ctx->stream, S.G, (long long)S.H * S.W, S.newid);
    OBIA_HIP_TRY(hipGetLastError());
    long long total = 0;
    OBIA_TRY(read_back(ctx, &total, S.d_total, sizeof(long long)));
    if (n_segments_out) *n_segments_out = total;
    return OBIA_OK;
}

static int check_seeding(int seeding, obia_pick_fn picks) {
    if (seeding != OBIA_SEEDING_GRID && seeding != OBIA_SEEDING_SKIMAGE) { set_error("seeding must be OBIA_SEEDING_GRID or OBIA_SEEDING_SKIMAGE (got %d)", seeding); return OBIA_E_INVALID; }
    if (seeding == OBIA_SEEDING_SKIMAGE && !picks) { set_error("seeding = skimage needs a pick function"); return OBIA_E_INVALID; }
    return OBIA_OK;
}

static int tiled_slic_dev(obia_ctx *ctx, const float *img, const uint8_t *mask, int H, int W, int C,
                          const obia_tiling_params *tp, const obia_slic_params *sp, int seeding, obia_pick_fn picks, void *picks_user,
                          int32_t *labels_out, int64_t *n_segments_out) {
    TileState S;
    OBIA_TRY(check_seeding(seeding, picks));
    // OBIA_G_OCCUPANCY=0 (developer switch, read once per call): no occupancy map, the label passes read every block of the raster
    const char *occ_env = std::getenv("OBIA_G_OCCUPANCY");
    OBIA_TRY(tiler_init(ctx, S, img, mask, H, W, C, H, 0, tp, sp, labels_out, 0, !(occ_env && occ_env[0] == '0')));
    S.seeding = seeding; S.pick_fn = picks; S.pick_user = picks_user;
    OBIA_TRY(fill_async(ctx, labels_out, 0, sizeof(int32_t) * (size_t)H * W));
    const int nty = cdiv(H, tp->tile_size);
    OBIA_TRY(prefetch_white_plan(ctx, S, tp->white_order));               // features of all white tiles: one batch
    OBIA_TRY(tiler_run(ctx, S, false, 0, nty, -1));                       // pass 1: black tiles
    if (std::getenv("OBIA_DEBUG_FAIL_AFTER_BLACK")) {   // test hook (tests/test_gpu_edge_cases.py): an error while the white feature pass is still on its side stream
        set_error("debug: forced failure after the black pass");
        return OBIA_E_INVALID;
    }
    OBIA_TRY(prefetch_white_fetch(ctx, S));
    if (tp->white_order == 1) {                                           // pass 2, two parity classes of tile rows
        OBIA_TRY(tiler_run(ctx, S, true, 0, nty, 0));
        OBIA_TRY(tiler_run(ctx, S, true, 0, nty, 1));
    } else {
        OBIA_TRY(tiler_run(ctx, S, true, 0, nty, -1));                    // pass 2, the reference's raster order
    }
    return tiler_finalize(ctx, S, n_segments_out);
}

}  // namespace obia

struct obia_tiler {
    obia_ctx *ctx;
    obia::TileState S;
    int *seam_buf = nullptr;      // scratch of obia_tiler_import_seam: two counters + the list of new ids
    size_t seam_cap = 0;
};

using namespace obia;

// Prologue of the session's entry points: the null-tiler check, then the context's (common.hpp).  The error path of a session is
// quiesce(): the white tiles' feature pass runs on the side stream beside the black batch and is joined only when the white pass
// starts -- a failure in between must not return while that pass can still read the caller's raster and write arena memory.
static int enter(obia_tiler *t) {
    if (!t) { set_error("null tiler"); return OBIA_E_INVALID; }
    return enter(t->ctx, t);
}

extern "C" {

obia_tiler *obia_tiler_create(obia_ctx *ctx, const float *img_local, const uint8_t *mask_local, int H_local, int W, int C,
                              int H_global, int row0, const obia_tiling_params *tiling, const obia_slic_params *params,
                              int32_t *labels_local, int extra_ids) {
    if (enter(ctx) != OBIA_OK) return nullptr;   // (a context that another session holds is refused here: no frame begins)
    frame_begin(ctx, FRAME_TIMING);   // the session is one frame: obia_tiler_destroy() ends it
    obia_tiler *t = new obia_tiler();
    t->ctx = ctx;
    if (tiler_init(ctx, t->S, img_local, mask_local, H_local, W, C, H_global, row0, tiling, params, labels_local,
                   extra_ids < 0 ? 0 : extra_ids) != OBIA_OK) { delete t; return nullptr; }
    ctx->session = t;   // from here to obia_tiler_destroy the context serves this session alone (common.hpp: enter)
    return t;
}

void obia_tiler_destroy(obia_tiler *t) {
    if (!t) return;
    (void)enter(t->ctx, t);
    (void)quiesce(t->ctx, 0);   // (a session dropped half-way may have left the white feature pass on its side stream)
    if (t->seam_buf) (void)hipFree(t->seam_buf);
    resolve_timing(t->ctx);
    t->ctx->session = nullptr;
    delete t;
}

int obia_tiler_run(obia_tiler *t, int white, int tile_row_lo, int tile_row_hi, int row_parity) {
    OBIA_TRY(enter(t));
    const int rc = tiler_run(t->ctx, t->S, white != 0, tile_row_lo, tile_row_hi, row_parity);
    if (rc != OBIA_OK) return quiesce(t->ctx, rc);
    OBIA_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
    return OBIA_OK;
}

int obia_tiler_next_id(obia_tiler *t) { return t ? t->S.next_id : -1; }

int obia_tiler_set_seeding(obia_tiler *t, int seeding, obia_pick_fn picks, void *picks_user) {
    OBIA_TRY(enter(t));
    OBIA_TRY(check_seeding(seeding, picks));
    t->S.seeding = seeding; t->S.pick_fn = picks; t->S.pick_user = picks_user;
    return OBIA_OK;
}

int obia_tiler_set_segments(obia_tiler *t, int first_id, int count, const uint32_t *sizes_dev) {
    OBIA_TRY(enter(t));
    if (!sizes_dev || first_id < 1 || count < 0) { set_error("bad arguments"); return OBIA_E_INVALID; }
    if (first_id + count > t->S.id_cap) { set_error("segment id capacity exceeded (%d + %d > %d)", first_id, count, t->S.id_cap); return OBIA_E_NOMEM; }
    if (count == 0) return OBIA_OK;
    OBIA_HIP_TRY(hipMemcpyAsync(t->S.seg_size + first_id, sizes_dev, sizeof(uint32_t) * (size_t)count, hipMemcpyDeviceToDevice, t->ctx->stream));
    OBIA_TRY(fill_async(t->ctx, t->S.alive + first_id, 1, (size_t)count));
    if (first_id + count > t->S.next_id) t->S.next_id = first_id + count;
    OBIA_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
    return OBIA_OK;
}

int obia_tiler_get_alive(obia_tiler *t, uint8_t *alive_out_dev, int count) {
    OBIA_TRY(enter(t));
    if (!alive_out_dev || count < 0 || count > t->S.id_cap) { set_error("bad arguments"); return OBIA_E_INVALID; }
    OBIA_HIP_TRY(hipMemcpyAsync(alive_out_dev, t->S.alive, (size_t)count, hipMemcpyDeviceToDevice, t->ctx->stream));
    OBIA_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
    return OBIA_OK;
}

int obia_tiler_set_alive(obia_tiler *t, const uint8_t *alive_in_dev, int count) {
    OBIA_TRY(enter(t));
    if (!alive_in_dev || count < 0 || count > t->S.id_cap) { set_error("bad arguments"); return OBIA_E_INVALID; }
    OBIA_HIP_TRY(hipMemcpyAsync(t->S.alive, alive_in_dev, (size_t)count, hipMemcpyDeviceToDevice, t->ctx->stream));
    OBIA_HIP_TRY(hipStreamSynchronize(t->ctx->stream));
    return OBIA_OK;
}

int obia_tiler_import_seam(obia_tiler *t, const int32_t *codes_dev, int n, int my_rank, int owner_rank,
                           int32_t *fmap_dev, int fmap_cap, int32_t *code_of_dev, int32_t *ids_out_dev,
                           int *first_new_out, int *n_new_out, int *max_owner_id_out) {
    OBIA_TRY(enter(t));
    if (!codes_dev || !fmap_dev || !code_of_dev || !ids_out_dev || n < 0 || fmap_cap < 1 || my_rank < 0 || owner_rank < 0 ||
        my_rank > 126 || owner_rank > 126 || !first_new_out || !n_new_out || !max_owner_id_out) { set_error("bad arguments"); return OBIA_E_INVALID; }
    obia_ctx *ctx = t->ctx;
    *first_new_out = t->S.next_id; *n_new_out = 0; *max_owner_id_out = 0;
    if (n == 0) return OBIA_OK;
    // scratch outside the arena (the session's arena holds the tiler's persistent state): one small allocation kept by the session
    if (t->seam_cap < (size_t)n + 2) {
        if (t->seam_buf) (void)hipFree(t->seam_buf);
        t->seam_buf = nullptr; t->seam_cap = 0;
        if (hipMalloc(&t->seam_buf, sizeof(int) * ((size_t)n + 2)) != hipSuccess) { set_error("seam scratch allocation failed"); return OBIA_E_NOMEM; }
        t->seam_cap = (size_t)n + 2;
    }
    int *ctr = t->seam_buf, *new_list = t->seam_buf + 2;
    OBIA_TRY(fill_async(ctx, ctr, 0, sizeof(int) * 2));
    const int blocks = (int)grids::tiler_seam(n).x.n;
    hipLaunchKernelGGL(seam_mark_kernel, dim3(blocks), dim3(256), 0, ctx->stream, codes_dev, n, my_rank, owner_rank, fmap_dev, fmap_cap, new_list, ctr,
                       ids_out_dev);
    int h[2] = {0, 0};
    OBIA_TRY(read_back(ctx, h, ctr, sizeof(h)));   // the one read-back of an import: how many ids are new, the largest id on the seam
    *max_owner_id_out = h[1];
    const int n_new = h[0];
    if (t->S.next_id + n_new > t->S.id_cap) {
        // refused whole: the map entries seam_mark_kernel claimed go back to "not imported", the session's state was not touched
        hipLaunchKernelGGL(seam_unclaim_kernel, dim3((unsigned)grids::tiler_seam(n_new).x.n), dim3(256), 0, ctx->stream, new_list, n_new, fmap_dev);
        OBIA_HIP_TRY(hipStreamSynchronize(ctx->stream));
        set_error("segment id capacity exceeded (%d + %d > %d)", t->S.next_id, n_new, t->S.id_cap);
        return OBIA_E_NOMEM;
    }
    if (n_new > 0) {
        if (n_new <= SEAM_SORT)
            hipLaunchKernelGGL(seam_assign_sort_kernel, dim3(1), dim3(1024), 0, ctx->stream, new_list, n_new, t->S.next_id, owner_rank, fmap_dev, code_of_dev);
        else
            hipLaunchKernelGGL(seam_assign_count_kernel, dim3(256), dim3(256), 0, ctx->stream, new_list, n_new, t->S.next_id, owner_rank, fmap_dev, code_of_dev);
        hipLaunchKernelGGL(seam_translate_kernel, dim3(blocks), dim3(256), 0, ctx->stream, codes_dev, n, owner_rank, fmap_dev, fmap_cap, ids_out_dev);
        // registered like obia_tiler_set_segments(first, n_new, 0xffffffff ...): sizes follow from the caller's halo
        hipLaunchKernelGGL(seam_register_kernel, dim3(cdiv(n_new, 256)), dim3(256), 0, ctx->stream, t->S.seg_size, t->S.alive, t->S.next_id, n_new);
        t->S.next_id += n_new;
        // (the session's entry points return with their work done -- the caller reads ids_out on a stream of its own; an import
        // that brought nothing new was complete at the read-back above)
        OBIA_HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    *n_new_out = n_new;   // (when h[1] >= fmap_cap the ids beyond the map were not translated: the caller calls again with a larger map;
                          // what this call imported stays imported)
    OBIA_HIP_TRY(hipGetLastError());
    return OBIA_OK;
}

int obia_test_seam_sort_limit(void) { return SEAM_SORT; }

int obia_tiler_finalize(obia_tiler *t, int64_t *n_segments_out) {
    OBIA_TRY(enter(t));
    const int rc = tiler_finalize(t->ctx, t->S, n_segments_out);
    return rc == OBIA_OK ? rc : quiesce(t->ctx, rc);
}

int obia_tiled_slic_seeded_f32_dev(obia_ctx *ctx, const float *img, const uint8_t *mask, int H, int W, int C,
                                   const obia_tiling_params *tiling, const obia_slic_params *params, int seeding,
                                   obia_pick_fn picks, void *picks_user, int32_t *labels_out, int64_t *n_segments_out) {
    OBIA_TRY(enter(ctx));
    return call_frame(ctx, FRAME_TOTAL, [&] {
        return tiled_slic_dev(ctx, img, mask, H, W, C, tiling, params, seeding, picks, picks_user, labels_out, n_segments_out);
    });
}

int obia_tiled_slic_f32_dev(obia_ctx *ctx, const float *img, const uint8_t *mask, int H, int W, int C,
                            const obia_tiling_params *tiling, const obia_slic_params *params, int32_t *labels_out,
                            int64_t *n_segments_out) {
    return obia_tiled_slic_seeded_f32_dev(ctx, img, mask, H, W, C, tiling, params, OBIA_SEEDING_GRID, nullptr, nullptr, labels_out, n_segments_out);
}

int obia_tiled_slic_seeded_f32(obia_ctx *ctx, const float *img, const uint8_t *mask, int H, int W, int C,
                               const obia_tiling_params *tiling, const obia_slic_params *params, int seeding,
                               obia_pick_fn picks, void *picks_user, int32_t *labels_out, int64_t *n_segments_out) {
    OBIA_TRY(enter(ctx));
    if (!img || !labels_out || H <= 0 || W <= 0 || C <= 0) { set_error("bad arguments"); return OBIA_E_INVALID; }
    OBIA_TRY(check_seeding(seeding, picks));
    const size_t npix = (size_t)H * W;
    Staging s(ctx);
    const float *d_img = s.in(img, npix * C);
    const uint8_t *d_mask = s.in(mask, npix);
    int32_t *d_lab = s.out<int32_t>(npix);
    s.run([&] {
        return obia_tiled_slic_seeded_f32_dev(ctx, d_img, d_mask, H, W, C, tiling, params, seeding, picks, picks_user, d_lab, n_segments_out);
    });
    s.fetch(labels_out, d_lab, npix);
    return s.finish();
}

int obia_tiled_slic_f32(obia_ctx *ctx, const float *img, const uint8_t *mask, int H, int W, int C,
                        const obia_tiling_params *tiling, const obia_slic_params *params, int32_t *labels_out,
                        int64_t *n_segments_out) {
    return obia_tiled_slic_seeded_f32(ctx, img, mask, H, W, C, tiling, params, OBIA_SEEDING_GRID, nullptr, nullptr, labels_out, n_segments_out);
}

}  // extern "C"
