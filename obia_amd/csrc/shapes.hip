// shapes.hip -- area, raw moments, perimeter and bounding box of every segment of a label raster (include/obia_shapes.h): the one
// all-pixel pass of the shape columns.  DESIGN.md 3.5w.
//
// The tiles and the launch are those of adjacency.hip.  A workgroup of 256 stages a tile of TH x TW labels with a halo of one pixel on
// every side in LDS, already mapped to 0 .. N - 1 (segment), N (background) or N + 1 (outside the raster).  A wave holds two tile
// rows, a pixel per lane.  A superpixel row is a run of many equal labels, so the pixels are not added one by one: three ballots --
// "a run starts here", "the pixel above differs", "the pixel below differs" -- tell the first lane of every run where the run ends
// and how many of its upper and lower edges are border edges, and the sums of a run of a row are closed forms of its two ends.  Only
// that lane touches the table: a hash table in LDS keyed by segment, 32-bit accumulators in tile coordinates, the box as two bit
// masks (rows, columns) that an atomic OR fills.  A slot taken for the first time is noted in a list; the tile is flushed by walking
// the list: the sums are moved to raster coordinates and added with 64-bit integer atomics, the box goes out as four integer maxima
// (the two lower ends as H - r0 and W - c0, so that a zeroed table is the neutral element of all four), and the lane that flushed a
// slot clears it.  A last small kernel turns the two lower ends back.  A tile holds at most TH * TW segments in a table of twice as
// many slots, so nothing overflows.
//
// Nothing here takes memory from the context's workspace: every buffer is the caller's.  Every atomic is an integer atomic.
#include "common.hpp"
#include "../../include/obia_shapes.h"

#include <climits>

namespace obia {
namespace {

constexpr int TH = OBIA_ADJ_TILE_H, TW = OBIA_ADJ_TILE_W, CAP = OBIA_SHAPE_TABLE;
constexpr int SW = TW + 2, STAGED = (TH + 2) * SW;              // the staged tile: a halo of one pixel all round
constexpr int MAXSEG = TH * TW;                                 // segments a tile holds at the most
constexpr int NACC = 9;                                         // n, sum lr, sum lc, sum lr^2, sum lc^2, sum lr lc, perimeter, row mask, column mask
static_assert(TW == 32 && TH <= 32 && (TH * TW) % 256 == 0, "a tile row is half a wave; the rows of a tile fit a 32-bit mask");
static_assert((CAP & (CAP - 1)) == 0 && CAP > MAXSEG && CAP <= 65536, "the table holds every segment of a tile; a slot index fits 16 bits");
static_assert((long long)MAXSEG * (TW - 1) * (TW - 1) < INT_MAX, "a tile's sums fit 32 bits");
static_assert((size_t)CAP * 4 * (NACC + 1) + (size_t)MAXSEG * 2 + (size_t)STAGED * 4 + 16 <= 64 * 1024, "table, list and tile fit the LDS of a workgroup");

__global__ __launch_bounds__(256) void shape_tile_kernel(const int *__restrict__ labels, int H, int W, int start, int N,
                                                         unsigned long long *sums, int *box) {
    __shared__ int keys[CAP];                                    // segment + 1; 0: free
    __shared__ int acc[NACC][CAP];
    __shared__ unsigned short list[MAXSEG];                      // the slots taken, in the order they were taken
    __shared__ int lab[STAGED];
    __shared__ int s_n;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < CAP; i += 256) {
        keys[i] = 0;
        for (int k = 0; k < NACC; ++k) acc[k][i] = 0;
    }
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int ntx = (W + TW - 1) / TW, nty = (H + TH - 1) / TH;

    for (int ty = blockIdx.y; ty < nty; ty += gridDim.y)
        for (int tx = blockIdx.x; tx < ntx; tx += gridDim.x) {
            const int r0 = ty * TH, c0 = tx * TW;
            for (int i = tid; i < STAGED; i += 256) {
                const int r = i / SW, c = i - r * SW;
                const int gr = r0 + r - 1, gc = c0 + c - 1;
                int v = N + 1;
                if (gr >= 0 && gr < H && gc >= 0 && gc < W) {
                    const long long d = (long long)labels[(long long)gr * W + gc] - (long long)start;
                    v = (d >= 0 && d < (long long)N) ? (int)d : N;
                }
                lab[i] = v;
            }
            __syncthreads();
            for (int p = tid; p < TH * TW; p += 256) {           // whole trips: every lane of a wave takes part in the ballots
                const int r = p / TW, c = p - r * TW;
                const int at = (r + 1) * SW + c + 1;
                const int a = lab[at], left = lab[at - 1];
                const bool head = c == 0 || left != a;
                const unsigned long long heads = __ballot(head), ups = __ballot(lab[at - SW] != a), downs = __ballot(lab[at + SW] != a);
                if (!head || a >= N) continue;                   // background and the pixels outside the raster start runs and add nothing
                // the run ends before the next head of this tile row (lanes 0 .. 31 are one row, 32 .. 63 the next)
                const unsigned long long above = lane == 63 ? 0ull : heads & (~0ull << (lane + 1));
                int end = above ? __builtin_ctzll(above) : 64;
                const int row_end = (lane | 31) + 1;
                if (end > row_end) end = row_end;
                const int len = end - lane;                      // 1 .. 32
                const unsigned long long run = (len == 64 ? ~0ull : (1ull << len) - 1ull) << lane;
                const int cb = c + len - 1;                      // the run is the columns c .. cb of row r
                const int per = __popcll(ups & run) + __popcll(downs & run) + (left != a) + (lab[at + len] != a);
                const int slc = (c + cb) * len / 2;
                const int slc2 = cb * (cb + 1) * (2 * cb + 1) / 6 - (c - 1) * c * (2 * c - 1) / 6;
                unsigned slot = ((unsigned)a * 2654435761u) >> 16 & (CAP - 1);
                for (int probes = 0; probes < CAP; ++probes) {   // ends at a free slot: CAP > MAXSEG
                    const int seen = atomicCAS(&keys[slot], 0, a + 1);
                    if (seen == 0) {
                        const int k = atomicAdd(&s_n, 1);
                        if (k < MAXSEG) list[k] = (unsigned short)slot;   // always: a tile holds no more segments
                    }
                    if (seen == 0 || seen == a + 1) {
                        atomicAdd(&acc[0][slot], len);
                        if (r) atomicAdd(&acc[1][slot], len * r);
                        if (slc) atomicAdd(&acc[2][slot], slc);
                        if (r) atomicAdd(&acc[3][slot], len * r * r);
                        if (slc2) atomicAdd(&acc[4][slot], slc2);
                        if (r && slc) atomicAdd(&acc[5][slot], r * slc);
                        if (per) atomicAdd(&acc[6][slot], per);
                        atomicOr(&acc[7][slot], 1 << r);
                        atomicOr(&acc[8][slot], (int)(unsigned)(run >> (lane & 32)));
                        break;
                    }
                    slot = (slot + 1) & (CAP - 1);
                }
            }
            __syncthreads();
            const int n = s_n < MAXSEG ? s_n : MAXSEG;
            for (int e = tid; e < n; e += 256) {
                const int slot = list[e];
                const long long seg = keys[slot] - 1;
                const long long cnt = acc[0][slot], lr = acc[1][slot], lc = acc[2][slot], lr2 = acc[3][slot], lc2 = acc[4][slot], lrc = acc[5][slot];
                const long long R = r0, C = c0;
                unsigned long long *row = sums + seg * OBIA_SHAPE_SUMS;
                atomicAdd(&row[0], (unsigned long long)cnt);
                atomicAdd(&row[1], (unsigned long long)(lr + cnt * R));
                atomicAdd(&row[2], (unsigned long long)(lc + cnt * C));
                atomicAdd(&row[3], (unsigned long long)(lr2 + 2 * R * lr + cnt * R * R));
                atomicAdd(&row[4], (unsigned long long)(lc2 + 2 * C * lc + cnt * C * C));
                atomicAdd(&row[5], (unsigned long long)(lrc + R * lc + C * lr + cnt * R * C));
                atomicAdd(&row[6], (unsigned long long)acc[6][slot]);
                const unsigned rows = (unsigned)acc[7][slot], cols = (unsigned)acc[8][slot];   // not zero: the slot holds a run
                int *corner = box + seg * 4;
                atomicMax(&corner[0], H - (r0 + __builtin_ctz(rows)));
                atomicMax(&corner[1], W - (c0 + __builtin_ctz(cols)));
                atomicMax(&corner[2], r0 + 32 - __builtin_clz(rows));
                atomicMax(&corner[3], c0 + 32 - __builtin_clz(cols));
                keys[slot] = 0;                                  // the lane that read a slot clears it: no full clear per tile
                for (int k = 0; k < NACC; ++k) acc[k][slot] = 0;
            }
            __syncthreads();
            if (tid == 0) s_n = 0;
            __syncthreads();
        }
}

// the lower ends of the box were kept as H - r0 and W - c0 (above); a row without pixels stays all zeros
__global__ __launch_bounds__(256) void shape_box_kernel(const long long *__restrict__ sums, int *__restrict__ box, int n, int H, int W) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        if (sums[i * OBIA_SHAPE_SUMS] <= 0) continue;
        box[i * 4] = H - box[i * 4];
        box[i * 4 + 1] = W - box[i * 4 + 1];
    }
}

}  // namespace
}  // namespace obia

using namespace obia;

extern "C" {

int obia_shape_sums_dev(obia_ctx *ctx, const int32_t *labels, int H, int W, int32_t start_label, int32_t n_labels, int64_t *sums_out,
                        int32_t *box_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"shapes", "sums"};
    if (Buffers().out(sums_out, n_labels > 0).out(box_out, n_labels > 0).in(labels).bad()) return refuse.buffers();
    OBIA_TRY(refuse.labels(n_labels));
    OBIA_TRY(refuse.raster_below_2_31(H, W));
    const unsigned __int128 side = (unsigned __int128)(H > W ? H : W);
    if (side * side * (unsigned __int128)((long long)H * W) >= (unsigned __int128)1 << 63) {
        set_error("shapes: sums: max(H, W)^2 * H * W must be below 2^63 (no sum can overflow then), got %d x %d", H, W);
        return OBIA_E_UNSUPPORTED;
    }
    if (n_labels == 0) return OBIA_OK;
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        OBIA_TRY(fill_async(ctx, sums_out, 0, (size_t)n_labels * OBIA_SHAPE_SUMS * sizeof(int64_t)));
        OBIA_TRY(fill_async(ctx, box_out, 0, (size_t)n_labels * 4 * sizeof(int32_t)));
        hipLaunchKernelGGL(shape_tile_kernel, to_dim3(grids::adj_tiles(H, W)), dim3(256), 0, ctx->stream, labels, H, W, start_label, n_labels,
                           reinterpret_cast<unsigned long long *>(sums_out), box_out);
        OBIA_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(shape_box_kernel, to_dim3(grids::flat(n_labels)), dim3(256), 0, ctx->stream, reinterpret_cast<const long long *>(sums_out),
                           box_out, n_labels, H, W);
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}

}  // extern "C"
