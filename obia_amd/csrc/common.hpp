// common.hpp -- context, device workspace arena, error plumbing shared by the HIP translation units.
//
// An extern "C" function is its body between four shared pieces (the entry layer, below): enter(), the prologue; Buffers and Refusal
// (buffer_args.hpp), the argument checks -- every buffer listed once, every refusal worded in one place; call_frame(), for a call that
// returns with its work done; Staging, for a call that takes host pointers.  A new operator uses them and writes none of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/obia_hip.h"
#include "buffer_args.hpp"
#include "launch_grids.hpp"

struct obia_ctx;

namespace obia {

void set_error(const char *fmt, ...);   // (buffer_args.hpp declares it too: that header stands alone)

#define OBIA_HIP_TRY(expr)                                                                       \
    do {                                                                                         \
        hipError_t e__ = (expr);                                                                 \
        if (e__ != hipSuccess) {                                                                 \
            obia::set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(e__)); \
            return OBIA_E_HIP;                                                                   \
        }                                                                                        \
    } while (0)

#define OBIA_TRY(expr)            \
    do {                          \
        int rc__ = (expr);        \
        if (rc__ != OBIA_OK) return rc__; \
    } while (0)

// Bump allocator over a few large hipMalloc blocks.  reset() keeps the memory; when a call needed
// more than one block the blocks are merged into one at the next reset, so a steady-state call
// performs no hipMalloc at all.
class Arena {
  public:
    ~Arena() { release(); }
    void *alloc(size_t bytes);
    template <typename T> T *get(size_t n) { return static_cast<T *>(alloc(n * sizeof(T))); }
    void reset();
    void release();
    // mark()/rewind(): scoped reuse inside one call (per tile batch)
    struct Mark { size_t block, used, total; };
    Mark mark() const;
    void rewind(const Mark &m);
    size_t capacity() const;
    bool failed() const { return failed_; }
    // Test support (obia_test_poison_workspace_dev): makes the arena ONE block of at least `bytes` -- allocates, then resets, which
    // merges several blocks into one -- so that the next frame's reset() neither frees nor grows.  Returns the block (null: the
    // allocation failed) and its whole size.  Nothing may be running on the arena's memory.
    char *one_block(size_t bytes, size_t *size_out);

  private:
    struct Block { char *p; size_t size; size_t used; };
    std::vector<Block> blocks_;
    size_t high_water_ = 0, cur_total_ = 0, cur_ = 0;
    bool failed_ = false;
};

// The host tables of ONE planning phase -- the host code between two synchronisations -- as ONE upload.  add() copies a table into
// the blob's slot of the pinned ring and returns where it WILL be on the device: both sides are reserved as one block when the first
// table arrives (the device side from the arena, so it lives as long as the arena scope it was opened in), every table aligned to 16
// bytes.  flush() issues the one copy; it must stand in front of the first kernel that reads a table, and a blob is closed by it: the
// next add() opens another.  read_back() flushes an open blob before it waits, so no table is ever left behind a synchronisation.
// A table that does not fit into what is left of the block closes it (one more upload, nothing else).
class PlanBlob {
  public:
    template <typename T> T *add(obia_ctx *ctx, const T *host, size_t n) { return static_cast<T *>(add_bytes(ctx, host, n * sizeof(T))); }   // null: failed (the error is set)
    int flush(obia_ctx *ctx);
    void drop() { dev_ = host_ = nullptr; cap_ = used_ = 0; }   // forgets an open blob without uploading it
  private:
    void *add_bytes(obia_ctx *ctx, const void *host, size_t bytes);
    char *dev_ = nullptr, *host_ = nullptr;
    size_t cap_ = 0, used_ = 0;
};

struct Timing {
    double assign_ms = 0, prepass_ms = 0, feat_ms = 0, cc_ms = 0, zonal_ms = 0, total_ms = 0;
    double assign_px = 0, prepass_px = 0;   // pixels processed by the timed colour / pre-pass sweeps (sum over launches)
    double prepass_shared_px = 0;           // ... of prepass_px that no sweep evaluated: covered by a class representative's sweeps (shared pre-pass)
    double assign_store_px = 0;             // ... of the colour sweeps that also stored their labels (the last sweep of a batch)
    double feat_fused_px = 0;               // pixels whose feature planes were written by a sweep (fused feature pass) instead of the feature pass
    int sweeps = 0;
    int prepass_group_launches = 0;         // spatial pre-pass sweeps launched for one of two window groups (slic_sweep.hip: grouped pre-pass)
    int assign_group_launches = 0;          // colour sweeps launched for one of two window groups (grouped colour pass): 2 x max_iter per grouped batch
    int assign_group_batches = 0;           // ... and the batches they belong to (the serial number that ties a launch's span to its batch)
    double assign_launch_sum_ms = 0;        // plain sum of the durations of all colour-sweep launches, overlapping or not
    int batch_repeats = 0;                  // batches whose sweeps ran again with every sweep storing its labels (a valid pixel no window reached)
    // time during which at least one colour (pre-pass) sweep was running, over the whole call.  assign_ms is the time during which a
    // colour sweep runs, batch by batch: a serial launch adds its duration, a grouped colour pass (two window groups, two streams) the
    // UNION of its launches' intervals -- so assign_busy_ms equals assign_ms either way, and assign_launch_sum_ms is the larger.  The
    // sweeps of a grouped pre-pass overlap too: prepass_ms is a sum of overlapping durations and prepass_busy_ms, their union, the smaller
    double assign_busy_ms = 0, prepass_busy_ms = 0;
    // small commands issued in the frame, kernels not included: fills (fill_async, clear_ranges: one per launch), host -> device
    // uploads (upload_async, PlanBlob::flush) and device -> host read-backs (read_back, the sweeps' deferred one)
    int fills = 0, uploads = 0, readbacks = 0;
};

}  // namespace obia

struct obia_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    obia::Arena arena;
    void *pinned = nullptr;          // small pinned host staging buffer for scalar read-backs
    size_t pinned_bytes = 0;
    unsigned long long *defer_buf = nullptr;   // pinned landing area of a read-back that is looked at after a LATER synchronisation
    bool defer_pending = false;                // (slic_run_sweeps: the orphan flag and pixel counters of the sweeps)
    double defer_shared_px = 0;                // (and the pixel-sweeps a shared pre-pass covered without evaluating them)
    // visited map of the connectivity stage's component walks (cc.hip): every walk clears its own marks, so the map is all zero
    // between calls and is cleared as a whole only when it grows or after a call that did not complete (cc_visited_dirty)
    int32_t *cc_visited = nullptr;
    size_t cc_visited_px = 0;
    bool cc_visited_dirty = false;
    // what the last enforce_connectivity_batch decided (obia_test_cc_report, include/obia_testing.h lists the fields): reset at its
    // start, host stores only
    enum { CC_REPORT_FIELDS = 12 };
    int64_t cc_report[CC_REPORT_FIELDS] = {};
    char *up_buf = nullptr;          // pinned ring for small host -> device tables (upload_async): no stream sync per upload
    size_t up_bytes = 0, up_used = 0;
    obia::PlanBlob plan;             // the open planning phase's tables (one upload per phase)
    int profiling = 0;               // 0 off, 1 every span, 2 only the colour sweeps (obia_set_profiling)
    obia::Timing timing;
    // event pairs recorded around kernels of interest; resolved (one sync) at the end of the call
    struct Span { int kind; hipEvent_t a, b; int tag = 0; };   // tag (T_ASSIGN_GRP): 2 x grouped batch of the call + group
    std::vector<Span> spans;
    std::vector<hipEvent_t> event_pool;
    size_t events_used = 0;
    // side stream of the tiler's white feature pass beside the black sweeps (tiling.hip) and its fork / join events; created on
    // first use
    hipStream_t side = nullptr;
    hipEvent_t aux_fork = nullptr, aux_join = nullptr;
    // grouped spatial pre-pass (slic_sweep.hip: queue_sweeps): the second window group runs on `side` between events of its own -- the
    // white prefetch may hold aux_fork / aux_join across a batch's sweeps
    hipEvent_t grp_fork = nullptr, grp_join = nullptr;
    int spatial_residency[4] = {0, 0, 0, 0};   // workgroups of slic_spatial_kernel<4 (i + 1)> the device holds at once; 0: not asked yet
    int sweep_residency[64] = {};              // the same of the colour-sweep kernel variants (slic_sweep.hip: sweep_residency)
    // the open tiler session (obia_tiler_create sets it, obia_tiler_destroy clears it): its persistent state lives in the arena, so
    // enter() refuses every call but the session's own while it is set
    const void *session = nullptr;
};

namespace obia {

enum TimeKind { T_ASSIGN = 0, T_FEAT = 2, T_CC = 3, T_ZONAL = 4, T_TOTAL = 5, T_PREPASS = 6, T_ASSIGN_GRP = 7 };   // T_ASSIGN_GRP: a colour sweep of one window group

// Records a HIP event pair around a region of the context's stream when profiling is on; no host
// synchronisation happens until resolve_timing().
struct ScopedSpan {
    obia_ctx *ctx; bool on; size_t idx;
    ScopedSpan(obia_ctx *c, int kind);
    ~ScopedSpan();
};
// The same bookkeeping for ONE kernel: the event pair is handed to hipExtLaunchKernelGGL, which binds it to the dispatch
// itself, so the elapsed time is the kernel's own start-to-end (what a rocprofv3 kernel trace reports) and not the distance
// between two stream markers around it (that also times the dispatch, a few microseconds).  Both null when profiling is off.
struct KernelSpan {
    hipEvent_t a = nullptr, b = nullptr;
    KernelSpan() = default;   // no events: a launch that is not timed
    KernelSpan(obia_ctx *c, int kind, int tag = 0);
};
void begin_timing(obia_ctx *ctx);
void resolve_timing(obia_ctx *ctx);

int read_back(obia_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);  // async copy + stream sync
// Host table -> device without a stream synchronisation: the bytes are copied into a pinned ring first, so the caller's
// (pageable, short-lived) buffer is free at once; the ring is recycled at the next read_back (everything queued before it
// has then executed).
int upload_async(obia_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);
int fill_async(obia_ctx *ctx, void *dev_dst, int byte, size_t bytes);   // hipMemsetAsync on the context's stream

// Fills that stand next to each other in stream order as ONE launch (clear_ranges_kernel, context.cpp): the table of ranges is the
// kernel's argument, passed by value -- nothing is uploaded.  add() collects (an empty range is dropped; a seventeenth one launches
// the sixteen held), flush() launches; a set of one range is a plain fill.  Every set is flushed by hand: the destructor launches
// nothing.
struct ClearRange { void *p; unsigned long long bytes; unsigned value, pad; };
struct ClearTable { ClearRange r[16]; int n; };
class ClearSet {
  public:
    explicit ClearSet(obia_ctx *ctx) : ctx_(ctx) { t_.n = 0; }
    int add(void *dev, int byte, size_t bytes);
    int flush();
  private:
    obia_ctx *ctx_;
    ClearTable t_;
};

int side_stream(obia_ctx *ctx);   // makes sure `side` and the events of both its users exist
// Developer aid (OBIA_DEBUG_SYNC=1): synchronise the stream and report the stage on stderr, so that an asynchronous GPU fault
// is pinned on the stage that caused it.  A no-op otherwise.
void debug_sync(obia_ctx *ctx, const char *stage);

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
// The grid of a clamped launch (launch_grids.hpp: every clamp is a named host function there) as the launch takes it.
static inline dim3 to_dim3(const grids::Grid &g) { return dim3((unsigned)g.x.n, (unsigned)g.y.n); }
// Grid of a grid-stride kernel over n elements in workgroups of 256: one workgroup per 256 elements, 8192 at the most, one at the least.
static inline unsigned flat_grid(long long n) { return (unsigned)grids::flat(n).x.n; }

// ---- the entry layer: what every extern "C" function is made of besides its body (the argument checks: buffer_args.hpp) -----------

// Prologue, the first statement of every entry point that takes a context (the tiler's go through their session's): refuses a null
// context (OBIA_E_INVALID) before any HIP call and selects the context's device.  A context held by an open tiler session is refused
// too (OBIA_E_INVALID, "context is held by an open tiler session") unless `session` is that session: a frame of another call would
// reset -- and, with more than one block, free -- the arena the session's state lives in.
extern const char *const SESSION_HELD;   // the text of that refusal
int enter(obia_ctx *ctx, const void *session = nullptr);

// Error path of every entry point that returns with its work done: nothing this library queued may still be running when the caller
// gets the error back -- it is about to free the buffers.  Waits for the context's stream and its side stream, returns rc.
int quiesce(obia_ctx *ctx, int rc);

// Call frame of those entry points: resets the arena (and, with FRAME_TIMING, the timing record), runs the body (with FRAME_TOTAL
// inside a T_TOTAL span), then synchronises the stream and resolves the timing -- or, when the body failed, quiesces.
enum FrameOpts : unsigned { FRAME_PLAIN = 0, FRAME_TIMING = 1, FRAME_TOTAL = 2 | FRAME_TIMING };
void frame_begin(obia_ctx *ctx, unsigned opts);
int frame_end(obia_ctx *ctx, unsigned opts, int rc);
template <typename Body> int call_frame(obia_ctx *ctx, unsigned opts, Body &&body) {
    frame_begin(ctx, opts);
    int rc;
    if ((opts & FRAME_TOTAL) == FRAME_TOTAL) {
        ScopedSpan total(ctx, T_TOTAL);
        rc = body();
    } else {
        rc = body();
    }
    return frame_end(ctx, opts, rc);
}

// Temporary device buffers of a host-pointer entry point (plain allocations: what the caller sees is not part of the arena).  The
// first failure sticks -- every later step is skipped -- so a call reads: in() / out() ..., run(the _dev call), fetch() ..., finish().
class Staging {
  public:
    explicit Staging(obia_ctx *ctx) : ctx_(ctx) {}
    ~Staging() { (void)finish(); }
    Staging(const Staging &) = delete;
    Staging &operator=(const Staging &) = delete;
    template <typename T> T *in(const T *host, size_t n) { return static_cast<T *>(upload(host, n * sizeof(T))); }   // null stays null
    template <typename T> T *out(size_t n) { return static_cast<T *>(alloc(n * sizeof(T))); }
    template <typename T> void fetch(T *host, const T *dev, size_t n) { download(host, dev, n * sizeof(T)); }
    bool ok() const { return rc_ == OBIA_OK; }
    template <typename Call> void run(Call &&call) { if (ok()) rc_ = call(); }   // the inner call keeps its own error message
    int finish();   // synchronises the stream, then frees, on every path; returns the call's status
  private:
    void *alloc(size_t bytes);
    void *upload(const void *host, size_t bytes);
    void download(void *host, const void *dev, size_t bytes);
    obia_ctx *ctx_;
    int rc_ = OBIA_OK;
    bool open_ = true;
    std::vector<void *> bufs_;
};

// Loads of data that ONE workgroup reads ONCE per pass (feature planes in a sweep, the raster in the feature and statistics
// passes): non-temporal, so the lines do not displace what IS re-read from the caches -- centroid records, bin heads, accumulator
// lines.  Measured on the colour sweep: 0.2144 -> 0.2065 ms, 0.2143 -> 0.2087 ms per launch (two pairs on one box).
#if defined(__HIPCC__)
typedef float obia_v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld_stream_f4(const void *p) {
    const obia_v4f t = __builtin_nontemporal_load(reinterpret_cast<const obia_v4f *>(p));
    return make_float4(t.x, t.y, t.z, t.w);
}
// Order-preserving key of a float32 (zonal.hip, points.hip): unsigned order of the keys is numeric order of the floats, so an integer
// atomicMin / atomicMax on the key is a minimum / maximum of the value.  No finite float has the key 0.
__device__ __forceinline__ unsigned zkey(float f) {
    unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float zunkey(unsigned k) {
    unsigned b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(b);
}
#endif

}  // namespace obia
