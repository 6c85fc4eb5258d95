// context.cpp -- context lifetime, workspace arena, error string, timing spans, the entry layer (enter, call frame, Staging).
#include "common.hpp"
#include "../../include/obia_testing.h"

#include <algorithm>
#include <cstdlib>
#include <utility>

#include <cstdarg>

namespace obia {

static thread_local std::string g_last_error;

void set_error(const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

void *Arena::alloc(size_t bytes) {
    bytes = (bytes + 255) & ~size_t(255);
    if (bytes == 0) bytes = 256;
    for (; cur_ < blocks_.size(); ++cur_) {
        Block &b = blocks_[cur_];
        if (b.size - b.used >= bytes) {
            void *p = b.p + b.used;
            b.used += bytes;
            cur_total_ += bytes;
            if (cur_total_ > high_water_) high_water_ = cur_total_;
            return p;
        }
    }
    size_t want = bytes;
    size_t grow = blocks_.empty() ? (size_t(64) << 20) : 2 * blocks_.back().size;
    if (grow > (size_t(4) << 30)) grow = size_t(4) << 30;
    if (want < grow) want = grow;
    void *p = nullptr;
    if (hipMalloc(&p, want) != hipSuccess) {
        if (want == bytes || hipMalloc(&p, bytes) != hipSuccess) {
            failed_ = true;
            set_error("workspace hipMalloc of %zu bytes failed", bytes);
            return nullptr;
        }
        want = bytes;
    }
    blocks_.push_back(Block{static_cast<char *>(p), want, bytes});
    cur_ = blocks_.size() - 1;
    cur_total_ += bytes;
    if (cur_total_ > high_water_) high_water_ = cur_total_;
    return p;
}

Arena::Mark Arena::mark() const {
    Mark m;
    m.block = cur_ < blocks_.size() ? cur_ : blocks_.size();
    m.used = m.block < blocks_.size() ? blocks_[m.block].used : 0;
    m.total = cur_total_;
    return m;
}

void Arena::rewind(const Mark &m) {
    for (size_t i = m.block + 1; i < blocks_.size(); ++i) blocks_[i].used = 0;
    if (m.block < blocks_.size()) blocks_[m.block].used = m.used;
    cur_ = m.block;
    cur_total_ = m.total;
}

void Arena::reset() {
    failed_ = false;
    cur_total_ = 0;
    cur_ = 0;
    if (blocks_.size() > 1) {
        // merge: one block large enough for the high-water mark of the previous calls
        size_t total = 0;
        for (auto &b : blocks_) total += b.size;
        for (auto &b : blocks_) (void)hipFree(b.p);
        blocks_.clear();
        void *p = nullptr;
        if (hipMalloc(&p, high_water_ + (high_water_ >> 3)) == hipSuccess) blocks_.push_back(Block{static_cast<char *>(p), high_water_ + (high_water_ >> 3), 0});
        (void)total;
    } else if (!blocks_.empty()) {
        blocks_[0].used = 0;
    }
}

void Arena::release() {
    for (auto &b : blocks_) (void)hipFree(b.p);
    blocks_.clear();
}

char *Arena::one_block(size_t bytes, size_t *size_out) {
    reset();
    if (blocks_.size() != 1 || blocks_[0].size < bytes) {
        if (!alloc(bytes)) return nullptr;   // (a second block when the first is too small ...)
        reset();                             // (... which this merges with it: one block of the high-water mark and an eighth)
    }
    if (blocks_.size() != 1 || blocks_[0].size < bytes) { set_error("workspace hipMalloc of %zu bytes failed", bytes); return nullptr; }
    *size_out = blocks_[0].size;
    return blocks_[0].p;
}

size_t Arena::capacity() const {
    size_t t = 0;
    for (auto &b : blocks_) t += b.size;
    return t;
}

static hipEvent_t get_event(obia_ctx *ctx) {
    if (ctx->events_used == ctx->event_pool.size()) {
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        ctx->event_pool.push_back(e);
    }
    return ctx->event_pool[ctx->events_used++];
}

ScopedSpan::ScopedSpan(obia_ctx *c, int kind) : ctx(c), on(c->profiling == 1 || (c->profiling == 2 && kind == T_ASSIGN)), idx(0) {
    if (!on) return;
    obia_ctx::Span s{kind, get_event(ctx), get_event(ctx)};
    (void)hipEventRecord(s.a, ctx->stream);
    idx = ctx->spans.size();
    ctx->spans.push_back(s);
}
ScopedSpan::~ScopedSpan() {
    if (on) (void)hipEventRecord(ctx->spans[idx].b, ctx->stream);
}

int side_stream(obia_ctx *ctx) {
    if (!ctx->aux_fork) OBIA_HIP_TRY(hipEventCreateWithFlags(&ctx->aux_fork, hipEventDisableTiming));
    if (!ctx->aux_join) OBIA_HIP_TRY(hipEventCreateWithFlags(&ctx->aux_join, hipEventDisableTiming));
    if (!ctx->grp_fork) OBIA_HIP_TRY(hipEventCreateWithFlags(&ctx->grp_fork, hipEventDisableTiming));
    if (!ctx->grp_join) OBIA_HIP_TRY(hipEventCreateWithFlags(&ctx->grp_join, hipEventDisableTiming));
    if (!ctx->side) OBIA_HIP_TRY(hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
    return OBIA_OK;
}

KernelSpan::KernelSpan(obia_ctx *c, int kind, int tag) {
    if (!(c->profiling == 1 || (c->profiling == 2 && (kind == T_ASSIGN || kind == T_ASSIGN_GRP)))) return;
    a = get_event(c);
    b = get_event(c);
    c->spans.push_back(obia_ctx::Span{kind, a, b, tag});
}

void begin_timing(obia_ctx *ctx) {
    ctx->spans.clear();
    ctx->events_used = 0;
    ctx->timing = Timing();
}

void resolve_timing(obia_ctx *ctx) {
    if (!ctx->profiling) return;
    (void)hipStreamSynchronize(ctx->stream);
    // sweeps: [start, end) of every kernel on the clock of the first one (end = distance from the first kernel's start to this
    // kernel's end, start = end - the kernel's own duration), for the length of their union
    typedef std::vector<std::pair<double, double>> Intervals;
    auto union_ms = [](Intervals &v) {
        std::sort(v.begin(), v.end());
        double busy = 0, lo = 0, hi = -1;
        for (auto &x : v) {
            if (hi < lo || x.first > hi) { if (hi > lo) busy += hi - lo; lo = x.first; hi = x.second; }
            else if (x.second > hi) hi = x.second;
        }
        if (hi > lo) busy += hi - lo;
        return busy;
    };
    Intervals iv[2];
    std::vector<Intervals> grouped;   // the colour sweeps of every grouped batch (two window groups on two streams: slic_sweep.hip)
    hipEvent_t ref = nullptr;
    for (auto &s : ctx->spans) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, s.a, s.b) != hipSuccess) { (void)hipGetLastError(); continue; }   // (a launch that was skipped)
        if (s.kind == T_ASSIGN || s.kind == T_ASSIGN_GRP || s.kind == T_PREPASS) {
            if (!ref) ref = s.a;
            float end = 0;
            if (hipEventElapsedTime(&end, ref, s.b) == hipSuccess) {
                const std::pair<double, double> x((double)end - ms, (double)end);
                iv[s.kind == T_PREPASS ? 1 : 0].push_back(x);
                if (s.kind == T_ASSIGN_GRP) {
                    const size_t batch = (size_t)(s.tag >> 1);
                    if (grouped.size() <= batch) grouped.resize(batch + 1);
                    grouped[batch].push_back(x);
                }
            }
            else (void)hipGetLastError();
        }
        switch (s.kind) {
            case T_ASSIGN: ctx->timing.assign_ms += ms; ctx->timing.assign_launch_sum_ms += ms; ctx->timing.sweeps += 1; break;
            // class 0 is the time during which a colour sweep of the batch runs, per sweep of the batch: the two launches of a sweep
            // are one sweep (counted with group 0's), and the batch's time is the union below
            case T_ASSIGN_GRP: ctx->timing.assign_launch_sum_ms += ms; if (!(s.tag & 1)) ctx->timing.sweeps += 1; break;
            case T_FEAT: ctx->timing.feat_ms += ms; break;
            case T_CC: ctx->timing.cc_ms += ms; break;
            case T_ZONAL: ctx->timing.zonal_ms += ms; break;
            case T_TOTAL: ctx->timing.total_ms += ms; break;
            case T_PREPASS: ctx->timing.prepass_ms += ms; break;
            default: break;
        }
    }
    for (auto &g : grouped) ctx->timing.assign_ms += union_ms(g);
    ctx->timing.assign_busy_ms += union_ms(iv[0]);
    ctx->timing.prepass_busy_ms += union_ms(iv[1]);
    ctx->spans.clear();
}

int read_back(obia_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes) {
    if (bytes > ctx->pinned_bytes) {
        if (ctx->pinned) (void)hipHostFree(ctx->pinned);
        ctx->pinned = nullptr;
        size_t want = bytes < 4096 ? 4096 : bytes;
        OBIA_HIP_TRY(hipHostMalloc(&ctx->pinned, want, hipHostMallocDefault));
        ctx->pinned_bytes = want;
    }
    OBIA_TRY(ctx->plan.flush(ctx));   // no table stays behind a synchronisation (and the ring is recycled below)
    OBIA_HIP_TRY(hipMemcpyAsync(ctx->pinned, dev_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    ctx->timing.readbacks += 1;
    OBIA_HIP_TRY(hipStreamSynchronize(ctx->stream));
    ctx->up_used = 0;   // every upload queued so far has executed: the ring is free again
    memcpy(host_dst, ctx->pinned, bytes);
    return OBIA_OK;
}

void debug_sync(obia_ctx *ctx, const char *stage) {
    static const bool on = std::getenv("OBIA_DEBUG_SYNC") != nullptr;
    if (!on) return;
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    fprintf(stderr, "[obia debug] %s: %s\n", stage, e == hipSuccess ? "ok" : hipGetErrorString(e));
    fflush(stderr);
}

int fill_async(obia_ctx *ctx, void *dev_dst, int byte, size_t bytes) {
    if (bytes == 0) return OBIA_OK;
    OBIA_HIP_TRY(hipMemsetAsync(dev_dst, byte, bytes, ctx->stream));
    ctx->timing.fills += 1;
    return OBIA_OK;
}

// Every range in turn, all threads of the grid on each: 16-byte stores over the aligned body, single bytes for the at most 15 in
// front of it and the at most 15 behind it.  Nothing outside [p, p + bytes) is touched.  RAGGED = false: every range of the set
// starts and ends on a 16-byte boundary (ClearSet::flush looks), the kernel holds no byte store at all.
template <bool RAGGED> __global__ __launch_bounds__(256) void clear_ranges_kernel(const ClearTable T) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    for (int k = 0; k < T.n; ++k) {
        unsigned char *p = static_cast<unsigned char *>(T.r[k].p);
        const size_t n = T.r[k].bytes;
        const unsigned v = (T.r[k].value & 0xffu) * 0x01010101u;
        size_t head = RAGGED ? (16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15 : 0;
        if (head > n) head = n;
        const size_t nvec = (n - head) / 16, tail0 = head + nvec * 16;
        uint4 *pv = reinterpret_cast<uint4 *>(p + head);
        for (size_t i = tid; i < nvec; i += stride) pv[i] = make_uint4(v, v, v, v);
        if (RAGGED) {
            if (tid < head) p[tid] = (unsigned char)v;
            if (tid < n - tail0) p[tail0 + tid] = (unsigned char)v;
        }
    }
}

int ClearSet::add(void *dev, int byte, size_t bytes) {
    if (bytes == 0) return OBIA_OK;
    if (t_.n == 16) OBIA_TRY(flush());
    t_.r[t_.n++] = ClearRange{dev, (unsigned long long)bytes, (unsigned)byte & 0xffu, 0u};
    return OBIA_OK;
}

int ClearSet::flush() {
    const int n = t_.n;
    t_.n = 0;
    if (n == 0) return OBIA_OK;
    if (n == 1) return fill_async(ctx_, t_.r[0].p, (int)t_.r[0].value, (size_t)t_.r[0].bytes);
    unsigned long long longest = 0;
    bool ragged = false;
    for (int k = 0; k < n; ++k) {
        longest = std::max(longest, t_.r[k].bytes);
        ragged = ragged || ((reinterpret_cast<uintptr_t>(t_.r[k].p) | (uintptr_t)t_.r[k].bytes) & 15) != 0;
    }
    ClearTable t = t_;
    t.n = n;
    const dim3 grid(flat_grid((long long)((longest + 15) / 16)));
    if (ragged) hipLaunchKernelGGL(HIP_KERNEL_NAME(clear_ranges_kernel<true>), grid, dim3(256), 0, ctx_->stream, t);
    else hipLaunchKernelGGL(HIP_KERNEL_NAME(clear_ranges_kernel<false>), grid, dim3(256), 0, ctx_->stream, t);
    OBIA_HIP_TRY(hipGetLastError());
    ctx_->timing.fills += 1;
    return OBIA_OK;
}

constexpr size_t RING = 8u << 20;

static int ring_ready(obia_ctx *ctx) {
    if (ctx->up_buf) return OBIA_OK;
    void *p = nullptr;
    OBIA_HIP_TRY(hipHostMalloc(&p, RING, hipHostMallocDefault));
    ctx->up_buf = static_cast<char *>(p);
    ctx->up_bytes = RING;
    ctx->up_used = 0;
    return OBIA_OK;
}

void *PlanBlob::add_bytes(obia_ctx *ctx, const void *host, size_t bytes) {
    constexpr size_t BLOCK = 64u << 10;
    const size_t need = (bytes + 15) & ~size_t(15);
    if (dev_ && used_ + need > cap_ && flush(ctx) != OBIA_OK) return nullptr;
    if (ring_ready(ctx) != OBIA_OK) return nullptr;
    if (need > ctx->up_bytes / 2) {   // a table of megabytes: an upload of its own
        if (flush(ctx) != OBIA_OK) return nullptr;
        void *d = ctx->arena.alloc(need);
        return d && upload_async(ctx, d, host, bytes) == OBIA_OK ? d : nullptr;
    }
    if (!dev_) {
        const size_t cap = (std::max(need, BLOCK) + 63) & ~size_t(63);
        if (ctx->up_used + cap > ctx->up_bytes) {   // ring full: wait for what is queued, start over (no blob is open)
            if (hipStreamSynchronize(ctx->stream) != hipSuccess) { set_error("stream synchronisation failed (plan upload)"); return nullptr; }
            ctx->up_used = 0;
        }
        char *d = static_cast<char *>(ctx->arena.alloc(cap));
        if (!d) return nullptr;
        dev_ = d;
        host_ = ctx->up_buf + ctx->up_used;
        ctx->up_used += cap;
        cap_ = cap;
        used_ = 0;
    }
    void *d = dev_ + used_;
    if (bytes) memcpy(host_ + used_, host, bytes);
    used_ += need;
    return d;
}

int PlanBlob::flush(obia_ctx *ctx) {
    if (!dev_) return OBIA_OK;
    char *const dev = dev_, *const host = host_;
    const size_t used = used_, cap = cap_;
    dev_ = host_ = nullptr;
    cap_ = used_ = 0;
    // (the part of the slot nobody wrote goes back to the ring when nothing was taken behind it)
    if (ctx->up_buf && host + cap == ctx->up_buf + ctx->up_used) ctx->up_used -= cap - ((used + 63) & ~size_t(63));
    if (used == 0) return OBIA_OK;
    OBIA_HIP_TRY(hipMemcpyAsync(dev, host, used, hipMemcpyHostToDevice, ctx->stream));
    ctx->timing.uploads += 1;
    return OBIA_OK;
}

int upload_async(obia_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes) {
    if (bytes == 0) return OBIA_OK;
    ctx->timing.uploads += 1;
    OBIA_TRY(ring_ready(ctx));
    if (bytes > ctx->up_bytes) {   // too big for the ring: plain synchronous copy
        OBIA_TRY(ctx->plan.flush(ctx));   // (its slot of the ring is given up below)
        OBIA_HIP_TRY(hipMemcpyAsync(dev_dst, host_src, bytes, hipMemcpyHostToDevice, ctx->stream));
        OBIA_HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx->up_used = 0;
        return OBIA_OK;
    }
    if (ctx->up_used + bytes > ctx->up_bytes) {   // ring full: wait for what is queued, start over
        OBIA_TRY(ctx->plan.flush(ctx));
        OBIA_HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx->up_used = 0;
    }
    char *slot = ctx->up_buf + ctx->up_used;
    memcpy(slot, host_src, bytes);
    OBIA_HIP_TRY(hipMemcpyAsync(dev_dst, slot, bytes, hipMemcpyHostToDevice, ctx->stream));
    ctx->up_used += (bytes + 63) & ~(size_t)63;
    return OBIA_OK;
}

const char *const SESSION_HELD = "context is held by an open tiler session";

int enter(obia_ctx *ctx, const void *session) {
    if (!ctx) { set_error("null context"); return OBIA_E_INVALID; }
    if (ctx->session && ctx->session != session) { set_error("%s", SESSION_HELD); return OBIA_E_INVALID; }
    if (hipSetDevice(ctx->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", ctx->device); return OBIA_E_HIP; }
    return OBIA_OK;
}

int quiesce(obia_ctx *ctx, int rc) {
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->side) (void)hipStreamSynchronize(ctx->side);
    return rc;
}

void frame_begin(obia_ctx *ctx, unsigned opts) {
    ctx->plan.drop();   // (a call that failed may have left tables behind: their device block goes with the arena)
    ctx->arena.reset();
    if (opts & FRAME_TIMING) begin_timing(ctx);
}

int frame_end(obia_ctx *ctx, unsigned opts, int rc) {
    if (rc != OBIA_OK) return quiesce(ctx, rc);
    OBIA_TRY(ctx->plan.flush(ctx));
    OBIA_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (opts & FRAME_TIMING) resolve_timing(ctx);
    return OBIA_OK;
}

void *Staging::alloc(size_t bytes) {
    if (!ok()) return nullptr;
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) {
        set_error("device allocation for host-pointer call failed");
        rc_ = OBIA_E_NOMEM;
        return nullptr;
    }
    bufs_.push_back(p);
    return p;
}

void *Staging::upload(const void *host, size_t bytes) {
    if (!host) return nullptr;
    void *p = alloc(bytes);
    if (p && hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, ctx_->stream) != hipSuccess) {
        set_error("host->device copy failed in a host-pointer call");
        rc_ = OBIA_E_HIP;
    }
    return p;
}

void Staging::download(void *host, const void *dev, size_t bytes) {
    if (ok() && hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, ctx_->stream) != hipSuccess) {
        set_error("device->host copy failed in a host-pointer call");
        rc_ = OBIA_E_HIP;
    }
}

int Staging::finish() {
    if (open_) {
        open_ = false;
        (void)hipStreamSynchronize(ctx_->stream);
        for (void *p : bufs_) (void)hipFree(p);
        bufs_.clear();
    }
    return rc_;
}

}  // namespace obia

using namespace obia;

extern "C" {

int obia_abi_version(void) { return OBIA_ABI_VERSION; }

const char *obia_last_error(void) { return g_last_error.c_str(); }

static obia_ctx *create_impl(int device_id, void *stream, bool own) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        set_error("no HIP device available");
        return nullptr;
    }
    if (device_id < 0 || device_id >= n) {
        set_error("device_id %d out of range (%d devices)", device_id, n);
        return nullptr;
    }
    if (hipSetDevice(device_id) != hipSuccess) {
        set_error("hipSetDevice(%d) failed", device_id);
        return nullptr;
    }
    obia_ctx *ctx = new obia_ctx();
    ctx->device = device_id;
    if (own) {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
            set_error("hipStreamCreate failed");
            delete ctx;
            return nullptr;
        }
        ctx->own_stream = true;
    } else {
        ctx->stream = static_cast<hipStream_t>(stream);
    }
    return ctx;
}

obia_ctx *obia_create(int device_id) { return create_impl(device_id, nullptr, true); }
obia_ctx *obia_create_on_stream(int device_id, void *hip_stream) { return create_impl(device_id, hip_stream, false); }

void obia_destroy(obia_ctx *ctx) {
    if (!ctx) return;
    if (ctx->session) { set_error("%s: obia_tiler_destroy comes first, the context was not destroyed", SESSION_HELD); return; }
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->arena.release();
    if (ctx->up_buf) (void)hipHostFree(ctx->up_buf);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->defer_buf) (void)hipHostFree(ctx->defer_buf);
    if (ctx->cc_visited) (void)hipFree(ctx->cc_visited);
    for (auto e : ctx->event_pool) (void)hipEventDestroy(e);
    if (ctx->side) (void)hipStreamDestroy(ctx->side);
    if (ctx->aux_fork) (void)hipEventDestroy(ctx->aux_fork);
    if (ctx->aux_join) (void)hipEventDestroy(ctx->aux_join);
    if (ctx->grp_fork) (void)hipEventDestroy(ctx->grp_fork);
    if (ctx->grp_join) (void)hipEventDestroy(ctx->grp_join);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int obia_synchronize(obia_ctx *ctx) {
    if (!ctx) { set_error("null context"); return OBIA_E_INVALID; }
    OBIA_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return OBIA_OK;
}

int obia_test_clear_ranges_dev(obia_ctx *ctx, void *const *dev_ptrs, const int64_t *bytes, const int32_t *values, int n) {
    OBIA_TRY(enter(ctx));
    if (!dev_ptrs || !bytes || !values || n < 0) { set_error("clear ranges: null array or negative count"); return OBIA_E_INVALID; }
    for (int i = 0; i < n; ++i)
        if (bytes[i] < 0 || (bytes[i] > 0 && !dev_ptrs[i])) { set_error("clear ranges: range %d is not a range", i); return OBIA_E_INVALID; }
    return call_frame(ctx, FRAME_TIMING, [&] {
        ClearSet clr(ctx);
        for (int i = 0; i < n; ++i) OBIA_TRY(clr.add(dev_ptrs[i], values[i], (size_t)bytes[i]));
        return clr.flush();
    });
}

// the words of the visited map that are not zero (0: there is no map, or it is flagged dirty and the next call clears it)
static int visited_nonzero(obia_ctx *ctx, int64_t *out) {
    *out = 0;
    if (!ctx->cc_visited || ctx->cc_visited_dirty || ctx->cc_visited_px == 0) return OBIA_OK;
    std::vector<int32_t> h(ctx->cc_visited_px);
    OBIA_HIP_TRY(hipMemcpy(h.data(), ctx->cc_visited, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost));
    *out = (int64_t)(h.size() - (size_t)std::count(h.begin(), h.end(), 0));
    return OBIA_OK;
}

int obia_test_poison_workspace_dev(obia_ctx *ctx, int64_t reserve_bytes, int byte, int64_t *held_out, int64_t *visited_nonzero_out) {
    OBIA_TRY(enter(ctx));   // (refuses a context held by a session: its state lives in the arena)
    if (byte < 0 || byte > 255 || reserve_bytes < 0) { set_error("poison: byte %d outside 0..255 or negative reserve", byte); return OBIA_E_INVALID; }
    (void)quiesce(ctx, 0);
    ctx->plan.drop();
    size_t size = 0;
    char *block = ctx->arena.one_block((size_t)reserve_bytes, &size);
    if (!block) return OBIA_E_NOMEM;
    OBIA_HIP_TRY(hipMemsetAsync(block, byte, size, ctx->stream));
    OBIA_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->pinned) memset(ctx->pinned, byte, ctx->pinned_bytes);
    if (ctx->up_buf && ctx->up_used == 0) memset(ctx->up_buf, byte, ctx->up_bytes);
    if (ctx->defer_buf && !ctx->defer_pending) memset(ctx->defer_buf, byte, sizeof(unsigned long long) * 513);
    int64_t nz = 0;
    OBIA_TRY(visited_nonzero(ctx, &nz));
    if (held_out) *held_out = (int64_t)ctx->arena.capacity();
    if (visited_nonzero_out) *visited_nonzero_out = nz;
    return OBIA_OK;
}

int obia_test_visited_nonzero(obia_ctx *ctx, int64_t *visited_nonzero_out) {
    if (!ctx || !visited_nonzero_out) { set_error("null context or null output"); return OBIA_E_INVALID; }
    if (hipSetDevice(ctx->device) != hipSuccess) { set_error("hipSetDevice(%d) failed", ctx->device); return OBIA_E_HIP; }
    (void)quiesce(ctx, 0);
    return visited_nonzero(ctx, visited_nonzero_out);
}

int64_t obia_workspace_bytes(obia_ctx *ctx) { return ctx ? (int64_t)ctx->arena.capacity() : 0; }

void obia_slic_default_params(obia_slic_params *p) {
    if (!p) return;
    p->n_segments = 100;
    p->compactness = 10.0;
    p->max_num_iter = 10;
    p->convert2lab = -1;
    p->enforce_connectivity = 1;
    p->min_size_factor = 0.5;
    p->max_size_factor = 3.0;
    p->slic_zero = 0;
    p->start_label = 1;
    p->normalize_bands = 0;
    p->exit_on_fixed_point = 0;
    p->reserved = 0;
    p->sigma_zyx[0] = p->sigma_zyx[1] = p->sigma_zyx[2] = 0.0;
    p->spacing_zyx[0] = p->spacing_zyx[1] = p->spacing_zyx[2] = 1.0;
}

int obia_set_profiling(obia_ctx *ctx, int enabled) {
    if (!ctx) { set_error("null context"); return OBIA_E_INVALID; }
    ctx->profiling = enabled < 0 ? 0 : (enabled > 2 ? 1 : enabled);
    return OBIA_OK;
}

double obia_last_timing(obia_ctx *ctx, int what) {
    if (!ctx) return -1.0;
    switch (what) {
        case 0: return ctx->timing.assign_ms;
        case 1: return (double)ctx->timing.sweeps;
        case 2: return ctx->timing.feat_ms;
        case 3: return ctx->timing.cc_ms;
        case 4: return ctx->timing.zonal_ms;
        case 5: return ctx->timing.total_ms;
        case 6: return ctx->timing.prepass_ms;
        case 7: return ctx->timing.assign_px;
        case 8: return ctx->timing.prepass_px;
        case 9: return ctx->timing.assign_store_px;
        case 10: return ctx->timing.assign_busy_ms;
        case 11: return ctx->timing.prepass_busy_ms;
        case 12: return (double)ctx->timing.batch_repeats;
        case 13: return ctx->timing.prepass_shared_px;
        case 14: return ctx->timing.feat_fused_px;
        case 15: return (double)ctx->timing.prepass_group_launches;
        case 16: return (double)ctx->timing.fills;
        case 17: return (double)ctx->timing.uploads;
        case 18: return (double)ctx->timing.readbacks;
        case 19: return (double)ctx->timing.assign_group_launches;
        case 20: return ctx->timing.assign_launch_sum_ms;
        default: return -1.0;
    }
}

}  // extern "C"
