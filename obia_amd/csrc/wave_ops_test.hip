// wave_ops_test.hip -- obia_test_wave_ops_dev (include/obia_testing.h): the primitives of wave_ops.hpp driven directly, at exactly the
// (primitive, workgroup size) pairs the library's kernels instantiate.  tests/test_gpu_wave_ops.py holds them to numpy.
#include "common.hpp"
#include "wave_ops.hpp"
#include "../../include/obia_testing.h"

namespace obia {
namespace {

enum WaveOp {
    OP_SCAN_IN_PLACE = 0,    // workgroup_exclusive_scan int32 -> int32 in place, int64 total      (polygons.hip)
    OP_SCAN_I32 = 1,         // ... out of place, int32 total                                      (seeds, quickshift, cc)
    OP_SCAN_I64 = 2,         // ... int32 -> int64                                                 (shap: 256, mask_seeds: 1024)
    OP_BLOCK_SCAN = 3,       // block_exclusive_scan                                               (polygons, seeds: 256, tiling: 1024)
    OP_BLOCK_SUM = 4,        // block_sum                                                          (counts: 256, tiling: 1024)
    OP_BLOCK_FLAG_RANK = 5,  // block_flag_rank of in[i] != 0                                      (quickshift, mask_seeds: 256)
    OP_BLOCK_SCAN_TWICE = 6  // block_exclusive_scan of in[i], then of in[i] + 1: the second result
};

// one workgroup; `scratch` is the buffer the int32 scans write: the first n int32 of out[] itself (no workspace)
template <int NT, int OP>
__global__ __launch_bounds__(NT) void wave_ops_scan_kernel(const int32_t *in, long long n, int32_t *scratch, int64_t *out, int64_t *totals) {
    if (OP == OP_SCAN_I64) {
        long long t;
        workgroup_exclusive_scan<NT>(in, (long long *)out, n, &t);
        if (threadIdx.x == 0) totals[0] = t;
        return;
    }
    __shared__ long long s_total;
    if (OP == OP_SCAN_IN_PLACE) {
        for (long long i = threadIdx.x; i < n; i += NT) scratch[i] = in[i];
        __syncthreads();
        workgroup_exclusive_scan<NT>(scratch, scratch, n, &s_total);
    } else {
        int t;
        workgroup_exclusive_scan<NT>(in, scratch, n, &t);
        if (threadIdx.x == 0) s_total = t;
    }
    __syncthreads();
    // widen in place, NT elements at a time from the END: out[i] covers scratch[2i] and scratch[2i + 1], which lie in this round (read
    // into registers before the barrier) or in a round that is already done
    for (long long b = (n - 1) / NT * NT; b >= 0; b -= NT) {
        const long long i = b + threadIdx.x;
        const int32_t v = i < n ? scratch[i] : 0;
        __syncthreads();
        if (i < n) out[i] = v;
        __syncthreads();
    }
    if (threadIdx.x == 0) totals[0] = s_total;
}

// ceil(n / NT) workgroups; a thread past n takes part with a zero
template <int NT, int OP>
__global__ __launch_bounds__(NT) void wave_ops_block_kernel(const int32_t *in, long long n, int64_t *out, int64_t *totals) {
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    const int v = i < n ? in[i] : 0;
    int r, total;
    if (OP == OP_BLOCK_SUM) r = total = block_sum<NT>(v);
    else if (OP == OP_BLOCK_FLAG_RANK) r = block_flag_rank<NT>(v != 0, total);
    else {
        r = block_exclusive_scan<NT>(v, total);
        if (OP == OP_BLOCK_SCAN_TWICE) r = block_exclusive_scan<NT>(i < n ? v + 1 : 0, total);
    }
    if (i < n) out[i] = r;
    if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

template <int NT, int OP> void launch_scan(obia_ctx *ctx, const int32_t *in, long long n, int32_t *scratch, int64_t *out, int64_t *totals) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(wave_ops_scan_kernel<NT, OP>), dim3(1), dim3(NT), 0, ctx->stream, in, n, scratch, out, totals);
}
template <int NT, int OP> void launch_block(obia_ctx *ctx, const int32_t *in, long long n, int64_t *out, int64_t *totals) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(wave_ops_block_kernel<NT, OP>), dim3((unsigned)cdiv(n, NT)), dim3(NT), 0, ctx->stream, in, n, out, totals);
}

}  // namespace
}  // namespace obia

using namespace obia;

extern "C" int obia_test_wave_ops_dev(obia_ctx *ctx, int op, int nt, const int32_t *in, int64_t n, int64_t *out, int64_t *totals_out) {
    OBIA_TRY(enter(ctx));
    const Refusal refuse{"wave ops", "test"};
    if (Buffers().out(out, n > 0).out(totals_out).in(in, n > 0).bad()) return refuse.buffers();
    OBIA_TRY(refuse.n_or_none(n));
    // the pairs served are the pairs the library instantiates (the comment of the declaration lists them)
    const bool served = nt == 1024 ? (op >= OP_SCAN_IN_PLACE && op <= OP_BLOCK_SCAN_TWICE && op != OP_BLOCK_FLAG_RANK)
                                   : nt == 256 && op >= OP_SCAN_I64 && op <= OP_BLOCK_SCAN_TWICE;
    if (!served) { set_error("wave ops: test: op %d with %d threads is not a pair the library uses", op, nt); return OBIA_E_INVALID; }
    return call_frame(ctx, FRAME_PLAIN, [&]() -> int {
        const long long m = n;
        if (op >= OP_BLOCK_SCAN && m == 0) return OBIA_OK;   // no workgroup, nothing written
        int32_t *scratch = reinterpret_cast<int32_t *>(out);   // the int32 scans run on the first half of out[], widened afterwards
        switch (op * 2 + (nt == 1024)) {
        case OP_SCAN_IN_PLACE * 2 + 1: launch_scan<1024, OP_SCAN_IN_PLACE>(ctx, in, m, scratch, out, totals_out); break;
        case OP_SCAN_I32 * 2 + 1: launch_scan<1024, OP_SCAN_I32>(ctx, in, m, scratch, out, totals_out); break;
        case OP_SCAN_I64 * 2: launch_scan<256, OP_SCAN_I64>(ctx, in, m, nullptr, out, totals_out); break;
        case OP_SCAN_I64 * 2 + 1: launch_scan<1024, OP_SCAN_I64>(ctx, in, m, nullptr, out, totals_out); break;
        case OP_BLOCK_SCAN * 2: launch_block<256, OP_BLOCK_SCAN>(ctx, in, m, out, totals_out); break;
        case OP_BLOCK_SCAN * 2 + 1: launch_block<1024, OP_BLOCK_SCAN>(ctx, in, m, out, totals_out); break;
        case OP_BLOCK_SUM * 2: launch_block<256, OP_BLOCK_SUM>(ctx, in, m, out, totals_out); break;
        case OP_BLOCK_SUM * 2 + 1: launch_block<1024, OP_BLOCK_SUM>(ctx, in, m, out, totals_out); break;
        case OP_BLOCK_FLAG_RANK * 2: launch_block<256, OP_BLOCK_FLAG_RANK>(ctx, in, m, out, totals_out); break;
        case OP_BLOCK_SCAN_TWICE * 2: launch_block<256, OP_BLOCK_SCAN_TWICE>(ctx, in, m, out, totals_out); break;
        case OP_BLOCK_SCAN_TWICE * 2 + 1: launch_block<1024, OP_BLOCK_SCAN_TWICE>(ctx, in, m, out, totals_out); break;
        }
        OBIA_HIP_TRY(hipGetLastError());
        return OBIA_OK;
    });
}
