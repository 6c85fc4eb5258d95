// slic_features.hpp -- the per-value arithmetic of the SLIC feature pass, shared by the feature kernels (slic.hip) and by the sweep
// that normalises the caller's raster on the fly (slic_sweep.hip: RAWIN).  Both translation units are compiled with
// -ffp-contract=off, so a value comes out with the same bits wherever it is computed.
#pragma once
#include <hip/hip_runtime.h>

namespace obia {

// order-preserving float <-> uint (the min / max keys of band_minmax_kernel)
__device__ __forceinline__ unsigned f2key(float f) {
    unsigned b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) {
    unsigned b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
    return __uint_as_float(b);
}

// min and (max - min) of band c of window p from the keys [window][C][2]: (band - min) / (max - min), segment_boundaries.py:16
__device__ __forceinline__ void feature_band_param(const unsigned *__restrict__ keys, long long p, int C, int c, float &mn, float &den) {
    mn = key2f(keys[(p * C + c) * 2 + 0]);
    den = key2f(keys[(p * C + c) * 2 + 1]) - mn;
}

// normalize_band of one value (IEEE division).  A constant or non-finite band gives 0: the problem is rejected on the host
__device__ __forceinline__ float feature_normalized(float x, float mn, float den) {
    float t = (x - mn) / den;
    if (!(fabsf(t) <= 3.0e38f)) t = 0.0f;
    return t;
}

}  // namespace obia
