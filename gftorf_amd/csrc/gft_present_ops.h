// gft_present_ops.h -- the per-pixel statements the display kernels share (k_present.hip, k_debugviz.hip): numpy's float32
// to8b, normalize_im, np.minimum / np.maximum and matplotlib's index into a 256-entry colour map, operation for operation.
// Nothing here may contract into a multiply-add.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

// np.minimum / np.maximum: a NaN on either side is the result
__device__ __forceinline__ float nmin(float a, float b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }
__device__ __forceinline__ float nmax(float a, float b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }

// np.clip(x, 0, 1): a NaN stays
__device__ __forceinline__ float clip01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

// torf_utils.py:11-12; a NaN gives 0
__device__ __forceinline__ uint32_t to8b(float x)
{
    const float s = 255.f * clip01(x);
    return s == s ? (uint32_t)(int)s : 0u;
}

// torf_utils.py:21-29 with span = hi - lo: a NaN (0 / 0 of a constant image, a NaN bound) becomes 0
__device__ __forceinline__ float norm01(float x, float lo, float span)
{
    const float n = (x - lo) / span;
    return clip01(n == n ? n : 0.f);
}

// to8b(cm.magma(1 - (d - znear) / span)) as one RGBA word: matplotlib's index of a float32 is trunc(x * 256), below 0 the
// first entry, 256 and above (x == 1 too) the last, a NaN the bad colour
__device__ __forceinline__ uint32_t magma(const uint32_t* table, float d, float znear, float span)
{
    const float x = 1.f - (d - znear) / span;
    int row;
    if (x != x) row = 256;
    else if (x < 0.f) row = 0;
    else {
        const float s = x * 256.f;
        row = s >= 256.f ? 255 : (int)s;
    }
    return table[row];
}
