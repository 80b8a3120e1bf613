// gft_tof_depth.h -- the ToF depth of scene/torf_utils.py:59-64 as one device function, shared by k_tof.hip (gft_tof_depth,
// the training log) and k_metrics.hip (the evaluation's l2_d_tof): both must form the same bits from the same phasor.
#pragma once
#include <hip/hip_runtime.h>

constexpr float TOF_TWO_PI = 6.283185307179586f, TOF_FOUR_PI = 12.566370614359172f, TOF_TINY = 1e-6f;

// depth_range / phase_offset: the device's value when there is one, else the one passed by value (a reference, so that
// a kernel argument is read only when it is the one taken)
__device__ __forceinline__ float gft_dev_or(const float* dev, const float& v) { return dev ? *dev : v; }

// torf_utils.py:60-64 in fp32, in its order
__device__ __forceinline__ float depth_from_tof(float re, float im, float depth_range, float phase_offset)
{
    const float real = fabsf(re) < TOF_TINY ? TOF_TINY : re;
    float phase = atan2f(im, real);
    phase -= phase_offset;
    phase = phase < 0.f ? phase + TOF_TWO_PI : phase;
    return phase * depth_range / TOF_FOUR_PI;
}

// torf_utils.py:53-57, the numpy variant render.py uses (k_present.hip): no clamp of the real part; every step one fp32
// operation of its own, the division correctly rounded
__device__ __forceinline__ float depth_from_tof_np(float re, float im, float depth_range, float phase_offset)
{
#pragma clang fp contract(off)
    float phase = atan2f(im, re);
    phase = __fsub_rn(phase, phase_offset);
    phase = phase < 0.f ? __fadd_rn(phase, TOF_TWO_PI) : phase;
    return __fdiv_rn(__fmul_rn(phase, depth_range), TOF_FOUR_PI);
}
