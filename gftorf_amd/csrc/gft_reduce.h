// gft_reduce.h -- the two-stage sum of the fused scalar terms (k_reg, k_tof, k_metrics, k_loss, k_flow), once.  No atomics, no
// memset; the number of rows depends on the sizes alone, so every result is bit-reproducible.  The order:
//
//   Stage one, workgroups of THREADS (a multiple of 64), B = gft_grid_blocks(total, THREADS, per_thread, max_blocks) of them:
//   lane l of workgroup b adds the elements i = b * THREADS + l + r * B * THREADS, r = 0, 1, ..., into its own sums from +0
//   (the kernel's grid-stride loop).  gft_fold_store: within each wave of 64, v = v + v[lane ^ o] for o = 32, 16, 8, 4, 2, 1
//   (all lanes end with the same bits), and lane 0 stores to sRed[k][wave].  After the caller's __syncthreads(),
//   gft_waves_total(sRed[k]) is ((w0 + w1) + w2) + ... in wave order: one row of partials per workgroup.
//
//   Stage two, one workgroup of THREADS: thread t adds the rows b = t, t + THREADS, ... in double (counts in unsigned long
//   long) -- that loop stays in the finish kernel, which knows what a row holds -- and stores to sSum[k][t].  gft_tree_sum:
//   sSum[k][t] += sSum[k][t + h] for h = THREADS / 2 ... 1; the total is sSum[k][0].
//
// tests/test_reduce_order.py restates stage one in numpy and compares the rows bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// workgroups of a grid-stride launch over `total` elements, `per_thread` of them per thread: 1 .. max_blocks
inline int64_t gft_grid_blocks(int64_t total, int threads, int per_thread, int max_blocks)
{
    const int64_t b = (total + threads * per_thread - 1) / (threads * per_thread);
    return b < 1 ? 1 : (b > max_blocks ? max_blocks : b);
}

__device__ __forceinline__ float gft_shfl_xor(float v, int o) { return __shfl_xor(v, o); }
__device__ __forceinline__ double gft_shfl_xor(double v, int o) { return __shfl_xor(v, o); }
__device__ __forceinline__ uint32_t gft_shfl_xor(uint32_t v, int o) { return (uint32_t)__shfl_xor((int)v, o); }

// stage one, before the barrier: the butterfly of v[0..N) and lane 0's store to sRed[k][wave]
template <int THREADS, typename T, int N>
__device__ __forceinline__ void gft_fold_store(T (&v)[N], T (*sRed)[THREADS / 64])
{
    static_assert(THREADS % 64 == 0, "whole waves");
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < N; k++) v[k] += gft_shfl_xor(v[k], o);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; k++) sRed[k][threadIdx.x >> 6] = v[k];
    }
}

template <int THREADS, typename T>
__device__ __forceinline__ void gft_fold_store(T v, T* sRed)
{
    T a[1] = {v};
    gft_fold_store<THREADS>(a, reinterpret_cast<T(*)[THREADS / 64]>(sRed));
}

// stage one, after the barrier: the waves' values in wave order.  (It starts from slot 0, not from +0: a lane sum starts at
// +0 and a sum of such is never -0, so 0 + w0 has the bits of w0.)
template <int THREADS, typename T>
__device__ __forceinline__ T gft_waves_total(const T* slots)
{
    T t = slots[0];
    for (int w = 1; w < THREADS / 64; w++) t += slots[w];
    return t;
}

template <int THREADS, typename T, int N>
__device__ __forceinline__ void gft_tree_step(T (&s)[N][THREADS], int tid, int h)
{
#pragma unroll
    for (int k = 0; k < N; k++) s[k][tid] += s[k][tid + h];
}

// stage two: the LDS tree over every s[k][THREADS] given (double sums, unsigned long long counts), one barrier per level
template <int THREADS, typename... S>
__device__ __forceinline__ void gft_tree_sum(S&... s)
{
    const int tid = threadIdx.x;
    __syncthreads();
    for (int h = THREADS / 2; h > 0; h >>= 1) {
        if (tid < h) (gft_tree_step<THREADS>(s, tid, h), ...);
        __syncthreads();
    }
}

__device__ __forceinline__ float sign_of(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// a visible row: the rasterizer's int32 radii > 0, or a bool mask
__device__ __forceinline__ bool gft_visible_row(const void* visible, int is_radii, int64_t r)
{
    return is_radii ? static_cast<const int32_t*>(visible)[r] > 0 : static_cast<const uint8_t*>(visible)[r] != 0;
}
