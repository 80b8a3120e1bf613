// bmm_order_probe.hip -- in which order could torch.bmm add the three products of a 3x3 by 3x1 batch item?  For every item the
// nine candidate results of out_i = R_i0 s_0 + R_i1 s_1 + R_i2 s_2: the six chains of fused multiply-adds
//   fma(R_ic, s_c, fma(R_ib, s_b, R_ia * s_a))      for the orders (a, b, c) = 012, 021, 102, 120, 201, 210
// and the three pairings of separately rounded products
//   (p_a + p_b) + p_c                                for (a, b | c) = 01|2, 02|1, 12|0.
// profiles/experiments/bmm_order_probe.py compares them with torch.bmm's bits and writes profiles/bmm_order_probe.json; the
// order gft_split_children uses (include/gftorf_densify.h) was chosen from that table.  Not part of the library.
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC bmm_order_probe.hip -o bmm_order_probe.so
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float chain(const float* R, const float* s, int a, int b, int c)
{
    return fmaf(R[c], s[c], fmaf(R[b], s[b], R[a] * s[a]));
}
__device__ __forceinline__ float pairs(const float* R, const float* s, int a, int b, int c)
{
    return (R[a] * s[a] + R[b] * s[b]) + R[c] * s[c];
}

// R [B, 3, 3], s [B, 3], out [9, B, 3]
__global__ __launch_bounds__(256) void k_candidates(int64_t B, const float* __restrict__ R, const float* __restrict__ s, float* __restrict__ out)
{
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < 3 * B; e += (int64_t)gridDim.x * 256) {
        const int64_t n = e / 3;
        float r[3], v[3];
        for (int j = 0; j < 3; j++) {
            r[j] = R[3 * e + j];
            v[j] = s[3 * n + j];
        }
        const int64_t plane = 3 * B;
        out[0 * plane + e] = chain(r, v, 0, 1, 2);
        out[1 * plane + e] = chain(r, v, 0, 2, 1);
        out[2 * plane + e] = chain(r, v, 1, 0, 2);
        out[3 * plane + e] = chain(r, v, 1, 2, 0);
        out[4 * plane + e] = chain(r, v, 2, 0, 1);
        out[5 * plane + e] = chain(r, v, 2, 1, 0);
        out[6 * plane + e] = pairs(r, v, 0, 1, 2);
        out[7 * plane + e] = pairs(r, v, 0, 2, 1);
        out[8 * plane + e] = pairs(r, v, 1, 2, 0);
    }
}

}  // namespace

extern "C" int bmm_order_candidates(void* stream, int64_t B, const float* R, const float* s, float* out)
{
    if (B <= 0 || B > ((int64_t)1 << 28) || !R || !s || !out) return 1;
    int64_t blocks = (3 * B + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(k_candidates, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, B, R, s, out);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
