// k_reg.hip -- the per-Gaussian regularisers of the training loss, forward and backward (include/gftorf_reg.h;
// train.py:237-240 motion, :266-267 depth distortion, :270-272 opacity entropy, :275-277 scale).  One grid-stride loop over
// the concatenation of the four inputs -- the floats of d_xyz, the rows of opacity, the rows of scaling, the floats of the
// distortion image --, summed in the two stages and the order of gft_reduce.h.  Scalar loads and stores only (callers pass
// views such as d_xyz[1:]: nothing is assumed of a pointer beyond its element's alignment; the whole pass moves ~21 bytes per
// Gaussian and is bound by its launches, not by its loads).
#include "gft_internal.h"
#include "gft_reduce.h"
#include "gftorf_reg.h"

namespace {

constexpr int REG_THREADS = 256, REG_PER_THREAD = 4, REG_MAX_BLOCKS = 1024, REG_RESULT_WORDS = 12;

struct RegArgs {
    int64_t nA, nB, nC, nD;                     // elements of the four segments (0 = absent): 3 Nd, P, P, pixels
    const float* __restrict__ d_xyz;
    const float* __restrict__ opacity;
    const uint8_t* __restrict__ motion_mask;
    const float* __restrict__ scaling;
    const void* __restrict__ visible;
    const float* __restrict__ dd;
    int opacity_is_raw, scaling_is_raw, scaling_cols, visible_is_radii;
    const float* __restrict__ weights_dev;
    float w[4];
    uint32_t* partials;                         // [blocks][GFT_REG_PARTIAL_WORDS]
    uint32_t* result;                           // [REG_RESULT_WORDS]
    int blocks;                                 // rows of partials
    const float* __restrict__ g;                // device, one float
    float* g_d_xyz;
    float* g_opacity;
    float* g_scaling;
    float* g_dd;
};

int64_t reg_blocks(int64_t total) { return gft_grid_blocks(total, REG_THREADS, REG_PER_THREAD, REG_MAX_BLOCKS); }

// torch's fp32 sigmoid expression, as k_assemble.hip's
__device__ __forceinline__ float opacity_of(const RegArgs& p, int64_t r)
{
    const float x = p.opacity[r];
    return p.opacity_is_raw ? 1.0f / (1.0f + expf(-x)) : x;
}

// the row's activated scales; with one column the value three times (gaussian_model.py:125 repeats it)
__device__ __forceinline__ void scales_of(const RegArgs& p, int64_t r, float s[3])
{
    if (p.scaling_cols == 3) {
        s[0] = p.scaling[3 * r]; s[1] = p.scaling[3 * r + 1]; s[2] = p.scaling[3 * r + 2];
        if (p.scaling_is_raw) { s[0] = expf(s[0]); s[1] = expf(s[1]); s[2] = expf(s[2]); }
    } else {
        const float v = p.scaling_is_raw ? expf(p.scaling[r]) : p.scaling[r];
        s[0] = s[1] = s[2] = v;
    }
}

__global__ __launch_bounds__(REG_THREADS) void k_reg_fwd(RegArgs p)
{
    __shared__ float sRed[4][REG_THREADS / 64];
    __shared__ uint32_t sCnt[2][REG_THREADS / 64];
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    uint32_t n[2] = {0u, 0u};
    const int64_t eB = p.nA + p.nB, eC = eB + p.nC, total = eC + p.nD;
    for (int64_t i = (int64_t)blockIdx.x * REG_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * REG_THREADS) {
        if (i < p.nA) {
            s[0] += fabsf(p.d_xyz[i]);
        } else if (i < eB) {
            const int64_t r = i - p.nA;
            if (p.motion_mask[r]) {
                // train.py:272 in fp32, in its order
                const float o = opacity_of(p, r);
                s[1] += -o * logf(o + 1e-10f) - (1.0f - o) * logf(1.0f - o + 1e-10f);
                n[0]++;
            }
        } else if (i < eC) {
            const int64_t r = i - eB;
            if (gft_visible_row(p.visible, p.visible_is_radii, r)) {
                float v[3];
                scales_of(p, r, v);
                const float m = p.scaling_cols == 3 ? (v[0] + v[1] + v[2]) / 3.0f : v[0];
                s[2] += m * m;
                n[1]++;
            }
        } else {
            s[3] += p.dd[i - eC];
        }
    }
    gft_fold_store<REG_THREADS>(s, sRed);
    gft_fold_store<REG_THREADS>(n, sCnt);
    __syncthreads();
    if (threadIdx.x < GFT_REG_PARTIAL_WORDS) {
        const int k = threadIdx.x;
        p.partials[(size_t)blockIdx.x * GFT_REG_PARTIAL_WORDS + k] =
            k < 4 ? __float_as_uint(gft_waves_total<REG_THREADS>(sRed[k])) : (k < 6 ? gft_waves_total<REG_THREADS>(sCnt[k - 4]) : 0u);
    }
}

// one workgroup: the rows of partials in a fixed order, in double; then the result block
__global__ __launch_bounds__(REG_THREADS) void k_reg_finish(RegArgs p)
{
    __shared__ double sSum[4][REG_THREADS];
    __shared__ unsigned long long sCnt[2][REG_THREADS];
    const int tid = threadIdx.x;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    unsigned long long n[2] = {0ull, 0ull};
    for (int b = tid; b < p.blocks; b += REG_THREADS) {
        const uint32_t* row = p.partials + (size_t)b * GFT_REG_PARTIAL_WORDS;
#pragma unroll
        for (int k = 0; k < 4; k++) s[k] += (double)__uint_as_float(row[k]);
        n[0] += row[4];
        n[1] += row[5];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) sSum[k][tid] = s[k];
    sCnt[0][tid] = n[0];
    sCnt[1][tid] = n[1];
    gft_tree_sum<REG_THREADS>(sSum, sCnt);
    if (tid != 0) return;
    const unsigned long long n_dyn = sCnt[0][0], n_vis = sCnt[1][0];
    const double recip[4] = {p.nA > 0 ? 1.0 / (double)p.nA : 0.0, 1.0 / (double)(n_dyn > 0 ? n_dyn : 1ull),
                             1.0 / (double)(n_vis > 0 ? n_vis : 1ull), p.nD > 0 ? 1.0 / (double)p.nD : 0.0};
    double total = 0.0;
    for (int k = 0; k < 4; k++) {
        const double mean = sSum[k][0] * recip[k];
        const float w = p.weights_dev ? p.weights_dev[k] : p.w[k];
        total += (double)w * mean;
        p.result[GFT_REG_MEANS + k] = __float_as_uint((float)mean);
        p.result[GFT_REG_RECIPS + k] = __float_as_uint((float)recip[k]);
    }
    p.result[GFT_REG_COUNTS] = (uint32_t)n_dyn;
    p.result[GFT_REG_COUNTS + 1] = (uint32_t)n_vis;
    p.result[GFT_REG_TOTAL] = __float_as_uint((float)total);
    p.result[GFT_REG_TOTAL + 1] = 0u;
}

// Elementwise over the index space of k_reg_fwd: every requested gradient in full.  The rows' arithmetic is in double: the
// entropy's derivative log(b) - log(a) cancels near o = 1/2 and the raw forms multiply by sigmoid' or exp, so in fp32 the
// result is a few ulp of the largest gradient off -- no better than eager autograd.  In double the only roundings left are
// the fp32 weight, the fp32 reciprocal of the result block and the store.  (The pass stays bound by its launch: ~200 double
// operations for a selected row.)
__global__ __launch_bounds__(REG_THREADS) void k_reg_bwd(RegArgs p)
{
    const double g = (double)*p.g;
    double c[4];
#pragma unroll
    for (int k = 0; k < 4; k++)
        c[k] = g * (double)(p.weights_dev ? p.weights_dev[k] : p.w[k]) * (double)__uint_as_float(p.result[GFT_REG_RECIPS + k]);
    const float c_mlp = (float)c[0], c_dd = (float)c[3];
    const int64_t eB = p.nA + p.nB, eC = eB + p.nC, total = eC + p.nD;
    for (int64_t i = (int64_t)blockIdx.x * REG_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * REG_THREADS) {
        if (i < p.nA) {
            p.g_d_xyz[i] = c_mlp * sign_of(p.d_xyz[i]);
        } else if (i < eB) {
            const int64_t r = i - p.nA;
            double v = 0.0;
            if (p.motion_mask[r]) {
                const double x = (double)p.opacity[r];
                const double o = p.opacity_is_raw ? 1.0 / (1.0 + exp(-x)) : x;
                const double a = o + 1e-10, b = 1.0 - o + 1e-10;
                // d/do of -o log(a) - (1 - o) log(b)
                v = c[1] * ((log(b) - log(a)) + ((1.0 - o) / b - o / a));
                if (p.opacity_is_raw) v *= o * (1.0 - o);           // sigmoid_backward
            }
            p.g_opacity[r] = (float)v;
        } else if (i < eC) {
            const int64_t r = i - eB;
            double gs[3] = {0.0, 0.0, 0.0};
            if (gft_visible_row(p.visible, p.visible_is_radii, r)) {
                double v[3];
                if (p.scaling_cols == 3) {
                    v[0] = (double)p.scaling[3 * r]; v[1] = (double)p.scaling[3 * r + 1]; v[2] = (double)p.scaling[3 * r + 2];
                } else {
                    v[0] = v[1] = v[2] = (double)p.scaling[r];
                }
                if (p.scaling_is_raw) { v[0] = exp(v[0]); v[1] = p.scaling_cols == 3 ? exp(v[1]) : v[0]; v[2] = p.scaling_cols == 3 ? exp(v[2]) : v[0]; }
                const double m = p.scaling_cols == 3 ? (v[0] + v[1] + v[2]) / 3.0 : v[0];
                const double t = c[2] * (2.0 * m) / 3.0;            // d(m^2)/d s_c = 2 m / 3
#pragma unroll
                for (int k = 0; k < 3; k++) gs[k] = p.scaling_is_raw ? t * v[k] : t;
            }
            if (p.scaling_cols == 3) {
                p.g_scaling[3 * r] = (float)gs[0]; p.g_scaling[3 * r + 1] = (float)gs[1]; p.g_scaling[3 * r + 2] = (float)gs[2];
            } else {
                p.g_scaling[r] = (float)(gs[0] + gs[1] + gs[2]);    // the repeat's backward: the three columns' sum
            }
        } else {
            p.g_dd[i - eC] = c_dd;
        }
    }
}

int fill(RegArgs& p, int64_t n_dxyz, int64_t P, int64_t pixels, const float* d_xyz, const float* opacity, const void* motion_mask,
         int32_t opacity_is_raw, const float* scaling, int32_t scaling_cols, int32_t scaling_is_raw, const void* visible,
         int32_t visible_is_radii, const float* weights_dev, float w_mlp, float w_oe, float w_scale, float w_dd, const char* who)
{
    if (n_dxyz < 0 || P < 0 || pixels < 0 || n_dxyz % 3 != 0)
        return gft_fail("%s: bad sizes n_dxyz=%lld P=%lld pixels=%lld", who, (long long)n_dxyz, (long long)P, (long long)pixels);
    if (P > 0x7fffffffll || n_dxyz > (1ll << 40) || pixels > (1ll << 40)) return gft_fail("%s: bad sizes: too large", who);
    if (opacity && !motion_mask) return gft_fail("%s: opacity without its motion_mask", who);
    if (motion_mask && !opacity) return gft_fail("%s: motion_mask without its opacity", who);
    if (scaling && !visible) return gft_fail("%s: scaling without its visible", who);
    if (visible && !scaling) return gft_fail("%s: visible without its scaling", who);
    if (scaling && scaling_cols != 1 && scaling_cols != 3) return gft_fail("%s: scaling_cols=%d is neither 1 nor 3", who, scaling_cols);
    const bool rows = opacity || scaling;
    p.nA = d_xyz ? n_dxyz : 0;
    p.nB = rows ? P : 0;
    p.nC = rows ? P : 0;
    p.d_xyz = d_xyz; p.opacity = opacity; p.motion_mask = static_cast<const uint8_t*>(motion_mask);
    p.scaling = scaling; p.visible = visible;
    p.opacity_is_raw = opacity_is_raw; p.scaling_is_raw = scaling_is_raw; p.scaling_cols = scaling ? scaling_cols : 3;
    p.visible_is_radii = visible_is_radii;
    p.weights_dev = weights_dev;
    p.w[0] = w_mlp; p.w[1] = w_oe; p.w[2] = w_scale; p.w[3] = w_dd;
    return 0;
}

}  // namespace

extern "C" int64_t gft_reg_blocks(int64_t n_dxyz, int64_t P, int64_t pixels)
{
    if (n_dxyz < 0 || P < 0 || pixels < 0) return 0;
    const int64_t total = n_dxyz + 2 * P + pixels;
    return total > 0 ? reg_blocks(total) : 0;
}

extern "C" int64_t gft_reg_result_words(void) { return REG_RESULT_WORDS; }

extern "C" int gft_reg_forward(void* hip_stream, int64_t n_dxyz, int64_t P, int64_t pixels, const float* d_xyz,
                               const float* opacity, const void* motion_mask, int32_t opacity_is_raw, const float* scaling,
                               int32_t scaling_cols, int32_t scaling_is_raw, const void* visible, int32_t visible_is_radii,
                               const float* depth_distortion, const float* weights_dev, float w_mlp, float w_oe, float w_scale,
                               float w_dd, void* partials, void* result)
{
    RegArgs p = {};
    if (fill(p, n_dxyz, P, pixels, d_xyz, opacity, motion_mask, opacity_is_raw, scaling, scaling_cols, scaling_is_raw, visible,
             visible_is_radii, weights_dev, w_mlp, w_oe, w_scale, w_dd, "gft_reg_forward"))
        return 1;
    if (!partials || !result) return gft_fail("gft_reg_forward: partials or result is NULL");
    p.dd = depth_distortion;
    p.nD = depth_distortion ? pixels : 0;
    p.partials = static_cast<uint32_t*>(partials);
    p.result = static_cast<uint32_t*>(result);
    // (the segments of absent terms are empty, those of a present opacity OR scaling both P long: gft_reg_blocks of the
    // caller's sizes is what is launched; a row segment whose tensor is absent selects nothing)
    if (p.nA + p.nB + p.nC + p.nD == 0) return gft_fail("gft_reg_forward: no term is given");
    p.blocks = (int)reg_blocks(p.nA + p.nB + p.nC + p.nD);
    if (!p.opacity) p.nB = 0;
    if (!p.scaling) p.nC = 0;
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(k_reg_fwd, dim3(p.blocks), dim3(REG_THREADS), 0, s, p);
    hipLaunchKernelGGL(k_reg_finish, dim3(1), dim3(REG_THREADS), 0, s, p);
    return gft_launched("gft_reg_forward");
}

extern "C" int gft_reg_backward(void* hip_stream, int64_t n_dxyz, int64_t P, int64_t pixels, const float* d_xyz,
                                const float* opacity, const void* motion_mask, int32_t opacity_is_raw, const float* scaling,
                                int32_t scaling_cols, int32_t scaling_is_raw, const void* visible, int32_t visible_is_radii,
                                const float* weights_dev, float w_mlp, float w_oe, float w_scale, float w_dd, const void* result,
                                const float* g_loss, float* g_d_xyz, float* g_opacity, float* g_scaling, float* g_dd)
{
    RegArgs p = {};
    if (fill(p, n_dxyz, P, pixels, d_xyz, opacity, motion_mask, opacity_is_raw, scaling, scaling_cols, scaling_is_raw, visible,
             visible_is_radii, weights_dev, w_mlp, w_oe, w_scale, w_dd, "gft_reg_backward"))
        return 1;
    if (!result || !g_loss) return gft_fail("gft_reg_backward: result or g_loss is NULL");
    if ((g_d_xyz && !d_xyz) || (g_opacity && !opacity) || (g_scaling && !scaling))
        return gft_fail("gft_reg_backward: a gradient without its tensor");
    p.result = static_cast<uint32_t*>(const_cast<void*>(result));
    p.g = g_loss;
    p.g_d_xyz = g_d_xyz; p.g_opacity = g_opacity; p.g_scaling = g_scaling; p.g_dd = g_dd;
    // only the segments with a gradient to write
    if (!g_d_xyz) p.nA = 0;
    p.nB = g_opacity ? P : 0;
    p.nC = g_scaling ? P : 0;
    p.nD = g_dd ? pixels : 0;
    const int64_t total = p.nA + p.nB + p.nC + p.nD;
    if (total == 0) return 0;
    hipLaunchKernelGGL(k_reg_bwd, dim3((unsigned)reg_blocks(total)), dim3(REG_THREADS), 0, (hipStream_t)hip_stream, p);
    return gft_launched("gft_reg_backward");
}
