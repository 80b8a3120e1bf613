// k_flowviz.hip -- the optical-flow debug images of F-ToRF training (include/gftorf_flowviz.h; train.py:380-398,
// scene/torf_utils.py:150-305): flow_to_image of (R, T), (T, T) and (T - R, T) as the sequence leaves them, for one direction.
// k_flowviz_maxrad: per-workgroup maxima of the float32 radius of the cleaned target, one word per workgroup.
// k_flowviz_images: every workgroup folds those words (a max does not depend on the order, so maxrad is exact), then walks
// runs of 1024 pixels, four per lane: a lane forms Rc, Tc and E of its pixels once and packs the 12 bytes of each image into
// three dwords, staged in LDS at the destination's offset within a dword (gft_byte_runs.h), so the images leave as whole
// dwords whatever 3 * H * W and the address of `out` are; the last lane of the image stages only the pixels it has.
// No atomics, no memset, the inputs are only read.
//
// The colour is numpy >= 2's float64 sequence operation for operation: nothing here may contract into a multiply-add, the
// divisions and square roots are the correctly rounded ones; atan2 is the one statement whose last bits may differ.
#include "gft_internal.h"
#include "gft_reduce.h"
#include "gft_byte_runs.h"
#include "gftorf_flowviz.h"

#pragma clang fp contract(off)

namespace {

constexpr int FLV_THREADS = 256, FLV_MAX_BLOCKS = 1024, FLV_RUN = GFT_FLOWVIZ_RUN, FLV_IMAGES = GFT_FLOWVIZ_IMAGES;
constexpr int FLV_RUN_PIXELS = FLV_THREADS * FLV_RUN;
constexpr int FLV_RUN_DWORDS = (FLV_RUN_PIXELS * 3 + 4 + 3) / 4;          // a staged run of 3-byte pixels, any offset in a dword
constexpr int FLV_WHEEL = GFT_FLOWVIZ_WHEEL_ROWS;
constexpr float FLV_UNKNOWN = 200.f;                                       // UNKNOWN_FLOW_THRESH

static_assert(FLV_RUN == 4 && FLV_IMAGES == 3, "a lane packs four 3-byte pixels of each of the three images into three dwords");
static_assert(FLV_MAX_BLOCKS % FLV_THREADS == 0, "the fold reads FLV_MAX_BLOCKS / FLV_THREADS words per thread");

// the Middlebury colour wheel: six segments, in each one channel at 255, one ramping floor(255 * j / n) up or down
struct Wheel {
    uint8_t rgb[FLV_WHEEL * 3];
};

constexpr Wheel make_wheel()
{
    Wheel w{};
    const int length[6] = {15, 6, 4, 11, 13, 6};
    const int full[6] = {0, 1, 1, 2, 2, 0};              // the channel at 255
    const int ramp[6] = {1, 0, 2, 1, 0, 2};              // the channel that ramps: up in the even segments, down in the odd
    int row = 0;
    for (int s = 0; s < 6; s++)
        for (int j = 0; j < length[s]; j++, row++) {
            const int r = 255 * j / length[s];
            w.rgb[3 * row + full[s]] = 255;
            w.rgb[3 * row + ramp[s]] = (uint8_t)((s & 1) ? 255 - r : r);
        }
    return w;
}

constexpr Wheel FLV_WHEEL_TABLE = make_wheel();
const Wheel h_wheel = FLV_WHEEL_TABLE;
__device__ const Wheel d_wheel = FLV_WHEEL_TABLE;

struct FlowvizArgs {
    int64_t pixels;
    int blocks;
    const float* flow;              // R: planes 0 and 1, flow_stride apart
    const float* gt;                // T: planes 0 and 1, gt_stride apart
    int64_t flow_stride, gt_stride;
    float* partials;                // [blocks + 1]: the workgroups' maxima, then maxrad
    uint8_t* out;                   // [3][pixels][3]
};

int64_t flv_blocks(int64_t pixels) { return gft_grid_blocks(pixels, FLV_THREADS, FLV_RUN, FLV_MAX_BLOCKS); }

// |x0| > 200 or |x1| > 200: false for a NaN, true for an infinity
__device__ __forceinline__ bool unknown(float x0, float x1) { return fabsf(x0) > FLV_UNKNOWN || fabsf(x1) > FLV_UNKNOWN; }

// T as the sequence leaves it: both 0 where unknown, then both 0 where either is a NaN
__device__ __forceinline__ void clean_target(float& t0, float& t1)
{
    if (unknown(t0, t1) || t0 != t0 || t1 != t1) t0 = t1 = 0.f;
}

// the workgroup's maximum in every thread (no NaN reaches it); sRed has one slot per wave
__device__ __forceinline__ float block_max(float v, float* sRed)
{
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = sRed[0];
    for (int k = 1; k < FLV_THREADS / 64; k++) t = fmaxf(t, sRed[k]);
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(FLV_THREADS) void k_flowviz_maxrad(FlowvizArgs p)
{
    __shared__ float sRed[FLV_THREADS / 64];
    float hi = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * FLV_THREADS + threadIdx.x; i < p.pixels; i += (int64_t)gridDim.x * FLV_THREADS) {
        float t0 = p.gt[i], t1 = p.gt[p.gt_stride + i];
        clean_target(t0, t1);
        hi = fmaxf(hi, __fsqrt_rn(t0 * t0 + t1 * t1));
    }
    hi = block_max(hi, sRed);
    if (threadIdx.x == 0) p.partials[blockIdx.x] = hi;
}

// compute_color of one pixel whose unknown components are already 0, as 0x00BBGGRR; `black`: the pixel was unknown
__device__ __forceinline__ uint32_t flow_colour(float x0, float x1, double den, bool black, const double* wheel)
{
    double u = (double)x0 / den, v = (double)x1 / den;
    const bool nan = u != u || v != v;
    if (nan) u = v = 0.0;
    const double rad = sqrt(u * u + v * v);
    const double a = atan2(-v, -u) / 3.141592653589793;
    const double fk = (a + 1.0) / 2.0 * (double)(FLV_WHEEL - 1) + 1.0;
    const double fl = floor(fk);
    int k0 = (int)fl;
    k0 = k0 < 1 ? 1 : (k0 > FLV_WHEEL ? FLV_WHEEL : k0);           // 1..55 for every finite u, v: the clamp guards the table only
    const int k1 = k0 == FLV_WHEEL ? 1 : k0 + 1;
    const double f = fk - fl;
    uint32_t word = 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double c0 = wheel[3 * (k0 - 1) + c], c1 = wheel[3 * (k1 - 1) + c];
        double col = (1.0 - f) * c0 + f * c1;
        col = rad <= 1.0 ? 1.0 - rad * (1.0 - col) : col * 0.75;
        const uint32_t byte = (nan || black) ? 0u : (uint32_t)(int)floor(255.0 * col);
        word |= (byte > 255u ? 255u : byte) << (8 * c);
    }
    return word;
}

__global__ __launch_bounds__(FLV_THREADS) void k_flowviz_images(FlowvizArgs p)
{
    __shared__ double sWheel[FLV_WHEEL * 3];                      // wheel / 255
    __shared__ uint32_t sRun[FLV_IMAGES][FLV_RUN_DWORDS];
    __shared__ float sRed[FLV_THREADS / 64];
    const int tid = threadIdx.x;
    for (int k = tid; k < FLV_WHEEL * 3; k += FLV_THREADS) sWheel[k] = (double)d_wheel.rgb[k] / 255.0;
    float hi = 0.f;
    for (int b = tid; b < p.blocks; b += FLV_THREADS) hi = fmaxf(hi, p.partials[b]);
    const float maxrad = block_max(hi, sRed);                     // its first barrier also publishes sWheel
    if (blockIdx.x == 0 && tid == 0) p.partials[p.blocks] = maxrad;
    const float scaled = maxrad * 1.1f;                           // maxrad *= 1.1 stays float32
    const double den = (double)scaled + 0x1p-52;                  // + np.finfo(float).eps

    const int64_t runs = (p.pixels + FLV_RUN_PIXELS - 1) / FLV_RUN_PIXELS;
    for (int64_t run = blockIdx.x; run < runs; run += gridDim.x) {
        const int64_t i0 = run * FLV_RUN_PIXELS, i = i0 + (int64_t)FLV_RUN * tid;
        const int64_t left = p.pixels - i0;
        const int n = left < FLV_RUN_PIXELS ? (int)left : FLV_RUN_PIXELS;          // pixels of this run
        const int64_t mine = p.pixels - i;
        const int m = mine >= FLV_RUN ? FLV_RUN : (mine > 0 ? (int)mine : 0);       // pixels of this lane
        uint32_t px[FLV_IMAGES][FLV_RUN] = {};
#pragma unroll
        for (int j = 0; j < FLV_RUN; j++) {
            if (j < m) {
                float r0 = p.flow[i + j], r1 = p.flow[p.flow_stride + i + j];
                float t0 = p.gt[i + j], t1 = p.gt[p.gt_stride + i + j];
                const bool unk_r = unknown(r0, r1);
                if (unk_r) r0 = r1 = 0.f;
                clean_target(t0, t1);
                float e0 = t0 - r0, e1 = t1 - r1;
                const bool unk_e = unknown(e0, e1);
                if (unk_e) e0 = e1 = 0.f;
                px[0][j] = flow_colour(r0, r1, den, unk_r, sWheel);
                px[1][j] = flow_colour(t0, t1, den, false, sWheel);
                px[2][j] = flow_colour(e0, e1, den, unk_e, sWheel);
            }
        }
#pragma unroll
        for (int k = 0; k < FLV_IMAGES; k++) {
            // four RGB pixels as three little-endian dwords
            const uint32_t w[3] = {px[k][0] | px[k][1] << 24, px[k][1] >> 8 | px[k][2] << 16, px[k][2] >> 16 | px[k][3] << 8};
            const int mis = (int)((uintptr_t)(p.out + 3 * ((int64_t)k * p.pixels + i0)) & 3u);
            if (m == FLV_RUN && mis == 0) {
#pragma unroll
                for (int d = 0; d < 3; d++) sRun[k][3 * tid + d] = w[d];
            } else {
                uint8_t* s = reinterpret_cast<uint8_t*>(sRun[k]) + mis + 3 * FLV_RUN * tid;
#pragma unroll
                for (int b = 0; b < 3 * FLV_RUN; b++)
                    if (b < 3 * m) s[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
            }
        }
        __syncthreads();
        for (int k = 0; k < FLV_IMAGES; k++) gft_put_run<FLV_THREADS>(p.out + 3 * ((int64_t)k * p.pixels + i0), 3 * n, sRun[k]);
        __syncthreads();
    }
}

bool bad_stride(int64_t s) { return s < 0 || s > (1ll << 40); }

}  // namespace

extern "C" int64_t gft_flowviz_blocks(int64_t pixels)
{
    if (pixels < 1) return 0;
    return flv_blocks(pixels);
}

extern "C" const uint8_t* gft_flowviz_wheel(void)
{
    return h_wheel.rgb;
}

extern "C" int gft_flowviz_images(void* hip_stream, int32_t H, int32_t W, const float* flow, int64_t flow_plane_stride, const float* gt,
                                  int64_t gt_plane_stride, void* partials, void* out)
{
    if (H < 1 || W < 1 || (int64_t)H * W > (1ll << 40)) return gft_fail("gft_flowviz_images: bad size H=%d W=%d", H, W);
    if (!flow || !gt || !out) return gft_fail("gft_flowviz_images: flow, gt or out is NULL");
    if (bad_stride(flow_plane_stride) || bad_stride(gt_plane_stride)) return gft_fail("gft_flowviz_images: bad plane stride");
    if (!partials || ((uintptr_t)partials & 3u)) return gft_fail("gft_flowviz_images: partials is NULL or not 4-byte aligned");
    FlowvizArgs p = {};
    p.pixels = (int64_t)H * W;
    p.blocks = (int)flv_blocks(p.pixels);
    p.flow = flow; p.gt = gt;
    p.flow_stride = flow_plane_stride; p.gt_stride = gt_plane_stride;
    p.partials = static_cast<float*>(partials);
    p.out = static_cast<uint8_t*>(out);
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(k_flowviz_maxrad, dim3(p.blocks), dim3(FLV_THREADS), 0, s, p);
    hipLaunchKernelGGL(k_flowviz_images, dim3(p.blocks), dim3(FLV_THREADS), 0, s, p);
    return gft_launched("gft_flowviz_images");
}
