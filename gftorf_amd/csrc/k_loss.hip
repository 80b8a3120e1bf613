// k_loss.hip -- SSIM + a pixel term of two images, forward and backward, one launch each (include/gftorf_loss.h;
// utils/loss_utils.py:17-33, 51-53, 76-123).  One 16x16 tile of one channel per workgroup: the 26x26 input patch (window 11,
// zero padding outside the image) goes through LDS, the window is applied as its two 1-D factors (rows, then columns).  The
// pixel term is a template parameter (GFT_PIXEL_*); the pixel-only kernels at the end are for a term without SSIM.
#include "gft_internal.h"
#include "gft_reduce.h"
#include "gftorf_loss.h"

#include <type_traits>

namespace {

constexpr int TS = GFT_SSIM_TILE, WN = GFT_SSIM_WINDOW, HALO = WN / 2, PS = TS + 2 * HALO;      // 16, 11, 5, 26

struct LossArgs {
    int C, H, W, tiles_x, tiles_y;
    const float* __restrict__ a;        // img1
    const float* __restrict__ b;        // img2
    float* maps;                        // [3][C][H][W]
    float* partials;                    // [blocks][2]
    const float* __restrict__ g_ssim; const float* __restrict__ g_l2;       // g_l2: the pixel term's, whatever its kind
    float scale_ssim, scale_l2;
    float* grad;
    float w[WN];
    int n;                              // channels of the pixel term (the first n)
    float e;                            // the weighted kinds' offset
};

// The pixel term of channel ch at plane offset o (utils/loss_utils.py:17-33).  The weights are detached: no gradient flows
// through them.  WEIGHTED_L1's weight is e + the amplitude of ALL C channels of img1 at the pixel.
template <int KIND>
__device__ __forceinline__ float pixel_weight(const float* __restrict__ a, size_t o, size_t HW, int C, float e, float va)
{
    if constexpr (KIND == GFT_PIXEL_WEIGHTED_L1) {
        float s = 0.f;
        for (int c = 0; c < C; c++) { const float v = a[(size_t)c * HW + o]; s = fmaf(v, v, s); }
        return e + sqrtf(s);
    } else if constexpr (KIND == GFT_PIXEL_WEIGHTED_L1_QUAD || KIND == GFT_PIXEL_WEIGHTED_L2_QUAD) {
        return e + fabsf(va);
    } else {
        return 1.f;
    }
}

// value of the term for d = a - b and weight wt
template <int KIND>
__device__ __forceinline__ float pixel_value(float d, float wt)
{
    if constexpr (KIND == GFT_PIXEL_L2) return d * d;
    else if constexpr (KIND == GFT_PIXEL_L1) return fabsf(d);
    else if constexpr (KIND == GFT_PIXEL_WEIGHTED_L2_QUAD) { const float r = d / wt; return r * r; }
    else return fabsf(d / wt);
}

// its derivative by a (sign(0) = 0: torch's abs backward)
template <int KIND>
__device__ __forceinline__ float pixel_grad(float d, float wt)
{
    if constexpr (KIND == GFT_PIXEL_L2) return 2.f * d;
    else if constexpr (KIND == GFT_PIXEL_L1) return sign_of(d);
    else if constexpr (KIND == GFT_PIXEL_WEIGHTED_L2_QUAD) return 2.f * (d / wt) / wt;
    else return sign_of(d) / wt;
}

// rows pass: Q quantities of a [PS][PS] patch -> [PS][TS]; columns pass by the caller
template <int Q>
__device__ __forceinline__ void rows_pass(const float (*src)[PS][PS + 1], float (*dst)[PS][TS + 1], const float* w, int tid)
{
    for (int i = tid; i < PS * TS; i += TS * TS) {
        const int r = i / TS, c = i % TS;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < WN; k++) s = fmaf(w[k], src[q][r][c + k], s);
            dst[q][r][c] = s;
        }
    }
}

template <int KIND>
__global__ __launch_bounds__(TS * TS) void k_ssim_pix_fwd(LossArgs p)
{
    __shared__ float sIn[5][PS][PS + 1];          // a, b, a a, b b, a b
    __shared__ float sRow[5][PS][TS + 1];
    __shared__ float sRed[2][TS * TS / 64];
    const int tid = threadIdx.x;
    const int ch = blockIdx.x / (p.tiles_x * p.tiles_y), t = blockIdx.x % (p.tiles_x * p.tiles_y);
    const int x0 = (t % p.tiles_x) * TS, y0 = (t / p.tiles_x) * TS;
    const size_t plane = (size_t)ch * p.H * p.W;
    for (int i = tid; i < PS * PS; i += TS * TS) {
        const int r = i / PS, c = i % PS, y = y0 + r - HALO, x = x0 + c - HALO;
        float va = 0.f, vb = 0.f;
        if (y >= 0 && y < p.H && x >= 0 && x < p.W) { va = p.a[plane + (size_t)y * p.W + x]; vb = p.b[plane + (size_t)y * p.W + x]; }
        sIn[0][r][c] = va; sIn[1][r][c] = vb; sIn[2][r][c] = va * va; sIn[3][r][c] = vb * vb; sIn[4][r][c] = va * vb;
    }
    __syncthreads();
    rows_pass<5>(sIn, sRow, p.w, tid);
    __syncthreads();
    const int ty = tid / TS, tx = tid % TS, y = y0 + ty, x = x0 + tx;
    float v[5];
#pragma unroll
    for (int q = 0; q < 5; q++) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < WN; k++) s = fmaf(p.w[k], sRow[q][ty + k][tx], s);
        v[q] = s;
    }
    float ssim = 0.f, sq = 0.f;
    if (y < p.H && x < p.W) {
        // loss_utils.py:101-117
        const float mu1 = v[0], mu2 = v[1];
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const float s1 = v[2] - mu1_sq, s2 = v[3] - mu2_sq, s12 = v[4] - mu12;
        const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
        const float A1 = 2.f * mu12 + C1, A2 = 2.f * s12 + C2, B1 = mu1_sq + mu2_sq + C1, B2 = s1 + s2 + C2;
        const float rB1 = 1.f / B1, rB2 = 1.f / B2;
        ssim = (A1 * A2) * (rB1 * rB2);
        const float va = sIn[0][ty + HALO][tx + HALO], vb = sIn[1][ty + HALO][tx + HALO];
        const float d = va - vb;
        if constexpr (KIND == GFT_PIXEL_L2) {
            sq = d * d;
        } else if (ch < p.n) {
            const size_t HW = (size_t)p.H * p.W;
            sq = pixel_value<KIND>(d, pixel_weight<KIND>(p.a, (size_t)y * p.W + x, HW, p.C, p.e, va));
        }
        if (p.maps) {
            // d ssim / d (mu1, sigma1^2, sigma12) with the three treated as independent ...
            const float dmu1 = 2.f * mu2 * A2 * rB1 * rB2 - 2.f * mu1 * ssim * rB1;
            const float ds1 = -ssim * rB2;
            const float ds12 = 2.f * A1 * rB1 * rB2;
            // ... and sigma1^2 = E[a a] - mu1^2, sigma12 = E[a b] - mu1 mu2 folded into the mu1 map
            const size_t o = plane + (size_t)y * p.W + x, N = (size_t)p.C * p.H * p.W;
            p.maps[o] = dmu1 - 2.f * mu1 * ds1 - mu2 * ds12;
            p.maps[N + o] = ds1;
            p.maps[2 * N + o] = ds12;
        }
    }
    float s[2] = {ssim, sq};
    gft_fold_store<TS * TS>(s, sRed);          // the two sums of this tile in the order of gft_reduce.h
    __syncthreads();
    if (tid == 0) {
        p.partials[2 * (size_t)blockIdx.x] = gft_waves_total<TS * TS>(sRed[0]);
        p.partials[2 * (size_t)blockIdx.x + 1] = gft_waves_total<TS * TS>(sRed[1]);
    }
}

template <int KIND>
__global__ __launch_bounds__(TS * TS) void k_ssim_pix_bwd(LossArgs p)
{
    __shared__ float sIn[3][PS][PS + 1];
    __shared__ float sRow[3][PS][TS + 1];
    const int tid = threadIdx.x;
    const int ch = blockIdx.x / (p.tiles_x * p.tiles_y), t = blockIdx.x % (p.tiles_x * p.tiles_y);
    const int x0 = (t % p.tiles_x) * TS, y0 = (t / p.tiles_x) * TS;
    const size_t plane = (size_t)ch * p.H * p.W, N = (size_t)p.C * p.H * p.W;
    for (int i = tid; i < PS * PS; i += TS * TS) {
        const int r = i / PS, c = i % PS, y = y0 + r - HALO, x = x0 + c - HALO;
        const bool in = y >= 0 && y < p.H && x >= 0 && x < p.W;
        const size_t o = plane + (size_t)(in ? y : 0) * p.W + (in ? x : 0);
#pragma unroll
        for (int q = 0; q < 3; q++) sIn[q][r][c] = in ? p.maps[q * N + o] : 0.f;
    }
    __syncthreads();
    rows_pass<3>(sIn, sRow, p.w, tid);
    __syncthreads();
    const int ty = tid / TS, tx = tid % TS, y = y0 + ty, x = x0 + tx;
    if (y >= p.H || x >= p.W) return;
    float v[3];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < WN; k++) s = fmaf(p.w[k], sRow[q][ty + k][tx], s);
        v[q] = s;
    }
    const size_t o = plane + (size_t)y * p.W + x;
    const float va = p.a[o], vb = p.b[o];
    // the window is symmetric: the adjoint of the zero-padded blur is the same blur
    const float gs = p.g_ssim ? *p.g_ssim * p.scale_ssim : 0.f, gl = p.g_l2 ? *p.g_l2 * p.scale_l2 : 0.f;
    if constexpr (KIND == GFT_PIXEL_L2) {
        p.grad[o] = gs * (v[0] + 2.f * va * v[1] + vb * v[2]) + gl * 2.f * (va - vb);
    } else {
        float gp = 0.f;
        if (ch < p.n) gp = gl * pixel_grad<KIND>(va - vb, pixel_weight<KIND>(p.a, (size_t)y * p.W + x, (size_t)p.H * p.W, p.C, p.e, va));
        p.grad[o] = gs * (v[0] + 2.f * va * v[1] + vb * v[2]) + gp;
    }
}

// Pixel term alone: a grid-stride loop over the pixels, no LDS patch, no halo, no maps.  Each thread takes the first n channels
// of its pixels (one weight per pixel for WEIGHTED_L1); stage one of gft_reduce.h gives one partial per workgroup.
constexpr int PIX_THREADS = 256, PIX_PER_THREAD = 4, PIX_MAX_BLOCKS = 1024;

int pix_blocks(int64_t pixels) { return (int)gft_grid_blocks(pixels, PIX_THREADS, PIX_PER_THREAD, PIX_MAX_BLOCKS); }

struct PixArgs {
    int C, n;
    int64_t HW;
    float e, scale;
    const float* __restrict__ a;
    const float* __restrict__ b;
    float* partials;                    // [blocks]
    const float* __restrict__ g;        // device, one float
    float* grad;
};

template <int KIND>
__global__ __launch_bounds__(PIX_THREADS) void k_pix_fwd(PixArgs p)
{
    __shared__ float sRed[PIX_THREADS / 64];
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * PIX_THREADS + threadIdx.x; i < p.HW; i += (int64_t)gridDim.x * PIX_THREADS) {
        float wt = 1.f;
        if constexpr (KIND == GFT_PIXEL_WEIGHTED_L1) wt = pixel_weight<KIND>(p.a, (size_t)i, (size_t)p.HW, p.C, p.e, 0.f);
        for (int c = 0; c < p.n; c++) {
            const size_t o = (size_t)c * p.HW + i;
            const float va = p.a[o], vb = p.b[o];
            if constexpr (KIND == GFT_PIXEL_WEIGHTED_L1_QUAD || KIND == GFT_PIXEL_WEIGHTED_L2_QUAD) wt = p.e + fabsf(va);
            s += pixel_value<KIND>(va - vb, wt);
        }
    }
    gft_fold_store<PIX_THREADS>(s, sRed);
    __syncthreads();
    if (threadIdx.x == 0) p.partials[blockIdx.x] = gft_waves_total<PIX_THREADS>(sRed) * p.scale;
}

// grad over all C channels: the term's gradient on the first n, 0 on the rest
template <int KIND>
__global__ __launch_bounds__(PIX_THREADS) void k_pix_bwd(PixArgs p)
{
    const float g = *p.g * p.scale;
    for (int64_t i = (int64_t)blockIdx.x * PIX_THREADS + threadIdx.x; i < p.HW; i += (int64_t)gridDim.x * PIX_THREADS) {
        float wt = 1.f;
        if constexpr (KIND == GFT_PIXEL_WEIGHTED_L1) wt = pixel_weight<KIND>(p.a, (size_t)i, (size_t)p.HW, p.C, p.e, 0.f);
        for (int c = 0; c < p.C; c++) {
            const size_t o = (size_t)c * p.HW + i;
            float v = 0.f;
            if (c < p.n) {
                const float va = p.a[o], vb = p.b[o];
                if constexpr (KIND == GFT_PIXEL_WEIGHTED_L1_QUAD || KIND == GFT_PIXEL_WEIGHTED_L2_QUAD) wt = p.e + fabsf(va);
                v = g * pixel_grad<KIND>(va - vb, wt);
            }
            p.grad[o] = v;
        }
    }
}

int fill(LossArgs& p, int32_t C, int32_t H, int32_t W, const float* a, const float* b, const float* window, const char* who)
{
    if (C <= 0 || H <= 0 || W <= 0) return gft_fail("%s: bad sizes C=%d H=%d W=%d", who, C, H, W);
    if (!a || !b || !window) return gft_fail("%s: NULL argument", who);
    p.C = C; p.H = H; p.W = W; p.n = C;
    p.tiles_x = (W + TS - 1) / TS; p.tiles_y = (H + TS - 1) / TS;
    p.a = a; p.b = b;
    for (int k = 0; k < WN; k++) p.w[k] = window[k];
    return 0;
}

// kind and n: n channels of the term, 1 <= n <= C; only WEIGHTED_L1 takes n < C
int check_kind(int32_t kind, int32_t C, int32_t n, const char* who)
{
    if (kind < GFT_PIXEL_L2 || kind > GFT_PIXEL_WEIGHTED_L2_QUAD) return gft_fail("%s: unknown pixel kind %d", who, kind);
    if (n < 1 || n > C) return gft_fail("%s: n=%d outside [1, C=%d]", who, n, C);
    if (n != C && kind != GFT_PIXEL_WEIGHTED_L1) return gft_fail("%s: n=%d != C=%d for kind %d", who, n, C, kind);
    return 0;
}

// f(std::integral_constant<int, KIND>) for the kind: one instantiation per kind of each kernel
template <typename F>
void by_kind(int32_t kind, F&& f)
{
    switch (kind) {
    case GFT_PIXEL_L2: f(std::integral_constant<int, GFT_PIXEL_L2>{}); break;
    case GFT_PIXEL_L1: f(std::integral_constant<int, GFT_PIXEL_L1>{}); break;
    case GFT_PIXEL_WEIGHTED_L1: f(std::integral_constant<int, GFT_PIXEL_WEIGHTED_L1>{}); break;
    case GFT_PIXEL_WEIGHTED_L1_QUAD: f(std::integral_constant<int, GFT_PIXEL_WEIGHTED_L1_QUAD>{}); break;
    default: f(std::integral_constant<int, GFT_PIXEL_WEIGHTED_L2_QUAD>{}); break;
    }
}

int image_forward(void* hip_stream, int32_t kind, int32_t C, int32_t H, int32_t W, int32_t n, float e, const float* img1,
                  const float* img2, const float* window, float* maps, float* partials, const char* who)
{
    LossArgs p = {};
    if (fill(p, C, H, W, img1, img2, window, who) || check_kind(kind, C, n, who)) return 1;
    if (!partials) return gft_fail("%s: partials is NULL", who);
    p.n = n; p.e = e; p.maps = maps; p.partials = partials;
    const int64_t blocks = gft_ssim_blocks(C, H, W);
    if (blocks > 0x7fffffffll) return gft_fail("%s: image too large", who);
    by_kind(kind, [&](auto k) {
        hipLaunchKernelGGL(k_ssim_pix_fwd<decltype(k)::value>, dim3((unsigned)blocks), dim3(TS * TS), 0, (hipStream_t)hip_stream, p);
    });
    return gft_launched(who);
}

int image_backward(void* hip_stream, int32_t kind, int32_t C, int32_t H, int32_t W, int32_t n, float e, const float* img1,
                   const float* img2, const float* window, const float* maps, const float* g_ssim, const float* g_pixel,
                   float scale_ssim, float scale_pixel, float* grad_img1, const char* who)
{
    LossArgs p = {};
    if (fill(p, C, H, W, img1, img2, window, who) || check_kind(kind, C, n, who)) return 1;
    if (!maps || !grad_img1) return gft_fail("%s: NULL argument", who);
    p.n = n; p.e = e;
    p.maps = const_cast<float*>(maps); p.g_ssim = g_ssim; p.g_l2 = g_pixel; p.scale_ssim = scale_ssim; p.scale_l2 = scale_pixel;
    p.grad = grad_img1;
    const int64_t blocks = gft_ssim_blocks(C, H, W);
    if (blocks > 0x7fffffffll) return gft_fail("%s: image too large", who);
    by_kind(kind, [&](auto k) {
        hipLaunchKernelGGL(k_ssim_pix_bwd<decltype(k)::value>, dim3((unsigned)blocks), dim3(TS * TS), 0, (hipStream_t)hip_stream, p);
    });
    return gft_launched(who);
}

}  // namespace

extern "C" int64_t gft_ssim_blocks(int32_t C, int32_t H, int32_t W)
{
    if (C <= 0 || H <= 0 || W <= 0) return 0;
    return (int64_t)C * ((W + TS - 1) / TS) * ((H + TS - 1) / TS);
}

extern "C" int gft_ssim_l2_forward(void* hip_stream, int32_t C, int32_t H, int32_t W, const float* img1, const float* img2,
                                   const float* window, float* maps, float* partials)
{
    return image_forward(hip_stream, GFT_PIXEL_L2, C, H, W, C, 0.f, img1, img2, window, maps, partials, "gft_ssim_l2_forward");
}

extern "C" int gft_ssim_l2_backward(void* hip_stream, int32_t C, int32_t H, int32_t W, const float* img1, const float* img2,
                                    const float* window, const float* maps, const float* g_ssim, const float* g_l2,
                                    float scale_ssim, float scale_l2, float* grad_img1)
{
    return image_backward(hip_stream, GFT_PIXEL_L2, C, H, W, C, 0.f, img1, img2, window, maps, g_ssim, g_l2, scale_ssim,
                          scale_l2, grad_img1, "gft_ssim_l2_backward");
}

extern "C" int gft_image_loss_forward(void* hip_stream, int32_t kind, int32_t C, int32_t H, int32_t W, int32_t n, float e,
                                      const float* img1, const float* img2, const float* window, float* maps, float* partials)
{
    return image_forward(hip_stream, kind, C, H, W, n, e, img1, img2, window, maps, partials, "gft_image_loss_forward");
}

extern "C" int gft_image_loss_backward(void* hip_stream, int32_t kind, int32_t C, int32_t H, int32_t W, int32_t n, float e,
                                       const float* img1, const float* img2, const float* window, const float* maps,
                                       const float* g_ssim, const float* g_pixel, float scale_ssim, float scale_pixel,
                                       float* grad_img1)
{
    return image_backward(hip_stream, kind, C, H, W, n, e, img1, img2, window, maps, g_ssim, g_pixel, scale_ssim, scale_pixel,
                          grad_img1, "gft_image_loss_backward");
}

extern "C" int64_t gft_pixel_loss_blocks(int32_t C, int32_t H, int32_t W)
{
    if (C <= 0 || H <= 0 || W <= 0) return 0;
    return pix_blocks((int64_t)H * W);
}

static int pix_fill(PixArgs& p, int32_t kind, int32_t C, int32_t H, int32_t W, int32_t n, float e, float scale,
                    const float* a, const float* b, const char* who)
{
    if (C <= 0 || H <= 0 || W <= 0) return gft_fail("%s: bad sizes C=%d H=%d W=%d", who, C, H, W);
    if (!a || !b) return gft_fail("%s: NULL argument", who);
    if (check_kind(kind, C, n, who)) return 1;
    p.C = C; p.n = n; p.HW = (int64_t)H * W; p.e = e; p.scale = scale; p.a = a; p.b = b;
    return 0;
}

extern "C" int gft_pixel_loss_forward(void* hip_stream, int32_t kind, int32_t C, int32_t H, int32_t W, int32_t n, float e,
                                      const float* img1, const float* img2, float scale, float* partials)
{
    PixArgs p = {};
    if (pix_fill(p, kind, C, H, W, n, e, scale, img1, img2, "gft_pixel_loss_forward")) return 1;
    if (!partials) return gft_fail("gft_pixel_loss_forward: partials is NULL");
    p.partials = partials;
    by_kind(kind, [&](auto k) {
        hipLaunchKernelGGL(k_pix_fwd<decltype(k)::value>, dim3(pix_blocks(p.HW)), dim3(PIX_THREADS), 0, (hipStream_t)hip_stream, p);
    });
    return gft_launched("gft_pixel_loss_forward");
}

extern "C" int gft_pixel_loss_backward(void* hip_stream, int32_t kind, int32_t C, int32_t H, int32_t W, int32_t n, float e,
                                       const float* img1, const float* img2, const float* g_pixel, float scale,
                                       float* grad_img1)
{
    PixArgs p = {};
    if (pix_fill(p, kind, C, H, W, n, e, scale, img1, img2, "gft_pixel_loss_backward")) return 1;
    if (!g_pixel || !grad_img1) return gft_fail("gft_pixel_loss_backward: NULL argument");
    p.g = g_pixel; p.grad = grad_img1;
    by_kind(kind, [&](auto k) {
        hipLaunchKernelGGL(k_pix_bwd<decltype(k)::value>, dim3(pix_blocks(p.HW)), dim3(PIX_THREADS), 0, (hipStream_t)hip_stream, p);
    });
    return gft_launched("gft_pixel_loss_backward");
}
