// k_present.hip -- a rendered view's display images (include/gftorf_present.h; render.py:105-189, :43-54).  One pass over up
// to 13 float planes that writes the uint8 images the reference forms in numpy, 27 bytes per pixel, into one sheet.
// k_present_minmax: min / max partials of dd, one row per workgroup.  k_present_view: every workgroup finishes those
// partials (at most 1024 rows, 4 per thread), then walks runs of 256 pixels: the 4-byte colour-map pixels and the two float
// images are stored per lane; the 3-byte HWC pixels and the 1-byte planes are staged in LDS at the destination's offset
// within a dword and leave as whole dwords, with byte stores only for a run's ragged head and tail.
// k_present_ranges_part / _finish: the (lo, hi) of the ground truth's real, imag and amp images, folded into six floats.
// k_present_quad: tof_to_image (scene/torf_utils.py:43-50) of the four quad planes, staged and stored as k_present_view's
// 3-byte pixels are.
// No atomics, no memset, scalar loads (each coalesced across the wave).
//
// The arithmetic is numpy's float32 sequence operation for operation: nothing here may contract into a multiply-add, and
// every division is the correctly rounded one (hipcc's default for fp32 `/`).  min and max propagate a NaN as np.min / np.max.
#include "gft_internal.h"
#include "gft_reduce.h"
#include "gft_tof_depth.h"
#include "gft_byte_runs.h"
#include "gft_present_magma.h"
#include "gft_present_ops.h"
#include "gft_present_seismic.h"
#include "gftorf_present.h"

#pragma clang fp contract(off)

namespace {

constexpr int PRS_THREADS = 256, PRS_MAX_BLOCKS = 1024, PRS_IMAGES = GFT_PRESENT_IMAGES;
constexpr int PRS_RUN3 = (PRS_THREADS * 3 + 4 + 3) / 4;      // dwords of a staged run of 3-byte pixels, any offset in a dword
constexpr int PRS_RUN1 = (PRS_THREADS + 4 + 3) / 4;
constexpr int PRS_BPP[PRS_IMAGES] = {3, 3, 3, 1, 4, 4, 4, 4, 1, 4, 4};

static_assert(GFT_MAGMA_ROWS == GFT_PRESENT_MAGMA_ROWS && GFT_PRESENT_PARTIAL_WORDS == 2 && GFT_PRESENT_RANGE_WORDS == 6, "header");
static_assert(PRS_MAX_BLOCKS % PRS_THREADS == 0, "the finish reads PRS_MAX_BLOCKS / PRS_THREADS rows per thread");

const uint32_t h_magma[GFT_MAGMA_ROWS] = {GFT_MAGMA_TABLE};
__device__ const uint32_t d_magma[GFT_MAGMA_ROWS] = {GFT_MAGMA_TABLE};
static_assert(GFT_SEISMIC_ROWS == GFT_PRESENT_SEISMIC_ROWS, "header");
const uint32_t h_seismic[GFT_SEISMIC_ROWS] = {GFT_SEISMIC_TABLE};
__device__ const uint32_t d_seismic[GFT_SEISMIC_ROWS] = {GFT_SEISMIC_TABLE};

struct PresentArgs {
    int64_t pixels;
    int blocks;
    const float* image;                         // 3 planes image_stride apart, or NULL
    const float* phasor;                        // phasor_planes planes phasor_stride apart, or NULL
    const float* depth;
    const float* acc;
    const float* dd;
    int64_t image_stride, phasor_stride;
    const float* ranges_dev;
    float ranges[GFT_PRESENT_RANGE_WORDS];
    const float* depth_range_dev;
    const float* phase_offset_dev;
    float depth_range, phase_offset, znear, zfar, mult;
    float* partials;                            // [blocks][2]
    uint8_t* out[PRS_IMAGES];                   // NULL for an image the groups do not produce
};

int64_t prs_blocks(int64_t pixels) { return gft_grid_blocks(pixels, PRS_THREADS, 1, PRS_MAX_BLOCKS); }

// nmin, nmax, clip01, to8b, norm01 and magma: gft_present_ops.h

// min or max of the workgroup's values in every thread; sRed has one slot per wave
template <bool MAX>
__device__ __forceinline__ float block_fold(float v, float* sRed)
{
    for (int o = 32; o > 0; o >>= 1) {
        const float w = __shfl_xor(v, o);
        v = MAX ? nmax(v, w) : nmin(v, w);
    }
    if ((threadIdx.x & 63) == 0) sRed[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = sRed[0];
    for (int k = 1; k < PRS_THREADS / 64; k++) t = MAX ? nmax(t, sRed[k]) : nmin(t, sRed[k]);
    __syncthreads();
    return t;
}

__global__ __launch_bounds__(PRS_THREADS) void k_present_minmax(PresentArgs p)
{
    __shared__ float sRed[PRS_THREADS / 64];
    float lo = INFINITY, hi = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * PRS_THREADS + threadIdx.x; i < p.pixels; i += (int64_t)gridDim.x * PRS_THREADS) {
        const float v = p.dd[i];
        lo = nmin(lo, v);
        hi = nmax(hi, v);
    }
    lo = block_fold<false>(lo, sRed);
    hi = block_fold<true>(hi, sRed);
    if (threadIdx.x == 0) {
        p.partials[2 * blockIdx.x] = lo;
        p.partials[2 * blockIdx.x + 1] = hi;
    }
}

// gft_put_run (gft_byte_runs.h) by this file's workgroup
__device__ __forceinline__ void put_run(uint8_t* dst, int nbytes, const uint32_t* lds) { gft_put_run<PRS_THREADS>(dst, nbytes, lds); }

__global__ __launch_bounds__(PRS_THREADS) void k_present_view(PresentArgs p)
{
    __shared__ uint32_t sMagma[GFT_MAGMA_ROWS];
    __shared__ uint32_t sRun3[3][PRS_RUN3];           // color, real, imag
    __shared__ uint32_t sRun1[6][PRS_RUN1];           // amp, quad 0..3, dd
    __shared__ float sRed[PRS_THREADS / 64];
    const int tid = threadIdx.x;
    for (int k = tid; k < GFT_MAGMA_ROWS; k += PRS_THREADS) sMagma[k] = d_magma[k];
    float dd_lo = 0.f, dd_span = 0.f;
    if (p.dd) {
        float lo = INFINITY, hi = -INFINITY;
        for (int b = tid; b < p.blocks; b += PRS_THREADS) {
            lo = nmin(lo, p.partials[2 * b]);
            hi = nmax(hi, p.partials[2 * b + 1]);
        }
        dd_lo = block_fold<false>(lo, sRed);
        dd_span = block_fold<true>(hi, sRed) - dd_lo;
    }
    float rg[GFT_PRESENT_RANGE_WORDS];
#pragma unroll
    for (int k = 0; k < GFT_PRESENT_RANGE_WORDS; k++) rg[k] = p.ranges_dev ? p.ranges_dev[k] : p.ranges[k];
    const float re_lo = rg[0], re_span = rg[1] - rg[0], im_lo = rg[2], im_span = rg[3] - rg[2], am_lo = rg[4], am_span = rg[5] - rg[4];
    const float dr = gft_dev_or(p.depth_range_dev, p.depth_range), off = gft_dev_or(p.phase_offset_dev, p.phase_offset);
    const float span = p.zfar - p.znear;
    const bool quad = p.out[GFT_PRESENT_QUAD] != nullptr;
    __syncthreads();

    const int64_t runs = (p.pixels + PRS_THREADS - 1) / PRS_THREADS;
    for (int64_t run = blockIdx.x; run < runs; run += gridDim.x) {
        const int64_t i0 = run * PRS_THREADS, i = i0 + tid;
        const int64_t left = p.pixels - i0;
        const int n = left < PRS_THREADS ? (int)left : PRS_THREADS;
        if (tid < n) {
            if (p.image) {
                uint8_t* s = reinterpret_cast<uint8_t*>(sRun3[0]) + ((uintptr_t)(p.out[GFT_PRESENT_COLOR] + 3 * i0) & 3u) + 3 * tid;
#pragma unroll
                for (int c = 0; c < 3; c++) s[c] = (uint8_t)to8b(p.image[c * p.image_stride + i]);
            }
            if (p.phasor) {
                const float re = p.phasor[i], im = p.phasor[p.phasor_stride + i];
#pragma unroll
                for (int c = 0; c < 2; c++) {
                    // graphics_utils.py:125-137 on the multiplied plane: red where positive, blue the negated negative part
                    const float v = (c ? im : re) * p.mult;
                    const float r = v <= 0.f ? 0.f : v, b = -(v >= 0.f ? 0.f : v);
                    const float lo = c ? im_lo : re_lo, sp = c ? im_span : re_span;
                    const int img = c ? GFT_PRESENT_IMAG : GFT_PRESENT_REAL;
                    uint8_t* s = reinterpret_cast<uint8_t*>(sRun3[1 + c]) + ((uintptr_t)(p.out[img] + 3 * i0) & 3u) + 3 * tid;
                    s[0] = (uint8_t)to8b(norm01(r, lo, sp));
                    s[1] = (uint8_t)to8b(norm01(0.f, lo, sp));
                    s[2] = (uint8_t)to8b(norm01(b, lo, sp));
                }
                {
                    uint8_t* s = reinterpret_cast<uint8_t*>(sRun1[0]) + ((uintptr_t)(p.out[GFT_PRESENT_AMP] + i0) & 3u) + tid;
                    s[0] = (uint8_t)to8b(norm01(p.phasor[2 * p.phasor_stride + i] * p.mult, am_lo, am_span));
                }
                if (quad) {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        uint8_t* s = reinterpret_cast<uint8_t*>(sRun1[1 + k]) +
                                     ((uintptr_t)(p.out[GFT_PRESENT_QUAD] + k * p.pixels + i0) & 3u) + tid;
                        s[0] = (uint8_t)to8b(fabsf(p.phasor[(3 + k) * p.phasor_stride + i]));
                    }
                }
                const float d = depth_from_tof_np(re, im, dr, off);
                reinterpret_cast<float*>(p.out[GFT_PRESENT_DEPTH_TOF_F])[i] = d;
                reinterpret_cast<uint32_t*>(p.out[GFT_PRESENT_DEPTH_TOF])[i] = magma(sMagma, d, p.znear, span);
            }
            if (p.depth) {
                const float d = p.depth[i];
                reinterpret_cast<uint32_t*>(p.out[GFT_PRESENT_DEPTH])[i] = magma(sMagma, d, p.znear, span);
                if (p.acc) {
                    const float dn = d / p.acc[i];
                    reinterpret_cast<float*>(p.out[GFT_PRESENT_DEPTH_NORM_F])[i] = dn;
                    reinterpret_cast<uint32_t*>(p.out[GFT_PRESENT_DEPTH_NORM])[i] = magma(sMagma, dn, p.znear, span);
                }
            }
            if (p.dd) {
                uint8_t* s = reinterpret_cast<uint8_t*>(sRun1[5]) + ((uintptr_t)(p.out[GFT_PRESENT_DD] + i0) & 3u) + tid;
                s[0] = (uint8_t)to8b(norm01(p.dd[i], dd_lo, dd_span));
            }
        }
        __syncthreads();
        if (p.image) put_run(p.out[GFT_PRESENT_COLOR] + 3 * i0, 3 * n, sRun3[0]);
        if (p.phasor) {
            put_run(p.out[GFT_PRESENT_REAL] + 3 * i0, 3 * n, sRun3[1]);
            put_run(p.out[GFT_PRESENT_IMAG] + 3 * i0, 3 * n, sRun3[2]);
            put_run(p.out[GFT_PRESENT_AMP] + i0, n, sRun1[0]);
            if (quad) {
                for (int k = 0; k < 4; k++) put_run(p.out[GFT_PRESENT_QUAD] + k * p.pixels + i0, n, sRun1[1 + k]);
            }
        }
        if (p.dd) put_run(p.out[GFT_PRESENT_DD] + i0, n, sRun1[5]);
        __syncthreads();
    }
}

// the six values of one pixel's ground truth folded into lo / hi: the red / blue images of planes 0 and 1 with their zero
// green channel (graphics_utils.py:125-137), and plane 2
__global__ __launch_bounds__(PRS_THREADS) void k_present_ranges_part(int64_t pixels, const float* __restrict__ gt, int64_t stride,
                                                                     float* __restrict__ partials)
{
    __shared__ float sRed[PRS_THREADS / 64];
    float r[GFT_PRESENT_RANGE_WORDS] = {0.f, 0.f, 0.f, 0.f, INFINITY, -INFINITY};       // the green channel is 0 everywhere
    for (int64_t i = (int64_t)blockIdx.x * PRS_THREADS + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * PRS_THREADS) {
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const float v = gt[c * stride + i];
            const float red = v <= 0.f ? 0.f : v, blue = -(v >= 0.f ? 0.f : v);
            r[2 * c] = nmin(nmin(r[2 * c], red), blue);
            r[2 * c + 1] = nmax(nmax(r[2 * c + 1], red), blue);
        }
        const float a = gt[2 * stride + i];
        r[4] = nmin(r[4], a);
        r[5] = nmax(r[5], a);
    }
#pragma unroll
    for (int k = 0; k < GFT_PRESENT_RANGE_WORDS; k++) {
        const float t = (k & 1) ? block_fold<true>(r[k], sRed) : block_fold<false>(r[k], sRed);
        if (threadIdx.x == 0) partials[(size_t)blockIdx.x * GFT_PRESENT_RANGE_WORDS + k] = t;
    }
}

// one workgroup: the rows of partials, then ranges = min / max (ranges, this view's)
__global__ __launch_bounds__(PRS_THREADS) void k_present_ranges_finish(int blocks, const float* __restrict__ partials, float* ranges)
{
    __shared__ float sRed[PRS_THREADS / 64];
#pragma unroll
    for (int k = 0; k < GFT_PRESENT_RANGE_WORDS; k++) {
        float v = (k & 1) ? -INFINITY : INFINITY;
        for (int b = threadIdx.x; b < blocks; b += PRS_THREADS) {
            const float w = partials[(size_t)b * GFT_PRESENT_RANGE_WORDS + k];
            v = (k & 1) ? nmax(v, w) : nmin(v, w);
        }
        const float t = (k & 1) ? block_fold<true>(v, sRed) : block_fold<false>(v, sRed);
        if (threadIdx.x == 0) ranges[k] = (k & 1) ? nmax(ranges[k], t) : nmin(ranges[k], t);
    }
}

__global__ void k_present_ranges_reset(float* ranges)
{
    if (threadIdx.x < GFT_PRESENT_RANGE_WORDS) ranges[threadIdx.x] = (threadIdx.x & 1) ? -INFINITY : INFINITY;
}

// tof_to_image of one value as an RGBx word: np.clip(x, -0.5, 0.5) keeps a NaN; Normalize(-0.5, 0.5) of a float32 is
// (c - -0.5) / 1 in float32; matplotlib's index of that is trunc(n * 256) with 256 (n == 1) taken as 255, a NaN the bad colour
__device__ __forceinline__ uint32_t seismic(const uint32_t* table, float x)
{
    const float c = x < -0.5f ? -0.5f : (x > 0.5f ? 0.5f : x);
    const float n = c + 0.5f;
    int row;
    if (n != n) row = 256;
    else {
        const float s = n * 256.f;
        row = s >= 256.f ? 255 : (int)s;
    }
    return table[row];
}

struct QuadArgs {
    int64_t pixels;
    const float* phasor;            // 7 planes `stride` apart
    int64_t stride;
    int plane[4];                   // 3 + permutation[k]
    int has_gt, tonemap;
    uint8_t* out;                   // [4][pixels][3]
};

__global__ __launch_bounds__(PRS_THREADS) void k_present_quad(QuadArgs p)
{
    __shared__ uint32_t sSeismic[GFT_SEISMIC_ROWS];
    __shared__ uint32_t sRun3[4][PRS_RUN3];
    const int tid = threadIdx.x;
    for (int k = tid; k < GFT_SEISMIC_ROWS; k += PRS_THREADS) sSeismic[k] = d_seismic[k];
    __syncthreads();
    const int64_t runs = (p.pixels + PRS_THREADS - 1) / PRS_THREADS;
    for (int64_t run = blockIdx.x; run < runs; run += gridDim.x) {
        const int64_t i0 = run * PRS_THREADS, i = i0 + tid;
        const int64_t left = p.pixels - i0;
        const int n = left < PRS_THREADS ? (int)left : PRS_THREADS;
        if (tid < n) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                // render_ftorf_viz_traj.py:238-243: minus 0.5 with a ground truth, then the tonemap x / (1 + x)
                float v = p.phasor[p.plane[k] * p.stride + i];
                if (p.has_gt) v = v - 0.5f;
                if (p.tonemap) v = v / (1.f + v);
                const uint32_t w = seismic(sSeismic, v);
                uint8_t* s = reinterpret_cast<uint8_t*>(sRun3[k]) + ((uintptr_t)(p.out + 3 * (k * p.pixels + i0)) & 3u) + 3 * tid;
                s[0] = (uint8_t)w;
                s[1] = (uint8_t)(w >> 8);
                s[2] = (uint8_t)(w >> 16);
            }
        }
        __syncthreads();
        for (int k = 0; k < 4; k++) put_run(p.out + 3 * (k * p.pixels + i0), 3 * n, sRun3[k]);
        __syncthreads();
    }
}

// offsets of the images the groups produce, -1 for the others; the sheet's bytes, or 0 for groups that make no sense
int64_t prs_layout(int64_t pixels, int groups, int64_t* offsets)
{
    const int all = GFT_PRESENT_HAS_COLOR | GFT_PRESENT_HAS_PHASOR | GFT_PRESENT_HAS_QUAD | GFT_PRESENT_HAS_DEPTH | GFT_PRESENT_HAS_ACC |
                    GFT_PRESENT_HAS_DD;
    if (pixels < 1 || pixels > (1ll << 40) || groups <= 0 || (groups & ~all)) return 0;
    if ((groups & GFT_PRESENT_HAS_QUAD) && !(groups & GFT_PRESENT_HAS_PHASOR)) return 0;
    if ((groups & GFT_PRESENT_HAS_ACC) && !(groups & GFT_PRESENT_HAS_DEPTH)) return 0;
    const int needs[PRS_IMAGES] = {GFT_PRESENT_HAS_COLOR, GFT_PRESENT_HAS_PHASOR, GFT_PRESENT_HAS_PHASOR, GFT_PRESENT_HAS_PHASOR,
                                   GFT_PRESENT_HAS_QUAD, GFT_PRESENT_HAS_DEPTH, GFT_PRESENT_HAS_PHASOR, GFT_PRESENT_HAS_ACC,
                                   GFT_PRESENT_HAS_DD, GFT_PRESENT_HAS_PHASOR, GFT_PRESENT_HAS_ACC};
    int64_t pos = 0;
    for (int k = 0; k < PRS_IMAGES; k++) {
        const bool on = (groups & needs[k]) != 0;
        if (offsets) offsets[k] = on ? pos : -1;
        if (on) pos += (PRS_BPP[k] * pixels + GFT_PRESENT_ALIGN - 1) / GFT_PRESENT_ALIGN * GFT_PRESENT_ALIGN;
    }
    return pos;
}

bool bad_stride(int64_t s) { return s < 0 || s > (1ll << 40); }

}  // namespace

extern "C" int64_t gft_present_blocks(int64_t pixels)
{
    if (pixels < 1) return 0;
    return prs_blocks(pixels);
}

extern "C" int64_t gft_present_sheet_bytes(int32_t H, int32_t W, int32_t groups, int64_t* offsets_out)
{
    if (H < 1 || W < 1) return 0;
    return prs_layout((int64_t)H * W, groups, offsets_out);
}

extern "C" const uint8_t* gft_present_magma(void)
{
    return reinterpret_cast<const uint8_t*>(h_magma);
}

extern "C" int gft_present_view(void* hip_stream, int32_t H, int32_t W, const float* image, int64_t image_stride, const float* phasor,
                                int64_t phasor_stride, int32_t phasor_planes, const float* depth, const float* acc, const float* dd,
                                const float* ranges_dev, const float* ranges_host, const float* depth_range_dev, float depth_range,
                                const float* phase_offset_dev, float phase_offset, float znear, float zfar, float tof_multiplier,
                                void* partials, void* sheet)
{
    if (H < 1 || W < 1 || (int64_t)H * W > (1ll << 40)) return gft_fail("gft_present_view: bad size H=%d W=%d", H, W);
    if (!image && !phasor && !depth && !dd) return gft_fail("gft_present_view: no image, phasor, depth or dd is given");
    if (phasor ? phasor_planes < 3 : phasor_planes != 0)
        return gft_fail("gft_present_view: phasor_planes=%d: a phasor has at least 3 planes, and 0 are given without one", phasor_planes);
    if (acc && !depth) return gft_fail("gft_present_view: acc without depth");
    if (phasor && !ranges_dev && !ranges_host) return gft_fail("gft_present_view: phasor without ranges");
    if (bad_stride(image_stride) || bad_stride(phasor_stride)) return gft_fail("gft_present_view: bad plane stride");
    if (dd && (!partials || ((uintptr_t)partials & 3u))) return gft_fail("gft_present_view: dd needs partials, NULL or not 4-byte aligned");
    if (!sheet || ((uintptr_t)sheet & (GFT_PRESENT_ALIGN - 1))) return gft_fail("gft_present_view: sheet is NULL or not 16-byte aligned");
    const int groups = (image ? GFT_PRESENT_HAS_COLOR : 0) | (phasor ? GFT_PRESENT_HAS_PHASOR : 0) |
                       (phasor_planes == 7 ? GFT_PRESENT_HAS_QUAD : 0) | (depth ? GFT_PRESENT_HAS_DEPTH : 0) |
                       (acc ? GFT_PRESENT_HAS_ACC : 0) | (dd ? GFT_PRESENT_HAS_DD : 0);
    PresentArgs p = {};
    p.pixels = (int64_t)H * W;
    int64_t offsets[PRS_IMAGES];
    if (prs_layout(p.pixels, groups, offsets) < 1) return gft_fail("gft_present_view: bad groups %d", groups);
    for (int k = 0; k < PRS_IMAGES; k++) p.out[k] = offsets[k] < 0 ? nullptr : static_cast<uint8_t*>(sheet) + offsets[k];
    p.blocks = (int)prs_blocks(p.pixels);
    p.image = image; p.phasor = phasor; p.depth = depth; p.acc = acc; p.dd = dd;
    p.image_stride = image_stride; p.phasor_stride = phasor_stride;
    p.ranges_dev = phasor ? ranges_dev : nullptr;
    if (phasor && !ranges_dev)
        for (int k = 0; k < GFT_PRESENT_RANGE_WORDS; k++) p.ranges[k] = ranges_host[k];
    p.depth_range_dev = depth_range_dev; p.phase_offset_dev = phase_offset_dev;
    p.depth_range = depth_range; p.phase_offset = phase_offset;
    p.znear = znear; p.zfar = zfar; p.mult = tof_multiplier;
    p.partials = static_cast<float*>(partials);
    hipStream_t s = (hipStream_t)hip_stream;
    if (dd) hipLaunchKernelGGL(k_present_minmax, dim3(p.blocks), dim3(PRS_THREADS), 0, s, p);
    hipLaunchKernelGGL(k_present_view, dim3(p.blocks), dim3(PRS_THREADS), 0, s, p);
    return gft_launched("gft_present_view");
}

extern "C" int gft_present_ranges(void* hip_stream, int64_t pixels, const float* gt_tof, int64_t stride, void* partials, float* ranges)
{
    if (pixels < 1 || pixels > (1ll << 40)) return gft_fail("gft_present_ranges: bad size pixels=%lld", (long long)pixels);
    if (!gt_tof || !ranges) return gft_fail("gft_present_ranges: gt_tof or ranges is NULL");
    if (bad_stride(stride)) return gft_fail("gft_present_ranges: bad plane stride");
    if (!partials || ((uintptr_t)partials & 3u)) return gft_fail("gft_present_ranges: partials is NULL or not 4-byte aligned");
    const int blocks = (int)prs_blocks(pixels);
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(k_present_ranges_part, dim3(blocks), dim3(PRS_THREADS), 0, s, pixels, gt_tof, stride, static_cast<float*>(partials));
    hipLaunchKernelGGL(k_present_ranges_finish, dim3(1), dim3(PRS_THREADS), 0, s, blocks, static_cast<const float*>(partials), ranges);
    return gft_launched("gft_present_ranges");
}

extern "C" int gft_present_ranges_reset(void* hip_stream, float* ranges)
{
    if (!ranges) return gft_fail("gft_present_ranges_reset: ranges is NULL");
    hipLaunchKernelGGL(k_present_ranges_reset, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, ranges);
    return gft_launched("gft_present_ranges_reset");
}

extern "C" const uint8_t* gft_present_seismic(void)
{
    return reinterpret_cast<const uint8_t*>(h_seismic);
}

extern "C" int gft_present_quad(void* hip_stream, int32_t H, int32_t W, const float* phasor, int64_t phasor_stride,
                                const int32_t* permutation, int32_t has_gt, int32_t tonemap, void* out)
{
    if (H < 1 || W < 1 || (int64_t)H * W > (1ll << 40)) return gft_fail("gft_present_quad: bad size H=%d W=%d", H, W);
    if (!phasor || !permutation || !out) return gft_fail("gft_present_quad: NULL argument");
    if (bad_stride(phasor_stride)) return gft_fail("gft_present_quad: bad plane stride");
    QuadArgs p = {};
    p.pixels = (int64_t)H * W;
    p.phasor = phasor;
    p.stride = phasor_stride;
    for (int k = 0; k < 4; k++) {
        if (permutation[k] < 0 || permutation[k] > 3) return gft_fail("gft_present_quad: permutation[%d]=%d is not in 0..3", k, permutation[k]);
        p.plane[k] = 3 + permutation[k];
    }
    p.has_gt = has_gt != 0;
    p.tonemap = tonemap != 0;
    p.out = static_cast<uint8_t*>(out);
    hipLaunchKernelGGL(k_present_quad, dim3((unsigned)prs_blocks(p.pixels)), dim3(PRS_THREADS), 0, (hipStream_t)hip_stream, p);
    return gft_launched("gft_present_quad");
}
