// k_debugviz.hip -- the debug images of the training loop's pipe.debug block (include/gftorf_debugviz.h; train.py:295-378).
// One pass over up to 20 float planes that writes the uint8 images the reference forms in numpy, 43 bytes per pixel, into
// one sheet.
// k_debugviz_minmax: (min, max) partials of the planes that are normalised by their own range -- |gt_amp - amp|,
// |gt_phase_depth - depth|, |gt_phase_depth - phase_depth|, dd and the planes of |quad - gt_quad| whose permutation entry is
// quad_index -- one row of 16 words per workgroup; every word of a row is written, so nothing needs clearing.
// k_debugviz_images: every workgroup folds those rows (at most 512, two per thread, in row order; then the butterfly and the
// waves in wave order), then walks runs of 1024 pixels, four per lane.  A lane reads four floats of every plane with one
// 16-byte load where the plane's address allows, forms its pixels once, stores the 4-byte colour-map pixels as one 16-byte
// word and stages the 1-byte and 3-byte pixels in LDS at the destination's offset within a 16-byte word (gft_byte_runs.h);
// the runs leave as 16-byte words, with byte stores only for a ragged head or tail (the quad planes of a frame whose pixel
// count is no multiple of 16, the last run).  The 1-byte runs are dealt to the four waves, one wave per run.
// No atomics, no memset, the inputs are only read, each once per launch.
//
// The arithmetic is numpy's float32 sequence operation for operation: nothing here may contract into a multiply-add, and
// every division is the correctly rounded one.  min and max propagate a NaN as np.min / np.max.
#include "gft_internal.h"
#include "gft_reduce.h"
#include "gft_byte_runs.h"
#include "gft_present_magma.h"
#include "gft_present_ops.h"
#include "gftorf_debugviz.h"

#pragma clang fp contract(off)

namespace {

constexpr int DBV_THREADS = 256, DBV_WAVES = DBV_THREADS / 64, DBV_MAX_BLOCKS = 512, DBV_RUN = GFT_DEBUGVIZ_RUN;
constexpr int DBV_IMAGES = GFT_DEBUGVIZ_IMAGES, DBV_WORDS = GFT_DEBUGVIZ_PARTIAL_WORDS, DBV_RANGES = GFT_DEBUGVIZ_RANGE_WORDS;
constexpr int DBV_RUN_PIXELS = DBV_THREADS * DBV_RUN;
constexpr int DBV_RUN1 = (DBV_RUN_PIXELS + 15 + 15) / 16;          // 16-byte words of a staged run of 1-byte pixels, any offset in a word
constexpr int DBV_RUN3 = (DBV_RUN_PIXELS * 3 + 15 + 15) / 16;
constexpr int DBV_PLANES1 = 10, DBV_SLOTS1 = DBV_PLANES1 + 12;    // the 1-byte images, then the planes of quad, quad_gt, quad_error
constexpr int DBV_BPP[DBV_IMAGES] = {4, 1, 1, 1, 1, 1, 1, 1, 1, 4, 4, 1, 3, 3, 3, 1, 4, 4, 4};
// the pairs of a row of partials: word 2 * pair is the min, 2 * pair + 1 the max
constexpr int PAIR_AMP = 0, PAIR_DEPTH = 1, PAIR_PHASE = 2, PAIR_DD = 3, PAIR_QUAD = 4;

static_assert(DBV_RUN == 4, "a lane packs four 1-byte pixels into a dword and four 4-byte pixels into a 16-byte word");
static_assert(DBV_WORDS == 2 * (PAIR_QUAD + 4) && DBV_WORDS <= 64, "a row holds eight pairs; one thread per word finishes the fold");
static_assert(DBV_MAX_BLOCKS % DBV_THREADS == 0, "the fold reads DBV_MAX_BLOCKS / DBV_THREADS rows per thread");
static_assert(GFT_DEBUGVIZ_ALIGN == 16 && GFT_MAGMA_ROWS == 257, "header");

__device__ const uint32_t d_debug_magma[GFT_MAGMA_ROWS] = {GFT_MAGMA_TABLE};

struct DebugvizArgs {
    int64_t pixels;
    int blocks;
    const float* amp;                           // plane 2 of phasor, or NULL
    const float* gt_amp;                        // plane 2 of gt_phasor
    const float* depth;
    const float* pd;
    const float* gpd;
    const float* dd;
    const float* image;                         // 3 planes image_stride apart
    const float* gt_image;
    const float* quad;                          // planes 3..6 of phasor, quad_stride apart
    const float* gt_quad;                       // 4 planes gt_quad_stride apart
    int64_t image_stride, gt_image_stride, quad_stride, gt_quad_stride;
    int perm[4];
    const int32_t* quad_index_dev;
    int quad_index;
    const float* ranges_dev;
    float ranges[DBV_RANGES];
    float znear, zfar, mult;
    float* partials;                            // [blocks][16], or NULL when no pair is wanted
    uint8_t* out[DBV_IMAGES];                   // NULL for an image the groups do not produce
};

int64_t dbv_blocks(int64_t pixels) { return gft_grid_blocks(pixels, DBV_THREADS, DBV_RUN, DBV_MAX_BLOCKS); }

// pixels i .. i + m - 1 of a plane (m <= 4, i a multiple of 4): one 16-byte load where the address allows; the rest are 0
__device__ __forceinline__ void load4(const float* plane, int64_t i, int m, float (&v)[DBV_RUN])
{
    if (m == DBV_RUN && ((uintptr_t)(plane + i) & 15u) == 0) {
        const float4 t = *reinterpret_cast<const float4*>(plane + i);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < DBV_RUN; j++) v[j] = j < m ? plane[i + j] : 0.f;
    }
}

// the pixels of this lane in a walk of four per lane: how many of the four from i on exist
__device__ __forceinline__ int lane_pixels(int64_t pixels, int64_t i)
{
    const int64_t mine = pixels - i;
    return mine >= DBV_RUN ? DBV_RUN : (mine > 0 ? (int)mine : 0);
}

// the fold both launches end with: v[0 .. 16) are (min, max) pairs; afterwards thread k < 16 returns word k of the
// workgroup (the butterfly, then the waves in wave order), the other threads nothing of use.  One barrier.
__device__ __forceinline__ float fold_pairs(float (&v)[DBV_WORDS], float (*sRed)[DBV_WAVES])
{
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < DBV_WORDS; k++) {
            const float w = gft_shfl_xor(v[k], o);
            v[k] = (k & 1) ? nmax(v[k], w) : nmin(v[k], w);
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < DBV_WORDS; k++) sRed[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    float t = 0.f;
    if (threadIdx.x < DBV_WORDS) {
        const int k = threadIdx.x;
        t = sRed[k][0];
        for (int w = 1; w < DBV_WAVES; w++) t = (k & 1) ? nmax(t, sRed[k][w]) : nmin(t, sRed[k][w]);
    }
    return t;
}

__device__ __forceinline__ void fold_in(float (&v)[DBV_WORDS], int pair, float x)
{
    v[2 * pair] = nmin(v[2 * pair], x);
    v[2 * pair + 1] = nmax(v[2 * pair + 1], x);
}

__global__ __launch_bounds__(DBV_THREADS) void k_debugviz_minmax(DebugvizArgs p)
{
    __shared__ float sRed[DBV_WORDS][DBV_WAVES];
    float v[DBV_WORDS];
#pragma unroll
    for (int k = 0; k < DBV_WORDS; k++) v[k] = (k & 1) ? -INFINITY : INFINITY;
    const bool amp_on = p.out[GFT_DEBUGVIZ_AMP_ERROR] != nullptr, depth_on = p.out[GFT_DEBUGVIZ_DEPTH_ERROR] != nullptr;
    const bool phase_on = p.out[GFT_DEBUGVIZ_PHASE_DEPTH_ERROR] != nullptr, dd_on = p.out[GFT_DEBUGVIZ_DD] != nullptr;
    const int qi = p.quad_index_dev ? *p.quad_index_dev : p.quad_index;
    bool quad_on[4];
#pragma unroll
    for (int k = 0; k < 4; k++) quad_on[k] = p.out[GFT_DEBUGVIZ_QUAD_ERROR] != nullptr && p.perm[k] == qi;
    const int64_t step = (int64_t)gridDim.x * DBV_RUN_PIXELS;
    for (int64_t i = ((int64_t)blockIdx.x * DBV_THREADS + threadIdx.x) * DBV_RUN; i < p.pixels; i += step) {
        const int m = lane_pixels(p.pixels, i);
        float a[DBV_RUN], b[DBV_RUN], g[DBV_RUN];
        if (amp_on) {
            load4(p.amp, i, m, a);
            load4(p.gt_amp, i, m, b);
#pragma unroll
            for (int j = 0; j < DBV_RUN; j++)
                if (j < m) fold_in(v, PAIR_AMP, fabsf(b[j] - a[j] * p.mult));
        }
        if (depth_on || phase_on) load4(p.gpd, i, m, g);
        if (depth_on) {
            load4(p.depth, i, m, a);
#pragma unroll
            for (int j = 0; j < DBV_RUN; j++)
                if (j < m) fold_in(v, PAIR_DEPTH, fabsf(g[j] - a[j]));
        }
        if (phase_on) {
            load4(p.pd, i, m, a);
#pragma unroll
            for (int j = 0; j < DBV_RUN; j++)
                if (j < m) fold_in(v, PAIR_PHASE, fabsf(g[j] - a[j]));
        }
        if (dd_on) {
            load4(p.dd, i, m, a);
#pragma unroll
            for (int j = 0; j < DBV_RUN; j++)
                if (j < m) fold_in(v, PAIR_DD, a[j]);
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (quad_on[k]) {
                load4(p.quad + k * p.quad_stride, i, m, a);
                load4(p.gt_quad + p.perm[k] * p.gt_quad_stride, i, m, b);
#pragma unroll
                for (int j = 0; j < DBV_RUN; j++)
                    if (j < m) fold_in(v, PAIR_QUAD + k, fabsf(a[j] - b[j]));
            }
        }
    }
    const float t = fold_pairs(v, sRed);
    if (threadIdx.x < DBV_WORDS) p.partials[(size_t)blockIdx.x * DBV_WORDS + threadIdx.x] = t;
}

// four 1-byte pixels of a lane into the staged run of an image whose run begins at `dst`
__device__ __forceinline__ void stage1(uint4* run, const uint8_t* dst, int tid, int m, const uint32_t (&px)[DBV_RUN])
{
    const int mis = (int)((uintptr_t)dst & 15u);
    uint8_t* s = reinterpret_cast<uint8_t*>(run) + mis + DBV_RUN * tid;
    if (m == DBV_RUN && (mis & 3) == 0) {
        *reinterpret_cast<uint32_t*>(s) = px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24;
    } else {
#pragma unroll
        for (int j = 0; j < DBV_RUN; j++)
            if (j < m) s[j] = (uint8_t)px[j];
    }
}

// four RGB pixels (0x00BBGGRR) of a lane into the staged run of an [H, W, 3] image whose run begins at `dst`
__device__ __forceinline__ void stage3(uint4* run, const uint8_t* dst, int tid, int m, const uint32_t (&px)[DBV_RUN])
{
    const int mis = (int)((uintptr_t)dst & 15u);
    const uint32_t w[3] = {px[0] | px[1] << 24, px[1] >> 8 | px[2] << 16, px[2] >> 16 | px[3] << 8};
    uint8_t* s = reinterpret_cast<uint8_t*>(run) + mis + 3 * DBV_RUN * tid;
    if (m == DBV_RUN && (mis & 3) == 0) {
#pragma unroll
        for (int d = 0; d < 3; d++) reinterpret_cast<uint32_t*>(s)[d] = w[d];
    } else {
#pragma unroll
        for (int b = 0; b < 3 * DBV_RUN; b++)
            if (b < 3 * m) s[b] = (uint8_t)(w[b >> 2] >> (8 * (b & 3)));
    }
}

// four colour-map pixels of a lane: the image starts on a 16-byte boundary and i is a multiple of 4
__device__ __forceinline__ void store4(uint8_t* image, int64_t i, int m, const uint32_t (&px)[DBV_RUN])
{
    uint32_t* dst = reinterpret_cast<uint32_t*>(image) + i;
    if (m == DBV_RUN) {
        *reinterpret_cast<uint4*>(dst) = make_uint4(px[0], px[1], px[2], px[3]);
    } else {
#pragma unroll
        for (int j = 0; j < DBV_RUN; j++)
            if (j < m) dst[j] = px[j];
    }
}

// where the run of 1-byte slot `slot` begins in the sheet: the ten 1-byte images, then the planes of quad, quad_gt, quad_error
__device__ __forceinline__ uint8_t* slot_run(const DebugvizArgs& p, int slot, int64_t i0)
{
    constexpr int image[DBV_PLANES1] = {GFT_DEBUGVIZ_AMP, GFT_DEBUGVIZ_AMP_ERROR, GFT_DEBUGVIZ_SP, GFT_DEBUGVIZ_SP_ERROR,
                                        GFT_DEBUGVIZ_SP_TOF, GFT_DEBUGVIZ_SP_TOF_ERROR, GFT_DEBUGVIZ_SP_GT, GFT_DEBUGVIZ_DEPTH_ERROR,
                                        GFT_DEBUGVIZ_PHASE_DEPTH_ERROR, GFT_DEBUGVIZ_DD};
    if (slot < DBV_PLANES1) {
        uint8_t* o = p.out[image[slot]];
        return o ? o + i0 : nullptr;
    }
    const int q = slot - DBV_PLANES1;
    uint8_t* o = p.out[GFT_DEBUGVIZ_QUAD + q / 4];
    return o ? o + (q % 4) * p.pixels + i0 : nullptr;
}

enum { S_AMP, S_AMP_ERROR, S_SP, S_SP_ERROR, S_SP_TOF, S_SP_TOF_ERROR, S_SP_GT, S_DEPTH_ERROR, S_PHASE_ERROR, S_DD, S_QUAD,
       S_QUAD_GT = S_QUAD + 4, S_QUAD_ERROR = S_QUAD_GT + 4 };
static_assert(S_QUAD == DBV_PLANES1 && S_QUAD_ERROR + 4 == DBV_SLOTS1, "slot_run's order");

__global__ __launch_bounds__(DBV_THREADS) void k_debugviz_images(DebugvizArgs p)
{
    __shared__ uint4 sRun1[DBV_SLOTS1][DBV_RUN1];
    __shared__ uint4 sRun3[3][DBV_RUN3];              // color, color_gt, color_error
    __shared__ uint32_t sMagma[GFT_MAGMA_ROWS];
    __shared__ float sRed[DBV_WORDS][DBV_WAVES];
    __shared__ float sFold[DBV_WORDS];
    const int tid = threadIdx.x;
    for (int k = tid; k < GFT_MAGMA_ROWS; k += DBV_THREADS) sMagma[k] = d_debug_magma[k];
    if (p.partials) {
        float v[DBV_WORDS];
#pragma unroll
        for (int k = 0; k < DBV_WORDS; k++) v[k] = (k & 1) ? -INFINITY : INFINITY;
        for (int b = tid; b < p.blocks; b += DBV_THREADS) {
            const float4* row = reinterpret_cast<const float4*>(p.partials + (size_t)b * DBV_WORDS);
#pragma unroll
            for (int q = 0; q < DBV_WORDS / 4; q++) {
                const float4 t = row[q];
                v[4 * q] = nmin(v[4 * q], t.x);
                v[4 * q + 1] = nmax(v[4 * q + 1], t.y);
                v[4 * q + 2] = nmin(v[4 * q + 2], t.z);
                v[4 * q + 3] = nmax(v[4 * q + 3], t.w);
            }
        }
        const float t = fold_pairs(v, sRed);
        if (tid < DBV_WORDS) sFold[tid] = t;
    }
    __syncthreads();                                                  // sMagma and sFold
    float lo[DBV_WORDS / 2] = {}, span[DBV_WORDS / 2] = {};
    if (p.partials) {
#pragma unroll
        for (int k = 0; k < DBV_WORDS / 2; k++) {
            lo[k] = sFold[2 * k];
            span[k] = sFold[2 * k + 1] - lo[k];
        }
    }
    float rg[DBV_RANGES];
#pragma unroll
    for (int k = 0; k < DBV_RANGES; k++) rg[k] = p.ranges_dev ? p.ranges_dev[k] : p.ranges[k];
    const float zspan = p.zfar - p.znear;
    const int qi = p.quad_index_dev ? *p.quad_index_dev : p.quad_index;
    const bool has_amp = p.amp != nullptr, has_gt_amp = p.gt_amp != nullptr, has_depth = p.depth != nullptr, has_pd = p.pd != nullptr;
    const bool has_gpd = p.gpd != nullptr, has_quad = p.out[GFT_DEBUGVIZ_QUAD] != nullptr, has_gt_quad = p.out[GFT_DEBUGVIZ_QUAD_GT] != nullptr;
    const int wave = tid >> 6, lane = tid & 63;

    const int64_t runs = (p.pixels + DBV_RUN_PIXELS - 1) / DBV_RUN_PIXELS;
    for (int64_t run = blockIdx.x; run < runs; run += gridDim.x) {
        const int64_t i0 = run * DBV_RUN_PIXELS, i = i0 + (int64_t)DBV_RUN * tid;
        const int64_t left = p.pixels - i0;
        const int n = left < DBV_RUN_PIXELS ? (int)left : DBV_RUN_PIXELS;        // pixels of this run
        const int m = lane_pixels(p.pixels, i);                                 // pixels of this lane
        uint32_t px[DBV_RUN];
        if (m > 0) {
            // ---- the ToF block, train.py:295-338 (and :194-200 for the scattering phases)
            float amp[DBV_RUN] = {}, gamp[DBV_RUN] = {}, d[DBV_RUN] = {}, pd[DBV_RUN] = {}, gpd[DBV_RUN] = {};
            float sp[DBV_RUN] = {}, spt[DBV_RUN] = {}, gsp[DBV_RUN] = {};
            if (has_amp) {
                load4(p.amp, i, m, amp);
#pragma unroll
                for (int j = 0; j < DBV_RUN; j++) {
                    amp[j] = amp[j] * p.mult;
                    px[j] = to8b(norm01(amp[j], rg[0], rg[1] - rg[0]));
                }
                stage1(sRun1[S_AMP], slot_run(p, S_AMP, i0), tid, m, px);
            }
            if (has_gt_amp) load4(p.gt_amp, i, m, gamp);
            if (has_depth) {
                load4(p.depth, i, m, d);
#pragma unroll
                for (int j = 0; j < DBV_RUN; j++) px[j] = magma(sMagma, d[j], p.znear, zspan);
                store4(p.out[GFT_DEBUGVIZ_DEPTH], i, m, px);
            }
            if (has_pd) {
                load4(p.pd, i, m, pd);
#pragma unroll
                for (int j = 0; j < DBV_RUN; j++) px[j] = magma(sMagma, pd[j], p.znear, zspan);
                store4(p.out[GFT_DEBUGVIZ_PHASE_DEPTH], i, m, px);
            }
            if (has_gpd) {
                load4(p.gpd, i, m, gpd);
#pragma unroll
                for (int j = 0; j < DBV_RUN; j++) px[j] = magma(sMagma, gpd[j], p.znear, zspan);
                store4(p.out[GFT_DEBUGVIZ_PHASE_DEPTH_GT], i, m, px);
            }
            if (has_amp && has_gt_amp) {
#pragma unroll
                for (int j = 0; j < DBV_RUN; j++) px[j] = to8b(norm01(fabsf(gamp[j] - amp[j]), lo[PAIR_AMP], span[PAIR_AMP]));
                stage1(sRun1[S_AMP_ERROR], slot_run(p, S_AMP_ERROR, i0), tid, m, px);
            }
            if (has_gt_amp && has_gpd) {
#pragma unroll
                for (int j = 0; j < DBV_RUN; j++) {
                    gsp[j] = gamp[j] * (gpd[j] * gpd[j]);
                    px[j] = to8b(norm01(gsp[j], rg[6], rg[7] - rg[6]));
                }
                stage1(sRun1[S_SP_GT], slot_run(p, S_SP_GT, i0), tid, m, px);
            }
            if (has_amp && has_depth) {
#pragma unroll
                for (int j = 0; j < DBV_RUN; j++) {
                    sp[j] = amp[j] * (d[j] * d[j]);
                    px[j] = to8b(norm01(sp[j], rg[2], rg[3] - rg[2]));
                }
                stage1(sRun1[S_SP], slot_run(p, S_SP, i0), tid, m, px);
                if (has_gt_amp && has_gpd) {
#pragma unroll
                    for (int j = 0; j < DBV_RUN; j++) px[j] = to8b(fabsf(gsp[j] - sp[j]));
                    stage1(sRun1[S_SP_ERROR], slot_run(p, S_SP_ERROR, i0), tid, m, px);
                }
            }
            if (has_amp && has_pd) {
#pragma unroll
                for (int j = 0; j < DBV_RUN; j++) {
                    spt[j] = amp[j] * (pd[j] * pd[j]);
                    px[j] = to8b(norm01(spt[j], rg[4], rg[5] - rg[4]));
                }
                stage1(sRun1[S_SP_TOF], slot_run(p, S_SP_TOF, i0), tid, m, px);
                if (has_gt_amp && has_gpd) {
#pragma unroll
                    for (int j = 0; j < DBV_RUN; j++) px[j] = to8b(fabsf(gsp[j] - spt[j]));
                    stage1(sRun1[S_SP_TOF_ERROR], slot_run(p, S_SP_TOF_ERROR, i0), tid, m, px);
                }
            }
            if (has_gpd && has_depth) {
#pragma unroll
                for (int j = 0; j < DBV_RUN; j++) px[j] = to8b(norm01(fabsf(gpd[j] - d[j]), lo[PAIR_DEPTH], span[PAIR_DEPTH]));
                stage1(sRun1[S_DEPTH_ERROR], slot_run(p, S_DEPTH_ERROR, i0), tid, m, px);
            }
            if (has_gpd && has_pd) {
#pragma unroll
                for (int j = 0; j < DBV_RUN; j++) px[j] = to8b(norm01(fabsf(gpd[j] - pd[j]), lo[PAIR_PHASE], span[PAIR_PHASE]));
                stage1(sRun1[S_PHASE_ERROR], slot_run(p, S_PHASE_ERROR, i0), tid, m, px);
            }
            // ---- the colour images, :358-364
            if (p.image) {
                uint32_t cpx[3][DBV_RUN] = {};
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    float im[DBV_RUN], gt[DBV_RUN];
                    load4(p.image + c * p.image_stride, i, m, im);
                    load4(p.gt_image + c * p.gt_image_stride, i, m, gt);
#pragma unroll
                    for (int j = 0; j < DBV_RUN; j++) {
                        cpx[0][j] |= to8b(im[j]) << (8 * c);
                        cpx[1][j] |= to8b(gt[j]) << (8 * c);
                        cpx[2][j] |= to8b(fabsf(gt[j] - im[j])) << (8 * c);
                    }
                }
#pragma unroll
                for (int k = 0; k < 3; k++) stage3(sRun3[k], p.out[GFT_DEBUGVIZ_COLOR + k] + 3 * i0, tid, m, cpx[k]);
            }
            // ---- the depth distortion, :366-367
            if (p.dd) {
                float v[DBV_RUN];
                load4(p.dd, i, m, v);
#pragma unroll
                for (int j = 0; j < DBV_RUN; j++) px[j] = to8b(norm01(v[j], lo[PAIR_DD], span[PAIR_DD]));
                stage1(sRun1[S_DD], slot_run(p, S_DD, i0), tid, m, px);
            }
            // ---- the quad images, :369-378
            if (has_quad) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    float q[DBV_RUN], g[DBV_RUN];
                    load4(p.quad + k * p.quad_stride, i, m, q);
#pragma unroll
                    for (int j = 0; j < DBV_RUN; j++) px[j] = to8b(fabsf(q[j]));
                    stage1(sRun1[S_QUAD + k], slot_run(p, S_QUAD + k, i0), tid, m, px);
                    if (has_gt_quad) {
                        load4(p.gt_quad + p.perm[k] * p.gt_quad_stride, i, m, g);
#pragma unroll
                        for (int j = 0; j < DBV_RUN; j++) px[j] = to8b(fabsf(g[j]));
                        stage1(sRun1[S_QUAD_GT + k], slot_run(p, S_QUAD_GT + k, i0), tid, m, px);
                        const bool shown = p.perm[k] == qi;
#pragma unroll
                        for (int j = 0; j < DBV_RUN; j++)
                            px[j] = shown ? to8b(norm01(fabsf(q[j] - g[j]), lo[PAIR_QUAD + k], span[PAIR_QUAD + k])) : 0u;
                        stage1(sRun1[S_QUAD_ERROR + k], slot_run(p, S_QUAD_ERROR + k, i0), tid, m, px);
                    }
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < DBV_SLOTS1; s++) {
            if ((s & (DBV_WAVES - 1)) == wave) {
                uint8_t* dst = slot_run(p, s, i0);
                if (dst) gft_put_run16<64>(dst, n, sRun1[s], lane);
            }
        }
        if (p.image) {
#pragma unroll
            for (int k = 0; k < 3; k++) gft_put_run16<DBV_THREADS>(p.out[GFT_DEBUGVIZ_COLOR + k] + 3 * i0, 3 * n, sRun3[k], tid);
        }
        __syncthreads();
    }
}

// the inputs each image needs; offsets of the images the groups produce, -1 for the others; the sheet's bytes, or 0
int64_t dbv_layout(int64_t pixels, int groups, int64_t* offsets)
{
    constexpr int P = GFT_DEBUGVIZ_HAS_PHASOR, GP = GFT_DEBUGVIZ_HAS_GT_PHASOR, D = GFT_DEBUGVIZ_HAS_DEPTH, PD = GFT_DEBUGVIZ_HAS_PHASE_DEPTH;
    constexpr int GPD = GFT_DEBUGVIZ_HAS_GT_PHASE_DEPTH, DD = GFT_DEBUGVIZ_HAS_DD, C = GFT_DEBUGVIZ_HAS_COLOR, Q = GFT_DEBUGVIZ_HAS_QUAD;
    constexpr int GQ = GFT_DEBUGVIZ_HAS_GT_QUAD, all = P | GP | D | PD | GPD | DD | C | Q | GQ;
    if (pixels < 1 || pixels > (1ll << 40) || groups <= 0 || (groups & ~all)) return 0;
    if ((groups & Q) && !(groups & P)) return 0;
    if ((groups & GQ) && !(groups & Q)) return 0;
    const int needs[DBV_IMAGES] = {D, P, P | GP, P | D, P | D | GP | GPD, P | PD, P | PD | GP | GPD, GP | GPD, GPD | D, PD, GPD, GPD | PD,
                                   C, C, C, DD, Q, GQ, GQ};
    int64_t pos = 0;
    for (int k = 0; k < DBV_IMAGES; k++) {
        const bool on = (groups & needs[k]) == needs[k];
        if (offsets) offsets[k] = on ? pos : -1;
        if (on) pos += (DBV_BPP[k] * pixels + GFT_DEBUGVIZ_ALIGN - 1) / GFT_DEBUGVIZ_ALIGN * GFT_DEBUGVIZ_ALIGN;
    }
    return pos;
}

bool bad_stride(int64_t s) { return s < 0 || s > (1ll << 40); }

}  // namespace

extern "C" int64_t gft_debugviz_blocks(int64_t pixels)
{
    if (pixels < 1) return 0;
    return dbv_blocks(pixels);
}

extern "C" int64_t gft_debugviz_sheet_bytes(int32_t H, int32_t W, int32_t groups, int64_t* offsets_out)
{
    if (H < 1 || W < 1) return 0;
    return dbv_layout((int64_t)H * W, groups, offsets_out);
}

extern "C" int gft_debugviz_images(void* hip_stream, int32_t H, int32_t W, const float* phasor, int64_t phasor_stride, int32_t phasor_planes,
                                   const float* gt_phasor, int64_t gt_phasor_stride, const float* depth, const float* phase_depth,
                                   const float* gt_phase_depth, const float* dd, const float* image, int64_t image_stride,
                                   const float* gt_image, int64_t gt_image_stride, const float* gt_quad, int64_t gt_quad_stride,
                                   const int32_t* permutation, const int32_t* quad_index_dev, int32_t quad_index, const float* ranges_dev,
                                   const float* ranges_host, float znear, float zfar, float tof_multiplier, void* partials, void* sheet)
{
    if (H < 1 || W < 1 || (int64_t)H * W > (1ll << 40)) return gft_fail("gft_debugviz_images: bad size H=%d W=%d", H, W);
    if (phasor ? phasor_planes < 3 : phasor_planes != 0)
        return gft_fail("gft_debugviz_images: phasor_planes=%d: a phasor has at least 3 planes, and 0 are given without one", phasor_planes);
    if ((image != nullptr) != (gt_image != nullptr)) return gft_fail("gft_debugviz_images: image and gt_image are given together");
    if (gt_quad && phasor_planes != 7) return gft_fail("gft_debugviz_images: gt_quad needs a phasor of exactly 7 planes, got %d", phasor_planes);
    if (bad_stride(phasor_stride) || bad_stride(gt_phasor_stride) || bad_stride(image_stride) || bad_stride(gt_image_stride) ||
        bad_stride(gt_quad_stride))
        return gft_fail("gft_debugviz_images: bad plane stride");
    if (!sheet || ((uintptr_t)sheet & (GFT_DEBUGVIZ_ALIGN - 1))) return gft_fail("gft_debugviz_images: sheet is NULL or not 16-byte aligned");
    const int groups = (phasor ? GFT_DEBUGVIZ_HAS_PHASOR : 0) | (gt_phasor ? GFT_DEBUGVIZ_HAS_GT_PHASOR : 0) | (depth ? GFT_DEBUGVIZ_HAS_DEPTH : 0) |
                       (phase_depth ? GFT_DEBUGVIZ_HAS_PHASE_DEPTH : 0) | (gt_phase_depth ? GFT_DEBUGVIZ_HAS_GT_PHASE_DEPTH : 0) |
                       (dd ? GFT_DEBUGVIZ_HAS_DD : 0) | (image ? GFT_DEBUGVIZ_HAS_COLOR : 0) | (phasor_planes == 7 ? GFT_DEBUGVIZ_HAS_QUAD : 0) |
                       (gt_quad ? GFT_DEBUGVIZ_HAS_GT_QUAD : 0);
    DebugvizArgs p = {};
    p.pixels = (int64_t)H * W;
    int64_t offsets[DBV_IMAGES];
    if (dbv_layout(p.pixels, groups, offsets) < 1) return gft_fail("gft_debugviz_images: the inputs given (groups %d) produce no image", groups);
    for (int k = 0; k < DBV_IMAGES; k++) p.out[k] = offsets[k] < 0 ? nullptr : static_cast<uint8_t*>(sheet) + offsets[k];
    const bool ranged = p.out[GFT_DEBUGVIZ_AMP] || p.out[GFT_DEBUGVIZ_SP_GT];          // every scattering phase needs one of the two
    if (ranged && !ranges_dev && !ranges_host) return gft_fail("gft_debugviz_images: amp and the scattering phases need ranges");
    const bool folded = p.out[GFT_DEBUGVIZ_AMP_ERROR] || p.out[GFT_DEBUGVIZ_DEPTH_ERROR] || p.out[GFT_DEBUGVIZ_PHASE_DEPTH_ERROR] ||
                        p.out[GFT_DEBUGVIZ_DD] || p.out[GFT_DEBUGVIZ_QUAD_ERROR];
    if (folded && (!partials || ((uintptr_t)partials & 15u)))
        return gft_fail("gft_debugviz_images: the self-normalised images need partials, NULL or not 16-byte aligned");
    if (gt_quad) {
        if (!permutation) return gft_fail("gft_debugviz_images: gt_quad needs a permutation");
        for (int k = 0; k < 4; k++) {
            if (permutation[k] < 0 || permutation[k] > 3)
                return gft_fail("gft_debugviz_images: permutation[%d]=%d is not in 0..3", k, permutation[k]);
            p.perm[k] = permutation[k];
        }
    }
    p.blocks = (int)dbv_blocks(p.pixels);
    p.amp = phasor ? phasor + 2 * phasor_stride : nullptr;
    p.gt_amp = gt_phasor ? gt_phasor + 2 * gt_phasor_stride : nullptr;
    p.depth = depth; p.pd = phase_depth; p.gpd = gt_phase_depth; p.dd = dd;
    p.image = image; p.gt_image = gt_image;
    p.quad = phasor_planes == 7 ? phasor + 3 * phasor_stride : nullptr;
    p.gt_quad = gt_quad;
    p.image_stride = image_stride; p.gt_image_stride = gt_image_stride; p.quad_stride = phasor_stride; p.gt_quad_stride = gt_quad_stride;
    p.quad_index_dev = gt_quad ? quad_index_dev : nullptr;
    p.quad_index = quad_index;
    p.ranges_dev = ranged ? ranges_dev : nullptr;
    if (ranged && !ranges_dev)
        for (int k = 0; k < DBV_RANGES; k++) p.ranges[k] = ranges_host[k];
    p.znear = znear; p.zfar = zfar; p.mult = tof_multiplier;
    p.partials = folded ? static_cast<float*>(partials) : nullptr;
    hipStream_t s = (hipStream_t)hip_stream;
    if (folded) hipLaunchKernelGGL(k_debugviz_minmax, dim3(p.blocks), dim3(DBV_THREADS), 0, s, p);
    hipLaunchKernelGGL(k_debugviz_images, dim3(p.blocks), dim3(DBV_THREADS), 0, s, p);
    return gft_launched("gft_debugviz_images");
}
