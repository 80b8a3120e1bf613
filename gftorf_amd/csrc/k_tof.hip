// k_tof.hip -- the ToF depth of scene/torf_utils.py:59-64 and the scalars of the training log (include/gftorf_tof.h;
// train.py:188-200, 402-433).  k_tof_depth: one pixel per thread, grid-stride.  k_tof_log_sums: one grid-stride loop over
// the concatenation of the pixels and the Gaussians' amplitude coefficients, summed in the two stages and the order of
// gft_reduce.h; k_tof_log_finish writes the log's row (into a ring when there is a cursor) and advances the cursor.  Scalar
// loads only (a pixel's nine loads are each coalesced across the wave; the pass moves 36 bytes per pixel, and per Gaussian
// one float amp_stride floats from the last one's plus its visibility).
#include "gft_internal.h"
#include "gft_reduce.h"
#include "gft_tof_depth.h"
#include "gftorf_tof.h"

namespace {

constexpr int TOF_THREADS = 256, TOF_MAX_BLOCKS = 1024, TOF_SUMS = 11;
constexpr float TOF_SH_C0 = 0.28209479177387814f;              // utils/sh_utils.py C0

static_assert(GFT_TOF_PARTIAL_WORDS == TOF_SUMS + 1, "eleven sums and the visible count");
static_assert(GFT_TOF_LOG_EXTRAS + GFT_TOF_LOG_MAX_EXTRAS == GFT_TOF_LOG_WORDS, "the extras end the row");

struct TofArgs {
    int64_t pixels, P;                          // P = 0 without amplitude coefficients
    const float* __restrict__ phasor;           // planes 0, 1, 2 at phasor_stride
    const float* __restrict__ gt_phasor;
    int64_t phasor_stride, gt_stride;
    const float* __restrict__ depth;
    const float* __restrict__ gt_depth;         // or NULL
    const float* __restrict__ dd;               // or NULL
    const float* __restrict__ amp;              // or NULL; rows amp_stride floats apart
    int64_t amp_stride;
    const void* __restrict__ visible;           // or NULL
    int visible_is_radii;
    const float* __restrict__ depth_range_dev;
    const float* __restrict__ phase_offset_dev;
    float depth_range, phase_offset, tof_multiplier;
    uint32_t* partials;                         // [blocks][GFT_TOF_PARTIAL_WORDS]
    int blocks;
    const float* extras[GFT_TOF_LOG_MAX_EXTRAS];
    int num_extras;
    uint32_t* rows;                             // [slots][GFT_TOF_LOG_WORDS]
    uint32_t slots;
    uint32_t* cursor;                           // or NULL
};

int64_t tof_blocks(int64_t total) { return gft_grid_blocks(total, TOF_THREADS, 1, TOF_MAX_BLOCKS); }

__global__ __launch_bounds__(TOF_THREADS) void k_tof_depth(int64_t pixels, const float* __restrict__ tof, int64_t plane_stride,
                                                           const float* __restrict__ depth_range_dev, float depth_range,
                                                           const float* __restrict__ phase_offset_dev, float phase_offset,
                                                           float* __restrict__ out)
{
    const float dr = gft_dev_or(depth_range_dev, depth_range), off = gft_dev_or(phase_offset_dev, phase_offset);
    for (int64_t i = (int64_t)blockIdx.x * TOF_THREADS + threadIdx.x; i < pixels; i += (int64_t)gridDim.x * TOF_THREADS)
        out[i] = depth_from_tof(tof[i], tof[plane_stride + i], dr, off);
}

__global__ __launch_bounds__(TOF_THREADS) void k_tof_log_sums(TofArgs p)
{
    __shared__ float sRed[TOF_SUMS][TOF_THREADS / 64];
    __shared__ uint32_t sCnt[TOF_THREADS / 64];
    float s[TOF_SUMS];
#pragma unroll
    for (int k = 0; k < TOF_SUMS; k++) s[k] = 0.f;
    uint32_t n = 0u;
    const float dr = gft_dev_or(p.depth_range_dev, p.depth_range), off = gft_dev_or(p.phase_offset_dev, p.phase_offset);
    const int64_t total = p.pixels + p.P;
    for (int64_t i = (int64_t)blockIdx.x * TOF_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * TOF_THREADS) {
        if (i < p.pixels) {
            // train.py:188-200 per pixel: numpy's float32 arithmetic in its order
            const float amp = p.phasor[2 * p.phasor_stride + i] * p.tof_multiplier;
            const float gt_amp = p.gt_phasor[2 * p.gt_stride + i];
            const float pd = depth_from_tof(p.phasor[i], p.phasor[p.phasor_stride + i], dr, off);
            const float gpd = depth_from_tof(p.gt_phasor[i], p.gt_phasor[p.gt_stride + i], dr, off);
            const float d = p.depth[i];
            const float sp = amp * (d * d), sp_tof = amp * (pd * pd), gsp = gt_amp * (gpd * gpd);
            s[GFT_TOF_LOG_SP] += sp;
            s[GFT_TOF_LOG_SP_TOF] += sp_tof;
            s[GFT_TOF_LOG_GSP] += gsp;
            s[GFT_TOF_LOG_SP_ERR] += fabsf(gsp - sp);
            s[GFT_TOF_LOG_SP_TOF_ERR] += fabsf(gsp - sp_tof);
            if (p.gt_depth) s[GFT_TOF_LOG_DEPTH_ERR] += fabsf(d - p.gt_depth[i]);
            s[GFT_TOF_LOG_TOF_DEPTH_ERR] += fabsf(pd - gpd);
            s[GFT_TOF_LOG_AMP_ERR] += fabsf(amp - gt_amp);
            if (p.dd) s[GFT_TOF_LOG_DD] += p.dd[i];
        } else {
            const int64_t r = i - p.pixels;
            const float v = p.amp[r * p.amp_stride] * TOF_SH_C0 + 0.5f;          // sh_utils.py SH2PA
            s[GFT_TOF_LOG_GS_SP] += v;
            if (p.visible && gft_visible_row(p.visible, p.visible_is_radii, r)) {
                s[GFT_TOF_LOG_GS_SP_VISIBLE] += v;
                n++;
            }
        }
    }
    gft_fold_store<TOF_THREADS>(s, sRed);
    gft_fold_store<TOF_THREADS>(n, sCnt);
    __syncthreads();
    if (threadIdx.x < GFT_TOF_PARTIAL_WORDS) {
        const int k = threadIdx.x;
        p.partials[(size_t)blockIdx.x * GFT_TOF_PARTIAL_WORDS + k] =
            k < TOF_SUMS ? __float_as_uint(gft_waves_total<TOF_THREADS>(sRed[k])) : gft_waves_total<TOF_THREADS>(sCnt);
    }
}

// one workgroup: the rows of partials in a fixed order, in double; then the log's row and the cursor
__global__ __launch_bounds__(TOF_THREADS) void k_tof_log_finish(TofArgs p)
{
    __shared__ double sSum[TOF_SUMS][TOF_THREADS];
    __shared__ unsigned long long sCnt[1][TOF_THREADS];
    const int tid = threadIdx.x;
    double s[TOF_SUMS];
#pragma unroll
    for (int k = 0; k < TOF_SUMS; k++) s[k] = 0.0;
    unsigned long long n = 0ull;
    for (int b = tid; b < p.blocks; b += TOF_THREADS) {
        const uint32_t* row = p.partials + (size_t)b * GFT_TOF_PARTIAL_WORDS;
#pragma unroll
        for (int k = 0; k < TOF_SUMS; k++) s[k] += (double)__uint_as_float(row[k]);
        n += row[TOF_SUMS];
    }
#pragma unroll
    for (int k = 0; k < TOF_SUMS; k++) sSum[k][tid] = s[k];
    sCnt[0][tid] = n;
    gft_tree_sum<TOF_THREADS>(sSum, sCnt);
    if (tid != 0) return;
    const unsigned long long n_vis = sCnt[0][0];
    const uint32_t seq = p.cursor ? *p.cursor : 0u;
    uint32_t* out = p.rows + (size_t)(seq % p.slots) * GFT_TOF_LOG_WORDS;
    const double per_pixel = 1.0 / (double)p.pixels;
    for (int k = 0; k <= GFT_TOF_LOG_DD; k++) out[k] = __float_as_uint((float)(sSum[k][0] * per_pixel));
    out[GFT_TOF_LOG_GS_SP] = __float_as_uint(p.P > 0 ? (float)(sSum[GFT_TOF_LOG_GS_SP][0] / (double)p.P) : 0.f);
    out[GFT_TOF_LOG_GS_SP_VISIBLE] = __float_as_uint(n_vis > 0 ? (float)(sSum[GFT_TOF_LOG_GS_SP_VISIBLE][0] / (double)n_vis) : 0.f);
    out[GFT_TOF_LOG_VISIBLE] = (uint32_t)n_vis;
    out[GFT_TOF_LOG_PRESENT] = (p.gt_depth ? GFT_TOF_HAS_GT_DEPTH : 0u) | (p.dd ? GFT_TOF_HAS_DD : 0u) |
                               (p.amp ? GFT_TOF_HAS_AMP : 0u) | (p.visible ? GFT_TOF_HAS_VISIBLE : 0u);
    out[GFT_TOF_LOG_NUM_EXTRAS] = (uint32_t)p.num_extras;
    out[GFT_TOF_LOG_SEQ] = seq;
    out[GFT_TOF_LOG_SEQ + 1] = 0u;
    for (int k = 0; k < GFT_TOF_LOG_MAX_EXTRAS; k++)
        out[GFT_TOF_LOG_EXTRAS + k] = k < p.num_extras ? __float_as_uint(*p.extras[k]) : 0u;
    if (p.cursor) *p.cursor = seq + 1u;
}

}  // namespace

extern "C" int gft_tof_depth(void* hip_stream, int64_t pixels, const float* tof, int64_t plane_stride, const float* depth_range_dev,
                             float depth_range, const float* phase_offset_dev, float phase_offset, float* out)
{
    if (pixels < 0 || pixels > (1ll << 40)) return gft_fail("gft_tof_depth: bad sizes pixels=%lld", (long long)pixels);
    if (pixels == 0) return 0;
    if (!tof || !out) return gft_fail("gft_tof_depth: tof or out is NULL");
    if (plane_stride < 0 || plane_stride > (1ll << 40)) return gft_fail("gft_tof_depth: bad plane_stride=%lld", (long long)plane_stride);
    hipLaunchKernelGGL(k_tof_depth, dim3((unsigned)tof_blocks(pixels)), dim3(TOF_THREADS), 0, (hipStream_t)hip_stream, pixels, tof,
                       plane_stride, depth_range_dev, depth_range, phase_offset_dev, phase_offset, out);
    return gft_launched("gft_tof_depth");
}

extern "C" int64_t gft_tof_log_blocks(int64_t pixels, int64_t P)
{
    if (pixels < 1 || P < 0) return 0;
    return tof_blocks(pixels + P);
}

extern "C" int gft_tof_log_row(void* hip_stream, int64_t pixels, int64_t P, const float* phasor, int64_t phasor_plane_stride,
                               const float* depth, const float* gt_phasor, int64_t gt_plane_stride, const float* depth_range_dev,
                               float depth_range, const float* phase_offset_dev, float phase_offset, float tof_multiplier,
                               const float* gt_depth, const float* depth_distortion, const float* amp, int64_t amp_stride,
                               const void* visible, int32_t visible_is_radii, const float* const* extras, int32_t num_extras,
                               void* partials, void* rows, int64_t slots, void* cursor)
{
    if (pixels < 1 || P < 0 || pixels > (1ll << 40) || P > 0x7fffffffll)
        return gft_fail("gft_tof_log_row: bad sizes pixels=%lld P=%lld", (long long)pixels, (long long)P);
    if (!phasor || !depth || !gt_phasor) return gft_fail("gft_tof_log_row: phasor, depth or gt_phasor is NULL");
    if (phasor_plane_stride < 0 || gt_plane_stride < 0 || phasor_plane_stride > (1ll << 40) || gt_plane_stride > (1ll << 40))
        return gft_fail("gft_tof_log_row: bad plane stride");
    if (visible && !amp) return gft_fail("gft_tof_log_row: visible without the amplitude coefficients");
    if (amp && P > 0 && (amp_stride < 1 || amp_stride > (1ll << 20))) return gft_fail("gft_tof_log_row: bad amp_stride=%lld", (long long)amp_stride);
    if (num_extras < 0 || num_extras > GFT_TOF_LOG_MAX_EXTRAS)
        return gft_fail("gft_tof_log_row: num_extras=%d is not in 0..%d", num_extras, GFT_TOF_LOG_MAX_EXTRAS);
    if (num_extras > 0 && !extras) return gft_fail("gft_tof_log_row: extras is NULL");
    for (int k = 0; k < num_extras; k++)
        if (!extras[k]) return gft_fail("gft_tof_log_row: extras[%d] is NULL", k);
    if (!partials || !rows) return gft_fail("gft_tof_log_row: partials or rows is NULL");
    if (slots < 1 || slots > 0x7fffffffll) return gft_fail("gft_tof_log_row: bad slots=%lld", (long long)slots);
    TofArgs p = {};
    if (!amp || P == 0) { amp = nullptr; visible = nullptr; P = 0; }
    p.pixels = pixels; p.P = P;
    p.phasor = phasor; p.gt_phasor = gt_phasor; p.phasor_stride = phasor_plane_stride; p.gt_stride = gt_plane_stride;
    p.depth = depth; p.gt_depth = gt_depth; p.dd = depth_distortion;
    p.amp = amp; p.amp_stride = amp_stride; p.visible = visible; p.visible_is_radii = visible_is_radii;
    p.depth_range_dev = depth_range_dev; p.phase_offset_dev = phase_offset_dev;
    p.depth_range = depth_range; p.phase_offset = phase_offset; p.tof_multiplier = tof_multiplier;
    p.partials = static_cast<uint32_t*>(partials);
    p.blocks = (int)tof_blocks(pixels + P);
    for (int k = 0; k < num_extras; k++) p.extras[k] = extras[k];
    p.num_extras = num_extras;
    p.rows = static_cast<uint32_t*>(rows);
    p.slots = (uint32_t)slots;
    p.cursor = static_cast<uint32_t*>(cursor);
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(k_tof_log_sums, dim3(p.blocks), dim3(TOF_THREADS), 0, s, p);
    hipLaunchKernelGGL(k_tof_log_finish, dim3(1), dim3(TOF_THREADS), 0, s, p);
    return gft_launched("gft_tof_log_row");
}
