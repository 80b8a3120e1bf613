// k_metrics.hip -- a view's evaluation metrics (include/gftorf_metrics.h; train.py:535-579).  k_metrics_sums: one grid-stride
// loop over the pixels of up to eight plane pairs in two groups with pixel counts of their own, the loop running to the larger
// count and every group guarded: per-lane fp32 sums of |a - b| and (a - b)^2, widened to double for the two stages of
// gft_reduce.h (a lane sums two pixels of a 640x480 view; the 256 lanes' sums are then added without a rounding of their
// own).  k_metrics_finish forms the eight values, writes the row and lets one thread add them into the accumulator.  Scalar
// loads only (each coalesced across the wave; the pass moves 8 bytes per pixel and pair).
#include "gft_internal.h"
#include "gft_reduce.h"
#include "gft_tof_depth.h"
#include "gftorf_metrics.h"

namespace {

constexpr int MET_THREADS = 256, MET_MAX_BLOCKS = 1024, MET_PLANES = GFT_METRICS_MAX_PLANES;
constexpr int MET_SUMS = 2 * (MET_PLANES + 1);            // S1, S2 of the pairs read from memory, then of the ToF depth

static_assert(GFT_METRICS_PARTIAL_WORDS == 2 * MET_SUMS, "two doubles per pair and two for the ToF depth");
static_assert(GFT_METRICS_ROW_MSE == GFT_METRICS_VALUES && GFT_METRICS_ROW_PSNR == GFT_METRICS_ROW_MSE + MET_PLANES &&
              GFT_METRICS_ROW_PRESENT == GFT_METRICS_ROW_PSNR + MET_PLANES && GFT_METRICS_ROW_PLANES < GFT_METRICS_ROW_WORDS,
              "the row: the values, the planes' mse and psnr, two counts");
static_assert(GFT_METRICS_ACC_VIEWS == 2 * GFT_METRICS_VALUES && GFT_METRICS_ACC_PRESENT < GFT_METRICS_ACC_WORDS, "eight doubles, two words");

struct MetArgs {
    int64_t pixels_a, pixels_b;
    const float* a[MET_PLANES];                 // pair k: rendered ...
    const float* b[MET_PLANES];                 // ... and ground truth; [0, n_a) of pixels_a floats, [n_a, n_mem) of pixels_b
    int n_a, n_tof, has_depth, n_mem;           // n_mem = n_a + n_tof + has_depth pairs are read from memory
    const float* __restrict__ phasor;           // planes 0, 1 at phasor_stride, or NULL: the ToF depth pair, numbered n_mem
    const float* __restrict__ gt_depth;
    int64_t phasor_stride;
    const float* __restrict__ depth_range_dev;
    const float* __restrict__ phase_offset_dev;
    float depth_range, phase_offset;
    double* partials;                           // [blocks][MET_SUMS]
    int blocks;
    uint32_t* row;                              // [GFT_METRICS_ROW_WORDS] or NULL
    uint32_t* accum;                            // [GFT_METRICS_ACC_WORDS] or NULL
};

int64_t met_blocks(int64_t total) { return gft_grid_blocks(total, MET_THREADS, 1, MET_MAX_BLOCKS); }

__global__ __launch_bounds__(MET_THREADS) void k_metrics_sums(MetArgs p)
{
    __shared__ double sRed[MET_SUMS][MET_THREADS / 64];
    float s[MET_SUMS];
#pragma unroll
    for (int k = 0; k < MET_SUMS; k++) s[k] = 0.f;
    const float dr = gft_dev_or(p.depth_range_dev, p.depth_range), off = gft_dev_or(p.phase_offset_dev, p.phase_offset);
    const int64_t total = p.pixels_a > p.pixels_b ? p.pixels_a : p.pixels_b;
    for (int64_t i = (int64_t)blockIdx.x * MET_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * MET_THREADS) {
        const bool in_a = i < p.pixels_a, in_b = i < p.pixels_b;
#pragma unroll
        for (int k = 0; k < MET_PLANES; k++) {
            if (k < p.n_a ? in_a : (k < p.n_mem && in_b)) {
                const float d = p.a[k][i] - p.b[k][i];
                s[2 * k] += fabsf(d);
                s[2 * k + 1] += d * d;
            }
        }
        if (p.phasor && in_b) {
            const float d = depth_from_tof(p.phasor[i], p.phasor[p.phasor_stride + i], dr, off) - p.gt_depth[i];
            s[2 * MET_PLANES] += fabsf(d);
            s[2 * MET_PLANES + 1] += d * d;
        }
    }
    double w[MET_SUMS];
#pragma unroll
    for (int k = 0; k < MET_SUMS; k++) w[k] = (double)s[k];
    gft_fold_store<MET_THREADS>(w, sRed);
    __syncthreads();
    if (threadIdx.x < MET_SUMS) p.partials[(size_t)blockIdx.x * MET_SUMS + threadIdx.x] = gft_waves_total<MET_THREADS>(sRed[threadIdx.x]);
}

// utils/image_utils.py:18-19 on one plane's mse, in double: +inf at 0
__device__ __forceinline__ double met_psnr(double mse)
{
    return 20.0 * log10(1.0 / sqrt(mse));
}

// one workgroup: the rows of partials in a fixed order, in double; then the eight values, the row and the accumulator
__global__ __launch_bounds__(MET_THREADS) void k_metrics_finish(MetArgs p)
{
    __shared__ double sSum[MET_SUMS][MET_THREADS];
    __shared__ double mse[MET_PLANES], psnr[MET_PLANES];          // thread 0's alone: indexed by run-time pair numbers
    const int tid = threadIdx.x;
    double s[MET_SUMS];
#pragma unroll
    for (int k = 0; k < MET_SUMS; k++) s[k] = 0.0;
    for (int b = tid; b < p.blocks; b += MET_THREADS) {
        const double* part = p.partials + (size_t)b * MET_SUMS;
#pragma unroll
        for (int k = 0; k < MET_SUMS; k++) s[k] += part[k];
    }
#pragma unroll
    for (int k = 0; k < MET_SUMS; k++) sSum[k][tid] = s[k];
    gft_tree_sum<MET_THREADS>(sSum);
    if (tid != 0) return;
    const double na = (double)p.pixels_a, nb = (double)p.pixels_b;
    const int n_planes = p.n_mem + (p.phasor ? 1 : 0);
    double v[GFT_METRICS_VALUES];
    for (int k = 0; k < GFT_METRICS_VALUES; k++) v[k] = 0.0;
    for (int k = 0; k < MET_PLANES; k++) {
        // pair k's sums: the ToF depth's are kept behind those of the pairs read from memory
        const int src = (k == p.n_mem && p.phasor) ? MET_PLANES : k;
        mse[k] = k < n_planes ? sSum[2 * src + 1][0] / (k < p.n_a ? na : nb) : 0.0;
        psnr[k] = k < n_planes ? met_psnr(mse[k]) : 0.0;
    }
    uint32_t present = 0u;
    if (p.n_a > 0) {
        double l1 = 0.0, ps = 0.0;
        for (int k = 0; k < p.n_a; k++) { l1 += sSum[2 * k][0]; ps += psnr[k]; }
        v[GFT_METRICS_L1] = l1 / ((double)p.n_a * na);
        v[GFT_METRICS_PSNR] = ps / (double)p.n_a;
        present |= GFT_METRICS_HAS_COLOUR;
    }
    if (p.n_tof > 0) {
        double l1 = 0.0, l2 = 0.0, ps = 0.0;
        for (int k = p.n_a; k < p.n_a + p.n_tof; k++) { l1 += sSum[2 * k][0]; l2 += sSum[2 * k + 1][0]; ps += psnr[k]; }
        v[GFT_METRICS_L1_P] = l1 / ((double)p.n_tof * nb);
        v[GFT_METRICS_L2_P] = l2 / ((double)p.n_tof * nb);
        v[GFT_METRICS_PSNR_P] = ps / (double)p.n_tof;
        present |= GFT_METRICS_HAS_TOF;
    }
    if (p.has_depth) {
        const int k = p.n_mem - 1;
        v[GFT_METRICS_L1_D] = sSum[2 * k][0] / nb;
        v[GFT_METRICS_L2_D] = mse[k];
        present |= GFT_METRICS_HAS_DEPTH;
    }
    if (p.phasor) {
        v[GFT_METRICS_L2_D_TOF] = mse[p.n_mem];
        present |= GFT_METRICS_HAS_TOF_DEPTH;
    }
    if (p.row) {
        for (int k = 0; k < GFT_METRICS_VALUES; k++) p.row[k] = __float_as_uint((float)v[k]);
        for (int k = 0; k < MET_PLANES; k++) {
            p.row[GFT_METRICS_ROW_MSE + k] = __float_as_uint((float)mse[k]);
            p.row[GFT_METRICS_ROW_PSNR + k] = __float_as_uint((float)psnr[k]);
        }
        p.row[GFT_METRICS_ROW_PRESENT] = present;
        p.row[GFT_METRICS_ROW_PLANES] = (uint32_t)n_planes;
        for (int k = GFT_METRICS_ROW_PLANES + 1; k < GFT_METRICS_ROW_WORDS; k++) p.row[k] = 0u;
    }
    if (p.accum) {
        double* sums = reinterpret_cast<double*>(p.accum + GFT_METRICS_ACC_SUMS);
        for (int k = 0; k < GFT_METRICS_VALUES; k++) sums[k] += v[k];
        p.accum[GFT_METRICS_ACC_VIEWS] += 1u;
        p.accum[GFT_METRICS_ACC_PRESENT] |= present;
    }
}

__global__ void k_metrics_reset(uint32_t* accum)
{
    if (threadIdx.x < GFT_METRICS_ACC_WORDS) accum[threadIdx.x] = 0u;
}

bool bad_stride(int64_t s) { return s < 0 || s > (1ll << 40); }

}  // namespace

extern "C" int64_t gft_metrics_blocks(int64_t pixels)
{
    if (pixels < 1) return 0;
    return met_blocks(pixels);
}

extern "C" int gft_view_metrics(void* hip_stream, int64_t pixels_a, int32_t channels_a, const float* image, int64_t image_stride,
                                const float* gt_image, int64_t gt_image_stride, int64_t pixels_b, int32_t channels_b, const float* tof,
                                int64_t tof_stride, const float* gt_tof, int64_t gt_tof_stride, const float* depth, const float* gt_depth,
                                const float* phasor, int64_t phasor_stride, const float* depth_range_dev, float depth_range,
                                const float* phase_offset_dev, float phase_offset, void* partials, void* row, void* accum)
{
    if (channels_a < 0 || channels_b < 0 || channels_a > MET_PLANES || channels_b > MET_PLANES)
        return gft_fail("gft_view_metrics: bad channel counts channels_a=%d channels_b=%d", channels_a, channels_b);
    const bool group_b = channels_b > 0 || depth || phasor;
    const int planes = channels_a + channels_b + (depth ? 1 : 0) + (phasor ? 1 : 0);
    if (planes < 1) return gft_fail("gft_view_metrics: no plane pair is given");
    if (planes > MET_PLANES) return gft_fail("gft_view_metrics: %d plane pairs, at most %d fit one call", planes, MET_PLANES);
    if ((channels_a > 0 && (pixels_a < 1 || pixels_a > (1ll << 40))) || (group_b && (pixels_b < 1 || pixels_b > (1ll << 40))))
        return gft_fail("gft_view_metrics: bad sizes pixels_a=%lld pixels_b=%lld", (long long)pixels_a, (long long)pixels_b);
    if (channels_a > 0 && (!image || !gt_image)) return gft_fail("gft_view_metrics: image or gt_image is NULL");
    if (channels_b > 0 && (!tof || !gt_tof)) return gft_fail("gft_view_metrics: tof or gt_tof is NULL");
    if ((depth || phasor) && !gt_depth) return gft_fail("gft_view_metrics: depth or phasor without gt_depth");
    if (gt_depth && !depth && !phasor) return gft_fail("gft_view_metrics: gt_depth without depth or phasor");
    if (bad_stride(image_stride) || bad_stride(gt_image_stride) || bad_stride(tof_stride) || bad_stride(gt_tof_stride) ||
        bad_stride(phasor_stride))
        return gft_fail("gft_view_metrics: bad plane stride");
    if (!partials || ((uintptr_t)partials & 7u)) return gft_fail("gft_view_metrics: partials is NULL or not 8-byte aligned");
    if (!row && !accum) return gft_fail("gft_view_metrics: row and accum are both NULL");
    if ((uintptr_t)accum & 7u) return gft_fail("gft_view_metrics: accum is not 8-byte aligned");
    MetArgs p = {};
    p.pixels_a = channels_a > 0 ? pixels_a : 0;
    p.pixels_b = group_b ? pixels_b : 0;
    int k = 0;
    for (int c = 0; c < channels_a; c++, k++) { p.a[k] = image + c * image_stride; p.b[k] = gt_image + c * gt_image_stride; }
    for (int c = 0; c < channels_b; c++, k++) { p.a[k] = tof + c * tof_stride; p.b[k] = gt_tof + c * gt_tof_stride; }
    if (depth) { p.a[k] = depth; p.b[k] = gt_depth; k++; }
    p.n_a = channels_a; p.n_tof = channels_b; p.has_depth = depth ? 1 : 0; p.n_mem = k;
    p.phasor = phasor; p.gt_depth = gt_depth; p.phasor_stride = phasor_stride;
    p.depth_range_dev = depth_range_dev; p.phase_offset_dev = phase_offset_dev;
    p.depth_range = depth_range; p.phase_offset = phase_offset;
    p.partials = static_cast<double*>(partials);
    p.blocks = (int)met_blocks(p.pixels_a > p.pixels_b ? p.pixels_a : p.pixels_b);
    p.row = static_cast<uint32_t*>(row);
    p.accum = static_cast<uint32_t*>(accum);
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(k_metrics_sums, dim3(p.blocks), dim3(MET_THREADS), 0, s, p);
    hipLaunchKernelGGL(k_metrics_finish, dim3(1), dim3(MET_THREADS), 0, s, p);
    return gft_launched("gft_view_metrics");
}

extern "C" int gft_metrics_reset(void* hip_stream, void* accum)
{
    if (!accum || ((uintptr_t)accum & 7u)) return gft_fail("gft_metrics_reset: accum is NULL or not 8-byte aligned");
    hipLaunchKernelGGL(k_metrics_reset, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, static_cast<uint32_t*>(accum));
    return gft_launched("gft_metrics_reset");
}
