// k_detsum.hip -- the fixed-order sum of the partial rows a backward walk stored (include/gftorf_detsum.h states the order),
// as launches across the chip.  Used by the rasterizer's fixed-order backward (k_render.hip: 15 values, rows of 16 floats) and
// by the flow renderer's (k_features.hip: 3 or 6 values, rows of 8 floats).
//
// k_acc_reduce_det (k_render.hip) defines the order by walking the tiles one after the other in ONE workgroup.  The same sum
// is formed here per Gaussian instead: a Gaussian's tiles lie inside its tile rectangle (GeomView.rect), so the rank of a
// tile inside the rectangle, row by row, IS the ascending tile order.
//   k_detsum_block_sums / _top / _offsets : exclusive scan of GeomView.tiles (the rectangles' areas) -> a run of slots per
//                                           Gaussian; their total is R, the frame's instance count (<= the binning capacity)
//   k_detsum_index  : one workgroup per tile walks the entries some quadrant of the tile walked and records
//                     slot(Gaussian, tile) -> position in point_list + 1 (0: the tile's walk never came to that Gaussian)
//   k_detsum_pull   : one lane per (Gaussian, value) reads its slots in order and adds the four quadrant rows of each
// No step has a conflict, an atomic or anything that depends on the order in which workgroups run.
//
// Can a list hold a Gaussian outside its rectangle?  No: whole-frame binning makes one instance per tile of the rectangle
// (k_binning.hip), the supertile entries of tile-pull binning carry the rectangle clipped to the supertile and a tile takes
// an entry only if it lies inside (k_pull.hip entry_hits), and a completed tail is a culled subset of those.  The index
// is therefore sized by the rectangles: R slots.  (An entry outside its rectangle would be skipped, never written out of
// bounds: every index is checked.)
#include "gft_internal.h"

namespace {

constexpr int SCAN_THREADS = 1024;
constexpr int SCAN_ITEMS = 4;
constexpr int SCAN_CHUNK = SCAN_THREADS * SCAN_ITEMS;

struct DetSumArgs {
    int P, T, gx;
    uint32_t cap;                              // binning capacity of the frame = slots of the index
    const uint32_t* __restrict__ ctrl;
    const uint32_t* __restrict__ tiles;        // [P] area of the rectangle
    const ushort4* __restrict__ rect;          // [P]
    const uint2* __restrict__ ranges;          // [T]
    const uint32_t* __restrict__ quad_max;     // [T][4]
    const uint32_t* __restrict__ point_list;
    uint32_t* off;                             // [P]  first slot of every Gaussian
    uint32_t* bsum;                            // [ceil(P / SCAN_CHUNK)]
    uint32_t* slot;                            // [cap]
    const float* __restrict__ rows;            // [list slot][4][stride]
    float* out;                                // [P][out_stride]
    int nv, out_stride, accumulate;
};

// exclusive scan of one value per thread over a workgroup of SCAN_THREADS; `total` = the workgroup's sum
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t* s_w, uint32_t& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    __syncthreads();                           // (s_w of an earlier call has been read)
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    uint32_t woff = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SCAN_THREADS / 64; w++) {
        const uint32_t t = s_w[w];
        if (w < wave) woff += t;
        all += t;
    }
    total = all;
    return woff + x - v;
}

__device__ __forceinline__ uint32_t scan_items(const DetSumArgs& a, uint32_t* v)
{
    const int64_t first = (int64_t)blockIdx.x * SCAN_CHUNK + (int64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        v[k] = first + k < a.P ? a.tiles[first + k] : 0u;
        sum += v[k];
    }
    return sum;
}

__global__ __launch_bounds__(SCAN_THREADS) void k_detsum_block_sums(DetSumArgs a)
{
    __shared__ uint32_t s_w[SCAN_THREADS / 64];
    if (a.ctrl[GFT_CTRL_TOTAL] > a.cap) return;
    uint32_t v[SCAN_ITEMS], total;
    block_scan_excl(scan_items(a, v), s_w, total);
    if (threadIdx.x == 0) a.bsum[blockIdx.x] = total;
}

__global__ __launch_bounds__(SCAN_THREADS) void k_detsum_top(DetSumArgs a, int nb)
{
    __shared__ uint32_t s_w[SCAN_THREADS / 64];
    if (a.ctrl[GFT_CTRL_TOTAL] > a.cap) return;
    uint32_t carry = 0;
    for (int c0 = 0; c0 < nb; c0 += SCAN_THREADS) {
        const int i = c0 + (int)threadIdx.x;
        const uint32_t v = i < nb ? a.bsum[i] : 0u;
        uint32_t total;
        const uint32_t e = block_scan_excl(v, s_w, total);
        if (i < nb) a.bsum[i] = carry + e;
        carry += total;
    }
}

__global__ __launch_bounds__(SCAN_THREADS) void k_detsum_offsets(DetSumArgs a)
{
    __shared__ uint32_t s_w[SCAN_THREADS / 64];
    if (a.ctrl[GFT_CTRL_TOTAL] > a.cap) return;
    uint32_t v[SCAN_ITEMS], total;
    uint32_t run = a.bsum[blockIdx.x] + block_scan_excl(scan_items(a, v), s_w, total);
    const int64_t first = (int64_t)blockIdx.x * SCAN_CHUNK + (int64_t)threadIdx.x * SCAN_ITEMS;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        if (first + k < a.P) a.off[first + k] = run;
        run += v[k];
    }
}

__global__ __launch_bounds__(256) void k_detsum_index(DetSumArgs a)
{
    if (a.ctrl[GFT_CTRL_TOTAL] > a.cap) return;
    const int tile = (int)blockIdx.x;
    const uint4 qm = reinterpret_cast<const uint4*>(a.quad_max)[tile];
    const uint32_t walked = max(max(qm.x, qm.y), max(qm.z, qm.w));      // entries some quadrant of the tile walked
    if (walked == 0) return;
    const uint32_t r0 = a.ranges[tile].x;
    const uint32_t tx = (uint32_t)(tile % a.gx), ty = (uint32_t)(tile / a.gx);
    for (uint32_t c = threadIdx.x; c < walked; c += 256u) {
        const uint32_t p = r0 + c;
        const uint32_t g = a.point_list[p];
        if (g >= (uint32_t)a.P) continue;
        const ushort4 r = a.rect[g];
        if (tx < r.x || tx >= r.z || ty < r.y || ty >= r.w) continue;
        const uint32_t s = a.off[g] + (ty - r.y) * (uint32_t)(r.z - r.x) + (tx - r.x);
        if (s < a.cap) a.slot[s] = p + 1u;
    }
}

// STRIDE lanes per Gaussian: lane k adds value k.  The loads of UNROLL slots are issued together (a slot that is empty or past
// the end reads row 0 and is not added), the additions follow in slot order.
template <int STRIDE>
__global__ __launch_bounds__(256) void k_detsum_pull(DetSumArgs a)
{
    constexpr int UNROLL = 4;
    if (a.ctrl[GFT_CTRL_TOTAL] > a.cap) return;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t g = i / STRIDE;
    const int k = (int)(i - g * STRIDE);
    if (g >= a.P) return;
    const bool mine = k < a.nv;
    const uint32_t n = a.tiles[g];
    float* dst = a.out + g * a.out_stride + k;
    if (n == 0 || a.cap == 0) {
        if (mine && !a.accumulate) *dst = 0.f;
        return;
    }
    float acc = (mine && a.accumulate) ? *dst : 0.f;
    const uint32_t o = a.off[g];
    for (uint32_t r = 0; r < n; r += UNROLL) {
        uint32_t q[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const uint64_t s = (uint64_t)o + min(r + (uint32_t)u, n - 1u);
            q[u] = a.slot[min(s, (uint64_t)a.cap - 1u)];
            if (r + (uint32_t)u >= n || s >= a.cap) q[u] = 0u;
        }
        float v[UNROLL][4];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const float* row = a.rows + (size_t)(q[u] ? q[u] - 1u : 0u) * 4 * STRIDE + k;
#pragma unroll
            for (int w = 0; w < 4; w++) v[u][w] = row[w * STRIDE];
        }
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            float s = v[u][0];
            s += v[u][1];
            s += v[u][2];
            s += v[u][3];
            if (q[u] && s != 0.f) acc = acc + s;
        }
    }
    if (mine) *dst = acc;
}

// The comparator for row strides other than the rasterizer's: k_acc_reduce_det (k_render.hip) with the strides as arguments.
// One workgroup walks the tiles one after the other; it clears `out` first (behind the test of the frame: a frame that was
// not drawn leaves it untouched).
__global__ __launch_bounds__(1024) void k_detsum_serial(DetSumArgs a, int stride)
{
    if (a.ctrl[GFT_CTRL_TOTAL] > a.cap) return;
    const int tid = threadIdx.x;
    for (int64_t i = tid; i < (int64_t)a.P * a.out_stride; i += 1024) a.out[i] = 0.f;
    __threadfence();
    __syncthreads();
    for (int tile = 0; tile < a.T; tile++) {
        const uint4 qm = reinterpret_cast<const uint4*>(a.quad_max)[tile];
        const uint32_t walked = max(max(qm.x, qm.y), max(qm.z, qm.w));
        const uint2 rg = a.ranges[tile];
        for (uint32_t i = (uint32_t)tid; i < walked * (uint32_t)stride; i += 1024u) {
            const uint32_t c = i / (uint32_t)stride, k = i % (uint32_t)stride;
            if (k >= (uint32_t)a.nv) continue;
            const uint32_t p = rg.x + c;
            const float* row = a.rows + (size_t)p * 4 * stride + k;
            float s = row[0];
            s += row[stride];
            s += row[2 * stride];
            s += row[3 * stride];
            if (s != 0.f) {
                float* dst = a.out + (size_t)a.point_list[p] * a.out_stride + k;
                __hip_atomic_store(dst, __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + s,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        __threadfence();
        __syncthreads();
    }
}

size_t scan_blocks(int32_t P) { return ((size_t)(P > 0 ? P : 0) + SCAN_CHUNK - 1) / SCAN_CHUNK; }

DetSumArgs detsum_args(int P, int W, int H, const GeomView& g, const ImgView& im, const BinView& b, uint32_t cap,
                       const float* rows, int nv, float* out, int out_stride, bool accumulate)
{
    DetSumArgs a = {};
    a.P = P;
    a.gx = (W + GFT_TILE_X - 1) / GFT_TILE_X;
    a.T = a.gx * ((H + GFT_TILE_Y - 1) / GFT_TILE_Y);
    a.cap = cap;
    a.ctrl = im.ctrl; a.tiles = g.tiles; a.rect = g.rect;
    a.ranges = im.ranges; a.quad_max = im.tile_max; a.point_list = b.point_list;
    a.rows = rows; a.out = out; a.nv = nv; a.out_stride = out_stride; a.accumulate = accumulate ? 1 : 0;
    return a;
}

}  // namespace

size_t gft_detsum_index_words(int32_t P, int64_t binning_instances)
{
    const size_t p = (size_t)(P > 0 ? P : 0), cap = (size_t)(binning_instances > 0 ? binning_instances : 0);
    return p + scan_blocks(P) + cap;
}

hipError_t gft_launch_detsum(hipStream_t s, int P, int W, int H, const GeomView& g, const ImgView& im, const BinView& b,
                             uint32_t cap, const float* rows, int stride, int nv, float* out, int out_stride, bool accumulate,
                             uint32_t* index)
{
    if (P <= 0) return hipSuccess;
    if ((stride != 8 && stride != 16) || nv > stride) return hipErrorInvalidValue;
    DetSumArgs a = detsum_args(P, W, H, g, im, b, cap, rows, nv, out, out_stride, accumulate);
    const int nb = (int)scan_blocks(P);
    a.off = index; a.bsum = index + P; a.slot = a.bsum + nb;
    if (cap > 0) {
        const hipError_t e = gft_zero_async(a.slot, (size_t)cap * sizeof(uint32_t), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_detsum_block_sums, dim3(nb), dim3(SCAN_THREADS), 0, s, a);
        hipLaunchKernelGGL(k_detsum_top, dim3(1), dim3(SCAN_THREADS), 0, s, a, nb);
        hipLaunchKernelGGL(k_detsum_offsets, dim3(nb), dim3(SCAN_THREADS), 0, s, a);
        hipLaunchKernelGGL(k_detsum_index, dim3(a.T), dim3(256), 0, s, a);
    }
    const int64_t threads = (int64_t)P * stride;
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    if (stride == 16) hipLaunchKernelGGL(k_detsum_pull<16>, dim3(blocks), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_detsum_pull<8>, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t gft_launch_detsum_serial(hipStream_t s, int P, int W, int H, const ImgView& im, const BinView& b, uint32_t cap,
                                    const float* rows, int stride, int nv, float* out, int out_stride)
{
    if (P <= 0) return hipSuccess;
    DetSumArgs a = detsum_args(P, W, H, GeomView{}, im, b, cap, rows, nv, out, out_stride, true);
    if (cap == 0) a.T = 0;                     // no lists: `out` is cleared, nothing is walked
    hipLaunchKernelGGL(k_detsum_serial, dim3(1), dim3(1024), 0, s, a, stride);
    return hipGetLastError();
}
