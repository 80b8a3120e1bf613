// k_densify.hip -- per-Gaussian bookkeeping around the rasterizer (include/gftorf_densify.h): the
// statistics update of every iteration, the order-preserving row compaction of `t[mask]`, and the plan and the
// row mover of a whole densify_and_prune event, and the children of its split rows (k_split_children).
// HBM-bound byte work: coalesced reads, one pass.
#include "gft_internal.h"
#include "gft_reduce.h"
#include "gftorf_densify.h"

namespace {

constexpr int DN_BLOCK = 256;
constexpr int RK_ROWS = 4096;        // rows per rank workgroup (256 threads x 16 mask bytes)

// ---- statistics (scene/gaussian_model.py:648-654, train.py:443) ---------------------------------
__global__ __launch_bounds__(DN_BLOCK) void k_densify_stats(int64_t P, const float* __restrict__ grad, const float* __restrict__ pixels,
                                                            const int32_t* __restrict__ radii, const uint8_t* __restrict__ upd,
                                                            const uint8_t* __restrict__ apply, float* accum, float* denom, float* maxr)
{
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (i >= P || !upd[i]) return;
    if (maxr) maxr[i] = fmaxf(maxr[i], (float)radii[i]);                 // torch.max(float, int32) promotes to float
    if (apply && !apply[i]) return;
    const float px = pixels[i];
    if (accum) {
        // torch.norm(g[:, :2], dim=-1): the reduction `acc + v * v` of torch's norm kernels contracts to an fma,
        // on the host as on the device: sqrt(fma(y, y, x * x))
        const float gx = grad[3 * i], gy = grad[3 * i + 1];
        accum[i] += sqrtf(fmaf(gy, gy, gx * gx)) * px;
    }
    if (denom) denom[i] += px;
}

// ---- rank: per-workgroup counts, the last workgroup scans them ----------------------------------
struct RankArgs {
    int64_t P;
    const uint8_t* mask;
    int32_t* rank;
    uint32_t* block_sum;     // [blocks]
    uint32_t* total;         // 1 word
};

__device__ __forceinline__ uint32_t nz_bytes(uint32_t w)
{
    // number of non-zero bytes of a word (torch.bool holds 0 / 1, any non-zero byte counts)
    return ((w & 0xffu) != 0) + ((w & 0xff00u) != 0) + ((w & 0xff0000u) != 0) + ((w & 0xff000000u) != 0);
}

__global__ __launch_bounds__(DN_BLOCK) void k_rows_count(RankArgs a)
{
    __shared__ uint32_t wsum[DN_BLOCK / 64];
    const int64_t r0 = (int64_t)blockIdx.x * RK_ROWS + threadIdx.x * 16;
    uint32_t c = 0;
    if (r0 + 16 <= a.P && ((uintptr_t)(a.mask + r0) & 15) == 0) {
        const uint4 m = *reinterpret_cast<const uint4*>(a.mask + r0);
        c = nz_bytes(m.x) + nz_bytes(m.y) + nz_bytes(m.z) + nz_bytes(m.w);
    } else {
        for (int k = 0; k < 16; k++)
            if (r0 + k < a.P && a.mask[r0 + k]) c++;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor((int)c, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) a.block_sum[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// one workgroup: exclusive scan of the block sums in place, total
__device__ __forceinline__ void scan_block_sums(uint32_t* block_sum, int nblocks, uint32_t* total)
{
    __shared__ uint32_t part[1024];
    const int per = (nblocks + 1023) / 1024;
    const int b0 = threadIdx.x * per;
    uint32_t s = 0;
    for (int k = 0; k < per; k++)
        if (b0 + k < nblocks) s += block_sum[b0 + k];
    part[threadIdx.x] = s;
    __syncthreads();
    // Hillis-Steele over 1024 partials
    for (int o = 1; o < 1024; o <<= 1) {
        const uint32_t v = threadIdx.x >= o ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - s;            // exclusive prefix of this thread's first block
    for (int k = 0; k < per; k++)
        if (b0 + k < nblocks) {
            const uint32_t v = block_sum[b0 + k];
            block_sum[b0 + k] = run;
            run += v;
        }
    if (threadIdx.x == 1023) *total = part[1023];
}

__global__ __launch_bounds__(1024) void k_rows_scan(uint32_t* block_sum, int nblocks, uint32_t* total)
{
    scan_block_sums(block_sum, nblocks, total);
}

__global__ __launch_bounds__(DN_BLOCK) void k_rows_rank(RankArgs a)
{
    __shared__ uint32_t wsum[DN_BLOCK / 64];
    const int64_t r0 = (int64_t)blockIdx.x * RK_ROWS + threadIdx.x * 16;
    uint8_t m[16];
    uint32_t c = 0;
    for (int k = 0; k < 16; k++) {
        m[k] = (r0 + k < a.P) ? a.mask[r0 + k] : 0;
        c += m[k] != 0;
    }
    // exclusive prefix of c over the workgroup
    uint32_t inc = c;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t base = a.block_sum[blockIdx.x];
    for (int w = 0; w < wave; w++) base += wsum[w];
    uint32_t run = base + inc - c;
    for (int k = 0; k < 16; k++)
        if (r0 + k < a.P) {
            a.rank[r0 + k] = (int32_t)run;
            run += m[k] != 0;
        }
}

// ---- gather: dst[rank[i]] = src[i] where mask[i]; PIECE = bytes per thread access -------------------
template <typename T>
__global__ __launch_bounds__(DN_BLOCK) void k_rows_gather(int64_t P, int pieces /* per row */, const uint8_t* __restrict__ mask,
                                                          const int32_t* __restrict__ rank, const T* __restrict__ src, T* __restrict__ dst)
{
    const int64_t e = (int64_t)blockIdx.x * DN_BLOCK + threadIdx.x;
    const int64_t row = e / pieces;
    if (row >= P || !mask[row]) return;
    const int piece = (int)(e - row * pieces);
    dst[(int64_t)rank[row] * pieces + piece] = src[e];
}

}  // namespace

extern "C" int gft_densify_stats(void* hip_stream, int64_t P, const float* viewspace_grad, const float* pixels, const int32_t* radii,
                                 const uint8_t* update_filter, const uint8_t* apply_mask, float* xyz_gradient_accum, float* denom,
                                 float* max_radii2D)
{
    if (P < 0) return gft_fail("gft_densify_stats: P < 0");
    if (P == 0) return 0;
    if (!update_filter) return gft_fail("gft_densify_stats: update_filter is NULL");
    if ((xyz_gradient_accum && !viewspace_grad) || ((xyz_gradient_accum || denom) && !pixels) || (max_radii2D && !radii))
        return gft_fail("gft_densify_stats: an input of a requested statistic is NULL");
    hipLaunchKernelGGL(k_densify_stats, dim3((unsigned)((P + DN_BLOCK - 1) / DN_BLOCK)), dim3(DN_BLOCK), 0, (hipStream_t)hip_stream, P,
                       viewspace_grad, pixels, radii, update_filter, apply_mask, xyz_gradient_accum, denom, max_radii2D);
    GFT_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" size_t gft_rows_rank_scratch_bytes(int64_t P)
{
    const int64_t blocks = P <= 0 ? 0 : (P + RK_ROWS - 1) / RK_ROWS;
    return (size_t)(blocks + 64) * sizeof(uint32_t);
}

// the three launches of a ranking; the count stays on the device (*total_dev; NULL: behind the block sums in scratch)
static int rows_rank_launch(hipStream_t s, int64_t P, const uint8_t* mask, int32_t* rank, void* scratch, uint32_t* total_dev,
                            uint32_t** total_at)
{
    const int blocks = (int)((P + RK_ROWS - 1) / RK_ROWS);
    RankArgs a;
    a.P = P; a.mask = mask; a.rank = rank;
    a.block_sum = (uint32_t*)scratch;
    a.total = total_dev ? total_dev : a.block_sum + blocks;
    hipLaunchKernelGGL(k_rows_count, dim3(blocks), dim3(DN_BLOCK), 0, s, a);
    hipLaunchKernelGGL(k_rows_scan, dim3(1), dim3(1024), 0, s, a.block_sum, blocks, a.total);
    hipLaunchKernelGGL(k_rows_rank, dim3(blocks), dim3(DN_BLOCK), 0, s, a);
    GFT_CHECK_HIP(hipGetLastError());
    if (total_at) *total_at = a.total;
    return 0;
}

extern "C" int gft_rows_rank(void* hip_stream, int64_t P, const uint8_t* mask, int32_t* rank, void* scratch, int64_t* count)
{
    if (!count) return gft_fail("gft_rows_rank: count is NULL");
    *count = 0;
    if (P < 0 || P > 0x7fffffffll) return gft_fail("gft_rows_rank: bad row count");
    if (P == 0) return 0;
    if (!mask || !rank || !scratch) return gft_fail("gft_rows_rank: NULL argument");
    hipStream_t s = (hipStream_t)hip_stream;
    uint32_t* total = nullptr;
    if (rows_rank_launch(s, P, mask, rank, scratch, nullptr, &total)) return 1;
    uint32_t host = 0;
    GFT_CHECK_HIP(hipMemcpyAsync(&host, total, sizeof(host), hipMemcpyDeviceToHost, s));
    GFT_CHECK_HIP(hipStreamSynchronize(s));
    *count = host;
    return 0;
}

extern "C" int gft_rows_rank_dev(void* hip_stream, int64_t P, const uint8_t* mask, int32_t* rank, void* scratch, uint32_t* count_dev)
{
    if (!count_dev) return gft_fail("gft_rows_rank_dev: count_dev is NULL");
    if (P <= 0 || P > 0x7fffffffll) return gft_fail("gft_rows_rank_dev: bad row count");
    if (!mask || !rank || !scratch) return gft_fail("gft_rows_rank_dev: NULL argument");
    return rows_rank_launch((hipStream_t)hip_stream, P, mask, rank, scratch, count_dev, nullptr);
}

// mask[i] = 1 if row i of `a` ([P, ra] floats) or of `b` ([P, rb] floats) holds a value that is not zero (NaN counts,
// -0 does not): four lanes per row, 16-byte pieces when a row is a whole number of them
namespace {
__device__ __forceinline__ bool row_part_nonzero(const float* __restrict__ t, int64_t row, int r, int q)
{
    bool any = false;
    if (!t) return false;
    const float* p = t + row * r;
    if ((r & 3) == 0 && ((uintptr_t)t & 15) == 0) {
        for (int v = q; v < (r >> 2); v += 4) {
            const float4 x = reinterpret_cast<const float4*>(p)[v];
            any |= (x.x != 0.f) | (x.y != 0.f) | (x.z != 0.f) | (x.w != 0.f);
        }
    } else {
        for (int c = q; c < r; c += 4) any |= p[c] != 0.f;
    }
    return any;
}

__global__ __launch_bounds__(256) void k_rows_any_nonzero(int64_t P, int ra, const float* __restrict__ a, int rb,
                                                          const float* __restrict__ b, uint8_t* __restrict__ mask)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = t >> 2;
    const int q = (int)(t & 3);
    bool any = false;
    if (row < P) any = row_part_nonzero(a, row, ra, q) | row_part_nonzero(b, row, rb, q);
    int v = any ? 1 : 0;
    v |= __shfl_xor(v, 1);
    v |= __shfl_xor(v, 2);
    if (row < P && q == 0) mask[row] = (uint8_t)v;
}
}  // namespace

extern "C" int gft_rows_any_nonzero(void* hip_stream, int64_t P, int32_t row_floats_a, const float* a, int32_t row_floats_b,
                                    const float* b, uint8_t* mask)
{
    if (P < 0 || row_floats_a < 0 || row_floats_b < 0) return gft_fail("gft_rows_any_nonzero: negative size");
    if (P == 0) return 0;
    if (!mask) return gft_fail("gft_rows_any_nonzero: mask is NULL");
    if (P > ((int64_t)1 << 40)) return gft_fail("gft_rows_any_nonzero: P too large");
    hipLaunchKernelGGL(k_rows_any_nonzero, dim3((unsigned)((4 * P + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, P,
                       (int)row_floats_a, a, (int)row_floats_b, b, mask);
    GFT_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int gft_rows_gather(void* hip_stream, int64_t P, const uint8_t* mask, const int32_t* rank, const void* src, void* dst,
                               int64_t row_bytes)
{
    if (P < 0 || row_bytes < 0) return gft_fail("gft_rows_gather: negative size");
    if (P == 0 || row_bytes == 0) return 0;
    if (row_bytes % 4) return gft_fail("gft_rows_gather: row_bytes must be a multiple of 4");
    if (!mask || !rank || !src || !dst) return gft_fail("gft_rows_gather: NULL argument");
    if (((uintptr_t)src | (uintptr_t)dst) & 3) return gft_fail("gft_rows_gather: pointers must be 4-byte aligned");
    hipStream_t s = (hipStream_t)hip_stream;
    const bool wide = row_bytes % 16 == 0 && ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0);
    const int64_t pieces = row_bytes / (wide ? 16 : 4);
    const int64_t total = P * pieces;
    if (pieces > 0x7fffffffll || (total + DN_BLOCK - 1) / DN_BLOCK > 0x7fffffffll) return gft_fail("gft_rows_gather: too large");
    const dim3 grid((unsigned)((total + DN_BLOCK - 1) / DN_BLOCK));
    if (wide) hipLaunchKernelGGL(k_rows_gather<uint4>, grid, dim3(DN_BLOCK), 0, s, P, (int)pieces, mask, rank, (const uint4*)src, (uint4*)dst);
    else hipLaunchKernelGGL(k_rows_gather<uint32_t>, grid, dim3(DN_BLOCK), 0, s, P, (int)pieces, mask, rank, (const uint32_t*)src, (uint32_t*)dst);
    GFT_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- the fused densify_and_prune (gftorf_amd.densify.densify_and_prune_fused) ------------------------------------------
// The event is a function of per-row quantities, so it is planned once and every tensor is then moved once.  Both plan
// passes rank TWO flags of a row in the three launches of a ranking (count, scan, rank): a workgroup's two counts (at most
// RK_ROWS each) travel through its prefix sum in the halves of one word.
namespace {

struct Rank2 {
    uint32_t* block_sum;     // [2][blocks]: flag a's sums, then flag b's
    int blocks;
    uint32_t* totals;        // 2 words
};

// F: flags(row) -> bit 0 = flag a, bit 1 = flag b; emit(row, flags, rank a, rank b)
template <typename F>
__global__ __launch_bounds__(DN_BLOCK) void k_plan_count(F f, int64_t rows, Rank2 r)
{
    __shared__ uint32_t wsum[DN_BLOCK / 64];
    const int64_t r0 = (int64_t)blockIdx.x * RK_ROWS + threadIdx.x * 16;
    uint32_t c = 0;
    for (int k = 0; k < 16; k++)
        if (r0 + k < rows) {
            const uint32_t fl = f.flags(r0 + k);
            c += (fl & 1u) + ((fl & 2u) << 15);
        }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor((int)c, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        r.block_sum[blockIdx.x] = t & 0xffffu;
        r.block_sum[r.blocks + blockIdx.x] = t >> 16;
    }
}

// two workgroups: each scans one flag's block sums
__global__ __launch_bounds__(1024) void k_plan_scan(Rank2 r)
{
    scan_block_sums(r.block_sum + (int64_t)blockIdx.x * r.blocks, r.blocks, r.totals + blockIdx.x);
}

template <typename F>
__global__ __launch_bounds__(DN_BLOCK) void k_plan_rank(F f, int64_t rows, Rank2 r)
{
    __shared__ uint32_t wsum[DN_BLOCK / 64];
    const int64_t r0 = (int64_t)blockIdx.x * RK_ROWS + threadIdx.x * 16;
    uint32_t bits = 0, c = 0;                      // two flag bits per row of this thread
    for (int k = 0; k < 16; k++)
        if (r0 + k < rows) {
            const uint32_t fl = f.flags(r0 + k) & 3u;
            bits |= fl << (2 * k);
            c += (fl & 1u) + ((fl & 2u) << 15);
        }
    uint32_t inc = c;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)inc, o);
        if (lane >= o) inc += v;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t excl = inc - c;
    for (int w = 0; w < wave; w++) excl += wsum[w];
    uint32_t ra = r.block_sum[blockIdx.x] + (excl & 0xffffu);
    uint32_t rb = r.block_sum[r.blocks + blockIdx.x] + (excl >> 16);
    for (int k = 0; k < 16; k++)
        if (r0 + k < rows) {
            const uint32_t fl = (bits >> (2 * k)) & 3u;
            f.emit(r0 + k, fl, ra, rb);
            ra += fl & 1u;
            rb += fl >> 1;
        }
}

// classify: flag a = cloned, flag b = split (scene/gaussian_model.py:573-579, 605-608)
struct PlanClassify {
    const float* gnorm;      // [P] torch.norm(grads, dim=-1)
    const float* g;          // [P] grads
    const float* ms;         // [P] largest activated scaling
    float max_grad, dense_thr;
    uint8_t* cls;            // [P] 0 keep, 1 clone, 2 split
    int32_t* clone_src;      // [C] the cloned rows in order
    int32_t* split_src;      // [S] the split rows in order
    __device__ __forceinline__ uint32_t flags(int64_t i) const
    {
        const float m = ms[i];
        const uint32_t clone = (gnorm[i] >= max_grad) && (m <= dense_thr);
        const uint32_t split = (g[i] >= max_grad) && (m > dense_thr);
        return clone | (split << 1);
    }
    __device__ __forceinline__ void emit(int64_t i, uint32_t fl, uint32_t ra, uint32_t rb) const
    {
        cls[i] = (uint8_t)fl;
        if (fl & 1u) clone_src[ra] = (int32_t)i;
        if (fl & 2u) split_src[rb] = (int32_t)i;
    }
};

// layout over the virtual rows (P originals, C clones, N * S children): flag a = survives, flag b = survives and is dynamic
struct PlanLayout {
    int64_t P, C, S;
    const uint8_t* cls;
    const int32_t* clone_src;
    const int32_t* split_src;
    const float* op;         // [P] activated opacity
    const float* ms;         // [P]
    const float* child_ms;   // [N * S] largest activated scaling of a child's own new scaling
    float min_opacity, big_thr, small_thr;
    int use_size, screen_dead;
    const float* seg;        // [P, seg_cols] or NULL
    int seg_cols;
    int32_t* source_row;     // outputs, one entry per survivor
    uint8_t* kind;
    int32_t* child;
    int32_t* map_new;        // source_row, a child redirected to P + its index
    int32_t* map_state;      // source_row of a kept original, -1 for a new row
    uint8_t* motion_mask;
    int32_t* motion_rank;
    __device__ __forceinline__ void where(int64_t v, int32_t& src, int32_t& kd, int32_t& ch) const
    {
        if (v < P) { src = (int32_t)v; kd = 0; ch = -1; }
        else if (v < P + C) { src = clone_src[v - P]; kd = 1; ch = -1; }
        else { ch = (int32_t)(v - P - C); src = split_src[ch % S]; kd = 2; }
    }
    __device__ __forceinline__ uint32_t flags(int64_t v) const
    {
        int32_t src, kd, ch;
        where(v, src, kd, ch);
        if (kd == 0 && cls[src] == 2) return 0;
        bool dead = op[src] < min_opacity;
        if (use_size) {
            const float m = kd == 2 ? child_ms[ch] : ms[src];
            dead = dead || screen_dead || (m > big_thr) || (m < small_thr);
        }
        if (dead) return 0;
        return 1u | ((seg && seg[(int64_t)src * seg_cols] > 0.5f) ? 2u : 0u);
    }
    __device__ __forceinline__ void emit(int64_t v, uint32_t fl, uint32_t ra, uint32_t rb) const
    {
        if (!(fl & 1u)) return;
        int32_t src, kd, ch;
        where(v, src, kd, ch);
        source_row[ra] = src;
        kind[ra] = (uint8_t)kd;
        child[ra] = ch;
        map_new[ra] = kd == 2 ? (int32_t)(P + ch) : src;
        map_state[ra] = kd == 0 ? src : -1;
        if (seg) {
            motion_mask[ra] = (uint8_t)(fl >> 1);
            motion_rank[ra] = (int32_t)rb;
        }
    }
};

template <typename F>
int plan_rank(hipStream_t s, const F& f, int64_t rows, void* scratch, int64_t* counts)
{
    const int blocks = (int)((rows + RK_ROWS - 1) / RK_ROWS);
    Rank2 r;
    r.block_sum = (uint32_t*)scratch;
    r.blocks = blocks;
    r.totals = r.block_sum + 2 * (int64_t)blocks;
    hipLaunchKernelGGL(k_plan_count<F>, dim3(blocks), dim3(DN_BLOCK), 0, s, f, rows, r);
    hipLaunchKernelGGL(k_plan_scan, dim3(2), dim3(1024), 0, s, r);
    hipLaunchKernelGGL(k_plan_rank<F>, dim3(blocks), dim3(DN_BLOCK), 0, s, f, rows, r);
    GFT_CHECK_HIP(hipGetLastError());
    uint32_t host[2] = {0, 0};
    GFT_CHECK_HIP(hipMemcpyAsync(host, r.totals, sizeof(host), hipMemcpyDeviceToHost, s));
    GFT_CHECK_HIP(hipStreamSynchronize(s));
    counts[0] = host[0];
    counts[1] = host[1];
    return 0;
}

// dst[r] = row map[r] of src (map[r] < src_rows), row map[r] - src_rows of extra, or zero (map[r] < 0)
template <typename T>
__global__ __launch_bounds__(DN_BLOCK) void k_rows_remap(int64_t total, int pieces /* per row */, const int32_t* __restrict__ map,
                                                         const T* __restrict__ src, int64_t src_rows, const T* __restrict__ extra,
                                                         T* __restrict__ dst)
{
    const int64_t e = (int64_t)blockIdx.x * DN_BLOCK + threadIdx.x;
    if (e >= total) return;
    // (a 32-bit division where the element index allows: the 64-bit one is a long instruction sequence)
    const int64_t row = total <= 0xffffffffll ? (int64_t)((uint32_t)e / (uint32_t)pieces) : e / pieces;
    const int piece = (int)(e - row * pieces);
    const int64_t m = map[row];
    T v = {};
    if (m >= 0) {
        if (m < src_rows) v = src[m * pieces + piece];
        else if (extra) v = extra[(m - src_rows) * pieces + piece];
    }
    dst[e] = v;
}

}  // namespace

extern "C" size_t gft_densify_plan_scratch_bytes(int64_t rows)
{
    const int64_t blocks = rows <= 0 ? 0 : (rows + RK_ROWS - 1) / RK_ROWS;
    return (size_t)(2 * blocks + 64) * sizeof(uint32_t);
}

extern "C" int gft_densify_classify(void* hip_stream, int64_t P, const float* grad_norm, const float* grad, const float* max_scaling,
                                    float max_grad, float dense_threshold, uint8_t* row_class, int32_t* clone_rows, int32_t* split_rows,
                                    void* scratch, int64_t* counts)
{
    if (!counts) return gft_fail("gft_densify_classify: counts is NULL");
    counts[0] = counts[1] = 0;
    if (P < 0 || P > 0x7fffffffll) return gft_fail("gft_densify_classify: bad row count");
    if (P == 0) return 0;
    if (!grad_norm || !grad || !max_scaling || !row_class || !clone_rows || !split_rows || !scratch)
        return gft_fail("gft_densify_classify: NULL argument");
    PlanClassify f;
    f.gnorm = grad_norm; f.g = grad; f.ms = max_scaling;
    f.max_grad = max_grad; f.dense_thr = dense_threshold;
    f.cls = row_class; f.clone_src = clone_rows; f.split_src = split_rows;
    return plan_rank((hipStream_t)hip_stream, f, P, scratch, counts);
}

extern "C" int gft_densify_layout(void* hip_stream, int64_t P, int64_t C, int64_t S, int32_t N, const uint8_t* row_class,
                                  const int32_t* clone_rows, const int32_t* split_rows, const float* opacity, const float* max_scaling,
                                  const float* child_max_scaling, float min_opacity, int32_t use_size, int32_t screen_dead,
                                  float big_threshold, float small_threshold, const float* seg, int32_t seg_cols, int32_t* source_row,
                                  uint8_t* kind, int32_t* child, int32_t* map_new, int32_t* map_state, uint8_t* motion_mask,
                                  int32_t* motion_rank, void* scratch, int64_t* counts)
{
    if (!counts) return gft_fail("gft_densify_layout: counts is NULL");
    counts[0] = counts[1] = 0;
    if (P < 0 || C < 0 || S < 0 || N < 1 || C > P || S > P) return gft_fail("gft_densify_layout: bad row counts");
    const int64_t V = P + C + (int64_t)N * S;
    if (V > 0x7fffffffll) return gft_fail("gft_densify_layout: more than 2^31 - 1 virtual rows");
    if (V == 0) return 0;
    if (!row_class || !opacity || !max_scaling || !source_row || !kind || !child || !map_new || !map_state || !scratch ||
        (C && !clone_rows) || (S && (!split_rows || (use_size && !child_max_scaling))))
        return gft_fail("gft_densify_layout: NULL argument");
    if (seg && (seg_cols < 1 || !motion_mask || !motion_rank)) return gft_fail("gft_densify_layout: seg without its outputs");
    PlanLayout f;
    f.P = P; f.C = C; f.S = S;
    f.cls = row_class; f.clone_src = clone_rows; f.split_src = split_rows;
    f.op = opacity; f.ms = max_scaling; f.child_ms = child_max_scaling;
    f.min_opacity = min_opacity; f.big_thr = big_threshold; f.small_thr = small_threshold;
    f.use_size = use_size != 0; f.screen_dead = screen_dead != 0;
    f.seg = seg; f.seg_cols = seg_cols;
    f.source_row = source_row; f.kind = kind; f.child = child; f.map_new = map_new; f.map_state = map_state;
    f.motion_mask = motion_mask; f.motion_rank = motion_rank;
    return plan_rank((hipStream_t)hip_stream, f, V, scratch, counts);
}

extern "C" int gft_rows_remap(void* hip_stream, int64_t n_out, const int32_t* map, const void* src, int64_t src_rows, const void* extra,
                              void* dst, int64_t row_bytes)
{
    if (n_out < 0 || row_bytes < 0 || src_rows < 0) return gft_fail("gft_rows_remap: negative size");
    if (row_bytes % 4) return gft_fail("gft_rows_remap: row_bytes must be a multiple of 4");
    if (n_out == 0 || row_bytes == 0) return 0;
    if (src_rows > 0x7fffffffll) return gft_fail("gft_rows_remap: too many source rows");
    if (!map || !dst || (src_rows && !src)) return gft_fail("gft_rows_remap: NULL argument");
    const uintptr_t all = (uintptr_t)src | (uintptr_t)extra | (uintptr_t)dst;
    if (all & 3) return gft_fail("gft_rows_remap: pointers must be 4-byte aligned");
    hipStream_t s = (hipStream_t)hip_stream;
    const bool wide = row_bytes % 16 == 0 && (all & 15) == 0;
    const int64_t pieces = row_bytes / (wide ? 16 : 4);
    const int64_t total = n_out * pieces;
    if (pieces > 0x7fffffffll || (total + DN_BLOCK - 1) / DN_BLOCK > 0x7fffffffll) return gft_fail("gft_rows_remap: too large");
    const dim3 grid((unsigned)((total + DN_BLOCK - 1) / DN_BLOCK));
    if (wide) hipLaunchKernelGGL(k_rows_remap<uint4>, grid, dim3(DN_BLOCK), 0, s, total, (int)pieces, map, (const uint4*)src, src_rows,
                                 (const uint4*)extra, (uint4*)dst);
    else hipLaunchKernelGGL(k_rows_remap<uint32_t>, grid, dim3(DN_BLOCK), 0, s, total, (int)pieces, map, (const uint32_t*)src, src_rows,
                            (const uint32_t*)extra, (uint32_t*)dst);
    GFT_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- the children of the split rows (scene/gaussian_model.py:577-581, utils/general_utils.py:91-112) -----------------------
// One thread per split row j: its quaternion, activated scaling and position are read once from the model's own tensors, R
// is built once, and the position of child k * S + j is written for k < N -- consecutive lanes write consecutive rows.  The
// arithmetic is stated in include/gftorf_densify.h: every operation rounded on its own as eager torch rounds it, the rotation
// of the sample as one explicit chain of fused multiply-adds.
namespace {

constexpr int SC_MAX_BLOCKS = 1 << 16;

__global__ __launch_bounds__(DN_BLOCK) void k_split_children(int64_t P, int64_t S, int N, const int32_t* __restrict__ split_rows,
                                                             const float* __restrict__ xyz, const float4* __restrict__ rotation,
                                                             const float* __restrict__ scaling, const float* __restrict__ z,
                                                             float* __restrict__ new_xyz)
{
#pragma clang fp contract(off)
    for (int64_t j = (int64_t)blockIdx.x * DN_BLOCK + threadIdx.x; j < S; j += (int64_t)gridDim.x * DN_BLOCK) {
        const int64_t row = split_rows[j];
        const bool ok = row >= 0 && row < P;                   // (a row outside the model is read nowhere: its children are NaN)
        const float nan = __int_as_float(0x7fc00000);
        const float4 r = ok ? rotation[row] : make_float4(nan, nan, nan, nan);
        const float px = ok ? xyz[3 * row] : nan, py = ok ? xyz[3 * row + 1] : nan, pz = ok ? xyz[3 * row + 2] : nan;
        const float sx = ok ? scaling[3 * row] : nan, sy = ok ? scaling[3 * row + 1] : nan, sz = ok ? scaling[3 * row + 2] : nan;
        // build_rotation: q = r / |r|, (w, x, y, z) = q
        const float norm = sqrtf(r.x * r.x + r.y * r.y + r.z * r.z + r.w * r.w);
        const float qw = r.x / norm, qx = r.y / norm, qy = r.z / norm, qz = r.w / norm;
        const float R00 = 1.0f - 2.0f * (qy * qy + qz * qz), R01 = 2.0f * (qx * qy - qw * qz), R02 = 2.0f * (qx * qz + qw * qy);
        const float R10 = 2.0f * (qx * qy + qw * qz), R11 = 1.0f - 2.0f * (qx * qx + qz * qz), R12 = 2.0f * (qy * qz - qw * qx);
        const float R20 = 2.0f * (qx * qz - qw * qy), R21 = 2.0f * (qy * qz + qw * qx), R22 = 1.0f - 2.0f * (qx * qx + qy * qy);
        for (int k = 0; k < N; k++) {
            const int64_t c = (int64_t)k * S + j;
            // torch.normal(mean = 0, std): normal_(0, 1) * std + mean
            const float s0 = z[3 * c] * sx + 0.0f, s1 = z[3 * c + 1] * sy + 0.0f, s2 = z[3 * c + 2] * sz + 0.0f;
            new_xyz[3 * c] = fmaf(R02, s2, fmaf(R01, s1, R00 * s0)) + px;
            new_xyz[3 * c + 1] = fmaf(R12, s2, fmaf(R11, s1, R10 * s0)) + py;
            new_xyz[3 * c + 2] = fmaf(R22, s2, fmaf(R21, s1, R20 * s0)) + pz;
        }
    }
}

}  // namespace

extern "C" int gft_split_children(void* hip_stream, int64_t P, int64_t S, int32_t N, const int32_t* split_rows, const float* xyz,
                                  const float* rotation, const float* scaling, const float* z, float* new_xyz)
{
    if (P < 0 || S < 0 || N < 1 || S > P) return gft_fail("gft_split_children: bad row counts (P %lld, S %lld, N %d)", (long long)P, (long long)S, (int)N);
    if ((int64_t)N * S > 0x7fffffffll) return gft_fail("gft_split_children: more than 2^31 - 1 children");
    if (S == 0) return 0;
    if (!split_rows || !xyz || !rotation || !scaling || !z || !new_xyz) return gft_fail("gft_split_children: NULL argument");
    if ((uintptr_t)rotation & 15) return gft_fail("gft_split_children: rotation must be 16-byte aligned");
    if (((uintptr_t)xyz | (uintptr_t)scaling | (uintptr_t)z | (uintptr_t)new_xyz | (uintptr_t)split_rows) & 3)
        return gft_fail("gft_split_children: pointers must be 4-byte aligned");
    const dim3 grid((unsigned)gft_grid_blocks(S, DN_BLOCK, 1, SC_MAX_BLOCKS));
    hipLaunchKernelGGL(k_split_children, grid, dim3(DN_BLOCK), 0, (hipStream_t)hip_stream, P, S, (int)N, split_rows, xyz,
                       (const float4*)rotation, scaling, z, new_xyz);
    return gft_launched("gft_split_children");
}
