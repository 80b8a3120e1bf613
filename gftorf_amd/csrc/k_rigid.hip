// k_rigid.hip -- the rigidity and isometry priors over a neighbour table, forward and backward (include/gftorf_rigid.h;
// the reference's utils/loss_utils.py:46-72).  The forward is a grid-stride loop over the P * K edges, summed in the two
// stages and the order of gft_reduce.h.  The backward runs one lane per point: its own K edges in the order of k, then the
// edges that name it, in the order the table's transpose stores them; every edge's term is recomputed from the positions,
// nothing per edge is kept between the two passes, and no atomic is used.  Scalar loads and vector stores only.
#include "gft_internal.h"
#include "gft_reduce.h"
#include "gftorf_rigid.h"

namespace {

constexpr int RIGID_THREADS = 256, RIGID_PER_THREAD = 4, RIGID_MAX_BLOCKS = 1024, RIGID_RESULT_WORDS = 4;

struct RigidArgs {
    int64_t P, E;                               // points, edges = P * K
    int K;
    const int32_t* __restrict__ idx;            // [P, K]
    const int32_t* __restrict__ offsets;        // [P + 1]  the transpose of idx
    const int32_t* __restrict__ edges;          // [E]
    const float* __restrict__ w;                // [P, K]
    const float* __restrict__ prev;             // [P, 3], NULL: no rigidity term
    const float* __restrict__ curr;             // [P, 3]
    const float* __restrict__ d0;               // [P, K], NULL: no isometry term
    const float* __restrict__ weights_dev;
    float wt[2];
    uint32_t* partials;                         // [blocks][GFT_RIGID_PARTIAL_WORDS]
    uint32_t* result;                           // [RIGID_RESULT_WORDS]
    int blocks;
    const float* __restrict__ g;                // device, one float
    float* g_curr;
    float* g_prev;
};

struct Vec3 { float x, y, z; };

__device__ __forceinline__ Vec3 load3(const float* __restrict__ a, int64_t r) { return {a[3 * r], a[3 * r + 1], a[3 * r + 2]}; }
__device__ __forceinline__ Vec3 sub3(const Vec3& a, const Vec3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float norm3(const Vec3& v) { return sqrtf(v.x * v.x + v.y * v.y + v.z * v.z + 1e-16f); }

__global__ __launch_bounds__(RIGID_THREADS) void k_rigid_fwd(RigidArgs p)
{
    __shared__ float sRed[2][RIGID_THREADS / 64];
    float s[2] = {0.f, 0.f};
    for (int64_t e = (int64_t)blockIdx.x * RIGID_THREADS + threadIdx.x; e < p.E; e += (int64_t)gridDim.x * RIGID_THREADS) {
        const int64_t i = e / p.K, j = p.idx[e];
        const float w = p.w[e];
        const Vec3 u = sub3(load3(p.curr, i), load3(p.curr, j));
        if (p.prev) s[0] += w * norm3(sub3(sub3(load3(p.prev, i), load3(p.prev, j)), u));     // loss_utils.py:59
        if (p.d0) s[1] += fabsf(w * (sqrtf(p.d0[e] + 1e-16f) - norm3(u)));                    // :72
    }
    gft_fold_store<RIGID_THREADS>(s, sRed);
    __syncthreads();
    if (threadIdx.x < GFT_RIGID_PARTIAL_WORDS)
        p.partials[(size_t)blockIdx.x * GFT_RIGID_PARTIAL_WORDS + threadIdx.x] = __float_as_uint(gft_waves_total<RIGID_THREADS>(sRed[threadIdx.x]));
}

// one workgroup: the rows of partials in a fixed order, in double; then the result block
__global__ __launch_bounds__(RIGID_THREADS) void k_rigid_finish(RigidArgs p)
{
    __shared__ double sSum[2][RIGID_THREADS];
    const int tid = threadIdx.x;
    double s[2] = {0.0, 0.0};
    for (int b = tid; b < p.blocks; b += RIGID_THREADS) {
        s[0] += (double)__uint_as_float(p.partials[(size_t)b * GFT_RIGID_PARTIAL_WORDS]);
        s[1] += (double)__uint_as_float(p.partials[(size_t)b * GFT_RIGID_PARTIAL_WORDS + 1]);
    }
    sSum[0][tid] = s[0];
    sSum[1][tid] = s[1];
    gft_tree_sum<RIGID_THREADS>(sSum);
    if (tid != 0) return;
    double total = 0.0;
    for (int k = 0; k < 2; k++) {
        const double mean = sSum[k][0] / (double)p.E;
        total += (double)(p.weights_dev ? p.weights_dev[k] : p.wt[k]) * mean;
        p.result[GFT_RIGID_MEANS + k] = __float_as_uint((float)mean);
    }
    p.result[GFT_RIGID_TOTAL] = __float_as_uint((float)total);
    p.result[GFT_RIGID_TOTAL + 1] = 0u;
}

// The gradient of edge e = (m -> j) with respect to the positions of m; those of j are its negatives.  rig: d / d prev_m
// (d / d curr_m is its negative); iso: d / d curr_m.  fp32 terms of a few roundings each.
__device__ __forceinline__ void edge_terms(const RigidArgs& p, int64_t e, const Vec3& prev_m, const Vec3& curr_m, const Vec3& prev_j,
                                           const Vec3& curr_j, float c_rig, float c_iso, Vec3& rig, Vec3& iso)
{
    const float w = p.w[e];
    const Vec3 u = sub3(curr_m, curr_j);
    rig = {0.f, 0.f, 0.f};
    iso = {0.f, 0.f, 0.f};
    if (p.prev) {
        const Vec3 v = sub3(sub3(prev_m, prev_j), u);
        const float f = c_rig * w / norm3(v);
        rig = {f * v.x, f * v.y, f * v.z};
    }
    if (p.d0) {
        const float r = norm3(u);
        const float f = -c_iso * w * sign_of(w * (sqrtf(p.d0[e] + 1e-16f) - r)) / r;           // torch's abs: 0 at 0
        iso = {f * u.x, f * u.y, f * u.z};
    }
}

// One lane per point.  The sums are kept in double (their order is fixed either way; in double the sum adds no rounding of
// its own to the terms').  The loads of an edge depend on its index load: the pass is bound by those dependent 12-byte
// gathers, the unrolling keeps four edges' loads in flight.
__global__ __launch_bounds__(RIGID_THREADS) void k_rigid_bwd(RigidArgs p)
{
    const int64_t i = (int64_t)blockIdx.x * RIGID_THREADS + threadIdx.x;
    if (i >= p.P) return;
    const double g = (double)*p.g, inv = 1.0 / (double)p.E;
    const float c_rig = p.prev ? (float)(g * (double)(p.weights_dev ? p.weights_dev[0] : p.wt[0]) * inv) : 0.f;
    const float c_iso = p.d0 ? (float)(g * (double)(p.weights_dev ? p.weights_dev[1] : p.wt[1]) * inv) : 0.f;
    const Vec3 zero = {0.f, 0.f, 0.f};
    const Vec3 curr_i = load3(p.curr, i), prev_i = p.prev ? load3(p.prev, i) : zero;
    double ar[3] = {0.0, 0.0, 0.0}, ai[3] = {0.0, 0.0, 0.0};
#pragma unroll 4
    for (int k = 0; k < p.K; k++) {                             // edges i -> j
        const int64_t e = i * p.K + k, j = p.idx[e];
        Vec3 rig, iso;
        edge_terms(p, e, prev_i, curr_i, p.prev ? load3(p.prev, j) : zero, load3(p.curr, j), c_rig, c_iso, rig, iso);
        ar[0] += (double)rig.x; ar[1] += (double)rig.y; ar[2] += (double)rig.z;
        ai[0] += (double)iso.x; ai[1] += (double)iso.y; ai[2] += (double)iso.z;
    }
    const int first = p.offsets[i], last = p.offsets[i + 1];
#pragma unroll 4
    for (int t = first; t < last; t++) {                        // edges m -> i
        const int64_t e = p.edges[t], m = e / p.K;
        Vec3 rig, iso;
        edge_terms(p, e, p.prev ? load3(p.prev, m) : zero, load3(p.curr, m), prev_i, curr_i, c_rig, c_iso, rig, iso);
        ar[0] -= (double)rig.x; ar[1] -= (double)rig.y; ar[2] -= (double)rig.z;
        ai[0] -= (double)iso.x; ai[1] -= (double)iso.y; ai[2] -= (double)iso.z;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (p.g_curr) p.g_curr[3 * i + c] = (float)(ai[c] - ar[c]);
        if (p.g_prev) p.g_prev[3 * i + c] = (float)ar[c];
    }
}

int fill(RigidArgs& p, int64_t P, int32_t K, const int32_t* idx, const float* w, const float* prev, const float* curr, const float* d0,
         const float* weights_dev, float w_rigid, float w_iso, const char* who)
{
    if (P < 1 || K < 1) return gft_fail("%s: bad sizes P=%lld K=%d", who, (long long)P, K);
    if (P * (int64_t)K > 0x7fffffffll) return gft_fail("%s: P * K = %lld is too large", who, (long long)(P * (int64_t)K));
    if (!idx || !w || !curr) return gft_fail("%s: idx, w or curr is NULL", who);
    if (!prev && !d0) return gft_fail("%s: no term is given (prev and d0 are both NULL)", who);
    p.P = P; p.K = K; p.E = P * (int64_t)K;
    p.idx = idx; p.w = w; p.prev = prev; p.curr = curr; p.d0 = d0;
    p.weights_dev = weights_dev;
    p.wt[0] = w_rigid; p.wt[1] = w_iso;
    return 0;
}

}  // namespace

extern "C" int64_t gft_rigid_blocks(int64_t P, int32_t K)
{
    if (P < 1 || K < 1) return 0;
    return gft_grid_blocks(P * (int64_t)K, RIGID_THREADS, RIGID_PER_THREAD, RIGID_MAX_BLOCKS);
}

extern "C" int64_t gft_rigid_result_words(void) { return RIGID_RESULT_WORDS; }

extern "C" int gft_rigid_forward(void* hip_stream, int64_t P, int32_t K, const int32_t* idx, const float* w, const float* prev,
                                 const float* curr, const float* d0, const float* weights_dev, float w_rigid, float w_iso,
                                 void* partials, void* result)
{
    RigidArgs p = {};
    if (fill(p, P, K, idx, w, prev, curr, d0, weights_dev, w_rigid, w_iso, "gft_rigid_forward")) return 1;
    if (!partials || !result) return gft_fail("gft_rigid_forward: partials or result is NULL");
    p.partials = static_cast<uint32_t*>(partials);
    p.result = static_cast<uint32_t*>(result);
    p.blocks = (int)gft_rigid_blocks(P, K);
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(k_rigid_fwd, dim3(p.blocks), dim3(RIGID_THREADS), 0, s, p);
    hipLaunchKernelGGL(k_rigid_finish, dim3(1), dim3(RIGID_THREADS), 0, s, p);
    return gft_launched("gft_rigid_forward");
}

extern "C" int gft_rigid_backward(void* hip_stream, int64_t P, int32_t K, const int32_t* idx, const int32_t* offsets,
                                  const int32_t* edges, const float* w, const float* prev, const float* curr, const float* d0,
                                  const float* weights_dev, float w_rigid, float w_iso, const float* g_loss, float* g_curr,
                                  float* g_prev)
{
    RigidArgs p = {};
    if (fill(p, P, K, idx, w, prev, curr, d0, weights_dev, w_rigid, w_iso, "gft_rigid_backward")) return 1;
    if (!offsets || !edges || !g_loss) return gft_fail("gft_rigid_backward: offsets, edges or g_loss is NULL");
    if (!g_curr && !g_prev) return 0;
    if (g_prev && !prev) return gft_fail("gft_rigid_backward: g_prev without prev");
    p.offsets = offsets; p.edges = edges;
    p.g = g_loss; p.g_curr = g_curr; p.g_prev = g_prev;
    const unsigned blocks = (unsigned)((P + RIGID_THREADS - 1) / RIGID_THREADS);
    hipLaunchKernelGGL(k_rigid_bwd, dim3(blocks), dim3(RIGID_THREADS), 0, (hipStream_t)hip_stream, p);
    return gft_launched("gft_rigid_backward");
}
