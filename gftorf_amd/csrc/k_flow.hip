// k_flow.hip -- the F-ToRF scene-flow term, forward and backward, one launch each (include/gftorf_flow.h;
// scene/torf_utils.py:80-124 as train.py:243-261 composes it), and the drop-ins distance_to_points3d / project_points /
// project_flow through the same device helpers.  A grid-stride loop over the H*W pixels; stage one of gft_reduce.h gives one
// partial per workgroup and direction.
// Every camera matrix is read on the device at kernel entry; the 4x4 inverse is formed there, by every lane, in double.
#include "gft_internal.h"
#include "gft_reduce.h"
#include "gftorf_flow.h"

namespace {

// One pixel per thread up to FLOW_MAX_BLOCKS workgroups: the per-pixel work is a few dependent loads, so the latency of one
// iteration, not bandwidth, bounds a launch at the reference's 320x240.
constexpr int FLOW_THREADS = 256, FLOW_PER_THREAD = 1, FLOW_MAX_BLOCKS = 1024;
constexpr float FLOW_EPS = 1e-7f;       // project_points' xy / (z + 1e-7): no clamp, no sign guard

int flow_blocks(int64_t pixels) { return (int)gft_grid_blocks(pixels, FLOW_THREADS, FLOW_PER_THREAD, FLOW_MAX_BLOCKS); }

struct FlowArgs {
    int W, HW;
    const float* __restrict__ depth;                            // [1, H, W]
    const float* __restrict__ K;                                // colour intrinsics [3, 3]
    const float* __restrict__ w2v;                              // world_view_transform [4, 4]
    const float* __restrict__ K_tof;
    const float* __restrict__ w2v_tof;
    const float* __restrict__ flow[2];                          // [3, H, W] per direction, or NULL
    const float* __restrict__ gt[2];                            // [2, H, W]
    const float* __restrict__ g[2];                             // upstream gradients (device, one float each) or NULL
    const float* __restrict__ points3d;                         // gft_flow_project*: [3, H, W]
    const float* __restrict__ points2d;                         // gft_flow_project: [2, H, W] or NULL
    const float* __restrict__ grad_out;                         // gft_flow_project_backward: [2, H, W]
    float scale;
    float* partials;                                            // [blocks][2]
    float* grad[2];                                             // [3, H, W] per direction, or NULL
    float* out3d;                                               // [3, H, W]
    float* out2d;                                               // [2, H, W]
};

// The colour camera: intrinsics and rows 0..2 of inverse(world_view_transform).
struct ColourCam {
    float fx, fy, cx, cy;
    float inv[3][4];
};

// The ToF camera: K_tof and rows 0..2 of world_view_transform_tof^T (v[i][j] = w2v_tof[j][i]).
struct TofCam {
    float k[3][3];
    float v[3][4];
};

// inverse(m), m row-major 4x4, through the adjugate in double: rows 0..2 rounded to float.  Every lane computes the same.
__device__ __forceinline__ void inverse_rows(const float* __restrict__ mf, float (*inv)[4])
{
    double m[16];
#pragma unroll
    for (int k = 0; k < 16; k++) m[k] = (double)mf[k];
    double a[16];
    a[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    a[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    a[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    a[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    a[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    a[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    a[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    a[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    a[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    a[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    a[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    a[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    a[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    const double r = 1.0 / (m[0] * a[0] + m[1] * a[4] + m[2] * a[8] + m[3] * a[12]);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) inv[i][j] = (float)(a[i * 4 + j] * r);
}

__device__ __forceinline__ ColourCam load_colour(const float* __restrict__ K, const float* __restrict__ w2v)
{
    ColourCam c;
    c.fx = K[0]; c.fy = K[4]; c.cx = K[2]; c.cy = K[5];
    inverse_rows(w2v, c.inv);
    return c;
}

__device__ __forceinline__ TofCam load_tof(const float* __restrict__ K, const float* __restrict__ w2v)
{
    TofCam c;
#pragma unroll
    for (int k = 0; k < 9; k++) c.k[k / 3][k % 3] = K[k];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) c.v[i][j] = w2v[j * 4 + i];
    return c;
}

// distance_to_points3d at pixel (u, v) = (column, row)
__device__ __forceinline__ float3 unproject(const ColourCam& c, float d, int u, int v)
{
    const float uc = (float)u - c.cx, vc = (float)v - c.cy;
    const float a = uc / c.fx, b = vc / c.fy;
    const float z = d / sqrtf(a * a + b * b + 1.f);
    const float x = uc * z / c.fx, y = vc * z / c.fy;
    float r[3];
#pragma unroll
    for (int i = 0; i < 3; i++) r[i] = c.inv[i][0] * x + c.inv[i][1] * y + c.inv[i][2] * z + c.inv[i][3];
    return make_float3(r[0], r[1], r[2]);
}

// K_tof @ (world_view_transform_tof^T @ [p, 1])[:3]
__device__ __forceinline__ float3 to_tof(const TofCam& c, float3 p)
{
    float e[3], q[3];
#pragma unroll
    for (int i = 0; i < 3; i++) e[i] = c.v[i][0] * p.x + c.v[i][1] * p.y + c.v[i][2] * p.z + c.v[i][3];
#pragma unroll
    for (int i = 0; i < 3; i++) q[i] = c.k[i][0] * e[0] + c.k[i][1] * e[1] + c.k[i][2] * e[2];
    return make_float3(q[0], q[1], q[2]);
}

__device__ __forceinline__ float2 project(const TofCam& c, float3 p)
{
    const float3 q = to_tof(c, p);
    const float w = q.z + FLOW_EPS;
    return make_float2(q.x / w, q.y / w);
}

// d(r . project(p)) / dp: the transposed Jacobian of xy / (z + 1e-7) at p, through K_tof and the view rotation
__device__ __forceinline__ float3 project_vjp(const TofCam& c, float3 p, float r0, float r1)
{
    const float3 q = to_tof(c, p);
    const float w = q.z + FLOW_EPS;
    const float t[3] = {r0 / w, r1 / w, -(r0 * (q.x / w) + r1 * (q.y / w)) / w};
    float e[3], g[3];
#pragma unroll
    for (int j = 0; j < 3; j++) e[j] = c.k[0][j] * t[0] + c.k[1][j] * t[1] + c.k[2][j] * t[2];
#pragma unroll
    for (int j = 0; j < 3; j++) g[j] = c.v[0][j] * e[0] + c.v[1][j] * e[1] + c.v[2][j] * e[2];
    return make_float3(g[0], g[1], g[2]);
}

__device__ __forceinline__ float3 load3(const float* __restrict__ f, int HW, int i)
{
    return make_float3(f[i], f[HW + i], f[2 * HW + i]);
}

__device__ __forceinline__ float3 add3(float3 a, float3 b) { return make_float3(a.x + b.x, a.y + b.y, a.z + b.z); }

__global__ __launch_bounds__(FLOW_THREADS) void k_flow_fwd(FlowArgs p)
{
    __shared__ float sRed[2][FLOW_THREADS / 64];
    const ColourCam cc = load_colour(p.K, p.w2v);
    const TofCam tc = load_tof(p.K_tof, p.w2v_tof);
    float s[2] = {0.f, 0.f};
    for (int i = blockIdx.x * FLOW_THREADS + threadIdx.x; i < p.HW; i += gridDim.x * FLOW_THREADS) {
        const int v = i / p.W, u = i - v * p.W;
        const float3 pc = unproject(cc, p.depth[i], u, v);
        const float2 qc = project(tc, pc);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            if (!p.flow[k]) continue;
            const float2 qn = project(tc, add3(pc, load3(p.flow[k], p.HW, i)));
            const float ex = (qn.x - qc.x) - p.gt[k][i], ey = (qn.y - qc.y) - p.gt[k][p.HW + i];
            s[k] += ex * ex + ey * ey;
        }
    }
    gft_fold_store<FLOW_THREADS>(s, sRed);
    __syncthreads();
    if (threadIdx.x < 2) p.partials[blockIdx.x * 2 + threadIdx.x] = gft_waves_total<FLOW_THREADS>(sRed[threadIdx.x]) * p.scale;
}

__global__ __launch_bounds__(FLOW_THREADS) void k_flow_bwd(FlowArgs p)
{
    const ColourCam cc = load_colour(p.K, p.w2v);
    const TofCam tc = load_tof(p.K_tof, p.w2v_tof);
    float g[2];
#pragma unroll
    for (int k = 0; k < 2; k++) g[k] = p.g[k] ? 2.f * (*p.g[k] * p.scale) : 0.f;       // d(e^2)/de = 2e
    for (int i = blockIdx.x * FLOW_THREADS + threadIdx.x; i < p.HW; i += gridDim.x * FLOW_THREADS) {
        const int v = i / p.W, u = i - v * p.W;
        const float3 pc = unproject(cc, p.depth[i], u, v);
        const float2 qc = project(tc, pc);
#pragma unroll
        for (int k = 0; k < 2; k++) {
            if (!p.grad[k]) continue;
            const float3 pn = add3(pc, load3(p.flow[k], p.HW, i));
            const float2 qn = project(tc, pn);
            const float ex = (qn.x - qc.x) - p.gt[k][i], ey = (qn.y - qc.y) - p.gt[k][p.HW + i];
            const float3 d = project_vjp(tc, pn, g[k] * ex, g[k] * ey);
            p.grad[k][i] = d.x; p.grad[k][p.HW + i] = d.y; p.grad[k][2 * p.HW + i] = d.z;
        }
    }
}

__global__ __launch_bounds__(FLOW_THREADS) void k_flow_points(FlowArgs p)
{
    const ColourCam cc = load_colour(p.K, p.w2v);
    TofCam tc = {};
    if (p.out2d) tc = load_tof(p.K_tof, p.w2v_tof);
    for (int i = blockIdx.x * FLOW_THREADS + threadIdx.x; i < p.HW; i += gridDim.x * FLOW_THREADS) {
        const int v = i / p.W, u = i - v * p.W;
        const float3 pc = unproject(cc, p.depth[i], u, v);
        if (p.out3d) { p.out3d[i] = pc.x; p.out3d[p.HW + i] = pc.y; p.out3d[2 * p.HW + i] = pc.z; }
        if (p.out2d) {
            const float2 q = project(tc, pc);
            p.out2d[i] = q.x; p.out2d[p.HW + i] = q.y;
        }
    }
}

__global__ __launch_bounds__(FLOW_THREADS) void k_flow_project(FlowArgs p)
{
    const TofCam tc = load_tof(p.K_tof, p.w2v_tof);
    for (int i = blockIdx.x * FLOW_THREADS + threadIdx.x; i < p.HW; i += gridDim.x * FLOW_THREADS) {
        float3 pn = load3(p.points3d, p.HW, i);
        if (p.flow[0]) pn = add3(pn, load3(p.flow[0], p.HW, i));
        float2 q = project(tc, pn);
        if (p.points2d) { q.x = q.x - p.points2d[i]; q.y = q.y - p.points2d[p.HW + i]; }
        p.out2d[i] = q.x; p.out2d[p.HW + i] = q.y;
    }
}

__global__ __launch_bounds__(FLOW_THREADS) void k_flow_project_bwd(FlowArgs p)
{
    const TofCam tc = load_tof(p.K_tof, p.w2v_tof);
    for (int i = blockIdx.x * FLOW_THREADS + threadIdx.x; i < p.HW; i += gridDim.x * FLOW_THREADS) {
        float3 pn = load3(p.points3d, p.HW, i);
        if (p.flow[0]) pn = add3(pn, load3(p.flow[0], p.HW, i));
        const float3 d = project_vjp(tc, pn, p.grad_out[i], p.grad_out[p.HW + i]);
        p.grad[0][i] = d.x; p.grad[0][p.HW + i] = d.y; p.grad[0][2 * p.HW + i] = d.z;
    }
}

// sizes: the pixel index runs in int
int flow_sizes(FlowArgs& p, int32_t H, int32_t W, const char* who)
{
    if (H <= 0 || W <= 0 || (int64_t)H * W > INT32_MAX - FLOW_THREADS * FLOW_MAX_BLOCKS)
        return gft_fail("%s: bad sizes H=%d W=%d", who, H, W);
    p.W = W; p.HW = H * W;
    return 0;
}

}  // namespace

extern "C" int64_t gft_flow_loss_blocks(int32_t H, int32_t W)
{
    if (H <= 0 || W <= 0) return 0;
    return flow_blocks((int64_t)H * W);
}

extern "C" int gft_flow_loss_forward(void* hip_stream, int32_t H, int32_t W, const float* depth, const float* K,
                                     const float* w2v, const float* K_tof, const float* w2v_tof, const float* flow3d_fwd,
                                     const float* gt_fwd, const float* flow3d_bwd, const float* gt_bwd, float scale,
                                     float* partials)
{
    const char* who = "gft_flow_loss_forward";
    FlowArgs p = {};
    if (flow_sizes(p, H, W, who)) return 1;
    if (!depth || !K || !w2v || !K_tof || !w2v_tof || !partials) return gft_fail("%s: NULL argument", who);
    if ((flow3d_fwd && !gt_fwd) || (flow3d_bwd && !gt_bwd)) return gft_fail("%s: a flow direction without its gt", who);
    p.depth = depth; p.K = K; p.w2v = w2v; p.K_tof = K_tof; p.w2v_tof = w2v_tof;
    p.flow[0] = flow3d_fwd; p.flow[1] = flow3d_bwd; p.gt[0] = gt_fwd; p.gt[1] = gt_bwd;
    p.scale = scale; p.partials = partials;
    hipLaunchKernelGGL(k_flow_fwd, dim3(flow_blocks(p.HW)), dim3(FLOW_THREADS), 0, (hipStream_t)hip_stream, p);
    return gft_launched(who);
}

extern "C" int gft_flow_loss_backward(void* hip_stream, int32_t H, int32_t W, const float* depth, const float* K,
                                      const float* w2v, const float* K_tof, const float* w2v_tof, const float* flow3d_fwd,
                                      const float* gt_fwd, const float* flow3d_bwd, const float* gt_bwd, const float* g_fwd,
                                      const float* g_bwd, float scale, float* grad_fwd, float* grad_bwd)
{
    const char* who = "gft_flow_loss_backward";
    FlowArgs p = {};
    if (flow_sizes(p, H, W, who)) return 1;
    if (!depth || !K || !w2v || !K_tof || !w2v_tof) return gft_fail("%s: NULL argument", who);
    if ((flow3d_fwd && !gt_fwd) || (flow3d_bwd && !gt_bwd)) return gft_fail("%s: a flow direction without its gt", who);
    p.depth = depth; p.K = K; p.w2v = w2v; p.K_tof = K_tof; p.w2v_tof = w2v_tof;
    p.flow[0] = flow3d_fwd; p.flow[1] = flow3d_bwd; p.gt[0] = gt_fwd; p.gt[1] = gt_bwd;
    p.g[0] = g_fwd; p.g[1] = g_bwd; p.scale = scale;
    p.grad[0] = flow3d_fwd ? grad_fwd : nullptr; p.grad[1] = flow3d_bwd ? grad_bwd : nullptr;
    if (!p.grad[0] && !p.grad[1]) return 0;
    hipLaunchKernelGGL(k_flow_bwd, dim3(flow_blocks(p.HW)), dim3(FLOW_THREADS), 0, (hipStream_t)hip_stream, p);
    return gft_launched(who);
}

extern "C" int gft_flow_points(void* hip_stream, int32_t H, int32_t W, const float* depth, const float* K, const float* w2v,
                               const float* K_tof, const float* w2v_tof, float* points3d, float* points2d)
{
    const char* who = "gft_flow_points";
    FlowArgs p = {};
    if (flow_sizes(p, H, W, who)) return 1;
    if (!depth || !K || !w2v || (!points3d && !points2d)) return gft_fail("%s: NULL argument", who);
    if (points2d && (!K_tof || !w2v_tof)) return gft_fail("%s: points2d needs K_tof and w2v_tof", who);
    p.depth = depth; p.K = K; p.w2v = w2v; p.K_tof = K_tof; p.w2v_tof = w2v_tof; p.out3d = points3d; p.out2d = points2d;
    hipLaunchKernelGGL(k_flow_points, dim3(flow_blocks(p.HW)), dim3(FLOW_THREADS), 0, (hipStream_t)hip_stream, p);
    return gft_launched(who);
}

extern "C" int gft_flow_project(void* hip_stream, int32_t H, int32_t W, const float* K_tof, const float* w2v_tof,
                                const float* points3d, const float* flow3d, const float* points2d_curr, float* out)
{
    const char* who = "gft_flow_project";
    FlowArgs p = {};
    if (flow_sizes(p, H, W, who)) return 1;
    if (!K_tof || !w2v_tof || !points3d || !out) return gft_fail("%s: NULL argument", who);
    p.K_tof = K_tof; p.w2v_tof = w2v_tof; p.points3d = points3d; p.flow[0] = flow3d; p.points2d = points2d_curr; p.out2d = out;
    hipLaunchKernelGGL(k_flow_project, dim3(flow_blocks(p.HW)), dim3(FLOW_THREADS), 0, (hipStream_t)hip_stream, p);
    return gft_launched(who);
}

extern "C" int gft_flow_project_backward(void* hip_stream, int32_t H, int32_t W, const float* K_tof, const float* w2v_tof,
                                         const float* points3d, const float* flow3d, const float* grad_out, float* grad_flow3d)
{
    const char* who = "gft_flow_project_backward";
    FlowArgs p = {};
    if (flow_sizes(p, H, W, who)) return 1;
    if (!K_tof || !w2v_tof || !points3d || !grad_out || !grad_flow3d) return gft_fail("%s: NULL argument", who);
    p.K_tof = K_tof; p.w2v_tof = w2v_tof; p.points3d = points3d; p.flow[0] = flow3d; p.grad_out = grad_out;
    p.grad[0] = grad_flow3d;
    hipLaunchKernelGGL(k_flow_project_bwd, dim3(flow_blocks(p.HW)), dim3(FLOW_THREADS), 0, (hipStream_t)hip_stream, p);
    return gft_launched(who);
}
