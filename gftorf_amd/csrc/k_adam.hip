// k_adam.hip -- fused Adam step (gfx950): one pass, 16-byte accesses, HBM-bound (28 B per element).
// Arithmetic of torch/optim/adam.py `_single_tensor_adam` (no amsgrad / maximize), which the
// reference's optimizer follows (scene/gaussian_model.py:274, train.py:470).
#include "gft_internal.h"
#include "gftorf_optim.h"

#include <cmath>

namespace {

#define ADAM_BLOCK 256
#define ADAM_ITEMS 2      // 16-byte groups per thread of the dense multi-tensor kernel: 8 loads of 16 B in flight per thread

struct AdamArgs {
    int64_t n;
    float* p; const float* g; float* m; float* v;
    float one_m_beta1, beta2, one_m_beta2, step_size, bias2_sqrt, eps, weight_decay;
    float grad_scale;     // the clip coefficient (gft_grad_norm's out[1]); 1 when the caller gave none: g * 1 is g, bit for bit
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamArgs& a)
{
#pragma clang fp contract(off)
    g = g * a.grad_scale;                                     // clip_grad_norm_: grad.mul_(clip_coef_clamped), rounded on its own
    if (a.weight_decay != 0.f) g = g + a.weight_decay * p;
    m = m + a.one_m_beta1 * (g - m);                          // exp_avg.lerp_(grad, 1 - beta1)
    v = v * a.beta2 + (a.one_m_beta2 * g) * g;                // mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / a.bias2_sqrt + a.eps;
    p = p + (-a.step_size) * (m / denom);                     // addcdiv_(exp_avg, denom, value=-step_size)
}

// Several tensors in ONE launch (own learning rate and step count each; betas, eps, weight decay shared): the
// reference's optimizers hold 13 one-tensor groups of per-Gaussian parameters and the 36 tensors of the deformation
// network; at 100 k Gaussians a launch per tensor is bound by launch latency, not by HBM.  Workgroup b serves the
// tensor whose block range holds b (table in the kernel arguments).
struct AdamMultiArgs {
    int count;
    float one_m_beta1, beta2, one_m_beta2, eps, weight_decay;
    struct T { float* p; const float* g; float* m; float* v; int64_t n; float step_size, bias2_sqrt; uint32_t first_block; uint32_t pad; } t[GFT_ADAM_MAX_TENSORS];
};

// Learning rates and step counts on the device (gft_adam_step with lr / step / factors): one workgroup, thread c advances step[c] and leaves
// the two derived factors of tensor c where the update kernel behind it reads them.
struct AdamTickArgs {
    int count;
    double beta1, beta2;
    float* factors;
    const double* lr[GFT_ADAM_MAX_TENSORS];
    float* step[GFT_ADAM_MAX_TENSORS];
};

__global__ __launch_bounds__(64) void k_adam_tick(AdamTickArgs a)
{
    const int c = threadIdx.x;
    if (c >= a.count) return;
    const float t = *a.step[c] + 1.0f;
    *a.step[c] = t;
    const double lr = *a.lr[c];
    // torch/optim/adam.py: step_size = lr / (1 - beta1 ** step); bias_correction2_sqrt = (1 - beta2 ** step) ** 0.5
    a.factors[2 * c] = (float)(lr / (1.0 - pow(a.beta1, (double)t)));
    a.factors[2 * c + 1] = (float)sqrt(1.0 - pow(a.beta2, (double)t));
}

struct AdamBlock { int k; uint32_t blk; };     // the tensor's index in the launch's table, the workgroup's index within the tensor

// The opening of both update kernels: the tensor whose block range holds this workgroup, and its arguments in `s`.
// dev: step size and bias correction are the factors k_adam_tick left for the tensor, not the table's.
__device__ __forceinline__ AdamBlock adam_args_of_block(const AdamMultiArgs& a, bool dev, const float* factors, const float* grad_scale,
                                                        AdamArgs& s)
{
    int k = 0;
#pragma unroll 1
    for (int q = 1; q < a.count; q++)
        if (blockIdx.x >= a.t[q].first_block) k = q;
    s.n = a.t[k].n; s.p = a.t[k].p; s.g = a.t[k].g; s.m = a.t[k].m; s.v = a.t[k].v;
    s.one_m_beta1 = a.one_m_beta1; s.beta2 = a.beta2; s.one_m_beta2 = a.one_m_beta2; s.step_size = a.t[k].step_size;
    s.bias2_sqrt = a.t[k].bias2_sqrt; s.eps = a.eps; s.weight_decay = a.weight_decay;
    s.grad_scale = grad_scale ? *grad_scale : 1.f;
    if (dev) {          // (t[k].pad: the tensor's index in the caller's table = its slot in `factors`)
        s.step_size = factors[2 * a.t[k].pad];
        s.bias2_sqrt = factors[2 * a.t[k].pad + 1];
    }
    return {k, blockIdx.x - a.t[k].first_block};
}

template <bool DEV>
__global__ __launch_bounds__(ADAM_BLOCK) void k_adam_multi(AdamMultiArgs a, const float* __restrict__ factors,
                                                           const float* __restrict__ grad_scale)
{
    AdamArgs s;
    const uint32_t blk = adam_args_of_block(a, DEV, factors, grad_scale, s).blk;
    const int64_t n4 = s.n >> 2;
    // ADAM_ITEMS 16-byte groups per thread, all their loads issued before the arithmetic (index clamped, the stores
    // predicated): one group per thread kept too few bytes in flight for the HBM rate (3.7 TB/s)
    float4 p[ADAM_ITEMS], g[ADAM_ITEMS], m[ADAM_ITEMS], v[ADAM_ITEMS];
    int64_t idx[ADAM_ITEMS];
#pragma unroll
    for (int u = 0; u < ADAM_ITEMS; u++) {
        idx[u] = ((int64_t)blk * ADAM_ITEMS + u) * ADAM_BLOCK + threadIdx.x;
        const int64_t i = n4 > 0 ? (idx[u] < n4 ? idx[u] : n4 - 1) : 0;
        if (n4 > 0) {
            p[u] = reinterpret_cast<float4*>(s.p)[i];
            g[u] = reinterpret_cast<const float4*>(s.g)[i];
            m[u] = reinterpret_cast<float4*>(s.m)[i];
            v[u] = reinterpret_cast<float4*>(s.v)[i];
        }
    }
#pragma unroll
    for (int u = 0; u < ADAM_ITEMS; u++) {
        if (idx[u] < n4) {
            adam_one(p[u].x, g[u].x, m[u].x, v[u].x, s);
            adam_one(p[u].y, g[u].y, m[u].y, v[u].y, s);
            adam_one(p[u].z, g[u].z, m[u].z, v[u].z, s);
            adam_one(p[u].w, g[u].w, m[u].w, v[u].w, s);
            reinterpret_cast<float4*>(s.p)[idx[u]] = p[u];
            reinterpret_cast<float4*>(s.m)[idx[u]] = m[u];
            reinterpret_cast<float4*>(s.v)[idx[u]] = v[u];
        }
    }
    const int64_t tail = s.n & 3;
    if (blk == 0 && (int64_t)threadIdx.x < tail) {
        const int64_t e = (n4 << 2) + threadIdx.x;
        float pe = s.p[e], me = s.m[e], ve = s.v[e];
        adam_one(pe, s.g[e], me, ve, s);
        s.p[e] = pe; s.m[e] = me; s.v[e] = ve;
    }
}

// The same launch for tensors whose rows are Gaussians, restricted to the rows of a mask (opt-in: FusedAdam.step(visibility=...);
// the reference's optimizer is dense): a 16-byte group none of whose elements lies in a masked row is neither read
// nor written -- with 14 % of the Gaussians on screen the step moves 14 % of the bytes.
struct AdamRowsArgs {
    AdamMultiArgs m;
    const uint8_t* row_mask;
    uint32_t row_floats[GFT_ADAM_MAX_TENSORS];
};

template <bool DEV>
__global__ __launch_bounds__(ADAM_BLOCK) void k_adam_rows(AdamRowsArgs a, const float* __restrict__ factors,
                                                          const float* __restrict__ grad_scale)
{
    AdamArgs s;
    const auto [k, blk] = adam_args_of_block(a.m, DEV, factors, grad_scale, s);
    const uint32_t rf = a.row_floats[k];
    const int64_t n4 = s.n >> 2;
    const int64_t i = (int64_t)blk * ADAM_BLOCK + threadIdx.x;
    if (i < n4) {
        const uint64_t e0 = (uint64_t)i << 2;
        uint64_t row = e0 / rf;
        uint32_t rem = (uint32_t)(e0 - row * rf);
        bool on[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            on[j] = a.row_mask[row] != 0;
            if (++rem == rf) { rem = 0; row++; }
        }
        if (on[0] | on[1] | on[2] | on[3]) {
            float4 p = reinterpret_cast<float4*>(s.p)[i];
            const float4 g = reinterpret_cast<const float4*>(s.g)[i];
            float4 m = reinterpret_cast<float4*>(s.m)[i];
            float4 v = reinterpret_cast<float4*>(s.v)[i];
            float4 p1 = p, m1 = m, v1 = v;
            adam_one(p1.x, g.x, m1.x, v1.x, s);
            adam_one(p1.y, g.y, m1.y, v1.y, s);
            adam_one(p1.z, g.z, m1.z, v1.z, s);
            adam_one(p1.w, g.w, m1.w, v1.w, s);
            if (on[0]) { p.x = p1.x; m.x = m1.x; v.x = v1.x; }
            if (on[1]) { p.y = p1.y; m.y = m1.y; v.y = v1.y; }
            if (on[2]) { p.z = p1.z; m.z = m1.z; v.z = v1.z; }
            if (on[3]) { p.w = p1.w; m.w = m1.w; v.w = v1.w; }
            reinterpret_cast<float4*>(s.p)[i] = p;
            reinterpret_cast<float4*>(s.m)[i] = m;
            reinterpret_cast<float4*>(s.v)[i] = v;
        }
    }
    const int64_t tail = s.n & 3;
    if (blk == 0 && (int64_t)threadIdx.x < tail) {
        const int64_t e = (n4 << 2) + threadIdx.x;
        if (a.row_mask[(uint64_t)e / rf]) {
            float p = s.p[e], m = s.m[e], v = s.v[e];
            adam_one(p, s.g[e], m, v, s);
            s.p[e] = p; s.m[e] = m; s.v[e] = v;
        }
    }
}

// ---- gradient-norm clipping (torch.nn.utils.clip_grad_norm_, reference train.py:468) --------------------------------------
// The global L2 norm of a set of gradient tensors, and the coefficient torch scales them by, left on the device for the Adam
// kernels above (or for k_grad_scale).  One launch per GFT_ADAM_MAX_TENSORS spans, table in the kernel arguments as in
// k_adam_multi; a span may start on any 4-byte boundary (the network's gradients are consecutive views of one buffer):
// up to three scalars in front of the first 16-byte boundary, 16-byte groups, up to three scalars behind them.
// No atomics and no counters: every workgroup stores ONE partial sum, a double, and a one-workgroup kernel adds the partials
// in a fixed order -- the same bits every call, and every word that is read was written by the same call.
#define NORM_BLOCK 256
#define NORM_ITEMS 4      // 16-byte groups per thread, all loaded before the arithmetic: 16 KB per workgroup

struct GradSpanArgs {
    int count;
    uint32_t first_partial;     // (norm) this launch's workgroup b writes partials[first_partial + b]
    struct T { float* g; int64_t n; uint32_t first_block; uint32_t head; } t[GFT_ADAM_MAX_TENSORS];
};

// sum of one double per thread over the workgroup, in a fixed order; the result is valid in thread 0
__device__ __forceinline__ double norm_block_sum(double d, double* lds)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_down(d, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = d;
    __syncthreads();
    return lds[0] + lds[1] + lds[2] + lds[3];
}

// The span walk of k_grad_norm_partial and k_grad_scale: the span whose block range holds this workgroup (its blk-th), as up to
// three scalars in front of the first 16-byte boundary (head), n4 16-byte groups (body) and up to three scalars behind them.
struct GradSpan { float* g; int64_t n; uint32_t head; uint32_t blk; float4* body; int64_t n4; };

__device__ __forceinline__ GradSpan grad_span_of_block(const GradSpanArgs& a)
{
    int k = 0;
#pragma unroll 1
    for (int q = 1; q < a.count; q++)
        if (blockIdx.x >= a.t[q].first_block) k = q;
    GradSpan s;
    s.g = a.t[k].g;
    s.n = a.t[k].n;
    s.head = a.t[k].head;
    s.blk = blockIdx.x - a.t[k].first_block;
    s.body = reinterpret_cast<float4*>(s.g + s.head);
    s.n4 = (s.n - s.head) >> 2;
    return s;
}

__global__ __launch_bounds__(NORM_BLOCK) void k_grad_norm_partial(GradSpanArgs a, double* __restrict__ partials)
{
    __shared__ double lds[NORM_BLOCK / 64];
    const auto [g, n, head, blk, body, n4] = grad_span_of_block(a);
    float4 x[NORM_ITEMS];
    int64_t idx[NORM_ITEMS];
#pragma unroll
    for (int u = 0; u < NORM_ITEMS; u++) {
        idx[u] = ((int64_t)blk * NORM_ITEMS + u) * NORM_BLOCK + threadIdx.x;
        if (n4 > 0) x[u] = body[idx[u] < n4 ? idx[u] : n4 - 1];
    }
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < NORM_ITEMS; u++)
        if (idx[u] < n4) s += x[u].x * x[u].x + x[u].y * x[u].y + x[u].z * x[u].z + x[u].w * x[u].w;
    if (blk == 0) {         // the scalars in front of and behind the 16-byte groups: at most three each
        const uint32_t tail = (uint32_t)((n - head) & 3);
        if (threadIdx.x < head) { const float e = g[threadIdx.x]; s += e * e; }
        else if (threadIdx.x < head + tail) { const float e = g[(n4 << 2) + threadIdx.x]; s += e * e; }
    }
    const double d = norm_block_sum((double)s, lds);
    if (threadIdx.x == 0) partials[a.first_partial + blockIdx.x] = d;
}

__global__ __launch_bounds__(NORM_BLOCK) void k_grad_norm_final(const double* __restrict__ partials, uint32_t count, float max_norm,
                                                                float* __restrict__ out)
{
#pragma clang fp contract(off)
    __shared__ double lds[NORM_BLOCK / 64];
    double d = 0.0;
    for (uint32_t i = threadIdx.x; i < count; i += NORM_BLOCK) d += partials[i];
    d = norm_block_sum(d, lds);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(d);
        // torch/nn/utils/clip_grad.py: clip_coef = max_norm / (total_norm + 1e-6) -- which Tensor.__rtruediv__ forms as
        // reciprocal() * max_norm, two fp32 roundings -- then clamp(max=1.0), which lets a NaN through
        float c = (1.0f / (norm + 1e-6f)) * max_norm;
        c = c > 1.0f ? 1.0f : c;
        out[0] = norm;
        out[1] = c;
    }
}

__global__ __launch_bounds__(NORM_BLOCK) void k_grad_scale(GradSpanArgs a, const float* __restrict__ coef)
{
    const float c = *coef;
    if (c == 1.0f) return;          // g * 1 is g: nothing to store
    const auto [g, n, head, blk, body, n4] = grad_span_of_block(a);
    float4 x[NORM_ITEMS];
    int64_t idx[NORM_ITEMS];
#pragma unroll
    for (int u = 0; u < NORM_ITEMS; u++) {
        idx[u] = ((int64_t)blk * NORM_ITEMS + u) * NORM_BLOCK + threadIdx.x;
        if (n4 > 0) x[u] = body[idx[u] < n4 ? idx[u] : n4 - 1];
    }
#pragma unroll
    for (int u = 0; u < NORM_ITEMS; u++)
        if (idx[u] < n4) body[idx[u]] = make_float4(x[u].x * c, x[u].y * c, x[u].z * c, x[u].w * c);
    if (blk == 0) {
        const uint32_t tail = (uint32_t)((n - head) & 3);
        if (threadIdx.x < head) g[threadIdx.x] *= c;
        else if (threadIdx.x < head + tail) g[(n4 << 2) + threadIdx.x] *= c;
    }
}

}  // namespace

// fills the span table of a launch from spans [c0 ...]; returns the number of entries (< 0: error)
static int span_table(GradSpanArgs& a, float* const* grads, const int64_t* n, int32_t c0, int32_t count, uint64_t* blocks_out,
                      const char* who)
{
    int k = 0;
    uint64_t blocks = 0;
    for (int32_t c = c0; c < count && c < c0 + GFT_ADAM_MAX_TENSORS; c++) {
        if (n[c] < 0) { gft_fail("%s: span %d has n < 0", who, c); return -1; }
        if (n[c] == 0) continue;
        if (!grads[c]) { gft_fail("%s: span %d has a NULL pointer", who, c); return -1; }
        if (((uintptr_t)grads[c] & 3) != 0) { gft_fail("%s: span %d is not 4-byte aligned", who, c); return -1; }
        int64_t head = (int64_t)(((16 - ((uintptr_t)grads[c] & 15)) & 15) >> 2);
        if (head > n[c]) head = n[c];
        a.t[k].g = grads[c]; a.t[k].n = n[c]; a.t[k].head = (uint32_t)head; a.t[k].first_block = (uint32_t)blocks;
        const int64_t n4 = (n[c] - head) >> 2;
        const int64_t per_block = (int64_t)NORM_BLOCK * NORM_ITEMS;
        blocks += n4 > 0 ? (uint64_t)((n4 + per_block - 1) / per_block) : 1;
        k++;
    }
    if (blocks > 0x7fffffffull) { gft_fail("%s: too many elements for one launch", who); return -1; }
    a.count = k;
    *blocks_out = blocks;
    return k;
}

extern "C" size_t gft_grad_norm_scratch_bytes(int64_t total_elements, int32_t count)
{
    if (total_elements < 0 || count < 0) return 0;
    // a span of n elements takes at most n / (4 * NORM_BLOCK * NORM_ITEMS) + 1 workgroups, each with one double
    return sizeof(double) * (size_t)(total_elements / (4 * NORM_BLOCK * NORM_ITEMS) + count + 1);
}

extern "C" int gft_grad_norm(void* hip_stream, int32_t count, const float* const* grads, const int64_t* n, double max_norm,
                             void* scratch, size_t scratch_bytes, float* out)
{
    if (count < 0) return gft_fail("gft_grad_norm: count < 0");
    if (count == 0 && !out) return 0;
    if (count > 0 && (!grads || !n)) return gft_fail("gft_grad_norm: the span table is NULL");
    if (!out) return gft_fail("gft_grad_norm: out is NULL");
    uint64_t partials = 0;
    // (a first pass over the tables: nothing is launched unless the whole call fits the scratch buffer)
    for (int pass = 0; pass < 2; pass++) {
        partials = 0;
        for (int32_t c0 = 0; c0 < count; c0 += GFT_ADAM_MAX_TENSORS) {
            GradSpanArgs a;
            uint64_t blocks = 0;
            const int k = span_table(a, const_cast<float* const*>(grads), n, c0, count, &blocks, "gft_grad_norm");
            if (k < 0) return 1;
            if (k == 0) continue;
            if (pass == 1) {
                a.first_partial = (uint32_t)partials;
                hipLaunchKernelGGL(k_grad_norm_partial, dim3((unsigned)blocks), dim3(NORM_BLOCK), 0, (hipStream_t)hip_stream, a, (double*)scratch);
            }
            partials += blocks;
        }
        if (pass == 0 && partials > 0) {
            if (partials > 0x7fffffffull) return gft_fail("gft_grad_norm: too many elements");
            if (!scratch || ((uintptr_t)scratch & 7) != 0 || partials * sizeof(double) > scratch_bytes)
                return gft_fail("gft_grad_norm: scratch is NULL, not 8-byte aligned or smaller than %llu bytes (gft_grad_norm_scratch_bytes)",
                                (unsigned long long)(partials * sizeof(double)));
        }
    }
    hipLaunchKernelGGL(k_grad_norm_final, dim3(1), dim3(NORM_BLOCK), 0, (hipStream_t)hip_stream, (const double*)scratch, (uint32_t)partials,
                       (float)max_norm, out);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return gft_fail("gft_grad_norm: %s", hipGetErrorString(e));
    return 0;
}

extern "C" int gft_grad_scale(void* hip_stream, int32_t count, float* const* grads, const int64_t* n, const float* coef)
{
    if (count < 0) return gft_fail("gft_grad_scale: count < 0");
    if (count == 0) return 0;
    if (!grads || !n) return gft_fail("gft_grad_scale: the span table is NULL");
    if (!coef) return gft_fail("gft_grad_scale: coef is NULL");
    for (int32_t c0 = 0; c0 < count; c0 += GFT_ADAM_MAX_TENSORS) {
        GradSpanArgs a;
        a.first_partial = 0;
        uint64_t blocks = 0;
        const int k = span_table(a, grads, n, c0, count, &blocks, "gft_grad_scale");
        if (k < 0) return 1;
        if (k == 0) continue;
        hipLaunchKernelGGL(k_grad_scale, dim3((unsigned)blocks), dim3(NORM_BLOCK), 0, (hipStream_t)hip_stream, a, coef);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return gft_fail("gft_grad_scale: %s", hipGetErrorString(e));
    }
    return 0;
}

// fills the per-tensor table of a launch from tensors[c0 ...]; returns the number of entries (< 0: error).  row_floats: the
// row-masked launch (every tensor has `rows` rows); dev: learning rates and step counts are on the device, the table's are not read
static int adam_table(AdamMultiArgs& a, const gft_adam_tensor* tensors, int32_t c0, int32_t count, double beta1, double beta2,
                      double eps, double weight_decay, uint64_t* blocks_out, int64_t rows, uint32_t* row_floats, bool dev)
{
    a.one_m_beta1 = (float)(1.0 - beta1);
    a.beta2 = (float)beta2;
    a.one_m_beta2 = (float)(1.0 - beta2);
    a.eps = (float)eps;
    a.weight_decay = (float)weight_decay;
    int k = 0;
    uint64_t blocks = 0;
    for (int32_t c = c0; c < count && c < c0 + GFT_ADAM_MAX_TENSORS; c++) {
        const gft_adam_tensor& t = tensors[c];
        if (t.n < 0) { gft_fail("gft_adam_step: tensor %d has n < 0", c); return -1; }
        if (t.n == 0) continue;
        if (!dev && t.step < 1) { gft_fail("gft_adam_step: tensor %d: step must be >= 1", c); return -1; }
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq) { gft_fail("gft_adam_step: tensor %d has a NULL pointer", c); return -1; }
        if ((((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq) & 15) != 0) {
            gft_fail("gft_adam_step: pointers of tensor %d are not 16-byte aligned", c);
            return -1;
        }
        if (row_floats) {
            if (t.n % rows != 0 || t.n / rows > 0xffffffffll) { gft_fail("gft_adam_step: tensor %d does not have %lld rows", c, (long long)rows); return -1; }
            row_floats[k] = (uint32_t)(t.n / rows);
        }
        a.t[k].p = t.param; a.t[k].g = t.grad; a.t[k].m = t.exp_avg; a.t[k].v = t.exp_avg_sq; a.t[k].n = t.n;
        // torch/optim/adam.py: bias_correction1 = 1 - beta1 ** step; step_size = lr / bias_correction1;
        // bias_correction2_sqrt = (1 - beta2 ** step) ** 0.5 -- Python floats, rounded when they meet a tensor
        a.t[k].step_size = dev ? 0.f : (float)(t.lr / (1.0 - pow(beta1, (double)t.step)));
        a.t[k].bias2_sqrt = dev ? 1.f : (float)sqrt(1.0 - pow(beta2, (double)t.step));
        a.t[k].first_block = (uint32_t)blocks; a.t[k].pad = (uint32_t)(c - c0);
        const int64_t n4 = t.n >> 2;
        const int64_t per_block = (int64_t)ADAM_BLOCK * (row_floats ? 1 : ADAM_ITEMS);       // 16-byte groups per workgroup
        blocks += n4 > 0 ? (uint64_t)((n4 + per_block - 1) / per_block) : 1;
        k++;
    }
    if (blocks > 0x7fffffffull) { gft_fail("gft_adam_step: too many elements for one launch"); return -1; }
    a.count = k;
    *blocks_out = blocks;
    return k;
}

// the tick in front of an update with device-side rates: the counts of tensors [c0, c1) advance, their factors are left in
// factors[2 c ...]
static int adam_tick(void* hip_stream, int32_t c0, int32_t c1, const double* const* lr, float* const* step, float* factors, double beta1,
                     double beta2)
{
    AdamTickArgs tick;
    tick.count = c1 - c0; tick.beta1 = beta1; tick.beta2 = beta2; tick.factors = factors + 2 * (size_t)c0;
    for (int32_t c = c0; c < c1; c++) {
        if (!lr[c] || !step[c]) return gft_fail("gft_adam_step: tensor %d: lr / step pointer is NULL", c);
        tick.lr[c - c0] = lr[c]; tick.step[c - c0] = step[c];
    }
    hipLaunchKernelGGL(k_adam_tick, dim3(1), dim3(64), 0, (hipStream_t)hip_stream, tick);
    return 0;
}

extern "C" int gft_adam_step(void* hip_stream, int32_t count, const gft_adam_tensor* tensors, int64_t rows, const uint8_t* row_mask,
                             const double* const* lr, float* const* step, float* factors, double beta1, double beta2, double eps,
                             double weight_decay, const float* grad_scale)
{
    const bool dev = lr || step || factors;
    if (count < 0) return gft_fail("gft_adam_step: count < 0");
    if (count == 0 || (row_mask && !dev && rows == 0)) return 0;
    if (!tensors) return gft_fail("gft_adam_step: tensors is NULL");
    if (dev && (!lr || !step || !factors)) return gft_fail("gft_adam_step: lr, step and factors go together, one of them is NULL");
    if (!row_mask && rows != 0) return gft_fail("gft_adam_step: bad argument (rows without a row_mask)");
    // (a mask without rows: under device-side rates there would be counts to advance and nothing to update -- such tensors belong
    // in a dense call)
    if (row_mask && dev && rows <= 0) return gft_fail("gft_adam_step: rows must be > 0");
    if (row_mask && rows < 0) return gft_fail("gft_adam_step: bad argument (rows < 0)");
    for (int32_t c0 = 0; c0 < count; c0 += GFT_ADAM_MAX_TENSORS) {
        const int32_t c1 = count < c0 + GFT_ADAM_MAX_TENSORS ? count : c0 + GFT_ADAM_MAX_TENSORS;
        AdamRowsArgs a;         // (a.m alone is the dense kernel's argument)
        a.row_mask = row_mask;
        uint64_t blocks = 0;
        const int k = adam_table(a.m, tensors, c0, count, beta1, beta2, eps, weight_decay, &blocks, rows, row_mask ? a.row_floats : nullptr, dev);
        if (k < 0) return 1;
        // (the counts advance for every tensor of the table, as torch's capturable Adam advances state["step"] -- also for an
        // empty tensor, which takes no update)
        if (dev && adam_tick(hip_stream, c0, c1, lr, step, factors, beta1, beta2)) return 1;
        if (k == 0 && !dev) continue;
        if (k > 0) {
            const dim3 grid((unsigned)blocks), block(ADAM_BLOCK);
            const hipStream_t s = (hipStream_t)hip_stream;
            const float* f = dev ? factors + 2 * (size_t)c0 : nullptr;
            if (row_mask && dev) hipLaunchKernelGGL(k_adam_rows<true>, grid, block, 0, s, a, f, grad_scale);
            else if (row_mask) hipLaunchKernelGGL(k_adam_rows<false>, grid, block, 0, s, a, f, grad_scale);
            else if (dev) hipLaunchKernelGGL(k_adam_multi<true>, grid, block, 0, s, a.m, f, grad_scale);
            else hipLaunchKernelGGL(k_adam_multi<false>, grid, block, 0, s, a.m, f, grad_scale);
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return gft_fail("gft_adam_step: %s", hipGetErrorString(e));
    }
    return 0;
}
