// k_query.hip -- an iteration's deformation queries as one batch (include/gftorf_query.h; scene/gaussian_model.py:170-174,
// train.py:169-176, 248, 255).  Two elementwise kernels around the network's one call over K * n rows:
//   k_query_inputs    x [K, n, 3], t [K, n] from the raw positions, the dynamic rows (mask / rank / count on the device)
//                     and the K times
//   k_query_combine   R combinations of S blocks of [n, 3]: the forward (R = M outputs of S = K blocks of d_xyz) and, with
//                     the matrix read transposed, the backward (R = K blocks of g_d from S = M upstream gradients)
// Both move 12-48 bytes per point: grid-stride loops of at most QR_MAX_BLOCKS workgroups, scalar loads and stores (the blocks
// of [K, n, 3] start at multiples of 12 n bytes, so nothing wider is aligned in general), no LDS, no atomics, no memset.
#include "gft_internal.h"
#include "gftorf_query.h"

// every product is rounded on its own and the sums run in the documented order: the reference's statements bit for bit
#pragma clang fp contract(off)

namespace {

constexpr int QR_THREADS = 256, QR_MAX_BLOCKS = 2048;

unsigned qr_blocks(int64_t items)
{
    const int64_t b = (items + QR_THREADS - 1) / QR_THREADS;
    return (unsigned)(b < 1 ? 1 : (b > QR_MAX_BLOCKS ? QR_MAX_BLOCKS : b));
}

struct InputArgs {
    int64_t P, n, items;                        // items = max(P, n) with a mask, n without
    const float* __restrict__ xyz;
    const uint8_t* __restrict__ mask;
    const int32_t* __restrict__ rank;
    const uint32_t* __restrict__ count;
    const float* __restrict__ times_dev;
    float times[GFT_QUERY_MAX_TIMES];
    float scale;
    int K;
    float* __restrict__ x;
    float* __restrict__ t;
};

__device__ __forceinline__ void put_row(const InputArgs& a, const float tm[GFT_QUERY_MAX_TIMES], int64_t j, float vx, float vy, float vz)
{
#pragma unroll
    for (int k = 0; k < GFT_QUERY_MAX_TIMES; k++)
        if (k < a.K) {
            float* px = a.x + ((int64_t)k * a.n + j) * 3;
            px[0] = vx; px[1] = vy; px[2] = vz;
            a.t[(int64_t)k * a.n + j] = tm[k];
        }
}

__global__ __launch_bounds__(QR_THREADS) void k_query_inputs(InputArgs a)
{
    float tm[GFT_QUERY_MAX_TIMES];
#pragma unroll
    for (int k = 0; k < GFT_QUERY_MAX_TIMES; k++) tm[k] = k < a.K ? (a.times_dev ? a.times_dev[k] : a.times[k]) : 0.f;
    const int64_t count = a.mask ? (int64_t)*a.count : (a.P < a.n ? a.P : a.n);
    for (int64_t i = (int64_t)blockIdx.x * QR_THREADS + threadIdx.x; i < a.items; i += (int64_t)gridDim.x * QR_THREADS) {
        // the Gaussian i, when it is dynamic and its output row exists
        if (i < a.P) {
            const int64_t j = a.mask ? (a.mask[i] ? (int64_t)a.rank[i] : -1) : i;
            if (j >= 0 && j < a.n) put_row(a, tm, j, a.xyz[3 * i] * a.scale, a.xyz[3 * i + 1] * a.scale, a.xyz[3 * i + 2] * a.scale);
        }
        // the output row i, when no dynamic Gaussian writes it: the point 0
        if (i < a.n && i >= count) put_row(a, tm, i, 0.f, 0.f, 0.f);
    }
}

struct CombineArgs {
    int64_t total;                              // 3 n floats per block
    int R, S;                                   // outputs, inputs
    int c_row, c_col;                           // the coefficient of (r, s) is c[r * c_row + s * c_col] in coeffs_dev
    const float* __restrict__ coeffs_dev;
    float c[GFT_QUERY_MAX_OUTPUTS * GFT_QUERY_MAX_TIMES];      // by value: [r * 4 + s]
    const float* in[4];                         // NULL: zeros
    float* out[4];
};

__global__ __launch_bounds__(QR_THREADS) void k_query_combine(CombineArgs a)
{
    float c[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int s = 0; s < 4; s++) {
            float v = 0.f;
            if (r < a.R && s < a.S && a.in[s]) v = a.coeffs_dev ? a.coeffs_dev[r * a.c_row + s * a.c_col] : a.c[r * 4 + s];
            c[r][s] = v;
        }
    for (int64_t i = (int64_t)blockIdx.x * QR_THREADS + threadIdx.x; i < a.total; i += (int64_t)gridDim.x * QR_THREADS) {
        float v[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            // an operand no coefficient uses is not read
            const bool used = (c[0][s] != 0.f) | (c[1][s] != 0.f) | (c[2][s] != 0.f) | (c[3][s] != 0.f);
            v[s] = used ? a.in[s][i] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (r < a.R) {
                float acc = 0.f;
                bool first = true;
#pragma unroll
                for (int s = 0; s < 4; s++)
                    if (c[r][s] != 0.f) {
                        const float p = c[r][s] * v[s];
                        acc = first ? p : acc + p;
                        first = false;
                    }
                a.out[r][i] = acc;
            }
    }
}

int combine_launch(hipStream_t s, CombineArgs& a, const char* who)
{
    hipLaunchKernelGGL(k_query_combine, dim3(qr_blocks(a.total)), dim3(QR_THREADS), 0, s, a);
    return gft_launched(who);
}

int combine_sizes(int64_t n, int32_t K, int32_t M, const char* who)
{
    if (K < 1 || K > GFT_QUERY_MAX_TIMES) return gft_fail("%s: K=%d is not in 1..%d", who, (int)K, GFT_QUERY_MAX_TIMES);
    if (M < 1 || M > GFT_QUERY_MAX_OUTPUTS) return gft_fail("%s: M=%d is not in 1..%d", who, (int)M, GFT_QUERY_MAX_OUTPUTS);
    if (n < 0 || n > 0x7fffffffll) return gft_fail("%s: bad row count n=%lld", who, (long long)n);
    return 0;
}

}  // namespace

extern "C" int gft_query_inputs(void* hip_stream, int64_t P, const float* xyz, const uint8_t* mask, const int32_t* rank,
                                const uint32_t* count_dev, int64_t n, int32_t K, float scale, const float* times_dev,
                                const float* times_host, float* x, float* t)
{
    if (K < 1 || K > GFT_QUERY_MAX_TIMES) return gft_fail("gft_query_inputs: K=%d is not in 1..%d", (int)K, GFT_QUERY_MAX_TIMES);
    if (P < 0 || P > 0x7fffffffll || n < 0 || n > 0x7fffffffll)
        return gft_fail("gft_query_inputs: bad row counts P=%lld n=%lld", (long long)P, (long long)n);
    if (n == 0) return 0;
    const int given = (mask != nullptr) + (rank != nullptr) + (count_dev != nullptr);
    if (given != 0 && given != 3) return gft_fail("gft_query_inputs: mask, rank and count_dev come together or not at all");
    if (!times_dev && !times_host) return gft_fail("gft_query_inputs: times_dev and times_host are both NULL");
    if (!x || !t || (P > 0 && !xyz)) return gft_fail("gft_query_inputs: NULL argument");
    InputArgs a = {};
    a.P = P; a.n = n; a.items = (mask && P > n) ? P : n;
    a.xyz = xyz; a.mask = mask; a.rank = rank; a.count = count_dev;
    a.times_dev = times_dev;
    if (!times_dev)
        for (int k = 0; k < K; k++) a.times[k] = times_host[k];
    a.scale = scale; a.K = K; a.x = x; a.t = t;
    hipLaunchKernelGGL(k_query_inputs, dim3(qr_blocks(a.items)), dim3(QR_THREADS), 0, (hipStream_t)hip_stream, a);
    return gft_launched("gft_query_inputs");
}

extern "C" int gft_query_combine(void* hip_stream, int64_t n, int32_t K, int32_t M, const float* d, const float* coeffs_dev,
                                 const float* coeffs_host, float* const* out)
{
    if (combine_sizes(n, K, M, "gft_query_combine")) return 1;
    if (n == 0) return 0;
    if (!coeffs_dev && !coeffs_host) return gft_fail("gft_query_combine: coeffs_dev and coeffs_host are both NULL");
    if (!d || !out) return gft_fail("gft_query_combine: NULL argument");
    CombineArgs a = {};
    a.total = 3 * n; a.R = M; a.S = K; a.c_row = K; a.c_col = 1; a.coeffs_dev = coeffs_dev;
    for (int m = 0; m < M; m++) {
        if (!out[m]) return gft_fail("gft_query_combine: out[%d] is NULL", m);
        a.out[m] = out[m];
        for (int k = 0; k < K; k++) a.c[m * 4 + k] = coeffs_dev ? 0.f : coeffs_host[m * K + k];
    }
    for (int k = 0; k < K; k++) a.in[k] = d + (int64_t)k * a.total;
    return combine_launch((hipStream_t)hip_stream, a, "gft_query_combine");
}

extern "C" int gft_query_combine_backward(void* hip_stream, int64_t n, int32_t K, int32_t M, const float* const* g_out,
                                          const float* coeffs_dev, const float* coeffs_host, float* g_d)
{
    if (combine_sizes(n, K, M, "gft_query_combine_backward")) return 1;
    if (n == 0) return 0;
    if (!coeffs_dev && !coeffs_host) return gft_fail("gft_query_combine_backward: coeffs_dev and coeffs_host are both NULL");
    if (!g_out || !g_d) return gft_fail("gft_query_combine_backward: NULL argument");
    CombineArgs a = {};
    a.total = 3 * n; a.R = K; a.S = M; a.c_row = 1; a.c_col = K; a.coeffs_dev = coeffs_dev;
    for (int m = 0; m < M; m++) {
        a.in[m] = g_out[m];                     // NULL: the kernel takes its coefficients as 0
        for (int k = 0; k < K; k++) a.c[k * 4 + m] = coeffs_dev ? 0.f : coeffs_host[m * K + k];
    }
    for (int k = 0; k < K; k++) a.out[k] = g_d + (int64_t)k * a.total;
    return combine_launch((hipStream_t)hip_stream, a, "gft_query_combine_backward");
}
