// k_tracks.hip -- the F-ToRF motion tracks (include/gftorf_tracks.h; render_ftorf_viz_traj.py:262-347).
// k_tracks_integrate: one lane per Gaussian walks the T frames with its position in registers: the flow row of the frame is
// added (the reference's sequential float32 additions), the position is projected into the frame's ToF camera, and the lane
// keeps the running sums of the squared flow and of the world z.  The 12-byte rows (initial_pos, flow, pos_last) never meet
// a lane directly: a workgroup's rows are one contiguous run of floats -- with a motion mask too, since the ranks of its
// dynamic rows are consecutive --, which the workgroup reads as whole dwords into LDS, the next frame's run while this
// frame's is used (one barrier per frame).  The cameras and flow_index are read at wave-uniform addresses.  xy and step_ok
// are written once, coalesced over the Gaussians.  No atomics, no memset.
// k_tracks_table: the selected rows gathered into the table, one lane per Gaussian.
//
// Nothing here may contract into a multiply-add and every division is the correctly rounded one (hipcc's default for fp32
// `/`): the projection is the fixed sequence the header states.
#include "gft_internal.h"
#include "gftorf_tracks.h"

#pragma clang fp contract(off)

namespace {

constexpr int TRK_THREADS = 256;
constexpr int64_t TRK_MAX_ROWS = 1ll << 40;

__device__ __forceinline__ bool inside(float v, float hi) { return 0.f < v && v < hi; }      // a NaN is outside

__global__ __launch_bounds__(TRK_THREADS) void k_tracks_integrate(
    int64_t P, int64_t n, int T, int U, const float* __restrict__ pos0, const float* __restrict__ flow,
    const int32_t* __restrict__ flow_index, const float* __restrict__ Ks, const float* __restrict__ views,
    const uint8_t* __restrict__ mask, const int32_t* __restrict__ rank, float Hf, float Wf, float2* __restrict__ xy,
    float* __restrict__ pos_last, float* __restrict__ motion, float* __restrict__ mean_z, uint8_t* __restrict__ step_ok)
{
    __shared__ float sRow[2][3 * TRK_THREADS];
    const int tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * TRK_THREADS, i = i0 + tid;
    const int64_t end = i0 + TRK_THREADS < P ? i0 + TRK_THREADS : P;       // i0 < P: the grid is ceil(P / TRK_THREADS)
    const int rows = (int)(end - i0);
    const bool live = tid < rows;

    // the flow rows of this workgroup: [r0, r0 + cnt), clamped into [0, n) whatever the ranks hold
    int64_t r0 = i0, cnt = rows;
    if (mask) {
        r0 = rank[i0];
        cnt = (int64_t)rank[end - 1] + (mask[end - 1] ? 1 : 0) - r0;
    }
    r0 = r0 < 0 ? 0 : (r0 > n ? n : r0);
    cnt = cnt < 0 ? 0 : cnt;
    cnt = cnt > n - r0 ? n - r0 : cnt;
    cnt = cnt > TRK_THREADS ? TRK_THREADS : cnt;
    int slot = -1;                                                          // this lane's row of the staged run; -1: static
    if (live) {
        if (!mask) slot = tid < cnt ? tid : -1;
        else if (mask[i]) {
            const int64_t r = (int64_t)rank[i] - r0;
            slot = r >= 0 && r < cnt ? (int)r : -1;
        }
    }
    const int run = 3 * (int)cnt;

    for (int k = tid; k < 3 * rows; k += TRK_THREADS) sRow[1][k] = pos0[3 * i0 + k];
    if (run > 0) {
        const int u = min(max(flow_index[0], 0), U - 1);
        const float* src = flow + ((int64_t)u * n + r0) * 3;
        for (int k = tid; k < run; k += TRK_THREADS) sRow[0][k] = src[k];
    }
    __syncthreads();
    float x = 0.f, y = 0.f, z = 0.f;
    if (live) {
        x = sRow[1][3 * tid];
        y = sRow[1][3 * tid + 1];
        z = sRow[1][3 * tid + 2];
    }
    __syncthreads();                                                        // sRow[1] is the frame 1's run from here on

    float ox = 0.f, oy = 0.f, sum_m = 0.f, sum_z = 0.f;
    for (int t = 0; t < T; t++) {
        if (t + 1 < T && run > 0) {
            const int u = min(max(flow_index[t + 1], 0), U - 1);
            const float* src = flow + ((int64_t)u * n + r0) * 3;
            float* dst = sRow[(t + 1) & 1];
            for (int k = tid; k < run; k += TRK_THREADS) dst[k] = src[k];
        }
        if (live) {
            const float* M = views + 16 * (int64_t)t;
            const float* K = Ks + 9 * (int64_t)t;
            const float c0 = ((M[0] * x + M[4] * y) + M[8] * z) + M[12];
            const float c1 = ((M[1] * x + M[5] * y) + M[9] * z) + M[13];
            const float c2 = ((M[2] * x + M[6] * y) + M[10] * z) + M[14];
            const float h0 = (K[0] * c0 + K[1] * c1) + K[2] * c2;
            const float h1 = (K[3] * c0 + K[4] * c1) + K[5] * c2;
            const float h2 = (K[6] * c0 + K[7] * c1) + K[8] * c2;
            const float den = h2 + 1e-7f;
            const float px = h0 / den, py = h1 / den;
            xy[(int64_t)t * P + i] = make_float2(px, py);
            const bool ok = t == 0 ? inside(px, Wf) && inside(py, Hf)
                                   : inside(px, Wf - 1.f) && inside(py, Hf - 1.f) && inside(ox, Wf) && inside(oy, Hf);
            step_ok[(int64_t)t * P + i] = ok ? 1 : 0;
            ox = px;
            oy = py;
            sum_z = sum_z + z;
            if (slot >= 0) {
                const float* f = sRow[t & 1] + 3 * slot;
                const float fx = f[0], fy = f[1], fz = f[2];
                sum_m = sum_m + ((fx * fx + fy * fy) + fz * fz);
                if (t + 1 < T) {
                    x = x + fx;
                    y = y + fy;
                    z = z + fz;
                }
            }
        }
        __syncthreads();
    }
    if (live) {
        motion[i] = sum_m / (float)T;
        mean_z[i] = sum_z / (float)T;
        sRow[0][3 * tid] = x;
        sRow[0][3 * tid + 1] = y;
        sRow[0][3 * tid + 2] = z;
    }
    __syncthreads();
    for (int k = tid; k < 3 * rows; k += TRK_THREADS) pos_last[3 * i0 + k] = sRow[0][k];
}

__global__ __launch_bounds__(TRK_THREADS) void k_tracks_table(
    int64_t P, int T, int64_t S, const uint8_t* __restrict__ mask, const int32_t* __restrict__ rank, const float2* __restrict__ xy,
    const uint8_t* __restrict__ step_ok, const float* __restrict__ motion, int64_t* __restrict__ out_index,
    float2* __restrict__ out_xy, float* __restrict__ out_motion, uint8_t* __restrict__ out_ok)
{
    const int64_t i = (int64_t)blockIdx.x * TRK_THREADS + threadIdx.x;
    if (i >= P || !mask[i]) return;
    const int64_t r = rank[i];
    if (r < 0 || r >= S) return;
    out_index[r] = i;
    out_motion[r] = motion[i];
    for (int t = 0; t < T; t++) {
        out_xy[(int64_t)t * S + r] = xy[(int64_t)t * P + i];
        out_ok[(int64_t)t * S + r] = step_ok[(int64_t)t * P + i];
    }
}

// byte offsets of the parts: the int64 rows first, then the floats, the bytes last, so every part is aligned as it is
int64_t trk_layout(int32_t T, int64_t S, int64_t* offsets)
{
    if (T < 1 || S < 0 || S > TRK_MAX_ROWS) return -1;
    int64_t pos = 0;
    const int64_t bytes[GFT_TRACKS_PARTS] = {8 * S, 8 * S * T, 4 * S, S * T};
    for (int k = 0; k < GFT_TRACKS_PARTS; k++) {
        if (offsets) offsets[k] = pos;
        pos += bytes[k];
    }
    return pos;
}

}  // namespace

extern "C" int gft_tracks_integrate(void* hip_stream, int64_t P, int64_t n, int32_t T, int32_t U, const float* initial_pos,
                                    const float* flow, const int32_t* flow_index, const float* K, const float* world_view,
                                    const uint8_t* mask, const int32_t* rank, int32_t H, int32_t W, float* xy, float* pos_last,
                                    float* motion, float* mean_z, uint8_t* step_ok)
{
    if (P < 1 || P > TRK_MAX_ROWS || T < 1) return gft_fail("gft_tracks_integrate: bad size P=%lld T=%d", (long long)P, T);
    if (n < 0 || n > P || (n > 0 && U < 1)) return gft_fail("gft_tracks_integrate: bad flow size n=%lld U=%d", (long long)n, U);
    if (H < 1 || W < 1 || H >= (1 << 24) || W >= (1 << 24)) return gft_fail("gft_tracks_integrate: bad image size H=%d W=%d", H, W);
    if (!mask && n != P) return gft_fail("gft_tracks_integrate: without a mask n must be P, got n=%lld P=%lld", (long long)n, (long long)P);
    if (mask && !rank) return gft_fail("gft_tracks_integrate: mask without rank");
    if (!initial_pos || !K || !world_view || !xy || !pos_last || !motion || !mean_z || !step_ok || (n > 0 && (!flow || !flow_index)))
        return gft_fail("gft_tracks_integrate: NULL argument");
    if ((uintptr_t)xy & 7u) return gft_fail("gft_tracks_integrate: xy is not 8-byte aligned");
    const int64_t blocks = (P + TRK_THREADS - 1) / TRK_THREADS;
    if (blocks > 0x7fffffffll) return gft_fail("gft_tracks_integrate: too many rows");
    hipLaunchKernelGGL(k_tracks_integrate, dim3((unsigned)blocks), dim3(TRK_THREADS), 0, (hipStream_t)hip_stream, P, n, (int)T, (int)U,
                       initial_pos, flow, flow_index, K, world_view, mask, rank, (float)H, (float)W, reinterpret_cast<float2*>(xy),
                       pos_last, motion, mean_z, step_ok);
    return gft_launched("gft_tracks_integrate");
}

extern "C" int64_t gft_tracks_table_bytes(int32_t T, int64_t S, int64_t* offsets_out)
{
    const int64_t b = trk_layout(T, S, offsets_out);
    return b < 0 ? 0 : b;
}

extern "C" int gft_tracks_table(void* hip_stream, int64_t P, int32_t T, int64_t S, const uint8_t* mask, const int32_t* rank,
                                const float* xy, const uint8_t* step_ok, const float* motion, void* table)
{
    int64_t off[GFT_TRACKS_PARTS];
    if (P < 1 || P > TRK_MAX_ROWS || trk_layout(T, S, off) < 0 || S > P)
        return gft_fail("gft_tracks_table: bad size P=%lld T=%d S=%lld", (long long)P, T, (long long)S);
    if (S == 0) return 0;
    if (!mask || !rank || !xy || !step_ok || !motion || !table) return gft_fail("gft_tracks_table: NULL argument");
    if (((uintptr_t)table & 7u) || ((uintptr_t)xy & 7u)) return gft_fail("gft_tracks_table: table or xy is not 8-byte aligned");
    const int64_t blocks = (P + TRK_THREADS - 1) / TRK_THREADS;
    if (blocks > 0x7fffffffll) return gft_fail("gft_tracks_table: too many rows");
    uint8_t* base = static_cast<uint8_t*>(table);
    hipLaunchKernelGGL(k_tracks_table, dim3((unsigned)blocks), dim3(TRK_THREADS), 0, (hipStream_t)hip_stream, P, (int)T, S, mask, rank,
                       reinterpret_cast<const float2*>(xy), step_ok, motion, reinterpret_cast<int64_t*>(base + off[GFT_TRACKS_INDEX]),
                       reinterpret_cast<float2*>(base + off[GFT_TRACKS_XY]), reinterpret_cast<float*>(base + off[GFT_TRACKS_MOTION]),
                       base + off[GFT_TRACKS_STEP_OK]);
    return gft_launched("gft_tracks_table");
}
