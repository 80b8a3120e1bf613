// k_features.hip -- per-Gaussian features blended over a frame gft_forward has drawn, and the transpose of that blend
// (include/gftorf_features.h).  F-ToRF renders two 3-D scene flows per flow iteration as colors_precomp on the same detached
// geometry; one forward draws the frame, these kernels blend further features over it and return their gradient only.
//
// Work unit = one wave = one 8x8 quadrant, as in k_render_fwd / k_render_bwd.  The quadrant walks its tile's list front to
// back, [0, deepest contributor of the quadrant) at ranges[tile].x -- the list the backward walks: sorted heads, tails
// completed on demand, whole-frame and tile-pull binning and frames drawn by k_render_fwd_seg all leave it there.  Batches of
// 64 entries are staged through LDS and culled against the quadrant.  Per pixel, alpha is recomputed from the geometry record
// with the forward's arithmetic; an entry counts when it stands in front of the pixel's contributor count and passes the
// power / 1/255 tests, which is exactly the set the forward blended.  T is the running product from 1, so both kernels see
// the same alpha_i T_i:
//   k_feat_fwd<C>  out[c] = sum f_i[c] alpha_i T_i + T_final bg[c]
//   k_feat_bwd<C>  dL/df_i[c] = sum_p alpha_i T_i dL/dout[c]: the quadrant's 64 pixels are reduced per entry with
//                  v_permlane32_swap / v_permlane16_swap / row DPP, and the C sums go to the Gaussian's 32-byte accumulator
//                  row with one atomic wave instruction (C = 3: three lanes) or two (C = 6: three lanes each) -- either way
//                  one 64-byte line per entry (atomic lines are what this chip rations)
//   k_feat_out<C>  the rows, unpadded, into dL_dfeatures [P, C].
//   k_feat_bwd_det<C>  the same walk, but the reduced row of every (list entry, quadrant) is STORED at the entry's position in
//                  point_list (rows of FEAT_ROW floats, as RenderBwdArgs.det does for the rasterizer); the rows are then
//                  added in the one order of include/gftorf_detsum.h (k_detsum.hip): bit-reproducible gradients
#include "gft_internal.h"
#include "gft_render_walk.h"
#include "gftorf_features.h"

namespace {

constexpr int FEAT_ROW = 8;        // floats per accumulator row and per staged feature record

typedef unsigned int feat_u32x2 __attribute__((ext_vector_type(2)));

struct FeatArgs {
    int W, H, gx, T;
    const uint2* __restrict__ ranges;
    const uint32_t* __restrict__ point_list;
    const float4* __restrict__ rec_a;
    const float4* __restrict__ pix_state;
    const uint32_t* __restrict__ quad_max;
    const uint32_t* __restrict__ ctrl;
    uint32_t cap;
    const float* __restrict__ feat;      // forward: [P][C]
    const float* __restrict__ bg;        // forward: [C] planes via bsc / bsy / bsx, or NULL
    int64_t bsc, bsy, bsx;
    float* __restrict__ out;             // forward: [C][H][W]
    const float* __restrict__ g_out;     // backward: [C][H][W]
    float* __restrict__ acc;             // backward: [P][FEAT_ROW]; fixed-order backward: the partial rows [list slot][4][FEAT_ROW]
};

// unit v = 4 tile + quadrant; workgroups are dealt round-robin over the 8 XCDs: every XCD gets a contiguous run of units,
// the four quadrants of a tile (identical list reads) share its L2
__device__ __forceinline__ int feat_unit(int b, int V)
{
    const int chunk = (V + 7) >> 3;
    return (b & 7) * chunk + (b >> 3);
}

__device__ __forceinline__ float feat_swap32_add(float x, float y)
{
    // lanes 0-31: x[l] + x[l+32]; lanes 32-63: y[l-32] + y[l]
    const feat_u32x2 r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}

__device__ __forceinline__ float feat_swap16_add(float x, float y)
{
    // row0: x.r0 + x.r1; row1: y.r0 + y.r1; row2: x.r2 + x.r3; row3: y.r2 + y.r3
    const feat_u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}

// every lane of a 16-lane row gets the row's total
__device__ __forceinline__ float feat_row_sum(float x)
{
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x128, 0xf, 0xf, false));   // row_ror:8
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x124, 0xf, 0xf, false));   // row_ror:4
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x4e, 0xf, 0xf, false));    // quad_perm [2,3,0,1]
    x += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0xb1, 0xf, 0xf, false));    // quad_perm [1,0,3,2]
    return x;
}

// Feature records of a staged entry: FEAT_ROW floats = two float4 of LDS, the unused ones 0.
template <int C>
__device__ __forceinline__ void feat_stage(const float* __restrict__ feat, uint32_t id, float4* sF, int slot)
{
    if constexpr (C == 3) {
        const float* f = feat + (size_t)id * 3;
        sF[2 * slot] = make_float4(f[0], f[1], f[2], 0.f);
    } else {
        const float2* f = reinterpret_cast<const float2*>(feat + (size_t)id * 6);       // 24-byte rows: 8-byte aligned
        const float2 f0 = f[0], f1 = f[1], f2 = f[2];
        sF[2 * slot] = make_float4(f0.x, f0.y, f1.x, f1.y);
        sF[2 * slot + 1] = make_float4(f2.x, f2.y, 0.f, 0.f);
    }
}

// The walk of quadrant v, shared by both directions.  DET (backward only): an entry's sums are stored, not added.
template <int C, bool BWD, bool DET = false>
__device__ __forceinline__ void feat_walk(const FeatArgs& a, const int v, const int lane, float4* sA, float4* sF, uint32_t* sId)
{
    static_assert(C == 3 || C == 6, "feature blend: C is 3 or 6");
    auto wave_sync = [] { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); };
    const int tile = v >> 2, quad = v & 3;
    const int tx = tile % a.gx, ty = tile / a.gx;
    const int qx0 = tx * GFT_TILE_X + (quad & 1) * 8, qy0 = ty * GFT_TILE_Y + (quad >> 1) * 8;
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < a.W && py < a.H;
    const float pxf = (float)px, pyf = (float)py;
    const size_t HW = (size_t)a.H * a.W;
    const size_t pix = inside ? (size_t)a.W * py + px : 0;

    float T_final = 1.f;
    int n_contrib = 0;                     // pixels outside the image blend nothing
    float s[C];                            // forward: blended sums; backward: dL/dout of the pixel
#pragma unroll
    for (int k = 0; k < C; k++) s[k] = 0.f;
    if (inside && a.pix_state) {
        const float4 st = a.pix_state[pix];
        T_final = st.x;
        n_contrib = (int)__float_as_uint(st.y);
        if constexpr (BWD) {
#pragma unroll
            for (int k = 0; k < C; k++) s[k] = a.g_out[k * HW + pix];
        }
    }
    const int tmax = a.quad_max ? (int)a.quad_max[v] : 0;
    const uint32_t r0 = tmax > 0 ? a.ranges[tile].x : 0u;
    const float4 box = make_float4((float)qx0, (float)qy0, 7.f, 7.f);
    float T = 1.f;
    for (int base = 0; base < tmax; base += RB) {
        const int n = min(RB, tmax - base);
        bool reach = false;
        wave_sync();                                   // the previous batch has read LDS
        if (lane < n) {
            const uint32_t id = a.point_list[r0 + (uint32_t)(base + lane)];
            const float4 a0 = a.rec_a[2 * id], a1 = a.rec_a[2 * id + 1];
            sA[2 * lane] = a0;
            sA[2 * lane + 1] = a1;
            if constexpr (BWD && !DET) sId[lane] = id;
            else if constexpr (!BWD) feat_stage<C>(a.feat, id, sF, lane);
            reach = gft_splat_reaches_box(a0, a1, box.x, box.y, box.z, box.w);
        }
        uint64_t m = to_sgpr(wave_ballot(reach));
        wave_sync();
        while (m) {
            const int j = (int)__builtin_ctzll(m);
            m &= m - 1;
            const float4 a0 = sA[2 * j], a1 = sA[2 * j + 1];
            // (the forward blend's arithmetic: gft_render_walk.h)
            const float dx = a0.x - pxf, dy = a0.y - pyf;
            const float power = -0.5f * (a0.z * dx * dx + a1.x * dy * dy) - a0.w * dx * dy;
            const float alpha = fminf(0.99f, a1.y * gft_exp(power));
            const bool contrib = (base + j < n_contrib) && !(power > 0.0f) && !(alpha < 1.0f / 255.0f);
            if (wave_ballot(contrib) == 0ull) continue;          // wave-uniform skip
            // lanes that do not blend the entry use alpha = 0: w = 0, T unchanged
            const float al = contrib ? alpha : 0.f;
            const float w = al * T;
            T = T * (1.f - al);
            if constexpr (!BWD) {
                const float4 f0 = sF[2 * j];
                s[0] = fmaf(f0.x, w, s[0]); s[1] = fmaf(f0.y, w, s[1]); s[2] = fmaf(f0.z, w, s[2]);
                if constexpr (C == 6) {
                    const float4 f1 = sF[2 * j + 1];
                    s[3] = fmaf(f0.w, w, s[3]); s[4] = fmaf(f1.x, w, s[4]); s[5] = fmaf(f1.y, w, s[5]);
                }
            } else {
                // 64 pixels -> the C sums of this entry; afterwards lane 16 r holds value r (C = 3) or values 2 r, 2 r + 1
                // (C = 6): one (C = 3) or two (C = 6) atomic instructions of three lanes add them to the Gaussian's row
                float* row;
                if constexpr (DET) row = a.acc + ((size_t)(r0 + (uint32_t)(base + j)) * 4 + quad) * FEAT_ROW;
                else row = a.acc + (size_t)sId[j] * FEAT_ROW;
                if constexpr (C == 3) {
                    const float t = feat_swap16_add(feat_swap32_add(w * s[0], w * s[2]), feat_swap32_add(w * s[1], 0.f));
                    const float u = feat_row_sum(t);
                    if ((lane & 15) == 0 && (lane >> 4) < 3) {
                        if constexpr (DET) row[lane >> 4] = u;
                        else atomicAdd(row + (lane >> 4), u);
                    }
                } else {
                    const float s0 = feat_swap32_add(w * s[0], w * s[4]), s1 = feat_swap32_add(w * s[1], w * s[5]);
                    const float s2 = feat_swap32_add(w * s[2], 0.f), s3 = feat_swap32_add(w * s[3], 0.f);
                    const float u0 = feat_row_sum(feat_swap16_add(s0, s2)), u1 = feat_row_sum(feat_swap16_add(s1, s3));
                    if ((lane & 15) == 0 && (lane >> 4) < 3) {
                        if constexpr (DET) {
                            row[2 * (lane >> 4)] = u0;
                            row[2 * (lane >> 4) + 1] = u1;
                        } else {
                            atomicAdd(row + 2 * (lane >> 4), u0);
                            atomicAdd(row + 2 * (lane >> 4) + 1, u1);
                        }
                    }
                }
            }
        }
    }
    if constexpr (!BWD) {
        if (inside) {
#pragma unroll
            for (int k = 0; k < C; k++) {
                const float b = a.bg ? a.bg[k * a.bsc + (int64_t)py * a.bsy + (int64_t)px * a.bsx] : 0.f;
                a.out[k * HW + pix] = fmaf(T_final, b, s[k]);
            }
        }
    }
}

template <int C>
__global__ __launch_bounds__(64) void k_feat_fwd(FeatArgs a)
{
    __shared__ float4 sA[RB * 2];
    __shared__ float4 sF[RB * 2];
    if (a.ctrl && a.ctrl[GFT_CTRL_TOTAL] > a.cap) return;     // the frame did not fit its binning buffer: it was not drawn
    const int V = 4 * a.T;
    const int v = feat_unit((int)blockIdx.x, V);
    if (v >= V) return;
    feat_walk<C, false>(a, v, (int)threadIdx.x, sA, sF, nullptr);
}

template <int C>
__global__ __launch_bounds__(64) void k_feat_bwd(FeatArgs a)
{
    __shared__ float4 sA[RB * 2];
    __shared__ uint32_t sId[RB];
    if (a.ctrl[GFT_CTRL_TOTAL] > a.cap) return;
    const int V = 4 * a.T;
    const int v = feat_unit((int)blockIdx.x, V);
    if (v >= V) return;
    feat_walk<C, true>(a, v, (int)threadIdx.x, sA, nullptr, sId);
}

template <int C>
__global__ __launch_bounds__(64) void k_feat_bwd_det(FeatArgs a)
{
    __shared__ float4 sA[RB * 2];
    if (a.ctrl[GFT_CTRL_TOTAL] > a.cap) return;
    const int V = 4 * a.T;
    const int v = feat_unit((int)blockIdx.x, V);
    if (v >= V) return;
    feat_walk<C, true, true>(a, v, (int)threadIdx.x, sA, nullptr, nullptr);
}

template <int C>
__global__ __launch_bounds__(256) void k_feat_out(int P, const float* __restrict__ acc, float* __restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)P * C) return;
    const int64_t g = i / C;
    out[i] = acc[g * FEAT_ROW + (i - g * C)];
}

int feat_args(FeatArgs& a, const char* who, const gft_config* cfg, const void* geom, const void* img, const void* binning,
              int64_t binning_instances, int32_t C)
{
    if (!cfg) return gft_fail("%s: config is NULL", who);
    if (cfg->P < 0 || cfg->W <= 0 || cfg->H <= 0) return gft_fail("%s: bad sizes P=%d W=%d H=%d", who, cfg->P, cfg->W, cfg->H);
    if (C != 3 && C != 6) return gft_fail("%s: C must be 3 or 6, got %d", who, C);
    if (binning_instances < 0 || binning_instances > 0xffffffffll) return gft_fail("%s: bad instance count", who);
    if (!geom || !img || (binning_instances > 0 && !binning)) return gft_fail("%s: NULL scratch buffer", who);
    gft_layout L;
    gft_compute_layout(cfg->P, cfg->W, cfg->H, binning_instances, &L);
    const GeomView g = gft_geom_view(const_cast<void*>(geom), L);
    const ImgView im = gft_img_view(const_cast<void*>(img), L);
    const BinView b = gft_bin_view(const_cast<void*>(binning), L);
    a = FeatArgs{};
    a.W = cfg->W; a.H = cfg->H;
    a.gx = (cfg->W + GFT_TILE_X - 1) / GFT_TILE_X;
    a.T = a.gx * ((cfg->H + GFT_TILE_Y - 1) / GFT_TILE_Y);
    a.ranges = im.ranges; a.point_list = b.point_list; a.rec_a = g.rec_a;
    a.pix_state = im.pix_state; a.quad_max = im.tile_max;
    a.ctrl = im.ctrl; a.cap = (uint32_t)binning_instances;
    return 0;
}

int feat_blocks(const FeatArgs& a) { return 8 * ((4 * a.T + 7) / 8); }

int launched(const char* who)
{
    const hipError_t err = hipGetLastError();
    return err == hipSuccess ? 0 : gft_fail("%s: %s", who, hipGetErrorString(err));
}

}  // namespace

extern "C" int gft_render_features(void* hip_stream, const gft_config* cfg, const void* geom, const void* img,
                                   const void* binning, int64_t binning_instances, int32_t C, const float* features,
                                   const float* bg, float* out)
{
    const char* who = "gft_render_features";
    FeatArgs a;
    if (feat_args(a, who, cfg, geom, img, binning, binning_instances, C)) return 1;
    if (!out || (cfg->P > 0 && !features)) return gft_fail("%s: NULL argument", who);
    if (C == 6 && ((uintptr_t)features & 7u) != 0)
        return gft_fail("%s: C = 6 features must be 8-byte aligned (they are read as float2)", who);
    a.feat = features; a.out = out;
    a.bg = bg; a.bsc = cfg->bg_stride_c; a.bsy = cfg->bg_stride_y; a.bsx = cfg->bg_stride_x;
    hipStream_t s = (hipStream_t)hip_stream;
    if (cfg->P == 0) {
        // no Gaussian: no kernel of the forward ran, its scratch holds nothing and its outputs are zero -- so is this one
        a.pix_state = nullptr; a.quad_max = nullptr; a.ctrl = nullptr; a.bg = nullptr;
    }
    if (C == 3) hipLaunchKernelGGL(k_feat_fwd<3>, dim3(feat_blocks(a)), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(k_feat_fwd<6>, dim3(feat_blocks(a)), dim3(64), 0, s, a);
    return launched(who);
}

extern "C" int gft_render_features_backward(void* hip_stream, const gft_config* cfg, const void* geom, const void* img,
                                            const void* binning, int64_t binning_instances, int32_t C, const float* dL_dout,
                                            float* acc, float* dL_dfeatures)
{
    const char* who = "gft_render_features_backward";
    FeatArgs a;
    if (feat_args(a, who, cfg, geom, img, binning, binning_instances, C)) return 1;
    if (cfg->P == 0) return 0;
    if (!dL_dout || !acc || !dL_dfeatures) return gft_fail("%s: NULL argument", who);
    a.g_out = dL_dout; a.acc = acc;
    hipStream_t s = (hipStream_t)hip_stream;
    const hipError_t e = gft_zero_async(acc, (size_t)cfg->P * FEAT_ROW * sizeof(float), s);
    if (e != hipSuccess) return gft_fail("%s: %s", who, hipGetErrorString(e));
    if (C == 3) hipLaunchKernelGGL(k_feat_bwd<3>, dim3(feat_blocks(a)), dim3(64), 0, s, a);
    else hipLaunchKernelGGL(k_feat_bwd<6>, dim3(feat_blocks(a)), dim3(64), 0, s, a);
    const int64_t n = (int64_t)cfg->P * C;
    const int blocks = (int)((n + 255) / 256);
    if (C == 3) hipLaunchKernelGGL(k_feat_out<3>, dim3(blocks), dim3(256), 0, s, cfg->P, (const float*)acc, dL_dfeatures);
    else hipLaunchKernelGGL(k_feat_out<6>, dim3(blocks), dim3(256), 0, s, cfg->P, (const float*)acc, dL_dfeatures);
    return launched(who);
}

extern "C" size_t gft_feature_partials_bytes(int64_t binning_instances, int32_t W, int32_t H)
{
    return gft_point_list_slots(binning_instances, W, H) * 4 * FEAT_ROW * sizeof(float);
}

extern "C" int gft_render_features_backward_det(void* hip_stream, const gft_config* cfg, const void* geom, const void* img,
                                                const void* binning, int64_t binning_instances, int32_t C,
                                                const float* dL_dout, void* index, float* partials, float* dL_dfeatures)
{
    const char* who = "gft_render_features_backward_det";
    FeatArgs a;
    if (feat_args(a, who, cfg, geom, img, binning, binning_instances, C)) return 1;
    if (cfg->P == 0) return 0;
    if (!dL_dout || !dL_dfeatures || (binning_instances > 0 && !partials)) return gft_fail("%s: NULL argument", who);
    if (((uintptr_t)index & 3u) != 0) return gft_fail("%s: index must be 4-byte aligned", who);
    if (index && gft_point_list_slots(binning_instances, cfg->W, cfg->H) >= 0xffffffffull)
        return gft_fail("%s: the frame's id list is too long for the index", who);
    gft_layout L;
    gft_compute_layout(cfg->P, cfg->W, cfg->H, binning_instances, &L);
    const GeomView g = gft_geom_view(const_cast<void*>(geom), L);
    const ImgView im = gft_img_view(const_cast<void*>(img), L);
    const BinView b = gft_bin_view(const_cast<void*>(binning), L);
    a.g_out = dL_dout; a.acc = partials;
    hipStream_t s = (hipStream_t)hip_stream;
    if (binning_instances > 0) {
        // rows of (entry, quadrant) pairs no pixel touched must read as zero
        const hipError_t e = gft_zero_async(partials, gft_feature_partials_bytes(binning_instances, cfg->W, cfg->H), s);
        if (e != hipSuccess) return gft_fail("%s: %s", who, hipGetErrorString(e));
        if (C == 3) hipLaunchKernelGGL(k_feat_bwd_det<3>, dim3(feat_blocks(a)), dim3(64), 0, s, a);
        else hipLaunchKernelGGL(k_feat_bwd_det<6>, dim3(feat_blocks(a)), dim3(64), 0, s, a);
    }
    const hipError_t e = index
        ? gft_launch_detsum(s, cfg->P, cfg->W, cfg->H, g, im, b, a.cap, partials, FEAT_ROW, C, dL_dfeatures, C, false, (uint32_t*)index)
        : gft_launch_detsum_serial(s, cfg->P, cfg->W, cfg->H, im, b, a.cap, partials, FEAT_ROW, C, dL_dfeatures, C);
    if (e != hipSuccess) return gft_fail("%s: %s", who, hipGetErrorString(e));
    return launched(who);
}
