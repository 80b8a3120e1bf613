// k_pcd.hip -- the input point cloud (include/gftorf_pcd.h; scene/dataset_readers.py:110-150, 530-586, 904-973, 1067-1118;
// scene/gaussian_model.py:180-236).
// k_pcd_unproject: a thread per grid pixel of one ToF frame.  The distance is numpy's float32 depth_from_tof
// (gft_tof_depth.h); the near-plane point, its ray, sqrt(z^2 - x^2 - y^2) and the product with the inverse view matrix are
// float64 as numpy's are, the inverse formed from the 16 arguments by every lane (the adjugate, as k_flow.hip's).  Bound by
// its double arithmetic (about 250 double operations per pixel, 12 bytes read and up to 80 written).
// k_pcd_pack: a workgroup takes GFT_PCD_ROWS rows of storePly's file.  A thread forms its row in LDS at the row's byte offset
// in the workgroup's run (a 38-byte row is 9.5 dwords: neighbouring rows share one), so the staging is the file dword for
// dword and leaves as whole dwords.  256 rows are a whole number of dwords whatever the row's bytes, so a run begins on a
// dword and workgroups share none; only the file's last dword can be ragged, and gft_put_run (gft_byte_runs.h) stores its
// bytes singly.  k_pcd_unpack: the reverse, dwords of the chunk into LDS, a thread per row out of it.
// k_pcd_create: the rows of create_from_pcd's tensors, then the zeros of the three *_rest tensors as one flat fill.
// pack, unpack and create are bound by their HBM bytes.  No scalar loads of written memory, no memset; the status words are
// the only atomics (uint32 adds, taken only by a pixel or a colour the reference would raise on).
//
// The arithmetic is numpy's / torch's operation for operation: nothing here may contract into a multiply-add, and every
// division and square root is the correctly rounded one.
#include "gft_internal.h"
#include "gft_byte_runs.h"
#include "gft_tof_depth.h"
#include "gftorf_pcd.h"

#pragma clang fp contract(off)

namespace {

constexpr int PCD_THREADS = 256, PCD_ROWS = GFT_PCD_ROWS, PCD_MAX_BLOCKS = 4096;
constexpr int64_t PCD_MAX_ROWS = 1ll << 40;
constexpr float PCD_C0 = 0.28209479177387814f;       // utils/sh_utils.py:26 as numpy's float32 arithmetic takes it
static_assert(PCD_ROWS == PCD_THREADS && PCD_ROWS % 4 == 0, "a thread per row; a workgroup's rows begin on a dword of the file");

struct PcdUnproject {
    const float* tof;
    const void* rendered;
    int mode, rendered_f64, H, W, stride, Hp, Wp;
    double view[16], width_m, height_m, znear;
    const float* depth_range_dev;
    const float* phase_offset_dev;
    float depth_range, phase_offset;
    float* xyz;
    void* dist;
    float* amp;
    float* sh_color;
    float* color;
    float* sh_amp;
    float* amplitude;
    uint32_t* status;
};

// rows 0..2 of inverse(m), m row-major 4x4, through the adjugate in double.  Every lane computes the same.
__device__ __forceinline__ void inverse_rows(const double* m, double* inv)
{
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    const double c12 = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    const double r = 1.0 / (m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * c12);
#pragma unroll
    for (int k = 0; k < 12; k++) inv[k] *= r;
}

__global__ __launch_bounds__(PCD_THREADS) void k_pcd_unproject(PcdUnproject p)
{
    const int N = p.Hp * p.Wp;
    const int i = blockIdx.x * PCD_THREADS + threadIdx.x;
    if (i >= N) return;
    double inv[12];
    inverse_rows(p.view, inv);
    const int r = i / p.Wp, c = i - r * p.Wp;
    const int ys = r * p.stride, xs = c * p.stride;                                 // ys < H, xs < W: Hp = ceil(H / stride)
    const float* px = p.tof + ((int64_t)ys * p.W + xs) * 3;
    const float amp = px[2];
    const float dr = gft_dev_or(p.depth_range_dev, p.depth_range), off = gft_dev_or(p.phase_offset_dev, p.phase_offset);
    float z = depth_from_tof_np(px[0], px[1], dr, off);

    if (p.mode == GFT_PCD_FTORF_INIT) {
        // :929-946: the candidates z and z + depth_range / 2 kept in (znear, 10.5], float32 comparisons; with both kept the
        // amplitude at the reference's own index (i // Wp, i % Hp), compared with 0.04 in double, picks one
        const float z2 = __fadd_rn(z, dr * 0.5f), zn = (float)p.znear;
        const bool k1 = zn < z && z <= 10.5f, k2 = zn < z2 && z2 <= 10.5f;
        if (k1 && k2) {
            const int w_ = i % p.Hp;
            if (w_ < p.W) {
                if ((double)p.tof[((int64_t)r * p.W + w_) * 3 + 2] < 0.04) z = z2;
            } else {
                atomicAdd(p.status + 1, 1u);
                z = NAN;
            }
        } else if (k2) {
            z = z2;
        } else if (!k1) {
            atomicAdd(p.status, 1u);
            z = NAN;
        }
    }

    // :552-555, :562-564: the pixel on the near plane and its ray
    const double x0 = ((double)xs * 2.0 / (double)p.W - 1.0) * p.width_m / 2.0;
    const double y0 = ((double)ys * 2.0 / (double)p.H - 1.0) * p.height_m / 2.0;
    const double len = sqrt(x0 * x0 + y0 * y0 + p.znear * p.znear);
    const double xn = x0 / len, yn = y0 / len;
    const bool proxy = p.mode == GFT_PCD_PROXY, wide = proxy && p.rendered_f64;
    const int halves = p.mode == GFT_PCD_FTORF_INIT ? 1 : 2;
    for (int h = 0; h < halves; h++) {
        const int64_t row = (int64_t)h * N + i;
        double zd = (double)z, zz;
        float zf = z;
        if (proxy && h == 1) {
            const int64_t at = (int64_t)ys * p.W + xs;
            if (wide) zd = reinterpret_cast<const double*>(p.rendered)[at];
            else zd = (double)(zf = reinterpret_cast<const float*>(p.rendered)[at]);
        }
        // np.square keeps the distances' dtype: float32 unless the rendered image made the column float64
        if (wide) zz = zd * zd;
        else zz = (double)(zf * zf);
        const double X = xn * zd, Y = yn * zd;
        const double Z = sqrt(zz - X * X - Y * Y);
#pragma unroll
        for (int k = 0; k < 3; k++) p.xyz[row * 3 + k] = (float)(inv[4 * k] * X + inv[4 * k + 1] * Y + inv[4 * k + 2] * Z + inv[4 * k + 3]);
        if (wide) reinterpret_cast<double*>(p.dist)[row] = zd;
        else reinterpret_cast<float*>(p.dist)[row] = zf;
        if (p.amp) p.amp[row] = amp;
        // sh_utils.py:114-124 in float32
        const float sh_c = (amp - 0.5f) / PCD_C0;
        if (p.sh_color) p.sh_color[row] = sh_c;
        if (p.color) {
            const float rgb = sh_c * PCD_C0 + 0.5f;
            p.color[row * 3] = rgb;
            p.color[row * 3 + 1] = rgb;
            p.color[row * 3 + 2] = rgb;
        }
        const float sh_a = (amp * (zf * zf) - 0.5f) / PCD_C0;
        if (p.sh_amp) p.sh_amp[row] = sh_a;
        if (p.amplitude) p.amplitude[row] = sh_a * PCD_C0 + 0.5f;
    }
}

__device__ __forceinline__ double load_real(const void* p, int f64, int64_t i)
{
    return f64 ? reinterpret_cast<const double*>(p)[i] : (double)reinterpret_cast<const float*>(p)[i];
}

__device__ __forceinline__ void put_f32(uint8_t* at, float v)
{
    const uint32_t u = __float_as_uint(v);
#pragma unroll
    for (int k = 0; k < 4; k++) at[k] = (uint8_t)(u >> (8 * k));
}

__device__ __forceinline__ float get_f32(const uint8_t* at)
{
    uint32_t u = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) u |= (uint32_t)at[k] << (8 * k);
    return __uint_as_float(u);
}

// storePly's float -> u1 assignment (int(v), then the range check numpy makes): the byte, or 0 and a count
__device__ __forceinline__ uint8_t to_u1(double v, uint32_t* status)
{
    if (v > -1.0 && v < 256.0) return (uint8_t)(int)v;
    atomicAdd(status + (v != v ? 1 : 0), 1u);
    return 0;
}

__global__ __launch_bounds__(PCD_THREADS) void k_pcd_pack(int64_t P, int row_bytes, const float* __restrict__ xyz, const void* __restrict__ colors,
                                                          int colors_f64, const float* __restrict__ phases,
                                                          const float* __restrict__ amplitudes, const void* __restrict__ seg, int seg_f64,
                                                          uint8_t* __restrict__ body, double* __restrict__ colors_back,
                                                          double* __restrict__ seg_back, uint32_t* status)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t run[];                  // PCD_ROWS * row_bytes bytes
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * PCD_ROWS, row = row0 + tid;          // row0 < P
    const int rows = (int)(P - row0 < PCD_ROWS ? P - row0 : PCD_ROWS);
    uint8_t* dst = body + row0 * row_bytes;                                         // 4-byte aligned: body is, and row0 is a multiple of 256
    if (tid < rows) {
        uint8_t* at = reinterpret_cast<uint8_t*>(run) + tid * row_bytes;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            put_f32(at + 4 * k, xyz[row * 3 + k]);
            put_f32(at + 12 + 4 * k, 0.f);
            const uint8_t b = to_u1(load_real(colors, colors_f64, row * 3 + k), status);
            at[24 + k] = b;
            if (colors_back) colors_back[row * 3 + k] = (double)b / 255.0;
        }
        at += 27;
        if (phases) {
            put_f32(at, phases[row]);
            put_f32(at + 4, amplitudes[row]);
            at += 8;
        }
        if (seg) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const uint8_t b = to_u1(load_real(seg, seg_f64, row * 3 + k), status);
                at[k] = b;
                if (seg_back) seg_back[row * 3 + k] = (double)b / 255.0;
            }
        }
    }
    __syncthreads();
    gft_put_run<PCD_THREADS>(dst, rows * row_bytes, run);
}

struct PcdFields {
    int32_t offset[GFT_PCD_FIELDS];
};

__global__ __launch_bounds__(PCD_THREADS) void k_pcd_unpack(int64_t rows_total, int64_t row_first, int row_bytes, const uint8_t* __restrict__ chunk,
                                                            PcdFields f, float* __restrict__ xyz, float* __restrict__ normals,
                                                            double* __restrict__ colors, float* __restrict__ phases,
                                                            float* __restrict__ amplitudes, double* __restrict__ seg)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t run[];                  // PCD_ROWS * row_bytes bytes
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * PCD_ROWS;                            // row0 < rows_total
    const int rows = (int)(rows_total - row0 < PCD_ROWS ? rows_total - row0 : PCD_ROWS);
    // 4-byte aligned: chunk is, and row0 is a multiple of 256
    const uint32_t* src = reinterpret_cast<const uint32_t*>(chunk + row0 * row_bytes);
    const int total = rows * row_bytes;
    for (int w = tid; w * 4 < total; w += PCD_THREADS) run[w] = src[w];             // the last dword may end 3 bytes behind the rows
    __syncthreads();
    if (tid >= rows) return;
    const uint8_t* at = reinterpret_cast<const uint8_t*>(run) + tid * row_bytes;
    const int64_t row = row_first + row0 + tid;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (f.offset[k] >= 0) xyz[row * 3 + k] = get_f32(at + f.offset[k]);
        if (f.offset[3 + k] >= 0) normals[row * 3 + k] = get_f32(at + f.offset[3 + k]);
        if (f.offset[6 + k] >= 0) colors[row * 3 + k] = (double)at[f.offset[6 + k]] / 255.0;
        if (f.offset[11 + k] >= 0) seg[row * 3 + k] = (double)at[f.offset[11 + k]] / 255.0;
    }
    if (f.offset[9] >= 0) phases[row] = get_f32(at + f.offset[9]);
    if (f.offset[10] >= 0) amplitudes[row] = get_f32(at + f.offset[10]);
}

struct PcdCreate {
    int64_t P;
    int n, colors_f64, seg_f64, scaling_cols;
    const float* xyz;
    const void* colors;
    const float* phases;
    const float* amplitudes;
    const void* seg;
    const float* log_scale;
    const float* opacity;
    float inv_c0;
    float* out_xyz;
    float* dc_color;
    float* rest_color;
    float* dc_phase;
    float* rest_phase;
    float* dc_amp;
    float* rest_amp;
    float* scaling;
    float* rotation;
    float* out_opacity;
    float* out_seg;
    float* max_radii;
};

__global__ __launch_bounds__(PCD_THREADS) void k_pcd_create(PcdCreate p)
{
    const int64_t first = (int64_t)blockIdx.x * PCD_THREADS + threadIdx.x, step = (int64_t)gridDim.x * PCD_THREADS;
    const float opacity = *p.opacity;
    for (int64_t row = first; row < p.P; row += step) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            p.out_xyz[row * 3 + k] = p.xyz[row * 3 + k];
            // RGB2SH as torch evaluates it on the device: the division by the Python scalar C0 is a product with the float nearest 1 / C0
            p.dc_color[row * 3 + k] = ((float)load_real(p.colors, p.colors_f64, row * 3 + k) - 0.5f) * p.inv_c0;
            if (p.seg) p.out_seg[row * 3 + k] = (float)load_real(p.seg, p.seg_f64, row * 3 + k);
        }
        if (p.phases) p.dc_phase[row] = (p.phases[row] - 0.5f) * p.inv_c0;
        if (p.amplitudes) p.dc_amp[row] = (p.amplitudes[row] - 0.5f) * p.inv_c0;
        const float s = p.log_scale[row];
        for (int k = 0; k < p.scaling_cols; k++) p.scaling[row * p.scaling_cols + k] = s;
        p.rotation[row * 4] = 1.f;
        p.rotation[row * 4 + 1] = 0.f;
        p.rotation[row * 4 + 2] = 0.f;
        p.rotation[row * 4 + 3] = 0.f;
        p.out_opacity[row] = opacity;
        p.max_radii[row] = 0.f;
    }
    // the coefficients beside the DC one are zeros (`features_phase[:, 1:, 1:] = 1.0` selects nothing of a 1-channel tensor)
    const int64_t rest = p.P * p.n;
    for (int64_t e = first; e < 3 * rest; e += step) p.rest_color[e] = 0.f;
    if (p.phases)
        for (int64_t e = first; e < rest; e += step) p.rest_phase[e] = 0.f;
    if (p.amplitudes)
        for (int64_t e = first; e < rest; e += step) p.rest_amp[e] = 0.f;
}

size_t pcd_lds_bytes(int row_bytes) { return (size_t)PCD_ROWS * row_bytes; }

}  // namespace

extern "C" int gft_pcd_unproject(void* hip_stream, int32_t mode, int32_t H, int32_t W, int32_t stride, const float* tof, const void* rendered,
                                 int32_t rendered_f64, const double* view, double width_m, double height_m, double znear,
                                 const float* depth_range_dev, float depth_range, const float* phase_offset_dev, float phase_offset,
                                 float* xyz, void* dist, float* amp, float* sh_color, float* color, float* sh_amp, float* amplitude,
                                 uint32_t* status)
{
    if (mode != GFT_PCD_TORF_INIT && mode != GFT_PCD_FTORF_INIT && mode != GFT_PCD_PROXY) return gft_fail("gft_pcd_unproject: bad mode %d", mode);
    // the reference keeps pixel coordinates in int16
    if (H < 1 || W < 1 || H > 32767 || W > 32767 || stride < 1) return gft_fail("gft_pcd_unproject: bad H=%d W=%d stride=%d", H, W, stride);
    if (!tof || !view || !xyz || !dist) return gft_fail("gft_pcd_unproject: NULL pointer");
    if (mode == GFT_PCD_PROXY && !rendered) return gft_fail("gft_pcd_unproject: the proxy mode needs the rendered depth image");
    if (mode == GFT_PCD_FTORF_INIT && !status) return gft_fail("gft_pcd_unproject: the ftorf_init mode needs a status block");
    PcdUnproject p = {};
    p.tof = tof;
    p.rendered = mode == GFT_PCD_PROXY ? rendered : nullptr;
    p.mode = mode;
    p.rendered_f64 = mode == GFT_PCD_PROXY && rendered_f64;
    p.H = H;
    p.W = W;
    p.stride = stride;
    p.Hp = (H + stride - 1) / stride;
    p.Wp = (W + stride - 1) / stride;
    for (int k = 0; k < 16; k++) p.view[k] = view[k];
    p.width_m = width_m;
    p.height_m = height_m;
    p.znear = znear;
    p.depth_range_dev = depth_range_dev;
    p.phase_offset_dev = phase_offset_dev;
    p.depth_range = depth_range;
    p.phase_offset = phase_offset;
    p.xyz = xyz;
    p.dist = dist;
    p.amp = amp;
    p.sh_color = sh_color;
    p.color = color;
    p.sh_amp = sh_amp;
    p.amplitude = amplitude;
    p.status = status;
    const int64_t N = (int64_t)p.Hp * p.Wp;
    hipLaunchKernelGGL(k_pcd_unproject, dim3((unsigned)((N + PCD_THREADS - 1) / PCD_THREADS)), dim3(PCD_THREADS), 0, (hipStream_t)hip_stream, p);
    return gft_launched("gft_pcd_unproject");
}

extern "C" int32_t gft_pcd_row_bytes(int32_t has_pa, int32_t has_seg) { return 27 + (has_pa ? 8 : 0) + (has_seg ? 3 : 0); }

extern "C" int gft_pcd_pack(void* hip_stream, int64_t P, const float* xyz, const void* colors, int32_t colors_f64, const float* phases,
                            const float* amplitudes, const void* seg, int32_t seg_f64, uint8_t* body, double* colors_back,
                            double* seg_back, uint32_t* status)
{
    if (P < 0 || P > PCD_MAX_ROWS) return gft_fail("gft_pcd_pack: bad row count P=%lld", (long long)P);
    if ((phases == nullptr) != (amplitudes == nullptr)) return gft_fail("gft_pcd_pack: phases and amplitudes come together or not at all");
    if (seg_back && !seg) return gft_fail("gft_pcd_pack: seg_back without seg");
    if (P == 0) return 0;
    if (!xyz || !colors || !body || !status) return gft_fail("gft_pcd_pack: NULL pointer");
    if ((uintptr_t)body & 3u) return gft_fail("gft_pcd_pack: body is not 4-byte aligned");
    const int64_t blocks = (P + PCD_ROWS - 1) / PCD_ROWS;
    if (blocks > 0x7fffffffll) return gft_fail("gft_pcd_pack: too many rows");
    const int row_bytes = gft_pcd_row_bytes(phases != nullptr, seg != nullptr);
    hipLaunchKernelGGL(k_pcd_pack, dim3((unsigned)blocks), dim3(PCD_THREADS), pcd_lds_bytes(row_bytes), (hipStream_t)hip_stream, P, row_bytes, xyz,
                       colors, (int)colors_f64, phases, amplitudes, seg, (int)seg_f64, body, colors_back, seg_back, status);
    return gft_launched("gft_pcd_pack");
}

extern "C" int gft_pcd_unpack(void* hip_stream, int64_t rows, int64_t row0, int32_t row_bytes, const uint8_t* chunk, const int32_t* offsets,
                              float* xyz, float* normals, double* colors, float* phases, float* amplitudes, double* seg)
{
    if (rows < 0 || rows > PCD_MAX_ROWS || row0 < 0 || row0 > PCD_MAX_ROWS)
        return gft_fail("gft_pcd_unpack: bad rows=%lld row0=%lld", (long long)rows, (long long)row0);
    if (row_bytes < 1 || row_bytes > GFT_PCD_MAX_ROW_BYTES)
        return gft_fail("gft_pcd_unpack: row_bytes=%d, a file row holds 1..%d bytes", row_bytes, GFT_PCD_MAX_ROW_BYTES);
    if (!offsets) return gft_fail("gft_pcd_unpack: NULL argument");
    float* const f32[4] = {xyz, normals, phases, amplitudes};
    PcdFields f;
    for (int k = 0; k < GFT_PCD_FIELDS; k++) {
        const bool byte = (k >= 6 && k < 9) || k >= 11;
        const int32_t o = offsets[k];
        if (o < -1 || (o >= 0 && o + (byte ? 1 : 4) > row_bytes)) return gft_fail("gft_pcd_unpack: field %d at byte %d of a %d-byte row", k, o, row_bytes);
        const void* dest = k < 6 ? (const void*)f32[k / 3] : k < 9 ? (const void*)colors : k < 11 ? (const void*)f32[k - 7] : (const void*)seg;
        if (o >= 0 && rows > 0 && !dest) return gft_fail("gft_pcd_unpack: the destination of field %d is NULL", k);
        f.offset[k] = o;
    }
    if (rows == 0) return 0;
    if (!chunk) return gft_fail("gft_pcd_unpack: chunk is NULL");
    if ((uintptr_t)chunk & 3u) return gft_fail("gft_pcd_unpack: chunk is not 4-byte aligned");
    const int64_t blocks = (rows + PCD_ROWS - 1) / PCD_ROWS;
    if (blocks > 0x7fffffffll) return gft_fail("gft_pcd_unpack: too many rows");
    hipLaunchKernelGGL(k_pcd_unpack, dim3((unsigned)blocks), dim3(PCD_THREADS), pcd_lds_bytes(row_bytes), (hipStream_t)hip_stream, rows, row0,
                       (int)row_bytes, chunk, f, xyz, normals, colors, phases, amplitudes, seg);
    return gft_launched("gft_pcd_unpack");
}

extern "C" int gft_pcd_create(void* hip_stream, int64_t P, int32_t n, const float* xyz, const void* colors, int32_t colors_f64,
                              const float* phases, const float* amplitudes, const void* seg, int32_t seg_f64, const float* log_scale,
                              const float* opacity, float inv_c0, int32_t scaling_cols, float* out_xyz, float* dc_color, float* rest_color,
                              float* dc_phase, float* rest_phase, float* dc_amp, float* rest_amp, float* scaling, float* rotation,
                              float* out_opacity, float* out_seg, float* max_radii)
{
    if (P < 0 || P > PCD_MAX_ROWS) return gft_fail("gft_pcd_create: bad row count P=%lld", (long long)P);
    if (n < 0 || n > 1023) return gft_fail("gft_pcd_create: bad coefficient count n=%d", n);
    if (scaling_cols != 1 && scaling_cols != 3) return gft_fail("gft_pcd_create: scaling_cols=%d, must be 1 or 3", scaling_cols);
    if (P == 0) return 0;
    if (!xyz || !colors || !log_scale || !opacity || !out_xyz || !dc_color || !scaling || !rotation || !out_opacity || !max_radii)
        return gft_fail("gft_pcd_create: NULL pointer");
    if ((n > 0 && !rest_color) || (phases && (!dc_phase || (n > 0 && !rest_phase))) || (amplitudes && (!dc_amp || (n > 0 && !rest_amp))) ||
        (seg && !out_seg))
        return gft_fail("gft_pcd_create: an input has no output");
    PcdCreate p = {};
    p.P = P;
    p.n = n;
    p.colors_f64 = colors_f64;
    p.seg_f64 = seg_f64;
    p.scaling_cols = scaling_cols;
    p.xyz = xyz;
    p.colors = colors;
    p.phases = phases;
    p.amplitudes = amplitudes;
    p.seg = seg;
    p.log_scale = log_scale;
    p.opacity = opacity;
    p.inv_c0 = inv_c0;
    p.out_xyz = out_xyz;
    p.dc_color = dc_color;
    p.rest_color = rest_color;
    p.dc_phase = dc_phase;
    p.rest_phase = rest_phase;
    p.dc_amp = dc_amp;
    p.rest_amp = rest_amp;
    p.scaling = scaling;
    p.rotation = rotation;
    p.out_opacity = out_opacity;
    p.out_seg = out_seg;
    p.max_radii = max_radii;
    const int64_t work = P * (int64_t)(3 * n > 1 ? 3 * n : 1);
    int64_t blocks = (work + PCD_THREADS - 1) / PCD_THREADS;
    if (blocks > PCD_MAX_BLOCKS) blocks = PCD_MAX_BLOCKS;
    hipLaunchKernelGGL(k_pcd_create, dim3((unsigned)blocks), dim3(PCD_THREADS), 0, (hipStream_t)hip_stream, p);
    return gft_launched("gft_pcd_create");
}
