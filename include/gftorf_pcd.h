/*
 * gftorf_pcd.h -- C ABI of the input point cloud: ToF frames to world points, the cloud's PLY rows and the model's first
 * tensors (scene/dataset_readers.py:110-150, 530-586, 904-973, 1067-1118; scene/gaussian_model.py:180-236)
 * (libgftorf_rast.so, gfx950).
 *
 *   gft_pcd_unproject  the grid pixels of one ToF frame to world points: one launch per frame
 *   gft_pcd_pack       the rows of storePly's file, 27 / 30 / 35 / 38 bytes each, as they lie in the file: one launch
 *   gft_pcd_unpack     the reverse for a chunk of file rows already on the device: one launch per chunk
 *   gft_pcd_create     the tensors of GaussianModel.create_from_pcd in their final layout: one launch
 *
 * Device pointers; arrays marked HOST are read before the call returns.  Returns 0 on success (gft_last_error()).
 */
#ifndef GFTORF_PCD_H
#define GFTORF_PCD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFT_PCD_ROWS 256            /* rows per workgroup of pack and unpack */
#define GFT_PCD_MAX_ROW_BYTES 128   /* bytes of a file row unpack takes */
#define GFT_PCD_FIELDS 14           /* entries of unpack's offset table: x y z nx ny nz red green blue phase amplitude seg_* */
#define GFT_PCD_STATUS_WORDS 2      /* uint32 words of a status block */

/* modes of gft_pcd_unproject */
#define GFT_PCD_TORF_INIT 0         /* 2 N rows, the second half a copy of the first (dataset_readers.py:545, :559) */
#define GFT_PCD_FTORF_INIT 1        /* N rows, the distance unwrapped by the rule of :929-946 */
#define GFT_PCD_PROXY 2             /* 2 N rows, the first half from the frame, the second from `rendered` (:1092-1096) */

/* tof [H, W, 3] float32, contiguous.  The grid is Hp = ceil(H / stride) by Wp = ceil(W / stride), N = Hp * Wp, grid pixel i
 * reading image pixel ((i / Wp) * stride, (i % Wp) * stride).  view [16] HOST doubles: the row-major world-to-view matrix;
 * its inverse is formed in double on the device.  width_m / height_m: znear * tan(Fov / 2) * 2 of the two axes.
 * depth_range / phase_offset: the device value (one float) when the pointer is not NULL, else the one by value.
 * rendered (GFT_PCD_PROXY only) [H, W], float64 when rendered_f64 else float32.
 * Outputs, `rows` = N or 2 N of them, each pointer the frame's first row: xyz [rows, 3] float32; dist [rows] (float64 when
 * rendered_f64 in GFT_PCD_PROXY, else float32); and, each NULL or [rows] float32 ([rows, 3] for color): amp = tof[..., 2],
 * sh_color = RGB2SH(amp), color = SH2RGB(sh_color) three times, sh_amp = PA2SH(amp * dist^2), amplitude = SH2PA(sh_amp).
 * status [GFT_PCD_STATUS_WORDS] uint32 (GFT_PCD_FTORF_INIT only, added to): word 0 counts the pixels with no candidate kept,
 * word 1 those whose amplitude index (i / Wp, i % Hp) lies outside the image; such a pixel's outputs are NaN. */
int gft_pcd_unproject(void* hip_stream, int32_t mode, int32_t H, int32_t W, int32_t stride, const float* tof, const void* rendered,
                      int32_t rendered_f64, const double* view, double width_m, double height_m, double znear,
                      const float* depth_range_dev, float depth_range, const float* phase_offset_dev, float phase_offset, float* xyz,
                      void* dist, float* amp, float* sh_color, float* color, float* sh_amp, float* amplitude, uint32_t* status);

/* bytes of a file row: 27, + 8 with phase and amplitude, + 3 with the seg colours */
int32_t gft_pcd_row_bytes(int32_t has_pa, int32_t has_seg);

/* xyz [P, 3] float32; colors / seg [P, 3], float64 when the flag says so, else float32, already multiplied by 255; phases and
 * amplitudes [P] float32, both or neither; seg may be NULL.  Inputs need their element's alignment only.  body: P * row bytes
 * of the file behind its header, 4-byte aligned.  A colour v becomes the byte (int)v for -1 < v < 256; any other value
 * becomes 0 and is counted in status [GFT_PCD_STATUS_WORDS] (added to): word 0 the numbers (the infinities too), word 1 the NaNs.
 * colors_back / seg_back: NULL or [P, 3] float64, byte / 255.0 as fetchPly reads it.  P == 0 launches nothing. */
int gft_pcd_pack(void* hip_stream, int64_t P, const float* xyz, const void* colors, int32_t colors_f64, const float* phases,
                 const float* amplitudes, const void* seg, int32_t seg_f64, uint8_t* body, double* colors_back, double* seg_back,
                 uint32_t* status);

/* chunk: file rows row0 .. row0 + rows - 1, row_bytes each (<= GFT_PCD_MAX_ROW_BYTES), 4-byte aligned and readable up to the
 * next multiple of 4 bytes.  offsets [GFT_PCD_FIELDS] HOST: the byte offset within a row of x y z nx ny nz (float), red green
 * blue (uchar), phase amplitude (float), seg_red seg_green seg_blue (uchar), or -1 for a field the file does not have (its
 * destination is not written).  Destinations are whole tensors (row 0): xyz, normals [P, 3] float32; colors, seg [P, 3]
 * float64 = byte / 255.0; phases, amplitudes [P] float32.  rows == 0 launches nothing. */
int gft_pcd_unpack(void* hip_stream, int64_t rows, int64_t row0, int32_t row_bytes, const uint8_t* chunk, const int32_t* offsets,
                   float* xyz, float* normals, double* colors, float* phases, float* amplitudes, double* seg);

/* The tensors of create_from_pcd, each contiguous float32: xyz [P, 3]; colors / seg [P, 3] (float64 when the flag says so);
 * phases, amplitudes, seg NULL or as in gft_pcd_pack; log_scale [P] = log(sqrt(clamp_min(dist2, 1e-7))), formed by torch (the device's logf / sqrtf in a kernel do not give torch's bits); opacity: one float,
 * inverse_sigmoid(initial_opacity).  n = (max_sh_degree + 1)^2 - 1; inv_c0 = the float nearest 1 / C0, which torch's RGB2SH multiplies by;
 * scaling_cols 1 or 3.  Outputs: out_xyz [P, 3]; dc_color [P, 1, 3], rest_color [P, n, 3]; dc_phase / dc_amp [P, 1, 1] and
 * rest_phase / rest_amp [P, n, 1] (NULL without their input); scaling [P, scaling_cols]; rotation [P, 4]; out_opacity
 * [P, 1]; out_seg [P, 3]; max_radii [P]. */
int gft_pcd_create(void* hip_stream, int64_t P, int32_t n, const float* xyz, const void* colors, int32_t colors_f64,
                   const float* phases, const float* amplitudes, const void* seg, int32_t seg_f64, const float* log_scale,
                   const float* opacity, float inv_c0, int32_t scaling_cols, float* out_xyz, float* dc_color, float* rest_color,
                   float* dc_phase, float* rest_phase, float* dc_amp, float* rest_amp, float* scaling, float* rotation,
                   float* out_opacity, float* out_seg, float* max_radii);

#ifdef __cplusplus
}
#endif
#endif
