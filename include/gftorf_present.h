/*
 * gftorf_present.h -- C ABI of a rendered view's display images, render.py:105-189 and :43-54 (libgftorf_rast.so, gfx950).
 *
 * The reference's render program copies, per view, the colour image, the phasor, the depth, the accumulation and the depth
 * distortion to the host as float32 (over a dozen blocking copies, about 130 bytes per pixel) and forms the images it
 * writes in numpy: phasor2real_img_amp, normalize_im_gt, normalize_im, depth_from_tof, depth / acc, cm.magma(1 - (d - znear)
 * / (zfar - znear)) and to8b (scene/torf_utils.py:11-29, 53-57; utils/graphics_utils.py:117-137).  Here the uint8 images are
 * formed on the device, into one buffer (the "sheet") that one copy brings to the host:
 *   gft_present_view          the images of one view: two launches (min / max partials of dd, left out without dd; then
 *                             every workgroup finishes those partials and writes its pixels), no host read, no atomic, no
 *                             memset
 *   gft_present_ranges        folds one ground-truth ToF image into the six (lo, hi) of save_input's np.min / np.max over the
 *                             whole sequence (render.py:46-47, 61): a partials launch and a one-workgroup finish
 *   gft_present_ranges_reset  sets the six values to (+inf, -inf) pairs with a kernel
 *   gft_present_quad          the four quad images of render_ftorf_viz_traj.py:237-244 (tof_to_image, the seismic map): one launch
 *
 * Every statement is numpy's float32 sequence, operation for operation (no contraction, correctly rounded division), so
 * the bytes are the reference's; only arctan2 is not an IEEE operation.  With to8b(x) = trunc(255 * clip(x, 0, 1)), a NaN
 * giving 0, and norm(x, lo, hi) = (x - lo) / (hi - lo) with a NaN set to 0, then clipped to [0, 1]:
 *   color       [H, W, 3]  to8b(image[c])
 *   real, imag  [H, W, 3]  v = phasor[0 or 1] * tof_multiplier; R = v <= 0 ? 0 : v, G = 0, B = v >= 0 ? -0 : -v;
 *                          to8b(norm(., lo, hi)) of each with the (lo, hi) of `real` / `imag`
 *   amp         [H, W]     to8b(norm(phasor[2] * tof_multiplier, lo, hi)) with the (lo, hi) of `amp`
 *   quad        [4, H, W]  to8b(|phasor[3 + k]|), when the phasor has 7 planes
 *   depth, depth_tof, depth_norm  [H, W, 4]  magma(1 - (d - znear) / (zfar - znear)): d = depth; the ToF depth of phasor
 *                          planes 0 and 1 (not multiplied; numpy's depth_from_tof, which does not clamp the real part);
 *                          depth / acc.  magma(x) is row min(trunc(x * 256), 255) of gft_present_magma(), row 0 for x < 0
 *                          and row 256 = (0, 0, 0, 0) for a NaN, as matplotlib indexes a 256-entry map with a float32
 *   dd          [H, W]     to8b(norm(dd, min(dd), max(dd))); min and max propagate a NaN as np.min / np.max do
 *   depth_tof_f, depth_norm_f  float32 [H, W]: the two derived depths themselves
 *
 * Device pointers, fp32 inputs.  A plane is H * W contiguous floats; the planes of one tensor are `stride` floats apart.
 * Returns 0 on success (gft_last_error()).
 */
#ifndef GFTORF_PRESENT_H
#define GFTORF_PRESENT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* groups of inputs: what is given decides which images the sheet holds */
#define GFT_PRESENT_HAS_COLOR 1   /* image: color */
#define GFT_PRESENT_HAS_PHASOR 2  /* phasor, >= 3 planes: real, imag, amp, depth_tof, depth_tof_f */
#define GFT_PRESENT_HAS_QUAD 4    /* phasor of exactly 7 planes: quad */
#define GFT_PRESENT_HAS_DEPTH 8   /* depth: depth */
#define GFT_PRESENT_HAS_ACC 16    /* acc (with depth): depth_norm, depth_norm_f */
#define GFT_PRESENT_HAS_DD 32     /* dd: dd */

/* the images of a sheet, in the order they lie in it */
#define GFT_PRESENT_COLOR 0
#define GFT_PRESENT_REAL 1
#define GFT_PRESENT_IMAG 2
#define GFT_PRESENT_AMP 3
#define GFT_PRESENT_QUAD 4
#define GFT_PRESENT_DEPTH 5
#define GFT_PRESENT_DEPTH_TOF 6
#define GFT_PRESENT_DEPTH_NORM 7
#define GFT_PRESENT_DD 8
#define GFT_PRESENT_DEPTH_TOF_F 9
#define GFT_PRESENT_DEPTH_NORM_F 10
#define GFT_PRESENT_IMAGES 11

#define GFT_PRESENT_ALIGN 16        /* every image starts on such a boundary of the sheet */
#define GFT_PRESENT_PARTIAL_WORDS 2 /* floats of one row of gft_present_view's partials: min, max of dd */
#define GFT_PRESENT_RANGE_WORDS 6   /* lo, hi of real; of imag; of amp */
#define GFT_PRESENT_MAGMA_ROWS 257  /* 256 entries, then the NaN row */
#define GFT_PRESENT_SEISMIC_ROWS 257 /* 256 entries, then the NaN row */

/* Workgroups of a launch = rows of partials for an image of `pixels`; 0 when pixels < 1. */
int64_t gft_present_blocks(int64_t pixels);

/* Bytes of the sheet of an H x W view with the GFT_PRESENT_HAS_* groups `groups`; offsets_out (HOST, GFT_PRESENT_IMAGES
 * entries, or NULL) receives each image's byte offset, -1 for an image the groups do not produce.  0 for bad arguments
 * (H or W < 1, unknown bits, QUAD without PHASOR, ACC without DEPTH, no group). */
int64_t gft_present_sheet_bytes(int32_t H, int32_t W, int32_t groups, int64_t* offsets_out);

/* The 257 x 4 bytes of to8b(cm.magma(.)): rows 0..255 the map's entries, row 256 the NaN colour (HOST, static). */
const uint8_t* gft_present_magma(void);

/* image: 3 planes image_stride apart, or NULL.  phasor: phasor_planes (>= 3) planes phasor_stride apart, or NULL with
 * phasor_planes 0; exactly 7 planes add quad.  depth, acc (never without depth), dd: one plane each, or NULL.
 * ranges: the six (lo, hi) of real, imag, amp, read from ranges_dev (DEVICE, 6 floats) when that is not NULL, else from
 * ranges_host (HOST, 6 floats, read before the call returns); needed with phasor.  depth_range and phase_offset are read
 * from their _dev pointer (DEVICE, one float) when that is not NULL, else taken by value; needed with phasor.  znear, zfar:
 * the colour map's planes, needed with phasor or depth.
 * partials: gft_present_blocks(H * W) rows of GFT_PRESENT_PARTIAL_WORDS floats, needed with dd (else may be NULL).
 * sheet: gft_present_sheet_bytes of the groups given, 16-byte aligned; every byte of every image in it is written (the
 * up to 15 bytes between two images are not). */
int gft_present_view(void* hip_stream, int32_t H, int32_t W, const float* image, int64_t image_stride, const float* phasor,
                     int64_t phasor_stride, int32_t phasor_planes, const float* depth, const float* acc, const float* dd,
                     const float* ranges_dev, const float* ranges_host, const float* depth_range_dev, float depth_range,
                     const float* phase_offset_dev, float phase_offset, float znear, float zfar, float tof_multiplier,
                     void* partials, void* sheet);

/* gt_tof: planes 0..2 of `pixels` floats, stride apart (the ground truth is not multiplied).  ranges (DEVICE, 6 floats):
 * lo = min(lo, .), hi = max(hi, .) over the three channels of the red / blue images as the reference forms them (so the lo
 * of real and imag is at most 0), and over the amplitude plane; a NaN stays.  partials: gft_present_blocks(pixels) rows of
 * GFT_PRESENT_RANGE_WORDS floats. */
int gft_present_ranges(void* hip_stream, int64_t pixels, const float* gt_tof, int64_t stride, void* partials, float* ranges);

/* ranges (DEVICE, 6 floats) = (+inf, -inf) three times, by a kernel (no memset node) */
int gft_present_ranges_reset(void* hip_stream, float* ranges);

/* The 257 x 4 bytes of trunc(255 * seismic(.)): rows 0..255 matplotlib's `seismic` entries, row 256 the NaN colour (HOST,
 * static); the fourth byte of a row is not shown. */
const uint8_t* gft_present_seismic(void);

/* tof_to_image (scene/torf_utils.py:43-50) of the four quad planes, render_ftorf_viz_traj.py:237-244, in one launch.  phasor: 7
 * planes phasor_stride apart; permutation (HOST, 4 entries in 0..3, read before the call returns): image i shows plane 3 +
 * permutation[i].  v = plane value, minus 0.5f when has_gt, then v / (1 + v) when tonemap; c = clip(v, -0.5, 0.5), a NaN
 * stays; n = c + 0.5f; the pixel is the first three bytes of row min(trunc(n * 256), 255) of gft_present_seismic(), of row
 * 256 for a NaN -- matplotlib's index of the float32 Normalize(-0.5, 0.5).  out: uint8 [4, H, W, 3], every byte written. */
int gft_present_quad(void* hip_stream, int32_t H, int32_t W, const float* phasor, int64_t phasor_stride,
                     const int32_t* permutation, int32_t has_gt, int32_t tonemap, void* out);

#ifdef __cplusplus
}
#endif
#endif
