/*
 * gftorf_debugviz.h -- C ABI of the training loop's debug images, the pipe.debug block of train.py:295-378 (libgftorf_rast.so,
 * gfx950).
 *
 * Every debug_interval iterations the reference copies about twenty full float32 planes to the host, one blocking .cpu() each,
 * and forms the images it writes in numpy.  gft_debugviz_images forms the same uint8 images on the device, into one buffer
 * (the "sheet") that one copy brings to the host: at most two launches, no host read, no atomic, no memset, the same bits on
 * every call.  Launch 1 (left out when no image is normalised by its own range) writes one row of (min, max) pairs per
 * workgroup; launch 2 folds those rows in a fixed order inside every workgroup and writes every byte of every image.
 *
 * Every statement is numpy's float32 one, rounded on its own (no contraction, correctly rounded division); none is a
 * non-IEEE function -- the two ToF depths are inputs, as the loop has them (train.py:188-189) -- so the bytes are the
 * reference's.  With the conventions of gftorf_present.h: to8b(x) = trunc(255 * clip(x, 0, 1)), a NaN giving 0;
 * norm(x, lo, hi) = (x - lo) / (hi - lo) with a NaN set to 0, then clipped to [0, 1]; selfnorm(x) = norm(x, min(x), max(x)),
 * min and max propagating a NaN as np.min / np.max do (a plane with a NaN, or with max == min, comes out all 0); magma(d) =
 * to8b(cm.magma(1 - (d - znear) / (zfar - znear))), gftorf_present.h's `depth`.  With
 *   amp = phasor[2] * tof_multiplier, gt_amp = gt_phasor[2], sp = amp * (depth * depth),
 *   sp_tof = amp * (phase_depth * phase_depth), gt_sp = gt_amp * (gt_phase_depth * gt_phase_depth)
 * the images, in the order they lie in the sheet (r = the ranges, four (lo, hi) pairs):
 *   depth                             [H, W, 4]  magma(depth)
 *   amp                               [H, W]     to8b(norm(amp, r[0], r[1]))
 *   amp_error                         [H, W]     to8b(selfnorm(|gt_amp - amp|))
 *   scattering_phase                  [H, W]     to8b(norm(sp, r[2], r[3]))
 *   scattering_phase_error            [H, W]     to8b(|gt_sp - sp|)
 *   scattering_phase_tof_depth        [H, W]     to8b(norm(sp_tof, r[4], r[5]))
 *   scattering_phase_tof_depth_error  [H, W]     to8b(|gt_sp - sp_tof|)
 *   scattering_phase_gt               [H, W]     to8b(norm(gt_sp, r[6], r[7]))
 *   depth_error                       [H, W]     to8b(selfnorm(|gt_phase_depth - depth|))
 *   phase_depth, phase_depth_gt       [H, W, 4]  magma(phase_depth), magma(gt_phase_depth)
 *   phase_depth_error                 [H, W]     to8b(selfnorm(|gt_phase_depth - phase_depth|))
 *   color, color_gt, color_error      [H, W, 3]  to8b(image[c]), to8b(gt_image[c]), to8b(|gt_image[c] - image[c]|)
 *   dd                                [H, W]     to8b(selfnorm(dd))
 *   quad                              [4, H, W]  to8b(|phasor[3 + i]|)
 *   quad_gt                           [4, H, W]  to8b(|gt_quad[permutation[i]]|)
 *   quad_error                        [4, H, W]  to8b(selfnorm(|phasor[3 + i] - gt_quad[permutation[i]]|)) where permutation[i] ==
 *                                                quad_index, each such plane by its own min and max; all 0 elsewhere
 * The ranges are what train.py:317's zip pairs the three channels with: np.min / np.max over the training sequence of
 * gt_reals for amp, of gt_imags for scattering_phase, of gt_amps for scattering_phase_tof_depth; scattering_phase_gt (line 323)
 * has gt_scattering_phases'.  An image is produced when every input its formula names is given.
 *
 * Device pointers, fp32 inputs.  A plane is H * W contiguous floats; the planes of one tensor are `stride` floats apart.
 * Returns 0 on success (gft_last_error()).
 */
#ifndef GFTORF_DEBUGVIZ_H
#define GFTORF_DEBUGVIZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* groups of inputs: what is given decides which images the sheet holds */
#define GFT_DEBUGVIZ_HAS_PHASOR 1          /* phasor, >= 3 planes */
#define GFT_DEBUGVIZ_HAS_GT_PHASOR 2       /* gt_phasor, >= 3 planes */
#define GFT_DEBUGVIZ_HAS_DEPTH 4           /* depth */
#define GFT_DEBUGVIZ_HAS_PHASE_DEPTH 8     /* phase_depth */
#define GFT_DEBUGVIZ_HAS_GT_PHASE_DEPTH 16 /* gt_phase_depth */
#define GFT_DEBUGVIZ_HAS_DD 32             /* dd */
#define GFT_DEBUGVIZ_HAS_COLOR 64          /* image and gt_image */
#define GFT_DEBUGVIZ_HAS_QUAD 128          /* phasor of exactly 7 planes (never without HAS_PHASOR) */
#define GFT_DEBUGVIZ_HAS_GT_QUAD 256       /* gt_quad (never without HAS_QUAD) */

/* the images of a sheet, in the order they lie in it */
#define GFT_DEBUGVIZ_DEPTH 0
#define GFT_DEBUGVIZ_AMP 1
#define GFT_DEBUGVIZ_AMP_ERROR 2
#define GFT_DEBUGVIZ_SP 3
#define GFT_DEBUGVIZ_SP_ERROR 4
#define GFT_DEBUGVIZ_SP_TOF 5
#define GFT_DEBUGVIZ_SP_TOF_ERROR 6
#define GFT_DEBUGVIZ_SP_GT 7
#define GFT_DEBUGVIZ_DEPTH_ERROR 8
#define GFT_DEBUGVIZ_PHASE_DEPTH 9
#define GFT_DEBUGVIZ_PHASE_DEPTH_GT 10
#define GFT_DEBUGVIZ_PHASE_DEPTH_ERROR 11
#define GFT_DEBUGVIZ_COLOR 12
#define GFT_DEBUGVIZ_COLOR_GT 13
#define GFT_DEBUGVIZ_COLOR_ERROR 14
#define GFT_DEBUGVIZ_DD 15
#define GFT_DEBUGVIZ_QUAD 16
#define GFT_DEBUGVIZ_QUAD_GT 17
#define GFT_DEBUGVIZ_QUAD_ERROR 18
#define GFT_DEBUGVIZ_IMAGES 19

#define GFT_DEBUGVIZ_ALIGN 16         /* every image starts on such a boundary of the sheet */
#define GFT_DEBUGVIZ_PARTIAL_WORDS 16 /* floats of one row of partials: (min, max) of amp_error, depth_error,
                                         phase_depth_error, dd and of the four planes of quad_error */
#define GFT_DEBUGVIZ_RANGE_WORDS 8    /* lo, hi of amp; scattering_phase; scattering_phase_tof_depth; scattering_phase_gt */
#define GFT_DEBUGVIZ_RUN 4            /* pixels of one lane */

/* Workgroups of either launch = rows of partials for an image of `pixels`; 0 when pixels < 1 (HOST). */
int64_t gft_debugviz_blocks(int64_t pixels);

/* Bytes of the sheet of an H x W view with the GFT_DEBUGVIZ_HAS_* groups `groups`; offsets_out (HOST, GFT_DEBUGVIZ_IMAGES
 * entries, or NULL) receives each image's byte offset, -1 for an image the groups do not produce.  0 for bad arguments (H or
 * W < 1, unknown bits, QUAD without PHASOR, GT_QUAD without QUAD, groups that produce no image). */
int64_t gft_debugviz_sheet_bytes(int32_t H, int32_t W, int32_t groups, int64_t* offsets_out);

/* phasor: phasor_planes (>= 3) planes phasor_stride apart, plane 2 read, or NULL with phasor_planes 0; exactly 7 planes add
 * quad, of planes 3..6.  gt_phasor: planes gt_phasor_stride apart, plane 2 read, or NULL.  depth, phase_depth, gt_phase_depth,
 * dd: one plane each, or NULL.  image, gt_image: 3 planes each, both or neither.  gt_quad: 4 planes gt_quad_stride apart, or
 * NULL; never without a 7-plane phasor.  No input is written.
 * permutation (HOST, 4 entries in 0..3, read before the call returns) and quad_index, read from quad_index_dev (DEVICE, one
 * int32) when that is not NULL, else taken by value: needed with gt_quad.
 * ranges: read from ranges_dev (DEVICE, 8 floats) when that is not NULL, else from ranges_host (HOST, 8 floats, read before
 * the call returns); needed when amp, a scattering_phase image or scattering_phase_gt is produced.
 * znear, zfar: the colour map's planes, by value.  tof_multiplier: by value.
 * partials: gft_debugviz_blocks(H * W) rows of GFT_DEBUGVIZ_PARTIAL_WORDS floats, 16-byte aligned, needed when an image
 * normalised by its own range is produced (else may be NULL); nothing in it needs clearing.
 * sheet: gft_debugviz_sheet_bytes of the groups given, 16-byte aligned; every byte of every image in it is written (the up
 * to 15 bytes between two images are not).
 * Fails before any launch on bad sizes, pointers, strides, groups or permutation. */
int gft_debugviz_images(void* hip_stream, int32_t H, int32_t W, const float* phasor, int64_t phasor_stride, int32_t phasor_planes,
                        const float* gt_phasor, int64_t gt_phasor_stride, const float* depth, const float* phase_depth,
                        const float* gt_phase_depth, const float* dd, const float* image, int64_t image_stride,
                        const float* gt_image, int64_t gt_image_stride, const float* gt_quad, int64_t gt_quad_stride,
                        const int32_t* permutation, const int32_t* quad_index_dev, int32_t quad_index, const float* ranges_dev,
                        const float* ranges_host, float znear, float zfar, float tof_multiplier, void* partials, void* sheet);

#ifdef __cplusplus
}
#endif
#endif
