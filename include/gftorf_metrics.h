/*
 * gftorf_metrics.h -- C ABI of a view's evaluation metrics, train.py:535-579 (libgftorf_rast.so, gfx950).
 *
 * The reference's evaluation pass (train.py:508-603 training_report) renders every test and train camera and evaluates,
 * per view, the statements of train.py:535-566 eagerly: l1_loss and psnr of the colour image, l1_loss, l2_loss and psnr of
 * the selected ToF channels, depth_from_tof_torch of the rendered phasor (depth_range and the phase offset read with
 * .item()), l1_loss and l2_loss of the rendered depth and l2_loss of the ToF depth against the ground-truth distance, and
 * eight `+= x.mean().double()` (utils/image_utils.py:14-19 mse / psnr; utils/loss_utils.py l1_loss / l2_loss): ~45 small
 * launches and two blocking reads per view, none of which can sit in a captured graph; train.py:570-579 divides the eight
 * sums by the number of views.  Here:
 *   gft_view_metrics   the eight values of one view: two launches (the sums, then one workgroup that finishes them), no
 *                      host read, no atomic, no memset; written as a row of floats and / or added into an accumulator
 *   gft_metrics_reset  zeroes an accumulator
 *
 * Up to GFT_METRICS_MAX_PLANES plane pairs (rendered, ground truth) are read in one pass, in two groups with pixel counts
 * of their own (the colour camera and the ToF sensor have their own image sizes, gaussian_renderer/__init__.py:37-38,
 * 58-59).  The pairs are numbered in this order, and the per-plane words of a row are in that order too:
 *   group A  `channels_a` planes of `pixels_a` floats: the colour image
 *   group B  `pixels_b` floats per plane: `channels_b` selected ToF channels; then depth against gt_depth (when depth is
 *            given); then the ToF depth against gt_depth (when phasor is given), formed per pixel from planes 0 and 1 of
 *            `phasor` exactly as gft_tof_depth (gftorf_tof.h) forms it
 * Per pair: S1 = sum |a - b| and S2 = sum (a - b)^2, fp32 per thread, the threads' sums and the workgroups' rows added in
 * double in a fixed order.  With mse_c = S2_c / pixels and psnr_c = 20 log10(1 / sqrt(mse_c)) (+inf when mse_c is 0, as the
 * reference; no clamp):
 *   l1     = sum_c S1_c / (channels_a pixels_a)      psnr   = mean_c psnr_c                      over group A's planes
 *   l1_p, l2_p = sum_c S1_c, S2_c / (channels_b pixels_b),  psnr_p = mean_c psnr_c               over the ToF channels
 *   l1_d, l2_d = S1, S2 / pixels_b of the depth pair;  l2_d_tof = S2 / pixels_b of the ToF depth pair
 * An absent group leaves 0 in its values (the reference's sums stay at 0.0) and its GFT_METRICS_HAS_* bit cleared.  The
 * one difference from the reference: a view's value is added to the accumulator before it is rounded to float32, where the
 * reference adds the float32 mean.
 *
 * Device pointers, fp32.  A plane is `pixels` contiguous floats; the planes of one tensor are `stride` floats apart, so
 * phasor[:n], or one quad channel of the 7-plane tensor (channels_b = 1), is read in place.  No pointer needs more than its
 * element's alignment, `partials` and `accum` that of a double.  Returns 0 on success (gft_last_error()).
 */
#ifndef GFTORF_METRICS_H
#define GFTORF_METRICS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFT_METRICS_MAX_PLANES 8

/* the eight values, in the order of a row's first floats and of the accumulator's doubles */
#define GFT_METRICS_L1 0        /* train.py:537  l1_loss(rendered_image, gt_image) */
#define GFT_METRICS_PSNR 1      /* :538          psnr(rendered_image, gt_image).mean() */
#define GFT_METRICS_L1_P 2      /* :550          l1_loss(tof_rendered, tof_gt) */
#define GFT_METRICS_L2_P 3      /* :551          l2_loss(tof_rendered, tof_gt) */
#define GFT_METRICS_PSNR_P 4    /* :552          psnr(tof_rendered, tof_gt).mean() */
#define GFT_METRICS_L1_D 5      /* :564          l1_loss(rendered_depth, gt_depth) */
#define GFT_METRICS_L2_D 6      /* :565          l2_loss(rendered_depth, gt_depth) */
#define GFT_METRICS_L2_D_TOF 7  /* :566          l2_loss(rendered_depth_tof, gt_depth) */
#define GFT_METRICS_VALUES 8

/* one row, 4-byte words (floats unless noted) */
#define GFT_METRICS_ROW_MSE 8       /* float[GFT_METRICS_MAX_PLANES]: mse of every pair in their order, 0 beyond the last */
#define GFT_METRICS_ROW_PSNR 16     /* float[GFT_METRICS_MAX_PLANES]: psnr of every pair, 0 beyond the last */
#define GFT_METRICS_ROW_PRESENT 24  /* uint32: GFT_METRICS_HAS_* of the groups given */
#define GFT_METRICS_ROW_PLANES 25   /* uint32: pairs read (words 26 and 27 are 0) */
#define GFT_METRICS_ROW_WORDS 28

/* the accumulator block, 4-byte words: eight doubles, then two uint32 */
#define GFT_METRICS_ACC_SUMS 0      /* double[GFT_METRICS_VALUES]: the views' values added in the order they were given */
#define GFT_METRICS_ACC_VIEWS 16    /* uint32: views added */
#define GFT_METRICS_ACC_PRESENT 17  /* uint32: the OR of the views' GFT_METRICS_HAS_* */
#define GFT_METRICS_ACC_WORDS 18

#define GFT_METRICS_HAS_COLOUR 1
#define GFT_METRICS_HAS_TOF 2
#define GFT_METRICS_HAS_DEPTH 4
#define GFT_METRICS_HAS_TOF_DEPTH 8

/* 4-byte words of one row of `partials`: S1 and S2 (doubles) of the up to eight pairs read from memory, then of the ToF depth */
#define GFT_METRICS_PARTIAL_WORDS 36

/* Workgroups of a gft_view_metrics launch = rows of `partials`, for `pixels` = the larger of pixels_a and pixels_b.
 * 0 when pixels < 1. */
int64_t gft_metrics_blocks(int64_t pixels);

/* image, gt_image: channels_a planes of pixels_a floats, image_stride / gt_image_stride floats apart (channels_a = 0: no
 * group A, the pointers are not read).  tof, gt_tof: channels_b planes of pixels_b floats likewise.  depth, gt_depth
 * [pixels_b] or NULL (depth never without gt_depth); phasor: planes 0 and 1 of pixels_b floats phasor_stride apart, or
 * NULL (never without gt_depth).  depth_range is read from depth_range_dev (DEVICE, one float) when that is not NULL, else
 * taken by value; phase_offset likewise.  At least one pair, at most GFT_METRICS_MAX_PLANES in all.
 * partials [gft_metrics_blocks(max(pixels_a, pixels_b))][GFT_METRICS_PARTIAL_WORDS] is written in full.
 * row: GFT_METRICS_ROW_WORDS words, written in full, or NULL.  accum: GFT_METRICS_ACC_WORDS words, 8-byte aligned, or
 * NULL: one thread adds the eight values in double, in their order, then stores views + 1 and present | this view's. */
int gft_view_metrics(void* hip_stream, int64_t pixels_a, int32_t channels_a, const float* image, int64_t image_stride,
                     const float* gt_image, int64_t gt_image_stride, int64_t pixels_b, int32_t channels_b, const float* tof,
                     int64_t tof_stride, const float* gt_tof, int64_t gt_tof_stride, const float* depth, const float* gt_depth,
                     const float* phasor, int64_t phasor_stride, const float* depth_range_dev, float depth_range,
                     const float* phase_offset_dev, float phase_offset, void* partials, void* row, void* accum);

/* accum: GFT_METRICS_ACC_WORDS words, all set to 0 by a kernel (no memset node) */
int gft_metrics_reset(void* hip_stream, void* accum);

#ifdef __cplusplus
}
#endif
#endif
