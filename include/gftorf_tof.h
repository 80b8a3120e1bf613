/*
 * gftorf_tof.h -- C ABI of the ToF depth and of the training log's scalars (libgftorf_rast.so, gfx950).
 *
 * The reference's iteration log (train.py:188-200, 402-433) builds phase_depth and gt_phase_depth with
 * scene/torf_utils.py:59-64 depth_from_tof_torch (reading depth_range and the phase offset with .item()), copies five
 * images to the host, forms the scattering-phase maps and their errors in numpy and reduces them to scalars, next to two
 * means over get_features_phasor[:, 0, 1] (one through a boolean selection, a host read of the row count) and five .item()s
 * of loss terms: ~40 small launches, five image-sized copies and ~10 blocking reads per iteration, none of which can sit in
 * a captured graph.  Here:
 *   gft_tof_depth     depth_from_tof_torch as one launch, depth_range and the offset by value or read from the DEVICE
 *   gft_tof_log_row   every scalar of the log as one row of GFT_TOF_LOG_WORDS words: two launches (the sums, then one
 *                     workgroup that finishes them), no host read, no atomic, no memset; with a cursor the row goes into a
 *                     ring, so a captured call lands in the next slot at every replay
 *
 * depth_from_tof_torch in fp32, in the reference's order:
 *   real  = |re| < 1e-6f ? 1e-6f : re         (the threshold compared in fp32, as torch compares a Python scalar)
 *   phase = atan2f(im, real) - phase_offset;  phase += 2 pi where phase < 0;  depth = phase * depth_range / (4 pi)
 *
 * With amp = phasor[2] * tof_multiplier, gt_amp = gt_phasor[2], pd / gpd the ToF depth of phasor / gt_phasor,
 * sp = amp * depth^2, sp_tof = amp * pd^2, gsp = gt_amp * gpd^2 the row holds the means over the pixels listed below, the
 * mean of SH2PA(a) = a * C0 + 0.5 (C0 = 0.28209479177387814) over the amplitude coefficients a of all rows and of the
 * visible rows, the visible count, up to GFT_TOF_LOG_MAX_EXTRAS floats copied from the device, and a sequence number.
 * An absent optional input gives 0 in its slots and a cleared bit in GFT_TOF_LOG_PRESENT.  The one difference from the
 * reference: an EMPTY visible selection gives 0, where the mean of an empty tensor is NaN.
 *
 * Device pointers, fp32.  An image is `pixels` contiguous floats; a phasor is three such planes `plane_stride` floats apart
 * (gft_tof_depth reads planes 0 and 1 only), so the first planes of a wider tensor are taken in place.  No pointer needs
 * more than its element's alignment.  Returns 0 on success (gft_last_error()).
 */
#ifndef GFTORF_TOF_H
#define GFTORF_TOF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* one row of the log, 4-byte words (floats unless noted) */
#define GFT_TOF_LOG_SP 0             /* mean(sp)                    train_loss_patches/mean_scattering_phase */
#define GFT_TOF_LOG_SP_TOF 1         /* mean(sp_tof)                mean_scattering_phase_tof_depth */
#define GFT_TOF_LOG_GSP 2            /* mean(gsp)                   mean_scattering_phase_gt */
#define GFT_TOF_LOG_SP_ERR 3         /* mean(|gsp - sp|)            mean_scattering_phase_error */
#define GFT_TOF_LOG_SP_TOF_ERR 4     /* mean(|gsp - sp_tof|)        scattering_phase_tof_depth_error */
#define GFT_TOF_LOG_DEPTH_ERR 5      /* mean(|depth - gt_depth|)    mean_depth_error (0 without gt_depth) */
#define GFT_TOF_LOG_TOF_DEPTH_ERR 6  /* mean(|pd - gpd|)            mean_tof_depth_error */
#define GFT_TOF_LOG_AMP_ERR 7        /* mean(|amp - gt_amp|)        mean_amp_error */
#define GFT_TOF_LOG_DD 8             /* mean(depth_distortion)      dd_loss before its weight (0 without the image) */
#define GFT_TOF_LOG_GS_SP 9          /* mean(SH2PA(a)), all rows    mean_gs_scattering_phase (0 without coefficients) */
#define GFT_TOF_LOG_GS_SP_VISIBLE 10 /* the same over visible rows  mean_gs_scattering_phase_visible (0 when none is) */
#define GFT_TOF_LOG_VISIBLE 11       /* uint32: visible rows */
#define GFT_TOF_LOG_PRESENT 12       /* uint32: GFT_TOF_HAS_* of the optional inputs given */
#define GFT_TOF_LOG_NUM_EXTRAS 13    /* uint32: extras copied */
#define GFT_TOF_LOG_SEQ 14           /* uint32: the cursor's value when the row was written (0 without a cursor) */
#define GFT_TOF_LOG_EXTRAS 16        /* float[GFT_TOF_LOG_MAX_EXTRAS]: *extras[k], 0 beyond num_extras (word 15 is 0) */
#define GFT_TOF_LOG_MAX_EXTRAS 8
#define GFT_TOF_LOG_WORDS 24

#define GFT_TOF_HAS_GT_DEPTH 1
#define GFT_TOF_HAS_DD 2
#define GFT_TOF_HAS_AMP 4
#define GFT_TOF_HAS_VISIBLE 8

/* 4-byte words of one row of `partials`: eleven fp32 sums in the order of the row's means, one uint32 count */
#define GFT_TOF_PARTIAL_WORDS 12

/* out[i] = depth_from_tof_torch of (tof[i], tof[plane_stride + i]), i < pixels.  depth_range is read from
 * depth_range_dev (DEVICE, one float) when that is not NULL, else taken by value; phase_offset likewise. */
int gft_tof_depth(void* hip_stream, int64_t pixels, const float* tof, int64_t plane_stride, const float* depth_range_dev,
                  float depth_range, const float* phase_offset_dev, float phase_offset, float* out);

/* Workgroups of a gft_tof_log_row launch = rows of `partials`, for `pixels` pixels and P amplitude rows (0 without
 * coefficients).  0 when pixels < 1 or P < 0. */
int64_t gft_tof_log_blocks(int64_t pixels, int64_t P);

/* phasor, gt_phasor: three planes each; depth [pixels]; gt_depth, depth_distortion [pixels] or NULL.  amp: the first of P
 * amplitude coefficients `amp_stride` floats apart (get_features_phasor[:, 0, 1] in place, or _features_dc_amp), or NULL;
 * visible: bool [P] (visible_is_radii = 0) or the rasterizer's int32 radii [P] (1), visible where > 0, or NULL (never without
 * amp).  extras: HOST array of num_extras <= GFT_TOF_LOG_MAX_EXTRAS device pointers to one float each.
 * partials [gft_tof_log_blocks(pixels, amp ? P : 0)][GFT_TOF_PARTIAL_WORDS] is written in full.  rows: [slots] rows of
 * GFT_TOF_LOG_WORDS words.  With cursor (DEVICE, one uint32) the finish kernel writes row *cursor % slots with
 * seq = *cursor and then stores *cursor + 1; without it, row 0 with seq 0 (slots must be >= 1 either way). */
int gft_tof_log_row(void* hip_stream, int64_t pixels, int64_t P, const float* phasor, int64_t phasor_plane_stride,
                    const float* depth, const float* gt_phasor, int64_t gt_plane_stride, const float* depth_range_dev,
                    float depth_range, const float* phase_offset_dev, float phase_offset, float tof_multiplier,
                    const float* gt_depth, const float* depth_distortion, const float* amp, int64_t amp_stride,
                    const void* visible, int32_t visible_is_radii, const float* const* extras, int32_t num_extras,
                    void* partials, void* rows, int64_t slots, void* cursor);

#ifdef __cplusplus
}
#endif
#endif
