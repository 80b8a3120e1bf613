/*
 * gftorf_reg.h -- C ABI of the per-Gaussian regularisers of the training loss (libgftorf_rast.so, gfx950).
 *
 * Besides the image terms (gftorf_loss.h) and the scene-flow term (gftorf_flow.h) the reference adds four small terms to
 * `loss` (train.py:237-240, 266-277), each a mean:
 *   motion            lambda_mlp_reg * mean(|d_xyz|)                                                  over [Nd, 3]
 *   depth distortion  lambda_dd      * mean(depth_distortion)                                         over [1, H, W]
 *   opacity entropy   lambda_oe      * mean(-o log(o + 1e-10) - (1 - o) log(1 - o + 1e-10)),  o = get_opacity[get_motion_mask]
 *   scale             lambda_scale   * mean(mean(s, -1)^2),                                   s = get_scaling[visibility_filter]
 * In eager PyTorch that is ~20 launches forward and as many backward, and the two `t[bool_mask]` selections run `nonzero`
 * and read the row count back on the host.  Here: two launches forward (the sums, then one workgroup that finishes them),
 * one backward, over the concatenation of the four inputs.  Nothing reads a value back to the host, nothing uses an atomic
 * or a memset: every entry point can be captured in a graph, and the masks, the radii and the weights are read when the
 * kernels run.
 *
 * A term is absent when its tensor is NULL.  The one difference from the reference: an EMPTY selection (no True in the
 * mask, no visible row, Nd = 0) gives 0 for its term and zero gradients, where the mean of an empty tensor is NaN.
 *
 * Device pointers; fp32 tensors contiguous: d_xyz [Nd, 3] (n_dxyz = 3 * Nd floats), opacity [P] or [P, 1], scaling
 * [P, scaling_cols] with scaling_cols 3 or 1 (1: the reference's isotropic_gaussians, whose get_scaling repeats the column,
 * so the row mean is the value itself), depth_distortion `pixels` floats.  motion_mask is bool [P] (one byte per row,
 * non-zero = dynamic).  `visible` is bool [P] (visible_is_radii = 0) or the rasterizer's int32 radii [P]
 * (visible_is_radii = 1): a row is visible when the value is > 0.  With opacity_is_raw the kernels apply
 * o = 1 / (1 + exp(-raw)) first, with scaling_is_raw s = exp(raw) (scene/gaussian_model.py get_opacity / get_scaling), and
 * the gradients are those of the raw tensors.  No pointer needs more than its element's alignment.
 * Returns 0 on success (gft_last_error()).
 */
#ifndef GFTORF_REG_H
#define GFTORF_REG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4-byte words of one row of `partials`: four fp32 sums (motion, entropy, scale, distortion), two uint32 row counts (dynamic,
 * visible), two unused */
#define GFT_REG_PARTIAL_WORDS 8

/* the result block, 4-byte words: */
#define GFT_REG_MEANS 0      /* float[4]: the unweighted means -- motion, opacity entropy, scale, depth distortion */
#define GFT_REG_COUNTS 4     /* int32[2]: selected rows -- dynamic (motion_mask), visible */
#define GFT_REG_RECIPS 6     /* float[4]: 1 / (3 Nd), 1 / max(n_dynamic, 1), 1 / max(n_visible, 1), 1 / pixels (0 when absent) */
#define GFT_REG_TOTAL 10     /* float: sum of weight * mean over the four terms */

/* Workgroups of a gft_reg_forward launch = rows of `partials`, for the index space n_dxyz + 2 * P + pixels (pass 0 for an
 * absent term; P = 0 when neither opacity nor scaling is given).  0 when a size is negative or all are 0. */
int64_t gft_reg_blocks(int64_t n_dxyz, int64_t P, int64_t pixels);

/* 4-byte words of the result block */
int64_t gft_reg_result_words(void);

/* partials [gft_reg_blocks(...)][GFT_REG_PARTIAL_WORDS] and result [gft_reg_result_words()] are written in full.  The four
 * weights are read from weights_dev (DEVICE, four floats: mlp, oe, scale, dd) when it is not NULL, else taken by value.
 * opacity and motion_mask come together or not at all, and so do scaling and visible. */
int gft_reg_forward(void* hip_stream, int64_t n_dxyz, int64_t P, int64_t pixels, const float* d_xyz,
                    const float* opacity, const void* motion_mask, int32_t opacity_is_raw,
                    const float* scaling, int32_t scaling_cols, int32_t scaling_is_raw, const void* visible, int32_t visible_is_radii,
                    const float* depth_distortion, const float* weights_dev, float w_mlp, float w_oe, float w_scale, float w_dd,
                    void* partials, void* result);

/* Every gradient that is not NULL is written in full: d(*g_loss * total) / d its tensor, with *g_loss one float on the DEVICE
 * and `result` the block gft_reg_forward wrote for the same inputs.
 *   g_d_xyz   [Nd, 3]            sgn(x) w_mlp / (3 Nd); 0 at x == 0 (torch's abs)
 *   g_opacity [P]                0 in rows outside the mask; dE/do w_oe / n_dynamic inside, times o (1 - o) when raw
 *   g_scaling [P, scaling_cols]  0 in invisible rows; 2 m w_scale / (3 n_visible) per column with m the row mean, times
 *                                exp(raw) when raw; with one column the three columns' contributions summed
 *   g_dd      [pixels]           w_dd / pixels
 * A gradient whose tensor is NULL must be NULL. */
int gft_reg_backward(void* hip_stream, int64_t n_dxyz, int64_t P, int64_t pixels, const float* d_xyz,
                     const float* opacity, const void* motion_mask, int32_t opacity_is_raw,
                     const float* scaling, int32_t scaling_cols, int32_t scaling_is_raw, const void* visible, int32_t visible_is_radii,
                     const float* weights_dev, float w_mlp, float w_oe, float w_scale, float w_dd,
                     const void* result, const float* g_loss, float* g_d_xyz, float* g_opacity, float* g_scaling, float* g_dd);

#ifdef __cplusplus
}
#endif
#endif
