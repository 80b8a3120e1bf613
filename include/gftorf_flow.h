/*
 * gftorf_flow.h -- C ABI of the F-ToRF scene-flow term of the training loss (libgftorf_rast.so, gfx950).
 *
 * On every fourth frame after flow_loss_iter_start the reference (train.py:243-261) unprojects the rendered distance
 * (scene/torf_utils.py distance_to_points3d), projects the points into the ToF camera (project_points), adds each rendered
 * 3-D flow, projects again (project_flow) and compares the 2-D flow with the ground truth:
 *   forward_flow_l2 = mean((project(p + flow3d_fwd) - project(p) - gt_fwd)^2)   over [2, H, W], likewise backward.
 * In eager PyTorch that is ~100 small launches forward and backward and a torch.inverse that synchronises with the host.
 * Here: one launch forward for both directions, one backward, and every camera matrix is read on the device.
 *
 * Per pixel (u = column, v = row), with fx = K[0][0], fy = K[1][1], cx = K[0][2], cy = K[1][2] of the colour camera:
 *   z = d / sqrt(((u - cx) / fx)^2 + ((v - cy) / fy)^2 + 1),  x = (u - cx) * z / fx,  y = (v - cy) * z / fy
 *   p = rows 0..2 of inverse(world_view_transform) @ [x, y, z, 1]          (the matrix as stored: the transposed
 *                                                                           world-to-view matrix, as the reference does)
 *   project(p) = q[0..1] / (q[2] + 1e-7),  q = K_tof @ rows 0..2 of world_view_transform_tof^T @ [p, 1]
 * The 4x4 inverse is formed inside each launch in double precision and rounded to float; a singular matrix gives
 * non-finite values (nothing is checked on the host).
 *
 * Device pointers, fp32, contiguous: images planar [C, H, W], depth [1, H, W], K and K_tof [3, 3] row-major,
 * world_view_transform(_tof) [4, 4] row-major.  Returns 0 on success (gft_last_error()).  Nothing reads a value back to the
 * host and nothing uses a memset: every entry point can be captured in a graph.
 */
#ifndef GFTORF_FLOW_H
#define GFTORF_FLOW_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* workgroups of a gft_flow_loss_forward launch = rows of `partials` */
int64_t gft_flow_loss_blocks(int32_t H, int32_t W);

/* partials[b][k] = scale * (sum of the squared 2-D flow error of direction k over workgroup b's pixels), k = 0 forward,
 * 1 backward.  With scale = 1 / (2*H*W) the column sums are forward_flow_l2 and backward_flow_l2.  A direction whose flow3d
 * is NULL contributes 0 (its gt is then not read); a direction with a flow3d needs its gt [2, H, W]. */
int gft_flow_loss_forward(void* hip_stream, int32_t H, int32_t W, const float* depth, const float* K, const float* w2v,
                          const float* K_tof, const float* w2v_tof, const float* flow3d_fwd, const float* gt_fwd,
                          const float* flow3d_bwd, const float* gt_bwd, float scale, float* partials);

/* grad_fwd / grad_bwd [3, H, W] = d(*g_fwd * scale * sum of the forward error, likewise backward) / d flow3d.  g_fwd and g_bwd
 * are read on the DEVICE (one float each; NULL = 0).  A direction is skipped (its gradient not written) when its flow3d or
 * its grad is NULL.  The geometry is recomputed, not saved; depth and the ground truth get no gradient. */
int gft_flow_loss_backward(void* hip_stream, int32_t H, int32_t W, const float* depth, const float* K, const float* w2v,
                           const float* K_tof, const float* w2v_tof, const float* flow3d_fwd, const float* gt_fwd,
                           const float* flow3d_bwd, const float* gt_bwd, const float* g_fwd, const float* g_bwd, float scale,
                           float* grad_fwd, float* grad_bwd);

/* points3d [3, H, W] = distance_to_points3d(depth) and/or points2d [2, H, W] = project_points(points3d): either output may be
 * NULL, not both; K_tof and w2v_tof are read only for points2d. */
int gft_flow_points(void* hip_stream, int32_t H, int32_t W, const float* depth, const float* K, const float* w2v,
                    const float* K_tof, const float* w2v_tof, float* points3d, float* points2d);

/* out [2, H, W] = project(points3d + flow3d) - points2d_curr: project_flow, or project_points with flow3d = points2d_curr =
 * NULL (read as 0). */
int gft_flow_project(void* hip_stream, int32_t H, int32_t W, const float* K_tof, const float* w2v_tof, const float* points3d,
                     const float* flow3d, const float* points2d_curr, float* out);

/* grad_flow3d [3, H, W] = the transposed Jacobian of project() at points3d + flow3d applied to grad_out [2, H, W] (flow3d
 * NULL = 0). */
int gft_flow_project_backward(void* hip_stream, int32_t H, int32_t W, const float* K_tof, const float* w2v_tof,
                              const float* points3d, const float* flow3d, const float* grad_out, float* grad_flow3d);

#ifdef __cplusplus
}
#endif

#endif
