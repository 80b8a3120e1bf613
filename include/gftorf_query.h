/*
 * gftorf_query.h -- C ABI of an iteration's deformation queries as one batch (libgftorf_rast.so, gfx950).
 *
 * A dynamic iteration starts with `GaussianModel.query_dmlp` (scene/gaussian_model.py:170-174): the normalised positions
 * of the dynamic Gaussians, `get_xyz_normalized[get_motion_mask]`, and the frame's time go through the deformation network.
 * An F-ToRF iteration does that 2-3 times on the same points (train.py:169-176, 248, 255) and combines the results:
 *   d_xyz     = 0.25 * ((f - curr) * d_next + (next - f) * d_curr)        between two integer frames
 *   flow_next = d_xyz_next - d_xyz,  flow_prev = d_xyz_prev - d_xyz       on flow frames
 * Here the K times of an iteration are ONE batch of K * n rows for the network (gftorf_deform.h, per-row t):
 *   gft_query_inputs    x [K, n, 3] and t [K, n] from the model's raw positions, the dynamic rows and the K times
 *   gft_query_combine   M linear combinations of the K blocks of the network's d_xyz [K, n, 3], and its backward
 * Nothing allocates, blocks, reads a value back, issues a memset or uses an atomic: every entry point can be captured in a
 * graph, and the times, the coefficients, the positions and the rows are read when the kernels run.  Every output is written
 * in full.  Device pointers unless said otherwise; fp32 tensors contiguous, no pointer needs more than its element's alignment.
 * Returns 0 on success (gft_last_error()).
 */
#ifndef GFTORF_QUERY_H
#define GFTORF_QUERY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFT_QUERY_MAX_TIMES 4     /* K: the times of one batch */
#define GFT_QUERY_MAX_OUTPUTS 4   /* M: the combinations of one call */

/* x[k, j] = xyz[row_j] * scale and t[k, j] = times[k] for k < K, j < n, with row_j the j-th dynamic Gaussian.
 *   xyz [P, 3]      the model's raw positions; scale = 1.0f / scene_extent computed by the caller in fp32 (eager torch's
 *                   `_xyz / scene_extent` on the device multiplies by that reciprocal: the same bits)
 *   mask, rank      the dynamic rows as gft_rows_rank (gftorf_densify.h) leaves them: mask[P] bytes, non-zero = dynamic,
 *                   rank[P] = output row of a dynamic Gaussian; count_dev = the number of dynamic rows on the DEVICE.
 *                   All three NULL: every Gaussian is dynamic, row_j = j.
 *   times           K floats: read from times_dev (DEVICE) when the kernel runs if it is not NULL, else taken from
 *                   times_host (HOST, read during the call).
 * With fewer dynamic rows than n (the mask has changed since n was read) the surplus rows of x are the point 0; with more,
 * the rows whose rank is >= n are left out.  n == 0 launches nothing. */
int gft_query_inputs(void* hip_stream, int64_t P, const float* xyz, const uint8_t* mask, const int32_t* rank,
                     const uint32_t* count_dev, int64_t n, int32_t K, float scale, const float* times_dev,
                     const float* times_host, float* x, float* t);

/* out[m][j, c] = sum over k of C[m, k] * d[k][j, c], for m < M; d [K, n, 3], out: M HOST-side pointers to [n, 3] each.
 * C [M, K] row-major: read from coeffs_dev (DEVICE) when the kernel runs if it is not NULL, else taken from coeffs_host
 * (HOST, read during the call).  Every product is rounded to fp32 on its own (no fused multiply-add) and the terms are
 * added in increasing k.  A coefficient that is exactly 0 contributes nothing: its operand is not read, so a NaN there does
 * not spread; a row of C with the single coefficient 1 is a bit copy, a row of zeros gives +0. */
int gft_query_combine(void* hip_stream, int64_t n, int32_t K, int32_t M, const float* d, const float* coeffs_dev,
                      const float* coeffs_host, float* const* out);

/* g_d[k][j, c] = sum over m of C[m, k] * g_out[m][j, c], written in full over [K, n, 3]: a block that receives nothing is
 * zeros.  g_out: M HOST-side pointers, a NULL one counts as zeros.  Products rounded, terms added in increasing m, zero
 * coefficients skipped as above. */
int gft_query_combine_backward(void* hip_stream, int64_t n, int32_t K, int32_t M, const float* const* g_out,
                               const float* coeffs_dev, const float* coeffs_host, float* g_d);

#ifdef __cplusplus
}
#endif
#endif
