/*
 * gftorf_rigid.h -- C ABI of the local-rigidity priors of the dynamic Gaussians (libgftorf_rast.so, gfx950).
 *
 * The reference's utils/loss_utils.py ends with three functions its train.py never calls: find_knn (:35-44), rigidity_loss
 * (:46-60) and isometry_loss (:62-72).  With j = idx[i, k], w = w_i_j[i, k] and d0 = initial_xyz_to_knn_dist[i, k]:
 *   rigidity  mean over (i, k) of  w * sqrt(|(prev_i - prev_j) - (curr_i - curr_j)|^2 + 1e-16)
 *   isometry  mean over (i, k) of  |w * (sqrt(d0 + 1e-16) - sqrt(|curr_i - curr_j|^2 + 1e-16))|
 * find_knn builds the P x P matrix of torch.cdist and is neither exact nor free of the point itself; gft_rigid_knn is the
 * exact search of gftorf_knn.h with the neighbours kept.  The two means are one forward of two launches (the sums, then one
 * workgroup that finishes them) and one backward launch that walks, for every point, its own K edges and then the edges
 * that name it -- the transpose of the table -- in a stored order: no atomic, no memset, no host read, the same bits from run
 * to run, and every entry point can be captured in a graph.
 *
 * Device pointers; fp32 tensors contiguous: prev, curr [P, 3]; w, d0, dist2 [P, K]; idx int32 [P, K].
 * PRECONDITION of gft_rigid_forward and gft_rigid_backward: every idx[i, k] lies in [0, P), `offsets` [P + 1] is
 * non-decreasing from 0 to P * K and `edges` [P * K] holds edge numbers in [0, P * K).  The kernels do not check them.
 * Returns 0 on success (gft_last_error()).
 */
#ifndef GFTORF_RIGID_H
#define GFTORF_RIGID_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFT_RIGID_MAX_K 32          /* neighbours per point of gft_rigid_knn */

/* 4-byte words of one row of `partials`: two fp32 sums (rigidity, isometry) */
#define GFT_RIGID_PARTIAL_WORDS 2

/* the result block, 4-byte words: */
#define GFT_RIGID_MEANS 0           /* float[2]: the unweighted means -- rigidity, isometry (0 for an absent term) */
#define GFT_RIGID_TOTAL 2           /* float: w_rigid * rigidity + w_iso * isometry */

size_t gft_rigid_knn_scratch_bytes(int32_t P);

/* The K nearest OTHER points of every point: idx int32 [P, K] and dist2 fp32 [P, K], both written in full, row i ordered by
 * (dist2 ascending, index ascending).  Exact; the point itself is excluded by its index, so a duplicate of it is a neighbour
 * at distance 0.  dist2 is fma(dz, dz, fma(dy, dy, dx * dx)) of the fp32 differences, the expression of
 * gft_knn_mean_dist2: for K >= 3, (dist2[i][0] + dist2[i][1] + dist2[i][2]) / 3.0f is that function's value to the bit.
 * 1 <= K <= GFT_RIGID_MAX_K, P > K, P * K < 2^31.  points [P, 3] fp32, scratch of gft_rigid_knn_scratch_bytes(P). */
int gft_rigid_knn(void* hip_stream, int32_t P, int32_t K, const float* points, int32_t* idx, float* dist2, void* scratch);

/* Workgroups of a gft_rigid_forward launch = rows of `partials`, for P * K edges.  0 when P or K is below 1. */
int64_t gft_rigid_blocks(int64_t P, int32_t K);

/* 4-byte words of the result block */
int64_t gft_rigid_result_words(void);

/* partials [gft_rigid_blocks(P, K)][GFT_RIGID_PARTIAL_WORDS] and result [gft_rigid_result_words()] are written in full.
 * The rigidity term is present when prev is not NULL, the isometry term when d0 is not NULL; at least one is.  The two
 * weights are read from weights_dev (DEVICE, two floats: rigid, iso) when it is not NULL, else taken by value. */
int gft_rigid_forward(void* hip_stream, int64_t P, int32_t K, const int32_t* idx, const float* w, const float* prev,
                      const float* curr, const float* d0, const float* weights_dev, float w_rigid, float w_iso,
                      void* partials, void* result);

/* g_curr [P, 3] and g_prev [P, 3], each when it is not NULL, are written in full: d(*g_loss * total) / d curr and d prev, with
 * *g_loss one float on the DEVICE.  `offsets` and `edges` are the transpose of idx: edges[offsets[i] .. offsets[i + 1]) are
 * the edge numbers e = m * K + k with idx[m][k] == i, ascending.  Point i adds its own K edges in the order of k, then those
 * in the stored order.  g_prev without prev must be NULL (the isometry term does not read prev). */
int gft_rigid_backward(void* hip_stream, int64_t P, int32_t K, const int32_t* idx, const int32_t* offsets, const int32_t* edges,
                       const float* w, const float* prev, const float* curr, const float* d0, const float* weights_dev,
                       float w_rigid, float w_iso, const float* g_loss, float* g_curr, float* g_prev);

#ifdef __cplusplus
}
#endif
#endif
