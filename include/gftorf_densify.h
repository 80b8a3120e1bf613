/*
 * gftorf_densify.h -- C ABI of the per-Gaussian bookkeeping kernels of libgftorf_rast.so (gfx950).
 *
 * SURVEY section 8(f) row 4 (bookkeeping part; the optimizer part is gftorf_optim.h): the tensor
 * surgery around the rasterizer in the reference's training loop, which at 1 M Gaussians costs
 * more than a rasterizer step in eager PyTorch because every boolean-mask index is a
 * nonzero() with a host synchronisation plus a gather or a scatter:
 *
 *   every iteration (train.py:441-449, scene/gaussian_model.py:648-654):
 *       max_radii2D[vis] = max(max_radii2D[vis], radii[vis])
 *       xyz_gradient_accum[vis] += ||viewspace_grad[vis, :2]|| * pixels[vis]
 *       denom[vis] += pixels[vis]
 *     -> gft_densify_stats: one pass, in place.
 *
 *   every densification / pruning step (scene/gaussian_model.py:473-514, 571-631): `t[mask]` of
 *   the 11 parameter tensors, their two Adam moments and 3 statistics tensors
 *     -> gft_rows_rank once per mask (row -> output row, number of kept rows), then
 *        gft_rows_gather per tensor: order-preserving compaction, pure byte movement
 *        (bit-identical to `t[mask]`).
 *
 * Device pointers; every function returns 0 on success (gft_last_error()).
 */
#ifndef GFTORF_DENSIFY_H
#define GFTORF_DENSIFY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* In-place statistics update for the rows where update_filter (and apply_mask, when given: the
 * reference's `apply_mask` branch, valid there only when update_filter is a subset of it) is set.
 * viewspace_grad [P,3] (xy = pixel-space gradient of means2D), pixels [P] or [P,1], radii int32 [P];
 * update_filter / apply_mask: one byte per Gaussian (torch.bool), apply_mask may be NULL;
 * xyz_gradient_accum [P,1], denom [P,1], max_radii2D [P] (any of the three may be NULL = skip). */
int gft_densify_stats(void* hip_stream, int64_t P, const float* viewspace_grad, const float* pixels, const int32_t* radii,
                      const uint8_t* update_filter, const uint8_t* apply_mask, float* xyz_gradient_accum, float* denom,
                      float* max_radii2D);

/* rank[i] = number of set mask bytes before row i (int32 [P]); *count (host) = number of set bytes.
 * Blocks until the count has reached the host (the reference's `t[mask]` blocks the same way).
 * scratch: gft_rows_rank_scratch_bytes(P) bytes. */
size_t gft_rows_rank_scratch_bytes(int64_t P);
int gft_rows_rank(void* hip_stream, int64_t P, const uint8_t* mask, int32_t* rank, void* scratch, int64_t* count);
/* The same ranking with the count left on the device (*count_dev, a uint32) and nothing read back: the call does not
 * block and can be captured in a HIP graph.  P > 0. */
int gft_rows_rank_dev(void* hip_stream, int64_t P, const uint8_t* mask, int32_t* rank, void* scratch, uint32_t* count_dev);

/* mask[i] = 1 if row i of a ([P, row_floats_a]) or of b ([P, row_floats_b]) holds a value != 0 (a NaN counts, -0 does
 * not), else 0; either tensor may be NULL.  The rows of a backward that have an upstream gradient -- what
 * `~((a.abs().amax(1).maximum(b.abs().amax(1))) == 0)` is in eight eager launches and two full-size temporaries. */
int gft_rows_any_nonzero(void* hip_stream, int64_t P, int32_t row_floats_a, const float* a, int32_t row_floats_b,
                         const float* b, uint8_t* mask);

/* dst[rank[i]] = src[i] for every row i with mask[i] != 0; rows are row_bytes long (a multiple of 4),
 * src and dst 4-byte aligned (16-byte accesses are used when rows and both pointers allow). */
int gft_rows_gather(void* hip_stream, int64_t P, const uint8_t* mask, const int32_t* rank, const void* src, void* dst,
                    int64_t row_bytes);

/* ---- one densify_and_prune event as one plan and one pass over every tensor (scene/gaussian_model.py:571-640) ----
 * The event is a function of per-row quantities.  Its result lives in a virtual row space of V = P + C + N * S rows:
 * the P originals, the C clones in the order of their sources, the N * S children (child k * S + j belongs to the j-th
 * split row: `repeat(N, ...)` tiles the whole block).  Both plan calls rank two flags of a row in the three launches of
 * one ranking and block until their two counts have reached the host: two host reads per event.
 * scratch of either call: gft_densify_plan_scratch_bytes(rows) bytes, rows = P (classify) or V (layout). */
size_t gft_densify_plan_scratch_bytes(int64_t rows);

/* row_class[i] (one byte) = 1 cloned: grad_norm[i] >= max_grad and max_scaling[i] <= dense_threshold,
 *                           2 split:  grad[i] >= max_grad and max_scaling[i] > dense_threshold, 0 otherwise;
 * clone_rows [C] / split_rows [S] (int32, room for P entries each): the cloned / split rows in increasing order;
 * counts (host, 2 values) = C, S.  grad_norm / grad / max_scaling: float [P] (`torch.norm(grads, dim=-1)`, `grads`,
 * `get_scaling.max(1)`); the thresholds as float, the way torch compares a Python number with a float32 tensor. */
int gft_densify_classify(void* hip_stream, int64_t P, const float* grad_norm, const float* grad, const float* max_scaling,
                         float max_grad, float dense_threshold, uint8_t* row_class, int32_t* clone_rows, int32_t* split_rows,
                         void* scratch, int64_t* counts);

/* The final prune over the V virtual rows and where every survivor lands (survivors keep their virtual order).  A row
 * dies if it is a split original, if opacity < min_opacity (a clone's and a child's: their source's), or, with use_size,
 * if screen_dead or its largest scaling is > big_threshold or < small_threshold (a clone's: its source's max_scaling, a
 * child's: child_max_scaling [N * S] of its own new scaling).  Per survivor r (room for V entries each):
 *   source_row[r] int32  the original row it is, or was copied or split from
 *   kind[r]       uint8  0 kept original, 1 clone, 2 child
 *   child[r]      int32  the child's index k * S + j, -1 for the other kinds
 *   map_new[r]    int32  source_row[r], a child's P + child[r]      (gft_rows_remap of xyz / scaling with the children as extra)
 *   map_state[r]  int32  source_row[r] of a kept original, else -1  (gft_rows_remap of the Adam moments)
 * and with seg ([P, seg_cols] floats, may be NULL): motion_mask[r] (one byte) = seg[source_row[r], 0] > 0.5 and
 * motion_rank[r] (int32) = the number of set motion_mask bytes before r.  counts (host, 2 values) = number of survivors,
 * number of set motion_mask bytes.  P + C + N * S <= 2^31 - 1; any of P, C, S and the survivors may be 0. */
int gft_densify_layout(void* hip_stream, int64_t P, int64_t C, int64_t S, int32_t N, const uint8_t* row_class,
                       const int32_t* clone_rows, const int32_t* split_rows, const float* opacity, const float* max_scaling,
                       const float* child_max_scaling, float min_opacity, int32_t use_size, int32_t screen_dead,
                       float big_threshold, float small_threshold, const float* seg, int32_t seg_cols, int32_t* source_row,
                       uint8_t* kind, int32_t* child, int32_t* map_new, int32_t* map_state, uint8_t* motion_mask,
                       int32_t* motion_rank, void* scratch, int64_t* counts);

/* dst[r] = row map[r] of src when 0 <= map[r] < src_rows, row map[r] - src_rows of extra when map[r] >= src_rows (a zero
 * row when extra is NULL), a zero row when map[r] < 0; r < n_out, map int32.  One launch, every dst row written once;
 * rows are row_bytes long (a multiple of 4), the pointers 4-byte aligned (16-byte accesses are used when the rows and
 * all pointers allow). */
int gft_rows_remap(void* hip_stream, int64_t n_out, const int32_t* map, const void* src, int64_t src_rows, const void* extra,
                   void* dst, int64_t row_bytes);

/* The positions of the N * S children of the S split rows (scene/gaussian_model.py:577-581, build_rotation of
 * utils/general_utils.py:91-112) in one launch: child k * S + j (the virtual rows' order above) of split row split_rows[j] gets
 *   new_xyz [N * S, 3] = R(rotation[row]) . (z[child] * scaling[row]) + xyz[row]
 * xyz [P,3], rotation [P,4] raw (r, x, y, z; 16-byte aligned: one load per row), scaling [P,3] ACTIVATED (get_scaling),
 * z [N * S, 3] standard normals (torch.randn), read straight from the model's tensors: no gathered copies.  One thread per
 * split row, vector stores, no atomics, no memset, no host read.  S = 0 returns 0 without a launch; N < 1, S > P,
 * N * S > 2^31 - 1 and a NULL pointer with S > 0 are refused before anything touches a device.  A split row outside [0, P)
 * is not read: its children are NaN.
 * (The children's scaling, log(scaling / (0.8 N)), and its largest exp stay torch statements: this library's logf is the
 * compiler's of the day, torch.log the one torch was built with, and the two need not agree in the last bit.)
 *
 * The arithmetic, every operation rounded to float32 on its own (no contraction) unless stated:
 *   norm = sqrtf(r0 r0 + r1 r1 + r2 r2 + r3 r3) added left to right, q = r / norm (IEEE division), the nine entries of R as
 *   build_rotation writes them (1 - 2 (y y + z z), 2 (x y - r z), ...): what eager torch computes on the device; a zero
 *   quaternion gives NaN, as there.
 *   s_c = z_c * scaling_c + 0.0f: torch.normal(mean = zeros, std) after its normal_(0, 1); the add turns -0 into +0.
 *   new_xyz_i = fmaf(R_i2, s_2, fmaf(R_i1, s_1, R_i0 * s_0)) + xyz_i: an ascending chain of fused multiply-adds, then a
 *   separately rounded add.  The reference forms these three products inside torch.bmm, whose order and fusing belong to
 *   the BLAS solution picked for the batch count; this route states its own order.  Of the six chains and the three
 *   pairings of rounded products the ascending chain met torch.bmm's bits most often where it was measured (every
 *   element at batch counts 1 .. 900000 on an MI355X, profiles/bmm_order_probe.json); nothing relies on that.  Against
 *   float64 from the same float32 inputs:
 *   |new_xyz_i - exact| <= 16 eps (|s_0| + |s_1| + |s_2|) + 2 eps |exact|, eps = 2^-23. */
int gft_split_children(void* hip_stream, int64_t P, int64_t S, int32_t N, const int32_t* split_rows, const float* xyz,
                       const float* rotation, const float* scaling, const float* z, float* new_xyz);

#ifdef __cplusplus
}
#endif
#endif
