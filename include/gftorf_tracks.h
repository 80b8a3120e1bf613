/*
 * gftorf_tracks.h -- C ABI of the F-ToRF motion tracks, render_ftorf_viz_traj.py:262-347 (libgftorf_rast.so, gfx950).
 *
 * After its per-view loop the reference's track program integrates the Gaussians' flow over the sequence
 * (all_3D_pos[v] = all_3D_pos[v - 1] + gs_xyz_flow[v - 1]), projects every Gaussian into every view
 * (project_points_subset, scene/torf_utils.py:108-114) and then walks a Python double loop over frames and drawn
 * Gaussians that reads single elements from the device.  Here:
 *   gft_tracks_integrate  the whole sequence in one launch: one lane per Gaussian walks t = 0 .. T - 1 with its position in
 *                         registers; no atomic, no memset, no host read
 *   gft_tracks_table      the rows of a selection (mask and its exclusive rank, gft_rows_rank of gftorf_densify.h), in index
 *                         order, gathered into one contiguous buffer that one copy brings to the host: one launch
 *
 * The arithmetic is float32 without contraction, every division the correctly rounded one:
 *   pos[0] = initial_pos, pos[v] = pos[v - 1] + flow[flow_index[v - 1]]      (the reference's sequential additions)
 *   c_r = ((M[0][r] x + M[1][r] y) + M[2][r] z) + M[3][r]   r = 0..2, M = world_view[t] as the camera stores it (transposed)
 *   h_r = (K[r][0] c_0 + K[r][1] c_1) + K[r][2] c_2
 *   xy  = (h_0, h_1) / (h_2 + 1e-7f)
 *   motion = (sum_t ((f_x^2 + f_y^2) + f_z^2)) / T over all T frames' flows, mean_z = (sum_t pos[t].z) / T, both summed in
 *   increasing t from 0, so repeated calls give the same bits
 *   step_ok[0] = 0 < x < W and 0 < y < H;  step_ok[t >= 1] = 0 < x_t < W - 1 and 0 < y_t < H - 1 and 0 < x_(t-1) < W and
 *   0 < y_(t-1) < H; a NaN compares false
 *
 * Device pointers, fp32 unless stated.  Returns 0 on success (gft_last_error()).
 */
#ifndef GFTORF_TRACKS_H
#define GFTORF_TRACKS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* the parts of a track table, in the order they lie in it */
#define GFT_TRACKS_INDEX 0   /* int64 [S]: the Gaussian of each row */
#define GFT_TRACKS_XY 1      /* float [T, S, 2] */
#define GFT_TRACKS_MOTION 2  /* float [S] */
#define GFT_TRACKS_STEP_OK 3 /* uint8 [T, S] */
#define GFT_TRACKS_PARTS 4

/* initial_pos [P, 3]; flow [U, n, 3]; flow_index int32 [T] (DEVICE; values outside [0, U) are clamped into it); K [T, 3, 3];
 * world_view [T, 4, 4].  mask NULL: n == P and row i moves by flow row i.  Otherwise mask (one byte per Gaussian) and rank
 * (int32 [P], the number of set bytes before each row): a set row i moves by flow row rank[i] when that is below n, every
 * other row by exactly zero.  Outputs, every element written: xy [T, P, 2], pos_last [P, 3], motion [P], mean_z [P],
 * step_ok uint8 [T, P].  P, T >= 1; U >= 1 unless n == 0; 1 <= H, W < 2^24. */
int gft_tracks_integrate(void* hip_stream, int64_t P, int64_t n, int32_t T, int32_t U, const float* initial_pos, const float* flow,
                         const int32_t* flow_index, const float* K, const float* world_view, const uint8_t* mask,
                         const int32_t* rank, int32_t H, int32_t W, float* xy, float* pos_last, float* motion, float* mean_z,
                         uint8_t* step_ok);

/* Bytes of the table of S rows over T frames; offsets_out (HOST, GFT_TRACKS_PARTS entries, or NULL) receives each part's
 * byte offset.  0 for bad arguments (T < 1, S < 0); S == 0 gives 0 bytes and is valid. */
int64_t gft_tracks_table_bytes(int32_t T, int64_t S, int64_t* offsets_out);

/* table (8-byte aligned, gft_tracks_table_bytes(T, S) bytes): row rank[i] of every part = row i of xy [T, P, 2], step_ok
 * [T, P] and motion [P] for every i with mask[i] set and 0 <= rank[i] < S.  S == 0 launches nothing. */
int gft_tracks_table(void* hip_stream, int64_t P, int32_t T, int64_t S, const uint8_t* mask, const int32_t* rank, const float* xy,
                     const uint8_t* step_ok, const float* motion, void* table);

#ifdef __cplusplus
}
#endif
#endif
