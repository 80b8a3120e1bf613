/*
 * gftorf_ply.h -- C ABI of the Gaussian model's PLY rows, scene/gaussian_model.py:315-367 and 378-454 (libgftorf_rast.so,
 * gfx950).
 *
 * The body of the model's PLY file is its float32 values, one row per Gaussian, the columns of construct_list_of_attributes
 * in a fixed order.  The reference forms the rows on the host, one Python tuple per Gaussian, and reads them back column by
 * column.  Here:
 *   gft_ply_pack    every row of the "full" sheet [P, K_full] and, from the same read of the model, of the "sibr" sheet
 *                   [P, K_sibr] (the first K_sibr columns of the full row): one launch
 *   gft_ply_unpack  the reverse for a chunk of file rows already on the device: every destination tensor's rows from the
 *                   file columns a table names: one launch per chunk
 *
 * Nothing is computed: the float32 bit patterns are moved as they are (NaN payloads, denormals and -0.0 included).
 * A workgroup takes GFT_PLY_ROWS consecutive rows through an LDS tile of GFT_PLY_ROWS x K floats; K is at most
 * GFT_PLY_MAX_COLUMNS so that the tile fits.
 *
 * Device pointers, fp32; arrays marked HOST are read before the call returns.  Returns 0 on success (gft_last_error()).
 */
#ifndef GFTORF_PLY_H
#define GFTORF_PLY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFT_PLY_ROWS 64          /* rows per workgroup */
#define GFT_PLY_MAX_SOURCES 16   /* column blocks of a row (pack) or destination tensors (unpack) */
#define GFT_PLY_MAX_COLUMNS 240  /* floats of a sheet row or of a file row */

/* The full row is the concatenation of `count` column blocks, block k being widths[k] floats wide (HOST arrays of `count`
 * entries; the widths add up to K_full).  channels[k] says what fills block k:
 *   0      zeros (the normals); sources[k] is not looked at
 *   c >= 1 sources[k] is a contiguous [P, widths[k] / c, c] tensor and column ch * (widths[k] / c) + j of the block holds
 *          element [p, j, ch], which is transpose(1, 2).flatten(start_dim=1); c == 1 is a plain row copy.  widths[k] must
 *          be a multiple of c.
 * A block of width 0 is skipped and its pointer is not looked at.  Sources need 4-byte alignment only.
 * out_full [P, K_full] and out_sibr [P, K_sibr], 16-byte aligned; either may be NULL, not both.  K_sibr (1 .. K_full) is
 * read only with out_sibr.  P == 0 launches nothing. */
int gft_ply_pack(void* hip_stream, int64_t P, int32_t count, const float* const* sources, const int32_t* widths,
                 const int32_t* channels, int32_t K_full, int32_t K_sibr, float* out_full, float* out_sibr);

/* chunk [rows, K_file], 16-byte aligned: file rows row0 .. row0 + rows - 1.  dests (HOST, `count` device pointers): tensor k
 * is contiguous with widths[k] floats per row and its rows row0 .. row0 + rows - 1 are written (dests[k] is row 0 of the
 * tensor).  table (HOST, int32, sum of the widths entries): for every float of a destination row, tensor after tensor, the
 * file column it comes from, each in [0, K_file).  File columns the table does not name are ignored.  A tensor of width 0
 * is skipped and its pointer is not looked at.  rows == 0 launches nothing. */
int gft_ply_unpack(void* hip_stream, int64_t rows, int64_t row0, int32_t K_file, const float* chunk, int32_t count,
                   float* const* dests, const int32_t* widths, const int32_t* table);

#ifdef __cplusplus
}
#endif
#endif
