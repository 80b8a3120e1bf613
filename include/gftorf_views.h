/*
 * gftorf_views.h -- C ABI of the training views kept on the device: the first statement of an iteration, "make view v
 * current" (train.py:155-163, 184-187, 219-220), as one launch that a graph can hold (libgftorf_rast.so, gfx950).
 *
 *   gft_views_layout                  where a view's record and image groups lie in its slab of the arena and in the
 *                                     "current" buffer: a host function, no device needed
 *   gft_views_draw                    copies view v's slab into the current buffer, v by value or read from a device
 *                                     schedule that the launch itself advances: one launch
 *   gft_views_select_plane            out [1, H, W] = x[p] with p read on the device: one launch
 *   gft_views_select_plane_backward   the whole [C, H, W] gradient of it, zeros included: one launch
 *
 * A view is a record of F float32 and J int32 columns and up to GFT_VIEWS_MAX_GROUPS image groups, each either float32
 * planar [C, H, W] (GFT_VIEWS_F32) or uint8 interleaved [H, W, C], C <= 4 (GFT_VIEWS_U8).  The arena holds V slabs back to
 * back; the current buffer holds one view, every group as float32 planar [C, H, W], behind a header of
 * GFT_VIEWS_HEADER_BYTES.  Device pointers; arrays marked HOST are read before the call returns.  Except
 * gft_views_layout the functions return 0 on success (gft_last_error()).
 */
#ifndef GFTORF_VIEWS_H
#define GFTORF_VIEWS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFT_VIEWS_MAX_GROUPS 8      /* image groups of a view */
#define GFT_VIEWS_ALIGN 16          /* every group and the record start on a multiple of it, in the slab and in the current buffer */
#define GFT_VIEWS_HEADER_BYTES 16   /* the current buffer's first bytes: int32 words written by every draw */
#define GFT_VIEWS_INDEX_WORD 0      /* ... the drawn view */
#define GFT_VIEWS_CURSOR_WORD 1     /* ... the cursor value the draw used; -1 when the index came by value */
#define GFT_VIEWS_CHUNKS 1024       /* 16-byte chunks (and pixels of a uint8 group) one workgroup moves */

/* kinds of a group */
#define GFT_VIEWS_F32 0             /* float32 planar [C, H, W] in the slab */
#define GFT_VIEWS_U8 1              /* uint8 interleaved [H, W, C] in the slab, C <= 4; float(x) / 255.0f planar in the current buffer */

/* kinds, C, H, W [count] HOST.  Returns the bytes of one view's slab (a multiple of GFT_VIEWS_ALIGN), or 0 for a request that
 * cannot be laid out: no group and no record, count outside 0..GFT_VIEWS_MAX_GROUPS, F or J negative, a dimension below 1,
 * an unknown kind, a GFT_VIEWS_U8 group with C > 4, or a slab beyond 2^40 bytes.  *current_bytes: the bytes of the current
 * buffer.  slab_offsets / current_offsets [count + 1]: the byte offset of every group, then of the record (F floats directly
 * followed by J int32), in a slab and in the current buffer.  The output pointers may be NULL. */
int64_t gft_views_layout(int32_t F, int32_t J, int32_t count, const int32_t* kinds, const int32_t* C, const int32_t* H,
                         const int32_t* W, int64_t* current_bytes, int64_t* slab_offsets, int64_t* current_offsets);

/* arena: V slabs of the layout of (F, J, count, kinds, C, H, W), 16-byte aligned; current: the current buffer, 16-byte
 * aligned.  The view is `index` when order is NULL, else order[cursor[0] % N] (order int32 [N], cursor int32 [1], the
 * remainder taken of the cursor as an unsigned number); either way it is clamped to [0, V) before use.  With a schedule
 * the launch leaves cursor[0] + 1 in cursor[0]: every workgroup reads the old value, the last one to finish -- known by
 * `ticket`, an int32 word that is zero between launches and belongs to this schedule -- writes the new one and clears the
 * ticket.  Launches that share a cursor must follow one another on one stream.  No host read, no memset, no atomic but the
 * ticket's. */
int gft_views_draw(void* hip_stream, int32_t F, int32_t J, int32_t count, const int32_t* kinds, const int32_t* C, const int32_t* H,
                   const int32_t* W, const void* arena, void* current, int64_t V, int64_t index, const int32_t* order,
                   int32_t* cursor, int64_t N, int32_t* ticket);

/* x [C, H, W] float32 contiguous (4-byte aligned: a slice along the first dimension serves), out [H, W], plane = H * W.  i = *index_dev
 * when index_dev is not NULL, else `index`; with modulo > 0, i becomes its remainder in [0, modulo); with table (int32 [T])
 * p = table[clamp(i, 0, T - 1)], else p = i; p is clamped to [0, C).  out = x[p]. */
int gft_views_select_plane(void* hip_stream, int32_t C, int64_t plane, const float* x, int64_t index, const int32_t* index_dev,
                           int32_t modulo, const int32_t* table, int32_t T, float* out);

/* g_out [H, W], g_x [C, H, W]: plane p of g_x is g_out, every other plane zeros; every element of g_x is written. */
int gft_views_select_plane_backward(void* hip_stream, int32_t C, int64_t plane, const float* g_out, int64_t index,
                                    const int32_t* index_dev, int32_t modulo, const int32_t* table, int32_t T, float* g_x);

#ifdef __cplusplus
}
#endif
#endif
