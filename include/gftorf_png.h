/*
 * gftorf_png.h -- C ABI of the PNG encoder (libgftorf_rast.so, gfx950).
 *
 * The reference writes every image of a rendered view and of a debug iteration with imageio.imwrite(....png) on the host
 * (train.py:298-398, render.py:105-189, render_ftorf_viz_traj.py:237-259).  The images are bytes on the device already
 * (gftorf_present.h, gftorf_debugviz.h, gftorf_flowviz.h), so the files are formed there: gft_png_encode writes, for every
 * image of a batch, the complete bytes of a .png file into the image's slot of one device buffer and the file's byte count
 * into a device tensor.  Lossless, 8 bits per sample, 1, 3 or 4 channels (PNG colour types 0, 2 and 6), no interlace.  The
 * file bytes are this encoder's own (PNG files of the same pixels differ between encoders); what is promised is that any PNG
 * reader decodes a file to exactly the source bytes, that the bytes are the same from run to run, and the sizes stated below.
 *
 * THE FILE
 *   signature (8 bytes), IHDR (25), one IDAT chunk per segment, one closing IDAT chunk (21), IEND (12).
 *   The filtered stream of an image is its H scanlines of L = 1 + W * channels bytes each (filter type, then the filtered
 *   bytes).  It is cut into segments of GFT_PNG_SEGMENT bytes wherever rows fall; the last segment holds the rest.  Segment s
 *   becomes one IDAT chunk (length, "IDAT", data, CRC-32 of "IDAT" and the data) whose data is
 *     - in the first chunk only, the zlib header 78 01;
 *     - then one of two forms of the segment, each a whole number of bytes, so chunks join on byte boundaries:
 *       stored  00, n as two little-endian bytes, ~n likewise, the n bytes (a non-final stored deflate block): 5 + n bytes
 *       fixed   a non-final fixed-Huffman block (bits 0, then 1 0 for BTYPE 01), the segment's tokens, the end-of-block
 *               code (7 zero bits), an empty non-final stored block (3 zero bits, zero bits up to the next byte boundary,
 *               00 00 FF FF): (3 + token bits + 10 + 7) / 8 + 4 bytes.
 *       At level 1 the fixed form is taken when it is no longer than the stored form, else the stored form; at level 0 always
 *       the stored form.
 *   The closing IDAT chunk holds the final empty stored block 01 00 00 FF FF and the Adler-32 of the whole filtered stream,
 *   big endian.  So a file has (segments + 1) IDAT chunks and
 *       gft_png_bound(H, W, channels) = 8 + 25 + 2 + segments * (12 + 5) + H * L + 21 + 12
 *   is the size of every level-0 file exactly and an upper bound of every level-1 file.
 *
 * THE FILTER (level 1; level 0 gives every scanline type 0)
 *   Per scanline, among types 0 (None), 1 (Sub) and 2 (Up), the one with the least sum over the W * channels filtered bytes v
 *   of (v < 128 ? v : 256 - v); ties go to the lowest type.  The row above the first row is zeros.
 *
 * THE TOKENS (level 1)
 *   Matches never reach in front of the segment's first byte, so segments are independent.  With j counted from the
 *   segment's first byte, the candidate distances are, in this order, 1, 2, 3, 4 and L.  The length of candidate d at j is 0
 *   when j < d, else the count of consecutive k = j, j + 1, ... inside the segment with byte[k] == byte[k - d], cut at 258.
 *   The best candidate at j has the greatest length; ties go to the earlier candidate in the order above.
 *   A sixth candidate reaches any distance: with g(j) the four bytes at j read as a little-endian uint32 (j + 4 <= the
 *   segment's bytes) and bucket(j) = (g(j) * 2654435761 mod 2^32) >> (32 - GFT_PNG_HASH_BITS), p(j) is the least j' with
 *   bucket(j') == bucket(j).  Where p(j) < j, the candidate's distance is j - p(j) and its length the count of k = 0, 1, ...
 *   with j + k inside the segment and byte[j + k] == byte[p(j) + k], cut at 7; it replaces the best of the five only when
 *   its length is 4 or more and greater than theirs.  (The least position of a bucket does not depend on the order in which
 *   the positions are entered, so the finder is deterministic.)  One greedy parse
 *   from j = 0: where the best length is 3 or more, a match token (length, distance) and j += length; else a literal token
 *   and j += 1.  Tokens are coded with deflate's fixed Huffman codes (RFC 1951 3.2.6).
 *
 * LAUNCHES
 *   gft_png_encode enqueues three launches at level 1 (filter choice per scanline; one workgroup per segment that writes the
 *   segment's chunk and its Adler-32 part to the scratch; assembly of the files from the chunks) and two at level 0 (no
 *   filter choice), whatever `count` is.  No host read, no atomic on global memory, no memset; it can be captured in a graph.
 *
 * Returns 0 on success (gft_last_error()).
 */
#ifndef GFTORF_PNG_H
#define GFTORF_PNG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFT_PNG_SEGMENT 32768      /* bytes of the filtered stream per segment = per workgroup = per IDAT chunk */
#define GFT_PNG_MAX_IMAGES 64      /* images of one call */
#define GFT_PNG_HASH_BITS 12       /* 4096 buckets of the sixth match candidate */
#define GFT_PNG_CHUNK_SLOT 32800   /* scratch bytes per segment: the longest chunk (12 + 2 + 5 + GFT_PNG_SEGMENT), 16-byte granular */
#define GFT_PNG_MAX_STREAM 0x7fff0000ll /* H * L of one image, at most */

/* One image of a batch.  src: device, uint8, row y at src + y * row_stride, its W * channels bytes contiguous.  out_offset: the
 * byte offset of the image's slot in `out`; the slot is gft_png_bound(H, W, channels) bytes and slots must not overlap. */
typedef struct gft_png_image {
    const void* src;
    int64_t row_stride;
    int64_t out_offset;
    int32_t H, W, channels, reserved;
} gft_png_image;

/* host only: the slot size of an image and the upper bound of its file's bytes; -1 for a shape the encoder does not take
 * (H, W < 1, channels not 1, 3 or 4, H * L > GFT_PNG_MAX_STREAM) */
int64_t gft_png_bound(int32_t H, int32_t W, int32_t channels);

/* host only: bytes of scratch gft_png_encode needs for these images (only H, W and channels are read); -1 for a bad batch */
int64_t gft_png_scratch_bytes(int32_t count, const gft_png_image* images);

/* images: HOST table of `count` (1 .. GFT_PNG_MAX_IMAGES) entries, read before the call returns.  level: 0 or 1.
 * out: device bytes; file i is out[out_offset_i .. out_offset_i + sizes[i]).  out_bytes: the size of `out`, every slot must lie
 * inside.  sizes: device int64[count].  scratch: device, 16-byte aligned, scratch_bytes >= gft_png_scratch_bytes(count, images);
 * its content before the call does not matter and it must stay untouched until the launches have run. */
int gft_png_encode(void* hip_stream, int32_t count, const gft_png_image* images, int32_t level, void* out, int64_t out_bytes,
                   int64_t* sizes, void* scratch, int64_t scratch_bytes);

#ifdef __cplusplus
}
#endif
#endif
