/*
 * gftorf_detsum.h -- C ABI of the fixed-order sum behind the bit-reproducible backwards (libgftorf_rast.so, gfx950).
 *
 * In their fixed-order modes the rasterizer's backward (gft_backward with gft_backward_io.det_partials) and the feature
 * blend's (gftorf_features.h, gft_render_features_backward_det) STORE the row of sums of every (list entry, quadrant)
 * instead of adding it to the Gaussian's accumulator with float atomics: rows[(p * 4 + quadrant) * stride + k], p the
 * entry's position in the frame's id list.  The rows are then added in ONE order:
 *
 *   for a Gaussian g and a value k, visit the tiles whose list holds g in ascending tile index (tile = ty * tiles_x + tx);
 *   for each, form s = r0 + r1 + r2 + r3, the four quadrant rows added left to right;
 *   if s != 0, acc = acc + s, starting from 0.
 *
 * (A list holds a Gaussian at most once, and rows nothing was stored to read as zero.)  Two launches form that sum: the
 * comparator, one workgroup that walks the tiles one after the other (gft_backward; `index` = NULL below), and a grid-wide
 * one that gives every Gaussian a run of slots, one per tile of its tile rectangle in ascending tile order, records which
 * list position fills each slot and lets one lane per (Gaussian, value) add its rows in slot order (csrc/k_detsum.hip).
 * Both give the same bits; neither uses a float atomic, reads anything back to the host or issues a memset, so both can
 * be captured in a graph.  tests/detsum_ref.py restates the order in numpy.
 */
#ifndef GFTORF_DETSUM_H
#define GFTORF_DETSUM_H

#include <stddef.h>
#include <stdint.h>

#include "gftorf_rast.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of the grid-wide sum's index for a frame of P Gaussians whose binning buffer holds `binning_instances`: 4 per
 * Gaussian (its first slot), 4 per instance (the slot's list position) and the scan's block sums.  Host-only.  Any
 * contents: every call fills what it reads. */
size_t gft_detsum_index_bytes(int32_t P, int64_t binning_instances);

/* gft_backward in its fixed-order mode (io->det_partials is required) with the rows added by the grid-wide sum.  `index`:
 * device scratch of gft_detsum_index_bytes(cfg->P, num_rendered) bytes, 4-byte aligned; NULL: the comparator, exactly
 * gft_backward.  Everything else as gft_backward: same gradients, bit for bit, as the comparator gives. */
int gft_backward_det(void* hip_stream, const gft_config* cfg, const gft_backward_io* io, int64_t num_rendered, void* index);

#ifdef __cplusplus
}
#endif

#endif
