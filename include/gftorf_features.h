/*
 * gftorf_features.h -- C ABI of the feature blend (libgftorf_rast.so, gfx950): per-Gaussian features blended into an
 * image over a frame that gft_forward has already binned and blended, and the transpose of that blend.
 *
 * F-ToRF renders two per-Gaussian 3-D scene flows from the ToF camera on every flow iteration (the reference's
 * gaussian_renderer/__init__.py render_flow, called twice from train.py:249,256).  Both calls use the same geometry and
 * differ only in colors_precomp, and only the gradient of colors_precomp is used.  Here one gft_forward draws the frame
 * (binning, lists, per-pixel transmittance and contributor counts); these entry points read its scratch and
 *   forward:   out[c](p)       = sum_i f_i[c] alpha_i(p) T_i(p) + T_final(p) * bg[c](p)
 *   backward:  dL/df_i[c]      = sum_p alpha_i(p) T_i(p) dL/dout[c](p)          (reference backward.cu:757,788)
 * with alpha recomputed from the frame's geometry records exactly as the forward blend did (same exp, the 1/255 skip,
 * the 0.99 clamp, and the pixel's own contributor count as the stop rule).  Features are blended unclamped, like the
 * reference's colors_precomp.
 *
 * `cfg` is the gft_config of that forward (P, W, H and the background strides are read); `geom`, `img`, `binning` its
 * scratch buffers and `binning_instances` the capacity they were laid out for (the value passed to gft_forward /
 * gft_forward_enqueue / gft_forward_render).  A frame whose instances did not fit that buffer was not drawn: these calls then
 * write nothing either.  C is 3 or 6.  Device pointers, fp32, contiguous.  Nothing is read back to the host and nothing
 * uses a memset: both calls can be captured in a graph.  Returns 0 on success (gft_last_error()).
 */
#ifndef GFTORF_FEATURES_H
#define GFTORF_FEATURES_H

#include <stddef.h>
#include <stdint.h>

#include "gftorf_rast.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out [C, H, W] (written in full) from features [P, C].  bg: [C, H, W] addressed as bg[c*sc + y*sy + x*sx] with the
 * strides of cfg (bg_stride_c, _y, _x), or NULL for a zero background.  Channel c reads plane c: given the rasterizer's
 * 7-plane background, C = 6 blends channels 3..5 against its ToF planes 3..5 -- pass a background laid out for the features
 * (or NULL) when that is not what they should see.  C = 6 reads each feature row as three float2: `features` must be 8-byte
 * aligned (refused otherwise).  P = 0: zeros, like the rasterizer's outputs. */
int gft_render_features(void* hip_stream, const gft_config* cfg, const void* geom, const void* img, const void* binning,
                        int64_t binning_instances, int32_t C, const float* features, const float* bg, float* out);

/* dL_dfeatures [P, C] (written in full: zeros for Gaussians no pixel blended) from dL_dout [C, H, W].  acc: scratch of
 * P * 8 floats, any contents (cleared here by a kernel): the sums are added there with float atomics, one 32-byte row per
 * Gaussian, in the order the additions arrive: two runs of this call agree to rounding, not bit for bit.  The call below
 * is the one whose runs agree in every bit. */
int gft_render_features_backward(void* hip_stream, const gft_config* cfg, const void* geom, const void* img,
                                 const void* binning, int64_t binning_instances, int32_t C, const float* dL_dout, float* acc,
                                 float* dL_dfeatures);

/* The fixed-order backward: the same walk and the same per-(entry, quadrant) sums, produced by the same reduction, but every
 * sum is stored -- partials[(p * 4 + quadrant) * 8 + c], p the entry's position in the frame's id list -- and the rows are
 * added in the one order gftorf_detsum.h states.  Same inputs, same bits, however the workgroups were scheduled; the values
 * agree with the call above to rounding.
 *   partials: scratch of gft_feature_partials_bytes(binning_instances, W, H) bytes (128 per list slot; host-only size
 *             function), any contents: cleared here by a kernel (may be NULL when binning_instances is 0);
 *   index:    scratch of gft_detsum_index_bytes(cfg->P, binning_instances) bytes (gftorf_detsum.h) for the grid-wide sum, or
 *             NULL for the one-workgroup comparator (same bits, far slower);
 *   dL_dfeatures [P, C]: written in full, zeros for Gaussians no pixel blended; a frame that did not fit its binning buffer
 *             leaves it untouched, as above.  P = 0 returns at once.  No host read, no memset: capturable. */
size_t gft_feature_partials_bytes(int64_t binning_instances, int32_t W, int32_t H);
int gft_render_features_backward_det(void* hip_stream, const gft_config* cfg, const void* geom, const void* img,
                                     const void* binning, int64_t binning_instances, int32_t C, const float* dL_dout,
                                     void* index, float* partials, float* dL_dfeatures);

#ifdef __cplusplus
}
#endif

#endif
