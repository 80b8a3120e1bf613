/*
 * gftorf_flowviz.h -- C ABI of the optical-flow debug images of F-ToRF training, train.py:380-398 (libgftorf_rast.so, gfx950).
 *
 * The reference's debug block copies the rendered 2-D flow R and the target flow T of a direction to the host and runs
 * flow_to_image (scene/torf_utils.py:150-305) three times: on (R, T), on (T, T) and on (T - R, T).  flow_to_image writes
 * into its arguments, so the three calls are one sequence; gft_flowviz_images produces what the sequence produces, in two
 * launches, without a host read, an atomic or a memset, and leaves R and T as they are.
 *
 * With unk(X) = |X0| > 200 or |X1| > 200 (a NaN compares false, an infinity is unknown):
 *   Rc = R with both components 0 where unk(R); a NaN stays
 *   Tc = T with both components 0 where unk(T), then both 0 where either is a NaN
 *   maxrad = max over the pixels of sqrt(Tc0 * Tc0 + Tc1 * Tc1), every operation a rounded float32 one
 *   den = (double)(float)(maxrad * 1.1f) + 2^-52
 *   image(X), in float64: u = X0 / den, v = X1 / den; nan = isnan(u) | isnan(v), there u = v = 0; rad = sqrt(u * u + v * v);
 *     a = atan2(-v, -u) / pi; fk = (a + 1) / 2 * 54 + 1; k0 = floor(fk); k1 = k0 + 1, 56 wrapping to 1; f = fk - k0;
 *     per channel i: c0 = wheel[k0 - 1][i] / 255, c1 = wheel[k1 - 1][i] / 255, col = (1 - f) * c0 + f * c1;
 *     col = rad <= 1 ? 1 - rad * (1 - col) : col * 0.75; byte = floor(255 * col), 0 where nan
 *   viz = image(Rc), black where unk(R);  gt = image(Tc) (an unknown or NaN pixel of T comes out white, as in the reference);
 *   error: E = Tc - Rc in float32, Ec = E with both components 0 where unk(E); image(Ec), black where unk(E)
 * The float64 path is numpy >= 2's (float32 + np.finfo(float).eps is a float64, and so is a float32 array divided by it).
 * No statement contracts into a multiply-add; only atan2 is not an IEEE operation.
 *
 * Device pointers, fp32 inputs.  A plane is H * W contiguous floats; the two planes of a flow are `stride` floats apart.
 * Returns 0 on success (gft_last_error()).
 */
#ifndef GFTORF_FLOWVIZ_H
#define GFTORF_FLOWVIZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFT_FLOWVIZ_WHEEL_ROWS 55   /* the Middlebury colour wheel: segments of 15, 6, 4, 11, 13 and 6 entries */
#define GFT_FLOWVIZ_IMAGES 3        /* viz, gt, error: the order they lie in `out` */
#define GFT_FLOWVIZ_RUN 4           /* pixels of one lane: 12 bytes per image */

/* Workgroups of either launch for an image of `pixels`; the partials hold that many floats and one more, the folded
 * maxrad.  0 when pixels < 1. */
int64_t gft_flowviz_blocks(int64_t pixels);

/* The 55 x 3 bytes of the colour wheel, floor(255 * j / n) ramps (HOST, static). */
const uint8_t* gft_flowviz_wheel(void);

/* flow: planes 0 and 1 of R, flow_plane_stride apart; gt: planes 0 and 1 of T, gt_plane_stride apart; neither is written.
 * partials: gft_flowviz_blocks(H * W) + 1 floats, 4-byte aligned; after the call the last one is maxrad.
 * out: uint8 [3, H, W, 3] (viz, gt, error), any alignment, every byte written.
 * Fails before any launch on a NULL pointer, H < 1, W < 1 or a negative stride. */
int gft_flowviz_images(void* hip_stream, int32_t H, int32_t W, const float* flow, int64_t flow_plane_stride, const float* gt,
                       int64_t gt_plane_stride, void* partials, void* out);

#ifdef __cplusplus
}
#endif
#endif
