/*
 * gftorf_optim.h -- C ABI of the fused Adam step of libgftorf_rast.so (gfx950).
 *
 * SURVEY section 8(f) row 4 (optimizer part).  The reference updates its ~91 floats per Gaussian
 * with `torch.optim.Adam(l, lr=0.0, eps=1e-15)` (scene/gaussian_model.py:274, stepped at
 * train.py:470), whose default multi-tensor path runs one elementwise kernel per arithmetic
 * operation.  This is the same update (torch/optim/adam.py `_single_tensor_adam`, no amsgrad, no
 * maximize) in one pass: 16 B read + 12 B written per element.
 *
 *   g' = g + weight_decay * p
 *   m  = m + (1 - beta1) * (g' - m)                       (lerp)
 *   v  = beta2 * v + (1 - beta2) * g' * g'
 *   p  = p - (lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
 *
 * Device pointers, fp32; returns 0 on success (gft_last_error()).
 */
#ifndef GFTORF_OPTIM_H
#define GFTORF_OPTIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One entry of the table a step is given: a step updates several tensors in one launch per GFT_ADAM_MAX_TENSORS tensors.  Every
 * tensor has its own learning rate and step count (the reference keeps one tensor per parameter group, each with its own lr,
 * scene/gaussian_model.py:247-272); betas / eps / weight decay are shared. */
#define GFT_ADAM_MAX_TENSORS 40
typedef struct gft_adam_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;
    double lr;
    int64_t step;      /* 1-based count of this update */
} gft_adam_tensor;

/* The step.  Hyper-parameters as torch holds them (Python floats = double); derived factors (1 - beta, lr / (1 - beta1^t),
 * sqrt(1 - beta2^t)) are formed in double precision and rounded to fp32 once, as torch does.  Three optional inputs:
 *
 * row_mask, rows -- opt-in, NOT the reference's optimizer (which is dense): the update restricted to the rows of a mask, SURVEY
 *   section 8(f) row 4, "sparse Adam on visible Gaussians".  Every tensor has `rows` rows (n = rows x floats per row); row r takes
 *   the step when row_mask[r] != 0 (device pointer, one byte per row: e.g. `radii > 0` of the iteration's render, reference
 *   train.py:181 `visibility_filter`); the other rows' parameter and moments are left as they are (their moments do not decay).
 *   16-byte groups without a masked-in element are neither read nor written.  The mask is read when the kernel runs: a replayed
 *   graph follows the mask's contents of that replay.  With the learning rates in the table rows == 0 is a call with nothing to
 *   do; with them on the device rows must be > 0 (every count would advance with nothing to update).
 *
 * lr, step, factors -- the learning rates and step counts ON THE DEVICE: nothing the update depends on is baked into the call,
 *   so it can be captured in a HIP graph (torch.cuda.graphs around a whole training iteration) and replayed while the schedule
 *   moves the learning rates.  tensors[c].lr / .step are ignored; lr[c] (device, double: the Python float the reference's
 *   scheduler computes, scene/gaussian_model.py:294-310) and step[c] (device, fp32 count of updates DONE, as torch's capturable
 *   Adam keeps it) are read by a one-workgroup kernel in front of the update, which adds 1 to every step[c] -- one per tensor,
 *   empty ones included, whatever a mask holds -- and derives lr / (1 - beta1^t) and sqrt(1 - beta2^t) in double precision,
 *   rounded to fp32 once -- the factors the host forms otherwise, to the rounding of the device's double pow -- into
 *   factors[2 c], factors[2 c + 1] (device scratch, 2 * count floats).  lr and step are host arrays of device pointers, one per
 *   tensor, because optimizer state is edited tensor by tensor (scene/gaussian_model.py:456-540).
 *
 * grad_scale -- device pointer to one float, e.g. out + 1 of gft_grad_norm below: every gradient value is multiplied by
 *   *grad_scale, rounded to fp32, before anything else -- the update equals the one without it on gradients scaled by
 *   gft_grad_scale, bit for bit -- and the gradient memory is not written. */
int gft_adam_step(void* hip_stream, int32_t count, const gft_adam_tensor* tensors /*host*/,
                  int64_t rows, const uint8_t* row_mask      /* NULL: dense step, rows must be 0 */,
                  const double* const* lr, float* const* step, float* factors
                                                             /* all NULL: lr / step of the table (host);
                                                                all given: on the device, tick in front */,
                  double beta1, double beta2, double eps, double weight_decay,
                  const float* grad_scale                    /* device or NULL */);

/* ---- gradient-norm clipping: torch.nn.utils.clip_grad_norm_(parameters, max_norm) with the L2 norm (reference train.py:468).
 *
 * A set of gradient tensors is given as two host arrays: grads[c] (device pointer, fp32, any 4-byte alignment) and n[c]
 * (elements, >= 0; a span of 0 elements is skipped and its pointer is not looked at).
 *
 * gft_grad_norm:  out[0] = sqrt(sum of g^2 over all spans), out[1] = min(1, max_norm / (out[0] + 1e-6)), the coefficient
 * torch multiplies the gradients by, formed in fp32 as torch forms it (reciprocal, times max_norm, clamp: a NaN stays a NaN).
 * Squares are added in fp32 inside a thread (16 groups of four at most), everything above that in double; one double per
 * workgroup goes through `scratch` (device, 8-byte aligned, gft_grad_norm_scratch_bytes(sum of n, count) bytes: host-only
 * query, an upper bound) and is added in a fixed order: no atomics, no counters, nothing to clear beforehand, the same bits
 * every call.  Squares that overflow fp32 give inf, a NaN gives NaN in both outputs, as in torch.  count == 0 (or only
 * empty spans) writes out = {0, 1}; with count == 0 and out == NULL nothing is done.  No host read: capturable. */
size_t gft_grad_norm_scratch_bytes(int64_t total_elements, int32_t count);
int gft_grad_norm(void* hip_stream, int32_t count, const float* const* grads /*host array of device pointers*/,
                  const int64_t* n /*host*/, double max_norm, void* scratch /*device*/, size_t scratch_bytes,
                  float* out /*device, 2 floats*/);

/* g *= *coef over the same kind of table, in place (coef: device, e.g. out + 1 of gft_grad_norm).  Nothing is stored when
 * *coef == 1, the values being the same. */
int gft_grad_scale(void* hip_stream, int32_t count, float* const* grads /*host array of device pointers*/,
                   const int64_t* n /*host*/, const float* coef /*device*/);

#ifdef __cplusplus
}
#endif
#endif
