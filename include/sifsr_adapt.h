/* sifsr_adapt.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): fine-tuning a trained model.
 *
 * The scale-invariance-free loss needs no high-resolution target, so a trained ModelB_2 can be adapted to the granule it is about
 * to predict, on that granule's own tiles.  That takes three things the main header does not have:
 *   model_forward / model_backward   the network with FROZEN BatchNorm: normalisation by the running statistics in the forward
 *                                    AND in the backward, so a few dozen partly cloudy tiles neither couple through batch
 *                                    statistics nor move the running ones, and model.eval() predicts with the network that was
 *                                    optimised;
 *   dx / conv_in_dgrad               the gradient with respect to the network INPUT (sensitivity maps, the network as a
 *                                    differentiable block), in frozen and in batch-statistics mode;
 *   tile_targets                     the loss targets of the active tiles of a gappy granule (sifsr_gaps.h), on the device.
 * No reference counterpart.
 *
 * Conventions are those of sifsr_gaps.h: every pointer is a DEVICE pointer unless said otherwise (dense, row-major; `float` fp32,
 * `double` fp64, `unsigned char` one byte per pixel, `int` 32 bit, `long long` 64 bit), `stream` a hipStream_t passed as void*;
 * functions only enqueue work on `stream` and return 0, 1001 for a shape error, 1002 for an argument error, 1003 for a workspace
 * that is too small, or the hipError_t of a failed launch.  Nothing is launched when an error is returned.  The symbols carry the
 * prefix `sifsra_`, live in the same library and have their own declaration / export / memory-contract gate
 * (tests/test_adapt_host.py, tests/test_adapt_gpu.py); sifsr_abi_version() is unchanged.  fp32 only: there is no bf16 form.
 */
#ifndef SIFSR_ADAPT_H
#define SIFSR_ADAPT_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

/* ---- the network with frozen BatchNorm ---------------------------------------------------------------------------------------
 * Shapes, parameter / running-statistics / gradient layouts: sifsr_model_forward / sifsr_model_backward (sifsr_hip.h).
 * sifsra_model_workspace_bytes (host only) = sifsr_model_workspace_bytes(B, H, W, 1), 0 for an unsupported shape; both calls
 * below check `workspace_bytes` against it (1003).
 *
 * model_forward: sr is, bit for bit, sifsr_model_forward_ex(..., training = 0, compute = 0): the same launches, scale = gamma /
 * sqrtf(running_var + eps), shift = fma(-running_mean, scale, beta).  `running` is only read and there is no num_batches_tracked.
 * It runs in the training layout and leaves what the backward reads: every raw conv output, the pooled / residual / upsampled
 * tensors, scale / shift, and per layer mean = running_mean, invstd = 1 / sqrtf(running_var + eps).
 *
 * model_backward: the schedule of sifsr_model_backward.
 *   frozen = 1  on the workspace of sifsra_model_forward: at every BatchNorm layer dL/dy = scale * dz (the coefficients its
 *               consumers read are [scale, 0, 0] / [scale, shift, 0, 0]), dbeta = sum dz, dgamma = sum dz * xhat with the running
 *               statistics in xhat = (y - mean) * invstd -- where the sums arrive as (sum dz, sum dz*y), invstd * (sum dz*y - mean *
 *               sum dz) -- in float64 in the order of the batch-statistics finalize.  `scale` is the fp32 value the forward used.
 *   frozen = 0  on the workspace of a training-mode sifsr_model_forward(_ex): with dx == NULL every byte of `grads` and of the
 *               workspace is what sifsr_model_backward writes.
 *   dx          NULL, or (B, 2, H, W): the gradient with respect to x, by sifsra_conv_in_dgrad's kernel after the first layer's
 *               BatchNorm backward.  The SIFSR_HEAD_LINEAR switch counts as off in such a call.  `grads` does not depend on dx.
 * Non-finite data (sifsr_hip.h): sifsra_model_forward gives NaN for every sr pixel of an image whose x is not finite and leaves the
 * other images their bits; if d loss / d sr then holds a non-finite value, every element of `grads` and of dx is NaN.
 * Anything but 0 / 1 for `frozen`: 1002.  Null x / sr / dsr / params / running / grads / workspace: 1002. */
SIFSR_API size_t sifsra_model_workspace_bytes(int B, int H, int W);
SIFSR_API int sifsra_model_forward(const float* x, float* sr, const float* params, const float* running, void* workspace,
                                   size_t workspace_bytes, int B, int H, int W, float eps, void* stream);
SIFSR_API int sifsra_model_backward(const float* x, const float* dsr, const float* params, float* grads, float* dx, void* workspace,
                                    size_t workspace_bytes, int B, int H, int W, int frozen, void* stream);

/* ---- input gradient of the first convolution ---------------------------------------------------------------------------------
 * g, y (B, H, W, 16) NHWC, 16-byte aligned: the gradient with respect to relu(bn(y)) and the raw output of inbloc.bloc.0;
 * scale, shift (16); coef 3 x 16 float64 [scale | k1 | k0]; w (16, 2, 3, 3) OIHW -> dx (B, 2, H, W) NCHW, every element written:
 *   dy[co, q]    = (float)fma(coef[co], (double)(fmaf(y, scale, shift) > 0 ? g : 0), fma(k1[co], (double)y, k0[co]))
 *   dx[b, ci, p] = sum over (q, tap d) with clamp(q + d) == p, and co:  w[co, ci, d] * dy[co, q]
 * -- the adjoint of the replicate padding: an edge pixel also collects the taps that fell outside the image, a corner those of
 * both axes.  fp32 accumulation in a fixed order, no atomics: two runs are bit-equal.  B >= 1, H, W >= 3; else 1001. */
SIFSR_API int sifsra_conv_in_dgrad(const float* g, const float* y, const float* scale, const float* shift, const double* coef,
                                   const float* w, float* dx, int B, int H, int W, void* stream);

/* ---- loss targets of active tiles --------------------------------------------------------------------------------------------
 * filled (h, w) [K], valid (h, w) as sifsrg_fill left them; active, n_active as sifsrg_tiles_select left them for the same
 * (window, overlap, cover_edges).  Output tile i, 0 <= i < count, is tile active[(first + i) % n_active[0]] -- cyclic batching:
 *   lst_out     (count, 1, window, window)  (filled - mean_lst) * (1 / std_lst): the value sifsrg_tiles_prepare upsamples, bit for bit
 *   valid_out   (count, 1, window, window)  1 where valid is non-zero, else 0
 *   n_valid_out one int64: the number of ones in valid_out (8-byte aligned)
 * Every element of the three outputs is written; n_active[0] <= 0 gives zeros.  Nothing is read back to the host.
 * Layout errors as sifsrg_tiles_select, first < 0, count < 1 or count > 65535, std_lst == 0: 1001. */
SIFSR_API int sifsra_tile_targets(const float* filled, const unsigned char* valid, const int* active, const int* n_active, int first,
                                  int count, int h, int w, int window, int overlap, int cover_edges, float mean_lst, float std_lst,
                                  float* lst_out, unsigned char* valid_out, long long* n_valid_out, void* stream);

#endif /* SIFSR_ADAPT_H */
