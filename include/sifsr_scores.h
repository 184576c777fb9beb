/* sifsr_scores.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): scoring rasters that have gaps.
 *
 * sifsr_gaps.h predicts on granules with holes (NaN where the input was invalid) and sifsr_masked.h trains on partly valid patches;
 * the entry points below score both.  sifsr_eval_metrics on a raster with one NaN or one 0 K pixel returns a row of NaN or a
 * meaningless data range, and sifsr_psnr_ssim scores a masked batch against the blocky fill that the masked loss ignores.  Here
 *
 *     a term is counted iff every pixel its stencil reads is valid,
 *
 * and each mean divides by the number of terms counted.  No reference counterpart.
 *
 * Conventions are those of sifsr_masked.h: every pointer is a DEVICE pointer unless said otherwise (dense, row-major; `float` fp32,
 * `double` fp64, `int` 32 bit, `unsigned char` one byte per pixel), `stream` a hipStream_t passed as void*; functions only enqueue
 * work on `stream` and return 0, 1001 for a shape error, 1002 for an argument error, 1003 for a workspace that is too small, or the
 * hipError_t of a failed launch.  Nothing is launched when an error is returned.  No float atomics, no allocation, no host
 * synchronisation: both calls can be captured into a hipGraph.  The symbols carry the prefix `sifsrv_`, live in the same library
 * and have their own declaration / export / memory-contract gate (tests/test_scores_host.py, tests/test_scores_gpu.py);
 * sifsr_abi_version() is unchanged.
 */
#ifndef SIFSR_SCORES_H
#define SIFSR_SCORES_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

/* ---- per-pair evaluation table over the valid pixels ------------------------------------------------------------------------
 * sifsr_eval_metrics (sifsr_hip.h: same images, columns, taps, data_range and shape limits, H, W >= 16) with
 *   mask     (B, H, W) or NULL, any non-zero byte = usable
 *   counts5  (B, 5): n0, n1, n3, n4, ns below
 * A pixel is valid iff  V = isfinite(a) && a != 0 && isfinite(b) && b != 0 && (mask == NULL || mask != 0)   (a = ref, b = pred;
 * 0 K and NaN are the no-data values, as in sifsrg_fill).  With
 *   E_r(p)  all pixels q with |q - p|_inf <= r lie inside the image and are valid,
 *   S(p)    all pixels q INSIDE THE IMAGE with |q - p|_inf <= 4 are valid (the reflect border of get_output_ftm reads only those),
 * the columns are summed over, and divided by the size of,
 *   PSNR, RMSE               V    n0     point-wise
 *   RMSE_grad                E_1  n1     3 x 3 Sobel bank
 *   SSIM                     E_3  n3     7 x 7 window
 *   GSSIM                    E_4  n4     7 x 7 window of 3 x 3 magnitudes
 *   RMSE low / mean / high   S    ns     9 x 9 PSF of g = |a - ftm(a)|; the three sums divide by ns (the reference's divide-by-N)
 * R = max - min over the valid pixels of both images unless data_range >= 0.  q25 / q75 are numpy's 'linear' percentiles in float32
 * of the ns values of g on S (the interpolated ranks clamped to ns - 1).  A column whose count is 0 is NaN; PSNR with mse = 0 is +inf.
 *   * The value at an invalid pixel -- NaN, +-inf, 0, anything -- changes no output bit: terms are selected, never weighted.
 *   * With every pixel valid the sets are the interiors of sifsr_eval_metrics (N, (H-2)(W-2), (H-6)(W-6), (H-8)(W-8), N) and out8 is
 *     bit-identical to it: the kernels are the same code, the same tiles and the same summation order.
 *   * Row i of a batch is bit-identical to its own B = 1 call.
 * scratch: at least sifsrv_eval_metrics_scratch_bytes(B, H, W) bytes (0: unsupported shape), 256-byte aligned; smaller: 1003.  After
 * the call its first B*H*W floats hold g, with the bit pattern 0xFFFFFFFF (a NaN) at every pixel outside S, and from the next
 * multiple of 256 bytes on, B rows of four floats {R, q25, q75, unused}; the rest is private.
 * Null ref / pred / taps9 / scratch / out8 / counts5: 1002.  sifsrv_eval_metrics_scratch_bytes is host only. */
SIFSR_API size_t sifsrv_eval_metrics_scratch_bytes(int B, int H, int W);
SIFSR_API int sifsrv_eval_metrics(const float* ref, const float* pred, const unsigned char* mask, int B, int H, int W,
                                  const float* taps9, float data_range, void* scratch, size_t scratch_bytes, double* out8,
                                  int* counts5, void* stream);

/* ---- train-time PSNR / SSIM over the valid pixels ---------------------------------------------------------------------------
 * sifsr_psnr_ssim (sifsr_hip.h: pred, targ (B, 1, H, W), H, W >= 7) with
 *   valid    (B, H/scale, W/scale), one byte per cell of scale x scale pixels, any non-zero byte = valid; scale 1 or 4 (4: the LR
 *            mask of sifsrm_patches_fill, H % 4 == W % 4 == 0).  Validity is that byte alone: the images are not inspected.
 *   counts2  {images that contribute a PSNR, images that contribute an SSIM}
 * data_range = max - min of the valid target pixels of the whole batch.  Per image, PSNR is taken over V and SSIM over E_3 (above);
 * an image without a valid pixel (without an all-valid window) contributes no PSNR (SSIM).  out2 = the means over the contributing
 * images, NaN where there is none.  Every byte valid: out2 is bit-identical to sifsr_psnr_ssim.
 * scratch: at least sifsrv_psnr_ssim_scratch_bytes(B, H, W) bytes, 8-byte aligned; smaller: 1003.  B > 65535, scale not 1 or 4, H or W
 * no multiple of scale: 1001.  Null pred / targ / valid / scratch / out2 / counts2: 1002.  The scratch size call is host only. */
SIFSR_API size_t sifsrv_psnr_ssim_scratch_bytes(int B, int H, int W);
SIFSR_API int sifsrv_psnr_ssim(const float* pred, const float* targ, const unsigned char* valid, int scale, int B, int H, int W,
                               void* scratch, size_t scratch_bytes, float* out2, int* counts2, void* stream);

#endif /* SIFSR_SCORES_H */
