/* sifsr_degrade.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): the sensor model at any ratio.  A fine raster,
 * seen through the sensor's MTF and resampled by a non-integer factor: the reference's downscale_Aster_to_coarse (90 m -> 926.25 m,
 * utils.py:1759-1793), downscale_Aster_to_fine (90 m -> 231.656 m, :1796-1830), generic_downscale (:1642-1668) and, with `crop`, the
 * cut of downscale_LST_SR_to_LR (:1671-1706) at any factor, with the validity of every output.
 *
 * Conventions are those of sifsr_conserve.h: every pointer but `oh` / `ow` is a DEVICE pointer (dense, row-major; `float` fp32,
 * `unsigned char` one byte per pixel), `stream` a hipStream_t passed as void*; functions only enqueue work on `stream` and return 0,
 * 1001 for a shape or limit error, 1002 for an argument error, 1003 for a workspace that is too small, or the hipError_t of a failed
 * launch.  Nothing is launched when an error is returned.  The symbols carry the prefix `sifsrs_`, live in the same library and have
 * their own declaration / export / memory-contract gate (tests/test_degrade_host.py, tests/test_degrade_gpu.py); sifsr_abi_version()
 * is unchanged.
 *
 * ---- definitions ------------------------------------------------------------------------------------------------------------
 * Per axis of length n, with `factor` > 1, `mtf` in (0, 1) and the half width hw = hkw, or ceil(factor) when hkw = 0:
 *
 *   g     the 2 hw + 1 taps exp(-k^2 / (2 sigma^2)) / sum, sigma = sqrt(-ln(mtf) / 2) / (pi * 0.5 / factor), in float64: the separable
 *         factor of generate_psf_kernel(1.0, factor, mtf, hw) (the fp32 2-D kernel differs from g (x) g by 4e-10).
 *   pad   reflect by hw on each side without repeating the edge (index -k -> k, n - 1 + k -> n - 1 - k); needs n >= hw + 1.
 *         np = n + 2 hw.
 *   blur  g over the padded raster with padding = "same": taps beyond [0, np) meet zeros.  The blurred raster keeps np entries and
 *         its outer hw entries on each side are darkened -- the ZERO RING.  This is the reference's behaviour and is reproduced.
 *   resample  F.interpolate(scale_factor = 1 / factor, mode = "bicubic"): on = floor(np * (1 / factor)) in double,
 *         scale = (float)(1.0 / (1.0 / factor)); for output o: s = scale * (o + 0.5f) - 0.5f, each step rounded to fp32,
 *         f = floor(s), t = s - f; the blurred entries f - 1 .. f + 2, CLAMPED to [0, np - 1], with the Keys coefficients (A = -0.75)
 *         of t, evaluated in float64 from the fp32 t.  Every output has its own phase.
 *   crop  removes c = (int)(hw / factor) outputs on each side: output o of the call is output o + c of the resampler.
 *
 * The four steps are one banded operator R (on x n) per axis and the result is out = Ry . x . Rx^T.  Row o of R has its non-zero
 * weights inside 2 hw + 4 consecutive original pixels -- the STENCIL of o on that axis; o TOUCHES THE RING iff a blurred entry it
 * samples with a non-zero coefficient is nearer than hw to an end of the padded axis.
 *
 * Validity (the rule of sifsr_scores.h: a term counts iff everything its stencil reads is valid): with `valid` (h, w) bytes per
 * image, non-zero = valid, out_valid[oy, ox] = 1 iff every pixel of stencil(oy) x stencil(ox) is valid and neither oy nor ox touches
 * the ring, else 0; where it is 0, out holds `fill_value`; where it is 1, what invalid pixels hold -- NaN included -- changes no
 * output bit.  With valid = NULL every pixel is valid and out holds the reference's values everywhere, darkened ring included;
 * out_valid, when asked for, still marks the ring.
 *
 * ---- sifsrs_degrade ---------------------------------------------------------------------------------------------------------------
 * x (B, h, w), valid (B, h, w) or NULL, out (B, oh, ow) with (oh, ow) of sifsrs_out_shape, out_valid (B, oh, ow) or NULL.  Every
 * element of out and of out_valid is written; x and valid are not.  No buffer may overlap another.
 *
 * Arithmetic.  Weights and sums are float64: the table kernel forms each weight from g (float64, from the host) and the Keys
 * coefficients; the row pass and the column pass accumulate in float64 with fused multiply-adds in a fixed order and the result is
 * rounded to fp32 once.  Weights that are zero are skipped, not multiplied.  No atomics: the same inputs give the same bits.
 *
 * Launches: one table kernel (both axes), one row pass (x -> the (B, oh, w) float64 intermediate in the workspace), one column pass
 * -- a linear chain on `stream`, no allocation, no host synchronisation: it can be captured into a hipGraph.
 *
 * workspace: at least sifsrs_workspace_bytes(B, h, w, factor, hkw, crop) bytes, 16-byte aligned (else 1002); its contents before
 * the call do not matter and are unspecified after it.
 *
 * Limits: 1 <= B <= 65535, hw + 1 <= h, w <= 16384, 1 < factor <= 16, hkw >= 0 and 1 <= hw <= 16, 0 < mtf < 1, crop 0 or 1, both
 * output sides >= 1 after the crop; otherwise (a NaN factor or mtf included) 1001.  Null x / out / workspace (or oh / ow), x or out
 * not 4-byte aligned: 1002.  A smaller `workspace_bytes`: 1003.
 * sifsrs_out_shape and sifsrs_workspace_bytes are host only; the latter returns 0 for an invalid shape. */
#ifndef SIFSR_DEGRADE_H
#define SIFSR_DEGRADE_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

SIFSR_API int sifsrs_out_shape(int h, int w, double factor, int hkw, int crop, int* oh, int* ow);
SIFSR_API size_t sifsrs_workspace_bytes(int B, int h, int w, double factor, int hkw, int crop);
SIFSR_API int sifsrs_degrade(const float* x, const unsigned char* valid, float* out, unsigned char* out_valid, void* workspace,
                             size_t workspace_bytes, int B, int h, int w, double factor, double mtf, int hkw, int crop, float fill_value,
                             void* stream);

#endif /* SIFSR_DEGRADE_H */
