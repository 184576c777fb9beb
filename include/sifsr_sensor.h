/* sifsr_sensor.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): the differentiable sensor model at any ratio.
 * The adjoint of the banded operator of include/sifsr_degrade.h -- the gradient of the reference's downscale_LST_SR_to_LR(factor = f)
 * (utils.py:1671-1706), generic_downscale and downscale_Aster_to_* with respect to the fine raster -- and the reflect-border MTF
 * low-pass of get_output_ftm(factor = f) (utils.py:1833-1860) at any half width, forward and adjoint.
 *
 * Conventions are those of sifsr_degrade.h: every pointer is a DEVICE pointer (dense, row-major; `float` fp32, `unsigned char` one
 * byte per pixel), `stream` a hipStream_t passed as void*; functions only enqueue work on `stream` and return 0, 1001 for a shape
 * or limit error, 1002 for an argument error, 1003 for a workspace that is too small, or the hipError_t of a failed launch.  Nothing
 * is launched when an error is returned.  The symbols carry the prefix `sifsrt_`, live in the same library and have their own
 * declaration / export / memory-contract gate (tests/test_sensor_host.py, tests/test_sensor_gpu.py); sifsr_abi_version() is unchanged.
 *
 * ---- definitions ------------------------------------------------------------------------------------------------------------
 * R (on x n), per axis: the banded operator of sifsr_degrade.h for (n, factor, mtf, hkw, crop) -- the same table kernel writes its
 *         weights, from the same fp32 source coordinates.  STENCIL [lo(o), hi(o)] of output o: as there.  Both ends are
 *         non-decreasing in o (tests/test_sensor_host.py holds this over a sweep of sides, factors, half widths and crops), so the
 *         outputs whose stencil contains input pixel i are ONE run [o_lo(i), o_hi(i)], possibly empty -- the RANGE of i.  It has no
 *         small fixed length: 52 outputs at factor 1.25 with hkw 16.
 * L (n x n), per axis: the low-pass of get_output_ftm at half width hw = hkw, or ceil(factor) when hkw = 0: the 2 hw + 1 taps g of
 *         sifsr_degrade.h over the raster reflected by hw without repeating the edge (index -k -> k, n - 1 + k -> n - 1 - k; needs
 *         n >= hw + 1), no zero ring.  Row o of L has its weights inside [max(0, o - hw), min(n - 1, o + hw)], both reflections
 *         folded in; the range of pixel i is [max(0, i - hw), min(n - 1, i + hw)].
 *
 * Arithmetic, all three device entry points.  Weights and sums are float64; each output element is one chain of fused multiply-adds
 * in ascending index of what it sums over (input pixels for sifsrt_lowpass_fwd, output indices for the two adjoints), first along
 * one axis into a float64 intermediate in the workspace, then along the other; weights that are zero are skipped, not multiplied; the
 * result is rounded to fp32 once.  No atomics (each element is gathered by one thread): the same inputs give the same bits, and an
 * image gives the same bits alone and inside a batch.
 *
 * Launches: a linear chain on `stream`, no allocation, no host synchronisation: it can be captured into a hipGraph.
 * workspace: at least the stated number of bytes, 16-byte aligned (else 1002); its contents before the call do not matter and are
 * unspecified after it.  No buffer may overlap another.
 *
 * ---- sifsrt_degrade_bwd -----------------------------------------------------------------------------------------------------------
 * dout (B, oh, ow) with (oh, ow) of sifsrs_out_shape, out_valid (B, oh, ow) or NULL, dx (B, h, w).  dx = Ry^T . dout . Rx: the
 * gradient of sifsrs_degrade's `out` with respect to its `x`.  Where out_valid is 0 the output does not count: dout is not used
 * there and a NaN in it changes no bit of dx (sifsrs_degrade wrote fill_value there, which does not depend on x).  Every element of
 * dx is written; it is 0 where no counted output reads the pixel.  dout and out_valid are not written.
 * Launches: the table kernel of sifsrs_degrade (both axes), one range kernel (both axes: [o_lo, o_hi] per input index, by bisection
 * of the table's stencil ends), the adjoint column pass (dout -> the (B, oh, w) float64 intermediate; validity is applied here), the
 * adjoint row pass (-> dx).
 * Limits: those of sifsrs_degrade: 1 <= B <= 65535, hw + 1 <= h, w <= 16384, 1 < factor <= 16, hkw >= 0 and 1 <= hw <= 16,
 * 0 < mtf < 1, crop 0 or 1, both output sides >= 1 after the crop; otherwise (a NaN factor or mtf included) 1001.  Null dout / dx /
 * workspace, dout or dx not 4-byte aligned: 1002.  workspace_bytes < sifsrt_degrade_bwd_workspace_bytes(B, h, w, factor, hkw, crop):
 * 1003.
 *
 * ---- sifsrt_lowpass_fwd / sifsrt_lowpass_bwd -------------------------------------------------------------------------------------
 * x (B, h, w) -> out (B, h, w) = Ly . x . Lx^T; dout (B, h, w) -> dx (B, h, w) = Ly^T . dout . Lx.  Every element of out / dx is
 * written; x / dout are not.
 * Launches: one low-pass table kernel (both axes; it also writes the stencils), then for _fwd the row pass and the column pass of
 * sifsrs_degrade over the (B, h, w) float64 intermediate, for _bwd the range kernel and the two adjoint passes.
 * Limits: 1 <= B <= 65535, hw + 1 <= h, w <= 16384, 1 < factor <= 16, hkw >= 0 and 1 <= hw <= 16, 0 < mtf < 1; otherwise 1001.  Null
 * x / out / workspace, x or out not 4-byte aligned: 1002.  workspace_bytes < sifsrt_lowpass_workspace_bytes(B, h, w, factor, hkw)
 * (one size for both directions): 1003.
 *
 * sifsrt_degrade_bwd_workspace_bytes and sifsrt_lowpass_workspace_bytes are host only and return 0 for an invalid shape. */
#ifndef SIFSR_SENSOR_H
#define SIFSR_SENSOR_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

SIFSR_API size_t sifsrt_degrade_bwd_workspace_bytes(int B, int h, int w, double factor, int hkw, int crop);
SIFSR_API int sifsrt_degrade_bwd(const float* dout, const unsigned char* out_valid, float* dx, void* workspace, size_t workspace_bytes,
                                 int B, int h, int w, double factor, double mtf, int hkw, int crop, void* stream);
SIFSR_API size_t sifsrt_lowpass_workspace_bytes(int B, int h, int w, double factor, int hkw);
SIFSR_API int sifsrt_lowpass_fwd(const float* x, float* out, void* workspace, size_t workspace_bytes, int B, int h, int w, double factor,
                                 double mtf, int hkw, void* stream);
SIFSR_API int sifsrt_lowpass_bwd(const float* dout, float* dx, void* workspace, size_t workspace_bytes, int B, int h, int w, double factor,
                                 double mtf, int hkw, void* stream);

#endif /* SIFSR_SENSOR_H */
