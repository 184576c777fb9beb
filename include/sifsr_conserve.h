/* sifsr_conserve.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): does the super-resolved raster conserve the
 * observed one, and one residual correction that makes it.
 *
 * The whole training signal of the scale-invariance-free loss is Huber(D(SR), LST): the super-resolved raster, seen through the
 * sensor's MTF and decimated by 4, should be the raster the sensor observed.  At inference nothing measured that and nothing
 * enforced it, while every method the paper compares against ends in exactly this step (TsHARP's correction_linreg, the kriged
 * residual of ATPRK / AATPRK, DMS' residualAnalysis).  The one entry point below measures the residual LST - D(SR) over the cells
 * where it is defined and, on request, adds it back.  No reference counterpart.
 *
 * Conventions are those of sifsr_gaps.h: every pointer but `taps9` is a DEVICE pointer (dense, row-major; `float` fp32, `double`
 * float64, `unsigned char` one byte per pixel), `taps9` is a HOST pointer, `stream` a hipStream_t passed as void*; functions only
 * enqueue work on `stream` and return 0, 1001 for a shape error, 1002 for an argument error, 1003 for a workspace that is too
 * small, or the hipError_t of a failed launch.  Nothing is launched when an error is returned.  The symbols carry the prefix
 * `sifsrk_`, live in the same library and have their own declaration / export / memory-contract gate
 * (tests/test_conserve_host.py, tests/test_conserve_gpu.py); sifsr_abi_version() is unchanged.
 *
 * ---- definitions ------------------------------------------------------------------------------------------------------------
 * Rasters: sr (4h, 4w) [K], lst (h, w) [K], mask (h, w) bytes or NULL.  A CELL is an LST pixel (i, j) and the 4 x 4 sr pixels
 * [4i, 4i + 4) x [4j, 4j + 4) under it.
 *
 *   D   downscale_LST_SR_to_LR(., factor = 4, mtf) as csrc/loss.hip computes it: the separable 9-tap PSF `taps9` with reflect
 *       border (index -k -> k, n - 1 + k -> n - 1 - k) on the HR raster, then the bicubic /4 tap set k4 = (-3, 19, 19, -3) / 32 at
 *       rows / columns 4i .. 4i + 3.  Per axis that is ONE 12-tap filter q = k4 * taps9 over the HR indices 4i - 4 .. 4i + 7.
 *   U   cv2.resize(., INTER_CUBIC) x4 as csrc/pipeline.hip computes it: A = -0.75, half-pixel centres, source indices clamped at
 *       the RASTER edge (not at a tile edge).  HR index X reads the LR indices floor(X / 4) - 2 + (X % 4 >= 2) + (0 .. 3) with the
 *       coefficients of t = 0.625, 0.875, 0.125, 0.375 for X % 4 = 0, 1, 2, 3 (all of them dyadic: exact in fp32).
 *   c   cell validity: c[i, j] = isfinite(lst) && lst != 0 && (mask == NULL || mask != 0)   -- the rule of sifsrg_fill --
 *       && all 16 sr pixels of the cell are finite and non-zero   -- which covers fill_value = NaN and the 0 that cover = 0
 *       leaves where no tile reaches.
 *   r   the residual.  D at (i, j) reads the HR rows 4i - 4 .. 4i + 7, i.e. exactly the 3 x 3 cell neighbourhood, and the
 *       reflection at the raster edge stays inside it.  r[i, j] = lst[i, j] - D(sr)[i, j] is COUNTED iff c holds on the 3 x 3
 *       neighbourhood clipped to the raster; otherwise r[i, j] = 0.  (The rule of sifsr_scores.h: a term counts iff every pixel
 *       its stencil reads is valid.)  What an invalid pixel holds changes no output bit.
 *   one correction step   sr[p] += relax * U(r)[p] at every HR pixel p whose cell has c; every other pixel keeps its bits.
 *       Uncounted cells carry r = 0, so the correction fades out towards a gap and never pulls in filled values.
 *   statistics   over the counted cells, in float64: {count, bias = mean r, RMSE = sqrt(mean r^2), max |r|}; a row with nothing
 *       counted holds count 0 and NaN in the other three.
 *
 * ---- sifsrk_conserve ----------------------------------------------------------------------------------------------------------
 * stats (n_iter + 1, 4) float64: row 0 from sr as given, row k after the k-th step; n_iter = 0 is the pure check.
 * out (4h, 4w): the corrected raster, EVERY element written when n_iter >= 1 (pixels of cells without c: the bits of sr); with
 * n_iter = 0 out is not touched and may be NULL.  out may alias sr (the residual and the correction are separate launches);
 * partial overlap is not allowed.  sr, lst and mask are not written (unless out aliases sr).
 *
 * Arithmetic.  The definitions are in exact arithmetic on the fp32 taps.  The kernels form lst - D(sr) on deviations from a
 * per-workgroup constant c0 (the lst of the first cell of the workgroup's 8 x 8 cells that passes the lst part of c): with
 * S = sum(taps9), r = (lst - c0) - D(sr - c0) - c0 (S^2 - 1), so a 0.1 K residual is not the difference of two rounded 300 K
 * sums; q and S^2 - 1 are formed in float64 on the host and rounded to fp32 once.  Everything else is fp32 fused multiply-adds
 * in a fixed order; sums for the statistics are float64, added in a fixed order.  No atomics: the same inputs give the same
 * bits on every run.
 *
 * Launches: (n_iter + 1) residual kernels, n_iter correction kernels and one kernel that finishes the statistics -- a linear
 * chain on `stream`, no allocation, no host synchronisation: it can be captured into a hipGraph.
 *
 * workspace: at least sifsrk_workspace_bytes(h, w, n_iter) bytes, 8-byte aligned (else 1002); its contents before the call do not
 * matter.  After the call its first h * w floats hold r of the LAST statistics row (sifsr.conserve.consistency reads it); the
 * rest is unspecified.
 *
 * Limits: 3 <= h, w <= 16384 (the HR side must be >= 10 for the two reflect zones; the upper bound of sifsr_gaps.h),
 * 0 <= n_iter <= 64; otherwise 1001.  Null sr / lst / stats / workspace / taps9, null out with n_iter >= 1, sr or out not 16-byte
 * aligned, a non-finite relax: 1002.  A smaller `workspace_bytes`: 1003.
 * sifsrk_workspace_bytes is host only and returns 0 for an invalid shape. */
#ifndef SIFSR_CONSERVE_H
#define SIFSR_CONSERVE_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

SIFSR_API size_t sifsrk_workspace_bytes(int h, int w, int n_iter);
SIFSR_API int sifsrk_conserve(const float* sr, const float* lst, const unsigned char* mask, float* out, double* stats, void* workspace,
                              size_t workspace_bytes, int h, int w, const float* taps9, float relax, int n_iter, void* stream);

#endif /* SIFSR_CONSERVE_H */
