/* rbaselines_api.h -- the C entry points of the sharpening baselines at any ratio (sifsr/rbaselines.py, csrc/rbaselines.hip;
 * DESIGN.md §9 f24): the passes over the FINE raster of TsHARP, ATPRK, AATPRK and DMS for a fine raster (H, W) over a coarse
 * raster (h, w) with H / h == W / w == p / q in lowest terms, 1 < p / q <= 8.  Everything that reads coarse rasters alone
 * (sifsrb_linfit, _linfit_window, _residual, _semivariogram of include/sifsr_baselines.h; sifsrd_trainset, _weights, _fit of
 * include/sifsr_dms.h) has no ratio in it and is used as it is.
 *
 * The header lives inside the package, not under include/: the entry points are bound by sifsr/rbaselines.py itself on the handle
 * of sifsr._lib.lib(), with the types parsed from this file, and have their own declaration / export / memory-contract gate
 * (tests/test_rbaselines_host.py, tests/test_rbaselines_gpu.py).  The declaration style, the conventions and the status codes are
 * those of include/sifsr_baselines.h: every pointer is a DEVICE pointer to a dense array, `stream` a hipStream_t passed as void*;
 * functions only enqueue work on `stream` and return 0, 1001 (shape) or 1002 (argument), or the hipError_t of a failed launch.
 * The symbols carry the prefix `sifsrh_`; sifsr_abi_version() is unchanged.
 *
 * Geometry, checked by every entry point before it launches (1001): 1 <= B <= 65535; 1 <= h, w <= 16384; with g = gcd(H, h),
 * p = H / g, q = h / g: q < p <= 8 q, w % q == 0 and W == w / q * p.  The cell of fine pixel (Y, X) is (Y q / p, X q / p), integer
 * divisions: cell i holds the fine rows [ceil(i p / q), ceil((i + 1) p / q)), between floor(p / q) and ceil(p / q) of them.
 * Intermediate results are float64 with one rounding at a float32 store.  No atomics: every sum runs in a fixed order, so results
 * are the same bits every run and the images of a batch do not depend on each other.  Every output is written in full.
 */
#ifndef SIFSR_RBASELINES_API_H
#define SIFSR_RBASELINES_API_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

/* DMS stage 1: per coarse cell the NaN-ignoring mean and population standard deviation of the fine pixels of the cell (of
 * fine^4 when pow4 != 0), added in row-major order in float64; a cell whose pixels are all NaN gives NaN.  mean, std (B, h, w)
 * float64; std may be null (not computed).  One thread per cell. */
SIFSR_API int sifsrh_aggregate(const float* fine, double* mean, double* std, int B, int h, int w, int H, int W, int pow4,
                               void* stream);

/* The fused unmix + correction pass of sifsrb_sharpen at any ratio: the fine raster is read once and written once.  With
 * (r, c) the cell of the pixel, T = lst[r, c], I = ndvi_f, d = delta (B, h, w):
 *   mode 0 TsHARP (coef (B,2), lambdas unused, may be null)   u = (a0 + a1 I) * (T != 0 ? 1 : 0)      (a NaN index stays NaN)
 *                                                             out = u + d[r, c], out = u where u == 0
 *   mode 1 ATPRK  (coef (B,2), lambdas (B, s^2, 25))          u as above
 *   mode 2 AATPRK (coef (B,2,h,w), lambdas (B, s^2, 25))      u = |I| > 0 ? a0[r,c] + a1[r,c] I : 0    (a NaN index gives 0)
 *   modes 1, 2: integer scales only, q == 1 and s = p in 2..8 (1001 otherwise), h, w >= 5.  For 2 <= r < h-2, 2 <= c < w-2:
 *               out = u + sum_k lambdas[(Y % s) s + X % s, k] * d[5 x 5 block centred on (r, c), k], out = u where u == 0;
 *               the outer two coarse rows and columns get out = u.
 * A workgroup owns the fine rows of one coarse row over 256 fine columns; in modes 1 and 2 the image's weights and the five
 * residual rows under the workgroup (two columns of halo either side, zero outside the raster) sit in LDS.  A thread owns 4
 * consecutive fine pixels of a row; they move as one 16-byte access where W % 4 == 0 and both bases are 16-byte aligned, as two
 * 8-byte accesses where W % 2 == 0 and the bases are 8-byte aligned, else one by one.  All three paths give the same bits. */
SIFSR_API int sifsrh_sharpen(const float* lst, const float* ndvi_f, const double* coef, const double* delta,
                             const double* lambdas, float* out, int B, int h, int w, int H, int W, int mode, void* stream);

/* DMS stage 4 for a fine raster of any (H, W): sifsrd_predict's arithmetic per pixel (the E leaf tables of the image in LDS, the
 * leaf by binary search with `x <= threshold -> left`, the clamped ridge, the mean over the estimators in index order).  A NaN
 * index is stored as NaN; an image with nleaf[b, 0] == 0 is all NaN.  1 <= H, W <= 131072, 1 <= E <= 32.  16-byte accesses where
 * H * W % 4 == 0 and both bases are 16-byte aligned, else one by one, with the same bits. */
SIFSR_API int sifsrh_predict(const float* ndvi_f, const double* thresholds, const int* nleaf, const double* leaves, float* sr,
                             int B, int E, int H, int W, void* stream);

/* DMS stage 5 at any ratio: res = lst^4 - m4 per cell, m4 (B, h, w) = sifsrh_aggregate(sr, pow4 = 1); res resampled to (H, W) in
 * float64 with the operator of sifsrr_upsample (bicubic, A = -0.75, align_corners = False, indices clamped, floor and fraction
 * of the source coordinate from integers; the one device function of csrc/ratio.h, instantiated in double), and
 * out = (res_hr + sr^4)^(1/4) in the same pass; a negative radicand gives NaN.  2 H h and 2 W w must stay below 2^31 (the
 * resampler's integer phase): 1001 otherwise. */
SIFSR_API int sifsrh_correct(const float* lst, const float* sr, const double* m4, float* out, int B, int h, int w, int H, int W,
                             void* stream);

#endif /* SIFSR_RBASELINES_API_H */
