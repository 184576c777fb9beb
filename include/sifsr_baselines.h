/* sifsr_baselines.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): the classical sharpening baselines the
 * paper compares the network with -- TsHARP, ATPRK and AATPRK (reference utils.py:854-1606, thunmpy-derived nested Python loops).
 *
 * The data-sized parts -- the NDVI/LST regressions, the coarse residual, the empirical semivariogram of the residual and the fused
 * unmix + correction pass over the fine raster -- are the entry points below.  The two 2-parameter variogram fits and the 26 x 26
 * kriging system are a few thousand scalar operations per image and stay on the host (sifsr/baselines.py).
 *
 * Conventions are those of sifsr_hip.h: every pointer is a DEVICE pointer to a dense array, `stream` a hipStream_t passed as
 * void*; functions only enqueue work on `stream` and return 0, a SIFSR_ERR_* code (1001 shape, 1002 argument) or the hipError_t of
 * a failed launch.  The symbols carry the prefix `sifsrb_`, live in the same library, and have their own declaration / export /
 * memory-contract gate (tests/test_baselines_host.py, tests/test_baselines_gpu.py); sifsr_abi_version() is unchanged.
 *
 * Shapes: lst and ndvi_c are (B, h, w) float32 (coarse), ndvi_f and out are (B, 4h, 4w) float32 (fine), h, w >= 5.  Only the
 * reference's scale 4 and block size 5 are built.  Intermediate results are float64, as the reference computes (an evaluation
 * operator, like sifsr_fft2_attenuation): one rounding, at the final float32 store.  No atomics: every reduction runs in a fixed
 * order (wavefront shuffles, then LDS), so results are deterministic and the rows of a batch do not depend on each other.
 * Every output is written in full.
 * Any other ratio H / h <= 8 (kriging: integer scales 2..8): sifsr/rbaselines.py, csrc/rbaselines_api.h.
 */
#ifndef SIFSR_BASELINES_H
#define SIFSR_BASELINES_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

/* linear_fit (utils.py:854-874): ordinary least squares of T = lst on I = ndvi_c over the pixels with T > min_T (strict) and
 * isfinite(I), per image, centred sums in two passes like scipy.stats.linregress.  fit (B, 2) = [a0 = intercept, a1 = slope];
 * fewer than two valid pixels, or a constant index, give NaN (0 / 0), not an error.  One workgroup per image. */
SIFSR_API int sifsrb_linfit(const float* lst, const float* ndvi_c, double* fit, int B, int h, int w, float min_T, void* stream);

/* linear_fit_window (utils.py:1256-1330): per coarse pixel the same regression over its (2 radius + 1)^2 window when more than
 * 2/3 of the window is valid, else the image's global fit `fit` (B, 2) (sifsrb_linfit); every pixel within `radius` of a border
 * gets the global fit.  coef (B, 2, h, w): plane 0 = a0, plane 1 = a1.  1 <= radius <= 8.  One thread per coarse pixel. */
SIFSR_API int sifsrb_linfit_window(const float* lst, const float* ndvi_c, const double* fit, double* coef, int B, int h, int w,
                                   int radius, float min_T, void* stream);

/* The coarse residual (utils.py:907-913, :1366-1372): delta (B, h, w) = T - m, m = a0 + a1 * I where T > 0, else 0.
 * per_pixel = 0: coef is (B, 2) (TsHARP, ATPRK); per_pixel = 1: coef is (B, 2, h, w) (AATPRK). */
SIFSR_API int sifsrb_residual(const float* lst, const float* ndvi_c, const double* coef, int per_pixel, double* delta, int B,
                              int h, int w, void* stream);

/* The empirical semivariogram of the residual (utils.py:1008-1051).  The 15 distance classes are scc * sqrt(k),
 * k in {0,1,2,4,5,8,9,10,13,16,17,18,20,25,32}.  For every coarse pixel with 2 <= r < h-2, 2 <= c < w-2 and every class k > 0,
 *   gamma_w(k) = sum over the pairs i < j (row-major) of the 5 x 5 window at that distance of (d_i - d_j)^2 / (2 npairs(k));
 * gamma (B, 15): [k] = the mean of gamma_w(k) over the windows where it is not exactly 0, 0 where there is none (and where the
 * mean is NaN: the reference's Gamma_coarse[isnan] = 0); [0] = 0.
 * A workgroup owns a 16 x 16 tile of windows (the tile and its 2-pixel halo staged in LDS) and writes its 14 sums and counts
 * to `scratch`; a second kernel adds the tiles in index order.  scratch: sifsrb_semivariogram_scratch_bytes(B, h, w) bytes, written
 * in full before it is read. */
SIFSR_API size_t sifsrb_semivariogram_scratch_bytes(int B, int h, int w);
SIFSR_API int sifsrb_semivariogram(const double* delta, double* scratch, double* gamma, int B, int h, int w, void* stream);

/* The fused unmix + correction pass: one thread owns 4 consecutive fine pixels (the row segment of one coarse pixel): one 16-byte
 * load of ndvi_f, one 16-byte store of out.  With T = lst[r, c] of the containing coarse pixel, I = ndvi_f, d = delta:
 *   mode 0 TsHARP (coef (B,2), lambdas unused, may be null)        u = (a0 + a1 I) * (T != 0 ? 1 : 0)     (a NaN index stays NaN)
 *                                                                  out = u + d[r,c], out = u where u == 0
 *   mode 1 ATPRK  (coef (B,2), lambdas (B,16,25))                  u as above
 *   mode 2 AATPRK (coef (B,2,h,w), lambdas (B,16,25))              u = |I| > 0 ? a0[r,c] + a1[r,c] I : 0  (a NaN index gives 0)
 *   modes 1, 2, for 2 <= r < h-2 and 2 <= c < w-2:                 out = u + sum_k lambdas[(y%4)*4 + x%4, k] * d[5x5 block, k],
 *                                                                  out = u where u == 0; the outer two coarse rows and columns
 *                                                                  get no correction: out = u (utils.py:1195-1207).
 * The image's 16 x 25 weights and the 5 delta rows of the block's coarse row sit in LDS. */
SIFSR_API int sifsrb_sharpen(const float* lst, const float* ndvi_f, const double* coef, const double* delta,
                             const double* lambdas, float* out, int B, int h, int w, int mode, void* stream);

#endif /* SIFSR_BASELINES_H */
