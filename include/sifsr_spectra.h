/* sifsr_spectra.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): the Fourier-domain evaluation of
 * sifsr_fft2_attenuation for rasters whose sides need not be powers of two.
 *
 * The reference's evaluation pairs are what is left of a 256 x 256 prediction after reprojection to UTM, intersection with the ASTER
 * scene and a crop to the common rectangle (model_perf_aster_formatds.py:319-371): arbitrary l x c rectangles with both sides above
 * 40 pixels.  compare_methods.py:305-353 runs fft2 on exactly those, and the last four columns of performances.csv (FRR, FRO, FRU,
 * ATTENUATION_RMSE_ASTER_MODEL) come from it.  sifsr_fft2_attenuation is a radix-2 transform and refuses them.
 *
 * Conventions are those of sifsr_hip.h: `img`, `scratch`, `mag` and `spectrum` are DEVICE pointers (dense, row-major, fp32),
 * `stream` a hipStream_t passed as void*; the function only enqueues work on `stream` and returns 0, 1001 for a shape error, 1002
 * for an argument error (null img or scratch, both outputs null), 1003 for a scratch buffer that is too small, or the hipError_t of
 * a failed launch.  Nothing is launched when an error is returned.  The symbols carry the prefix `sifsrf_`, live in the same library
 * and have their own declaration / export / memory-contract gate (tests/test_spectra_host.py, tests/test_spectra_gpu.py);
 * sifsr_abi_version() is unchanged.
 *
 * ---- sifsrf_fft2_attenuation ------------------------------------------------------------------------------------------------------
 * For (B,H,W) images:
 *   mag      (optional, (B,H,W))  = np.fft.fftshift(np.abs(sp.fft.fft2(img)))            compare_methods.py:312-324
 *            bin k of an axis of length N lands at (k + N / 2) % N, N / 2 rounded down: for odd N that is fftshift's rule.
 *   spectrum (optional, (B,nr+1)) = us.compute_2D_attenuation_spectra(mag), centre (H / 2, W / 2), nr = min(H / 2, W / 2) - 1
 *            utils.py:598-636; element 0 is 1, element 1 + r the mean of ring r^2 < d^2 <= (r + 1)^2 in dB below the centre bin.
 *
 * Shapes: B >= 1; each side either a power of two in 4..2048 or any integer in 4..1024.  Otherwise 1001.
 *
 * Arithmetic: float64 throughout, stored as fp32.  An axis whose length is a power of two runs the radix-2 pass of
 * sifsr_fft2_attenuation; an image with two such sides runs that function's launches and gives its bits.  Any other axis of length
 * N runs Bluestein's chirp-z transform over the same in-LDS butterfly:
 *   w[n] = exp(-i pi n^2 / N), M the smallest power of two >= 2N - 1, a[n] = x[n] w[n] padded with zeros to M,
 *   b[n] = conj(w[|n|]) laid out circularly, X[k] = w[k] IFFT_M(FFT_M(a) FFT_M(b))[k],
 * with n^2 reduced mod 2N in integers before it becomes a phase, so that the phase is exact at every n.  FFT_M(b) depends on N alone
 * and is computed once per call and axis into `scratch`.  No atomics, fixed summation orders: the same inputs give the same bits on
 * every run, and image b of a batch gets the bits of its own B = 1 call.
 *
 * Launches: at most two filter prologues, the row pass, the column pass and, for `spectrum`, the two ring kernels -- a linear chain
 * on `stream`, no allocation, no host synchronisation.
 *
 * scratch: at least sifsrf_fft2_attenuation_scratch_bytes(B, H, W) bytes, 16-byte aligned: the bytes of
 * sifsr_fft2_attenuation_scratch_bytes plus 16 M bytes for each chirp axis.  Its contents before the call do not matter and are
 * unspecified after it.  sifsrf_fft2_attenuation_scratch_bytes is host only and returns 0 for a shape that is not accepted.
 * `img` is not written; nothing outside `mag`, `spectrum` and the stated scratch bytes is written. */
#ifndef SIFSR_SPECTRA_H
#define SIFSR_SPECTRA_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

SIFSR_API size_t sifsrf_fft2_attenuation_scratch_bytes(int B, int H, int W);
SIFSR_API int sifsrf_fft2_attenuation(const float* img, int B, int H, int W, void* scratch, size_t scratch_bytes, float* mag,
                                      float* spectrum, void* stream);

#endif /* SIFSR_SPECTRA_H */
