/* sifsr_products.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): from the raw integer rasters of a MODIS
 * granule to training patches and their statistics (reference process_modis.py:38-335 and data_preparation.py:83-102, nested
 * Python loops over 324 windows per granule with a GeoTIFF round trip per patch).
 *
 * The arithmetic between "arrays read from the HDF" and "tensors in the training loop" is four data-sized passes -- decode, a
 * per-window census of fill pixels, the ordered selection of the accepted windows, and the gather of their patches with per-patch
 * moments -- and those are the entry points below.  Reading HDF files, the 60/40 split and the merge of the per-patch moments
 * (64 bytes per patch) stay on the host (sifsr/products.py).
 *
 * Conventions are those of sifsr_hip.h: every pointer is a DEVICE pointer to a dense array, `stream` a hipStream_t passed as
 * void*; functions only enqueue work on `stream` (no allocation, no synchronisation: every call can be captured) and return 0, a
 * SIFSR_ERR_* code (1001 shape, 1002 argument) or the hipError_t of a failed launch.  The symbols carry the prefix `sifsrp_`, live
 * in the same library, and have their own declaration / export / memory-contract gate (tests/test_products_host.py,
 * tests/test_products_gpu.py); sifsr_abi_version() is unchanged.
 *
 * Shapes: lst_raw is (h, w) uint16 and qc (h, w) uint8 (coarse), nir and red are (4h, 4w) int16 (fine).  lst_k = 0.02f * raw,
 * nir = 0.0001f * raw, ndvi = (nir - red) / (nir + red): float32 in numpy's evaluation order, FP contraction off, the quotient
 * correctly rounded (0 / 0 = NaN, x / 0 = +-inf).  Float rasters and patches must be 16-byte aligned, nir and red 8-byte aligned
 * (16-byte accesses are used when they are 16-byte aligned and w is even); anything else is SIFSR_ERR_ARG.
 *
 * Windows and their order are those of the reference's generator us.split (utils.py:79-84), literally: the OUTER loop steps
 * col0 = 0, window, 2 window, ... while col0 < h, the INNER loop row0 = 0, window, ... while row0 < w, and the window is
 * raw[row0 : row0 + window, col0 : col0 + window].  k, the reference's 1-based cnt1, counts every step; a window is FULL when
 * row0 + window <= h and col0 + window <= w, and only full windows are ever accepted.  On a square raster (every MODIS granule)
 * this is "column blocks outer, row blocks inner, ragged edge windows counted"; on a non-square one the reference's exchanged
 * loop bounds are kept, so that k names the same window here and there.
 *   nwin = ceil(h / window) * ceil(w / window)                                     steps of the generator
 *   nfull = min(ceil(h / window), w / window) * min(ceil(w / window), h / window)  full windows among them
 * No atomics: integer sums are exact, the float64 moments are formed in a fixed order, so results are bit-reproducible and a
 * patch does not depend on the other patches.
 */
#ifndef SIFSR_PRODUCTS_H
#define SIFSR_PRODUCTS_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

/* us.read_LST / us.read_NIRRED / us.compute_NDVI (utils.py:338, :428-435, :71; predict.py:76-78) over whole rasters:
 * lst_k (h, w) and ndvi (4h, 4w), float32, written in full.  clip = 1: ndvi > 1 becomes 1, ndvi < -1 becomes -1, NaN stays
 * (process_modis.py:304-305).  h, w >= 1.  Eight pixels per thread: one 16-byte load per input, two 16-byte stores. */
SIFSR_API int sifsrp_decode(const unsigned short* lst_raw, const short* nir, const short* red, float* lst_k, float* ndvi, int h,
                            int w, int clip, void* stream);

/* The census: counts (nwin, 2) int32, row k - 1 of window k.  [0] = the bad LST pixels of the window: qc_mode 0
 * (process_MOD21A1D:179-183) raw == 0; qc_mode 1 (process_MOD11A1:95-107) raw == 0 or qc & 1 (qc may be null in mode 0).
 * [1] = the pixels of the matching 4 window x 4 window fine window whose float32 nir + red == 0.0f (process_modis.py:290).
 * A window that is not full gets [-1, -1].  Every row is written exactly once, by the one workgroup that owns the window.
 * window % 4 == 0, window <= h, window <= w. */
SIFSR_API int sifsrp_census(const unsigned short* lst_raw, const unsigned char* qc, const short* nir, const short* red,
                            int* counts, int h, int w, int window, int qc_mode, void* stream);

/* The selection: window k is accepted when 0 <= counts[k-1][0] <= max_bad and counts[k-1][1] == 0.  The accepted windows, in the
 * order of k, go to index (cap, 3) int32 as [k, row0, col0]; n_accepted (1) int32 gets their number.  Rows >= n_accepted are not
 * written.  cap >= nfull.  One wavefront: ballot + prefix population count per 64 windows. */
SIFSR_API int sifsrp_select(const int* counts, int* index, int* n_accepted, int h, int w, int window, int max_bad, int cap,
                            void* stream);

/* The gather: for i < n_accepted, with [k, row0, col0] = index[i],
 *   lst (cap, 1, window, window)        0.02f * raw of the window, Kelvin
 *   ndvi (cap, 1, 4 window, 4 window)   the NDVI of the fine window, clipped to [-1, 1] (process_modis.py:299-305)
 *   moments (cap, 8) float64            [count, mean, M2, min, max] of the LST patch, [mean, M2] of the NDVI patch (its count is
 *                                       16 count), 0; M2 = the sum of squared deviations from the patch's own mean.
 * Rows >= n_accepted are not written; an index row that does not name a full window is skipped.  One workgroup per patch; a
 * thread forms count / mean / M2 of each 16-byte chunk in registers and merges them with Chan's update, then lanes, then
 * wavefronts merge in a fixed order: no second pass over the patch. */
SIFSR_API int sifsrp_gather(const unsigned short* lst_raw, const short* nir, const short* red, const int* index,
                            const int* n_accepted, float* lst, float* ndvi, double* moments, int h, int w, int window, int cap,
                            void* stream);

#endif /* SIFSR_PRODUCTS_H */
