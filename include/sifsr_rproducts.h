/* sifsr_rproducts.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): sifsr_products.h at any ratio.  From the
 * raw integer rasters of a granule to training patches, their statistics and the counts the masked loss at a ratio needs, with
 * the fine window side `hr` as an argument: the reference's window rules, acceptance rules and order (us.split,
 * process_modis.py:88-112, :172-183, :281-305, data_preparation.py:32-39, :83-102), which it states at x4 only.
 *
 * Conventions are those of sifsr_products.h: every pointer is a DEVICE pointer to a dense array, `stream` a hipStream_t passed as
 * void*; functions only enqueue work on `stream` (no allocation, no synchronisation: every call can be captured) and return 0, a
 * SIFSR_ERR_* code (1001 shape, 1002 argument) or the hipError_t of a failed launch.  No atomics: integer sums are exact, the
 * float64 moments merge in a fixed order, so results are the same bits on every run.  The symbols carry the prefix `sifsrn_`, live
 * in the same library and are gated by tests/test_capi_gate.py (memory-contract cases: tests/test_rproducts_gpu.py);
 * sifsr_abi_version() is unchanged.
 *
 * Geometry.  p / q = hr / window in lowest terms.  A pair (window, hr) is TRAINABLE, and only such a pair is accepted by census
 * and gather, when
 *   (a) sifsrr_geometry(window, window, window, hr, 0, 0) accepts it: 1 <= window <= 64, hr a multiple of 8 in 24..256,
 *       window < hr <= 16 window,
 *   (b) hr <= 8 window, the limit of the fused loss (sifsr_rloss.h), and
 *   (c) the sensor model at factor hr / window sees (window, window) of an (hr, hr) patch: sifsrs_out_shape(hr, hr, hr / window,
 *       0, crop = 1).  (8, 24), (16, 40), (12, 24), (8, 32), (12, 40), (24, 56), (48, 160), (64, 160) and (64, 192) pass;
 *       (20, 24) does not: the crop of the sensor model leaves 21.
 * This is checked on the host before any launch; a pair that fails is SIFSR_ERR_SHAPE.
 *
 * Shapes: lst_raw is (h, w) uint16 and qc (h, w) uint8, h and w multiples of q with window <= h, w <= 16384; nir and red are
 * exactly (h p / q, w p / q) int16.  The fine window of the LST window (row0, col0) is rows [row0 p / q, row0 p / q + hr) and
 * columns [col0 p / q, col0 p / q + hr).  The window order, k, nwin, nfull and the full-window rule are those of sifsr_products.h,
 * word for word; they depend on the LST raster alone, which is why the selection is sifsrp_select, unchanged.  The arithmetic
 * (lst_k, nir, ndvi, the correctly rounded quotient) is that header's too, from the same device functions.
 *
 * Alignment: float rasters and patches must be 16-byte aligned (SIFSR_ERR_ARG otherwise); lst_raw, qc, nir and red need only the
 * alignment of their element, 2 bytes for the int16 rasters.  hr is a multiple of 8, so every fine window starts a multiple of 8
 * int16 into its row, and a thread always works on 8 consecutive int16 of a row; how it loads them is picked per call from the
 * base pointers of nir and red and the row pitch 2 fw bytes: one 16-byte access (bases on 16 bytes, fw % 8 == 0), two 8-byte
 * accesses (bases on 8 bytes, fw % 4 == 0) or eight 2-byte accesses (anything else, an odd fw included).  The three give the
 * same bits, moments included.  Stores into the patch arrays are 16 bytes wide.
 */
#ifndef SIFSR_RPRODUCTS_H
#define SIFSR_RPRODUCTS_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

/* sifsrp_decode with the fine size as an argument: lst_k (h, w) = 0.02f * raw and ndvi (fh, fw), float32, written in full;
 * clip = 1 clips ndvi to [-1, 1], NaN stays.  1 <= h <= fh, 1 <= w <= fw, h, w <= 16384, and fh / h == fw / w as rationals
 * (fh w == fw h), at most 16; anything else is SIFSR_ERR_SHAPE.  The rasters are read as flat arrays: the access width follows
 * the base pointers alone, and a tail of fewer than 8 pixels is done one by one. */
SIFSR_API int sifsrn_decode(const unsigned short* lst_raw, const short* nir, const short* red, float* lst_k, float* ndvi, int h,
                            int w, int fh, int fw, int clip, void* stream);

/* The census: counts (nwin, 2) int32, row k - 1 of window k.  [0] = the bad LST pixels of the window (qc_mode 0: raw == 0;
 * qc_mode 1: raw == 0 or qc & 1; qc may be null in mode 0), [1] = the pixels of the hr x hr fine window whose float32
 * nir + red == 0.0f.  A window that is not full gets [-1, -1].  Every row is written exactly once, by the one workgroup that
 * owns the window. */
SIFSR_API int sifsrn_census(const unsigned short* lst_raw, const unsigned char* qc, const short* nir, const short* red,
                            int* counts, int h, int w, int window, int hr, int qc_mode, void* stream);

/* The gather, after sifsrp_select(counts, index, n_accepted, h, w, window, max_bad, cap): for i < n_accepted, with
 * [k, row0, col0] = index[i],
 *   lst (cap, 1, window, window)   0.02f * raw of the window, Kelvin
 *   ndvi (cap, 1, hr, hr)          the NDVI of the fine window, clipped to [-1, 1]
 *   moments (cap, 8) float64       the columns of sifsrp_gather: [count, mean, M2, min, max] of the LST patch, [mean, M2] of the
 *                                  NDVI patch, 0.  The count of the NDVI patch is hr * hr and is not stored.
 * Rows >= n_accepted are not written; an index row that does not name a full window of the generator (row0 and col0 multiples of
 * window, inside the raster) is skipped.  cap >= nfull.  One workgroup per patch; the moments of 8 consecutive pixels are formed
 * in registers and merged per thread, then lanes, then wavefronts, in the order of sifsrp_gather: at hr == 4 window the two calls
 * give the same bits. */
SIFSR_API int sifsrn_gather(const unsigned short* lst_raw, const short* nir, const short* red, const int* index,
                            const int* n_accepted, float* lst, float* ndvi, double* moments, int h, int w, int window, int hr,
                            int cap, void* stream);

/* Per-patch counts for the masked loss at a ratio: valid (N, window, window) uint8, counts (N, 2) int64 (8-byte aligned).
 * counts[n] = {n1, n2}: n1 = the valid (non-zero) cells of patch n, n2 = the HR pixels (Y, X) of its hr x hr patch whose cell
 * (Y window / hr, X window / hr), rounded down, is valid.  Row n is what sifsrq_valid_counts gives for patch n alone; a batch's
 * counts are the sum of its rows.  N >= 1, 1 <= window <= hr <= 16384.  One workgroup per patch, integer arithmetic. */
SIFSR_API int sifsrn_patch_counts(const unsigned char* valid, long long* counts, int N, int window, int hr, void* stream);

/* The HR mask under an LR mask: valid (B, h, w) uint8, out (B, H, W) uint8, out[b, Y, X] = valid[b, Y h / H, X w / W] != 0 (0 or
 * 1; the divisions round down).  The rule of sifsrr_tiles_blend's masked form and of sifsr_rloss.h.  1 <= B <= 65535,
 * 1 <= h <= H <= 16384, 1 <= w <= W <= 16384.  Every byte of out is written. */
SIFSR_API int sifsrn_expand_valid(const unsigned char* valid, unsigned char* out, int B, int h, int w, int H, int W, void* stream);

#endif /* SIFSR_RPRODUCTS_H */
