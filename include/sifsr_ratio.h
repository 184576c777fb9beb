/* sifsr_ratio.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): whole-granule prediction at any ratio
 * hr / win between the network's raster and the LST raster.
 *
 * sifsr_mosaic.h and sifsr_gaps.h are x4 in their shape rules, their launch geometry and their resampler.  A model trained at
 * another ratio (sifsr_sensor.h: 64 x 64 -> 192 x 192, 160 x 160 or 128 x 128 patches) needs the same three steps -- cut and
 * resample the tiles, predict, blend -- with a bicubic resampler whose phase is exact at every ratio.  The entry points below
 * are those steps; the x4 entry points keep their kernels and their bits.
 *
 * Conventions are those of sifsr_mosaic.h and sifsr_gaps.h: every pointer is a DEVICE pointer (dense, row-major; `float` fp32,
 * `unsigned char` one byte per pixel, `int` 32 bit) except `out6` of sifsrr_geometry, `stream` a hipStream_t passed as void*;
 * functions only enqueue work on `stream` and return 0, 1001 for a shape error, 1002 for an argument error, or the hipError_t of
 * a failed launch.  Nothing is launched when an error is returned.  The symbols carry the prefix `sifsrr_`, live in the same
 * library and have their own declaration / export / memory-contract gate (tests/test_ratio_host.py, tests/test_ratio_gpu.py);
 * sifsr_abi_version() is unchanged.
 *
 * Geometry.  A tile is `win` LST pixels and `hr` network pixels on a side; the ratio is p / q = hr / win in lowest terms.
 *   1 <= win <= 64;  hr % 8 == 0 and 24 <= hr <= 256 (the model's rule);  win < hr <= 16 win;
 *   lst_h % q == 0 and lst_w % q == 0, win <= lst_h, lst_w <= 16384;  overlap % q == 0 and 0 <= 2 overlap <= win.
 * Anything else is 1001.  The NDVI raster and the output raster are (H, W) = (lst_h p / q, lst_w p / q).  Tile origins per axis,
 * `cover` and the numbering t = ty * Tx + tx are those of sifsr_mosaic.h (csrc/mosaic.h is the one definition); under the rules
 * above the stride, the flush origin and the overlap are whole pixels of both rasters: a tile at LST origin o starts at HR
 * pixel o p / q, and the HR overlap is R = overlap p / q.
 */
#ifndef SIFSR_RATIO_H
#define SIFSR_RATIO_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

/* ---- the geometry (host only, no GPU touched) ---------------------------------------------------------------------------------
 * out6 (a HOST array of 6 ints) = p, q, Ty, Tx, H, W.  Returns 0, 1001 for any violation of the rules above (out6 untouched),
 * 1002 for a null out6.  The return value is a status, not a count. */
SIFSR_API int sifsrr_geometry(int lst_h, int lst_w, int win, int hr, int overlap, int cover, int* out6);

/* ---- bicubic resampling ---------------------------------------------------------------------------------------------------------
 * x (B, h, w) -> out (B, H, W), every element written; H >= h >= 1, W >= w >= 1, each axis with its own ratio; h, w <= 16384,
 * H, W <= 32768, B <= 65535.  The operator is F.interpolate(size=(H, W), mode="bicubic", align_corners=False): A = -0.75,
 * half-pixel centres, indices clamped to the raster.  The phase is exact: the source coordinate of output d along an axis n -> N
 * is ((2d + 1) n - N) / (2N); its floor and its remainder are integers, and the fraction t is the one fp32 rounding of
 * remainder / (2N) (both below 2^24).  Only the four weights (Horner forms of the two cubic pieces, fused multiply-adds) and the
 * two sums of four terms (taps in increasing order, fused multiply-adds; along x first, then along y) are floating point.  With
 * N == n the fraction is 0, the weights are 0, 1, 0, 0 exactly and the axis is a bit-exact copy of finite values. */
SIFSR_API int sifsrr_upsample(const float* x, float* out, int B, int h, int w, int H, int W, void* stream);

/* ---- prepare --------------------------------------------------------------------------------------------------------------------
 * lst (lst_h, lst_w) [K], ndvi (H, W) -> x (T or cap, 2, hr, hr), T = Ty Tx.  Per tile: z-score of the win x win block, the
 * resampler above to hr x hr CLAMPED AT THE TILE, NDVI optional clip to [-1, 1] and z-score, concatenation -- what a training
 * patch sees.  It is the device function sifsrr_upsample runs: with mean 0 and std 1, plane 0 of tile t is bit-identical to
 * sifsrr_upsample of the block.
 *   active == NULL (then n_active must be NULL too; cap is not read): all T tiles in layout order, every element of x written.
 *   otherwise active / n_active are as sifsrg_tiles_select left them: x[i] is tile active[i] for i < min(n_active[0], cap), later
 *   tiles are untouched (their workgroups exit at once: n_active stays on the device); 1 <= cap, cap > T is allowed.
 * std == 0 and cap < 1: 1001.  Null lst / ndvi / x, or only one of active / n_active: 1002. */
SIFSR_API int sifsrr_tiles_prepare(const float* lst, const float* ndvi, float* x, const int* active, const int* n_active, int cap,
                                   int lst_h, int lst_w, int win, int hr, int overlap, int cover, float mean_lst, float std_lst,
                                   float mean_ndvi, float std_ndvi, int clip_ndvi, void* stream);

/* ---- blend ----------------------------------------------------------------------------------------------------------------------
 * sr (T, 1, hr, hr), or (>= n_active, 1, hr, hr) in the order of `active` when slot is given -> out (H, W), EVERY element written.
 * The feathered gather of sifsr_mosaic.h with tile side hr and R = overlap p / q: the same weight t(.), the same tile order
 * (increasing ty, then tx), no atomics, pixels no tile covers 0.  The covering tiles are found per output pixel
 * in integers: tile k of an axis covers HR pixel Y iff o_k p <= Y q < (o_k + win) p.  (The x4 kernel's group of four pixels does
 * not exist here: at win 16, hr 40, overlap 2 the HR stride is 35.)
 *   slot == NULL (then valid must be NULL too): all tiles, no mask.
 *   otherwise slot (T) and valid (lst_h, lst_w) are as sifsrg_tiles_select / sifsrg_fill left them: an output pixel (Y, X) whose
 *   LST cell (floor(Y q / p), floor(X q / p)) is invalid holds the bits of fill_value and reads no prediction; tiles with
 *   slot < 0 are skipped, tile k is read at sr[slot[k]].
 * Null sr / out, or only one of slot / valid: 1002. */
SIFSR_API int sifsrr_tiles_blend(const float* sr, const int* slot, const unsigned char* valid, float* out, int lst_h, int lst_w,
                                 int win, int hr, int overlap, int cover, float mean_lst, float std_lst, float fill_value,
                                 void* stream);

#endif /* SIFSR_RATIO_H */
