/* sifsr_gaps.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): gap-aware whole-granule prediction.
 *
 * Every real MOD11A1 / MOD21A1D granule has holes: cloud, ocean and fill pixels arrive as raw 0 = 0.0 K (process_modis.py:96,
 * :180 and predict.py:92 treat them as bad).  Fed to the per-tile z-score and the bicubic x4 of sifsr_mosaic.h as they are, a
 * 0 K pixel is about -55 sigma and spoils valid land tens of pixels around every gap; tiles that are all cloud or sea cost a
 * forward each; and the output does not say which pixels are predictions.  The entry points below
 *   fill     mark the valid pixels and give the invalid ones a neutral local mean (the network sees a raster without holes),
 *   select   keep the tiles of the layout of sifsr_mosaic.h that hold at least one valid pixel, in order,
 *   prepare  cut the network input of those tiles only, compact,
 *   blend    merge their predictions as sifsrx_tiles_blend does and write `fill_value` where the LST pixel is invalid.
 * No reference counterpart (predict.py predicts every block and writes whatever comes out).
 *
 * Conventions are those of sifsr_mosaic.h: every pointer is a DEVICE pointer (dense, row-major; `float` fp32, `unsigned char`
 * one byte per pixel, `int` 32 bit), `stream` a hipStream_t passed as void*; functions only enqueue work on `stream` and return
 * 0, 1001 for a shape error, 1002 for an argument error, 1003 for a workspace that is too small, or the hipError_t of a failed
 * launch.  Nothing is launched when an error is returned.  The symbols carry the prefix `sifsrg_`, live in the same library and
 * have their own declaration / export / memory-contract gate (tests/test_gaps_host.py, tests/test_gaps_gpu.py);
 * sifsr_abi_version() is unchanged.
 *
 * Tile layout, `win`, `overlap`, `cover` and the tile numbering t = ty*Tx + tx are those of sifsr_mosaic.h (csrc/mosaic.h is
 * the one definition); T = Ty*Tx.  win % 4 == 0, 4 <= win <= 64, a raster of at most 16384 x 16384 LST pixels.
 */
#ifndef SIFSR_GAPS_H
#define SIFSR_GAPS_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

/* ---- fill ------------------------------------------------------------------------------------------------------------------
 * lst (lst_h, lst_w) [K], mask (lst_h, lst_w) or NULL -> filled (lst_h, lst_w), valid (lst_h, lst_w); EVERY element of both
 * outputs is written.  1 <= lst_h, lst_w <= 16384.
 *
 * Validity:  valid[p] = isfinite(lst[p]) && lst[p] != 0 && (mask == NULL || mask[p] != 0), stored as 0 or 1.
 *
 * Fill: a push-pull pyramid.  Level 0 is the raster; level l + 1 has ceil(n_l / 2) cells per axis, down to 1 x 1 (a 1 x 1 raster
 * has one level above it).  A cell holds the float64 sum S and the integer count c of the VALID level-0 pixels under it;
 * children past the ragged edge contribute nothing.  Push, from the top:
 *   F_l(i, j) = (float)(S_l(i, j) / c_l(i, j))  if c_l(i, j) > 0,  else  F_{l+1}(i >> 1, j >> 1)
 *   filled[p] = lst[p] if valid[p], else F_1 of its parent.
 * In closed form: an invalid pixel gets the mean of the valid pixels of the smallest aligned dyadic block around it that holds
 * one -- a float64 sum, one float64 division, one rounding to fp32.  No valid pixel anywhere: filled is 0 everywhere.
 *
 * Bit-defined: a float64 sum of fp32 values is exact as long as it fits 53 bits.  Temperatures in [128, 512) K are multiples of
 * 2^-16 below 2^9, so the sum over any raster this call accepts (at most 2^28 pixels) is a multiple of 2^-16 below 2^37: 53
 * bits.  The order in which a kernel adds therefore does not matter, and the result is the same on every run and in every
 * restatement.  (For other values the sums may round; the order is fixed all the same: there are no atomics and nothing depends
 * on the order of workgroups.)
 *
 * The blocky interior of a large gap is never reported (sifsrg_tiles_blend masks it); only the network's receptive field at the
 * rim of a gap sees the fill, and there a local mean is the neutral value.
 *
 * workspace: scratch for the pyramid, at least sifsrg_fill_workspace_bytes(lst_h, lst_w) bytes, 8-byte aligned (else
 * SIFSR_ERR_ARG); its contents before the call do not matter and are unspecified after it.  A smaller `workspace_bytes`:
 * 1003.  Null lst / filled / valid / workspace: 1002.
 * sifsrg_fill_workspace_bytes is host only and returns 0 for an invalid shape. */
SIFSR_API size_t sifsrg_fill_workspace_bytes(int lst_h, int lst_w);
SIFSR_API int sifsrg_fill(const float* lst, const unsigned char* mask, float* filled, unsigned char* valid, void* workspace,
                          size_t workspace_bytes, int lst_h, int lst_w, void* stream);

/* ---- select ----------------------------------------------------------------------------------------------------------------
 * valid (lst_h, lst_w), any non-zero byte = valid.  A tile is ACTIVE iff its win x win window holds at least one valid pixel.
 *   active[0 .. n)   the active tile numbers in increasing order; entries from n on are untouched (active holds T ints)
 *   slot[t]          the position of tile t in `active`, or -1; all T entries written
 *   n_active[0]      n
 * One wavefront orders the tiles by ballot + prefix population count (as sifsrp_select does): no scan pass, no atomics.
 * Consequence: every tile that covers a valid pixel is active, so sifsrg_tiles_blend forms a valid pixel from exactly the tiles
 * sifsrx_tiles_blend would use. */
SIFSR_API int sifsrg_tiles_select(const unsigned char* valid, int* slot, int* active, int* n_active, int lst_h, int lst_w, int win,
                                  int overlap, int cover, void* stream);

/* ---- compact prepare -------------------------------------------------------------------------------------------------------
 * filled (lst_h, lst_w), ndvi (4 lst_h, 4 lst_w), active / n_active as sifsrg_tiles_select left them -> x (cap, 2, 4win, 4win).
 * For i < min(n_active[0], cap): x[i] is the network input of tile active[i], by the device function sifsrx_tiles_prepare runs
 * -- bit-identical to tile active[i] of sifsrx_tiles_prepare(filled, ndvi, ...).  Tiles from n_active[0] on are untouched (their
 * workgroups exit at once: n_active stays on the device).  NDVI is not sanitised: with clip_ndvi a NaN becomes -1 through
 * fmaxf / fminf, as in sifsrx_tiles_prepare.  1 <= cap (cap > T is allowed), std != 0; otherwise SIFSR_ERR_SHAPE. */
SIFSR_API int sifsrg_tiles_prepare(const float* filled, const float* ndvi, float* x, const int* active, const int* n_active, int cap,
                                   int lst_h, int lst_w, int win, int overlap, int cover, float mean_lst, float std_lst,
                                   float mean_ndvi, float std_ndvi, int clip_ndvi, void* stream);

/* ---- masked blend ----------------------------------------------------------------------------------------------------------
 * sr (>= n_active, 1, 4win, 4win) normalised predictions in the order of `active`, slot (T), valid (lst_h, lst_w) ->
 * out (4 lst_h, 4 lst_w), EVERY element written.  Per output pixel, with P its LST pixel:
 *   valid[P] == 0                      out = fill_value (the bits of the argument; NaN is a fine choice)
 *   else no tile covers the pixel      out = 0 (cover = 0 only), as in sifsrx_tiles_blend
 *   else                               the feathered gather of sifsrx_tiles_blend -- the same device function, the same tile
 *                                      order and arithmetic -- reading tile k at sr[slot[k]] and skipping tiles with slot < 0.
 * Every tile covering a valid pixel is active, so at valid pixels the result is bit-identical to sifsrx_tiles_blend on the full
 * tile set.  One thread owns the 4 output pixels of one row of an LST pixel: one byte of `valid`, 16-byte loads, one 16-byte
 * store; an invalid pixel reads no prediction. */
SIFSR_API int sifsrg_tiles_blend(const float* sr, const int* slot, const unsigned char* valid, float* out, int lst_h, int lst_w,
                                 int win, int overlap, int cover, float mean_lst, float std_lst, float fill_value, void* stream);

#endif /* SIFSR_GAPS_H */
