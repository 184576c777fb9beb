/* sifsr_mosaic.h -- extension of the C ABI of libsifsr_hip.so (include/sifsr_hip.h): seamless whole-granule prediction.
 *
 * The block loop of predict.py:84-103 cuts non-overlapping win x win LST windows and skips ragged edge tiles: the last
 * n mod win rows / columns of a granule stay 0, and neighbouring tiles -- each predicted on its own by a network with
 * replicate padding -- disagree at their borders.  The entry points below lay tiles at a stride smaller than the window,
 * push the last tile of each axis flush to the raster edge, and merge the predictions with a normalised feathered blend.
 * No reference counterpart; with overlap = 0 and cover = 0 the layout is the reference's.
 *
 * Conventions are those of sifsr_hip.h: every `float*` is a DEVICE pointer (fp32, dense), `stream` a hipStream_t passed as
 * void*; functions only enqueue work on `stream` and return 0, a SIFSR_ERR_* code (1001 shape, 1002 argument) or the
 * hipError_t of a failed launch.  The symbols carry the prefix `sifsrx_`, live in the same library, and have their own
 * declaration / export / memory-contract gate (tests/test_mosaic_host.py, tests/test_mosaic_gpu.py); sifsr_abi_version()
 * is unchanged.
 *
 * Tile layout, per axis: n = raster length in LST pixels, win = window (<= 64), overlap v with 0 <= v <= win/2, stride
 * s = win - v.
 *   cover = 0: origins k*s for every k with k*s + win <= n
 *   cover = 1: the same, plus a last tile at n - win when the regular tiles do not already end at n
 * Origins are strictly increasing; a raster (lst_h, lst_w) has Ty x Tx tiles, tile t = ty*Tx + tx at (origin_y(ty),
 * origin_x(tx)).  n < win, win > 64 (win < 1), overlap < 0 and 2*overlap > win are errors.
 */
#ifndef SIFSR_MOSAIC_H
#define SIFSR_MOSAIC_H
#include <stddef.h>

#ifndef SIFSR_API
#ifdef __cplusplus
#define SIFSR_API extern "C" __attribute__((visibility("default")))
#else
#define SIFSR_API
#endif
#endif

/* ---- the layout (host only, no GPU touched) ---------------------------------------------------
 * sifsrx_tile_count: tiles along one axis, 0 for invalid arguments.
 * sifsrx_tile_origin: origin (LST pixels) of tile k, -1 for invalid arguments or k outside [0, count). */
SIFSR_API int sifsrx_tile_count(int n, int win, int overlap, int cover);
SIFSR_API int sifsrx_tile_origin(int k, int n, int win, int overlap, int cover);

/* sifsr_tiles_prepare (granule form) for the layout above: lst (lst_h, lst_w), ndvi (4 lst_h, 4 lst_w) ->
 * x (Ty*Tx, 2, 4win, 4win), every element written.  Per tile the arithmetic is that of sifsr_tiles_prepare -- the two kernels
 * run one device function: z-score of the win x win block, bicubic x4 edge-clamped AT THE TILE (A = -0.75), NDVI optional clip
 * + z-score, concatenation -- so tile t is bit-identical to what sifsr_tiles_prepare gives for the same block.
 * win % 4 == 0, 4 <= win <= 64, std != 0; otherwise SIFSR_ERR_SHAPE (null pointers: SIFSR_ERR_ARG). */
SIFSR_API int sifsrx_tiles_prepare(const float* lst, const float* ndvi, float* x, int lst_h, int lst_w, int win, int overlap,
                                   int cover, float mean_lst, float std_lst, float mean_ndvi, float std_ndvi, int clip_ndvi,
                                   void* stream);

/* The merge: sr (Ty*Tx, 1, 4win, 4win) normalised predictions -> out (4 lst_h, 4 lst_w), EVERY element written.
 * Gather form: one thread owns 4 consecutive output pixels (one 16-byte store), finds the at most 3 x 3 tiles that cover them
 * arithmetically from the layout (two regular neighbours and the flush tile per axis) and reads 16 bytes of each: no atomics,
 * no scratch, a fixed summation order -- results are deterministic and bit-reproducible.
 * Weight, separable: with W = 4 win, R = 4 overlap and q in [0, W) the pixel's coordinate inside a tile,
 *   t(q) = 1 when R == 0, else t(q) = min(1, (q + 0.5) / R, (W - q - 0.5) / R)
 *   out = (sum_tiles t(qy) t(qx) sr) / (sum_tiles t(qy) t(qx)) * std_lst + mean_lst   where at least one tile covers the pixel,
 *   out = 0 elsewhere (the reference's np.zeros; reachable only with cover = 0).
 * Between two regular neighbours the weights sum to 1 exactly; the normalisation matters at the raster borders (one tile,
 * t < 1) and where the flush tile overlaps its neighbour by more than `overlap`.  With overlap = 0 the flush overlap is a
 * plain average, and with overlap = 0, cover = 0 the call equals sifsr_tiles_paste onto a zeroed raster.
 * win % 4 == 0, 4 <= win <= 64; otherwise SIFSR_ERR_SHAPE (null pointers: SIFSR_ERR_ARG). */
SIFSR_API int sifsrx_tiles_blend(const float* sr, float* out, int lst_h, int lst_w, int win, int overlap, int cover,
                                 float mean_lst, float std_lst, void* stream);

#endif /* SIFSR_MOSAIC_H */
