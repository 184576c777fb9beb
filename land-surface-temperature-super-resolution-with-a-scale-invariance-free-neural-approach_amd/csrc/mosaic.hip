// Seamless whole-granule prediction (C ABI: include/sifsr_mosaic.h): the input pipeline for tiles laid at a
// stride smaller than the window with the last tile of each axis flush to the raster edge (layout: mosaic.h), and the merge of
// the per-tile predictions by a normalised feathered blend.
//
//  * mosaic_prepare_kernel: tiles_prepare_kernel (pipeline.hip) with the tile's position taken from the layout; the per-tile
//    body is the same device function, so a tile's network input does not depend on which of the two cut it.
//  * mosaic_blend_kernel: a GATHER (body: mosaic_blend4 of mosaic.h, shared with the gap-aware blend of gaps.hip).  Each output pixel is covered by at most 3 x 3 tiles whose indices follow from two integer
//    divisions per axis, so one thread sums its own pixels in a fixed order: no atomics, no accumulation raster and weight raster
//    to zero, fill and divide (three more passes over the output), and bit-reproducible results.  Bandwidth-bound: every
//    prediction element is read once per pixel it contributes to (16-byte loads, contiguous along x inside a tile), every
//    output element is written once (one 16-byte store per thread, 1 KiB per wave).
#include "../../include/sifsr_mosaic.h"

#include "mosaic.h"

namespace {

__global__ __launch_bounds__(256) void mosaic_prepare_kernel(const float* __restrict__ lst, const float* __restrict__ ndvi,
                                                             float* __restrict__ x, const MosaicGeom gm, int win,
                                                             float mean_lst, float istd_lst, float mean_ndvi,
                                                             float istd_ndvi, int clip_ndvi) {
  __shared__ float src[8][64 + 1];
  mosaic_prepare_tile(lst, ndvi, x + (size_t)blockIdx.x * 2 * (4 * win) * (4 * win), gm, blockIdx.x, src, win, blockIdx.y * 16,
                      mean_lst, istd_lst, mean_ndvi, istd_ndvi, clip_ndvi);
}

// block = 64 x 4 threads: thread (i, j) owns output pixels [4*(64*blockIdx.x + i), +4) of row 4*blockIdx.y + j
__global__ __launch_bounds__(256) void mosaic_blend_kernel(const float* __restrict__ sr, float* __restrict__ out,
                                                           const MosaicGeom gm, float R, float mean, float std) {
  const int out_w = 4 * gm.lst_w, out_h = 4 * gm.ay.n;
  const int X = 4 * (blockIdx.x * 64 + threadIdx.x), Y = blockIdx.y * 4 + threadIdx.y;
  if (X >= out_w || Y >= out_h) return;
  st4(out + (size_t)Y * out_w + X, mosaic_blend4(sr, gm, R, mean, std, X, Y, [](int k) { return k; }));
}

}  // namespace

int launch_mosaic_prepare(const float* lst, const float* ndvi, float* x, int lst_h, int lst_w, int win, int overlap, int cover,
                          float mean_lst, float std_lst, float mean_ndvi, float std_ndvi, int clip_ndvi, hipStream_t s) {
  MosaicGeom gm;
  if (!mosaic_geom(lst_h, lst_w, win, overlap, cover, &gm) || std_lst == 0.f || std_ndvi == 0.f) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(mosaic_prepare_kernel, dim3(gm.ay.count * gm.ax.count, (4 * win) / 16), dim3(256), 0, s, lst, ndvi, x, gm,
                     win, mean_lst, 1.f / std_lst, mean_ndvi, 1.f / std_ndvi, clip_ndvi);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int launch_mosaic_blend(const float* sr, float* out, int lst_h, int lst_w, int win, int overlap, int cover, float mean_lst,
                        float std_lst, hipStream_t s) {
  MosaicGeom gm;
  if (!mosaic_geom(lst_h, lst_w, win, overlap, cover, &gm)) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(mosaic_blend_kernel, dim3((lst_w + 63) / 64, lst_h), dim3(64, 4), 0, s, sr, out, gm, (float)(4 * overlap),
                     mean_lst, std_lst);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

// ---- C ABI (include/sifsr_mosaic.h) ----
int sifsrx_tile_count(int n, int win, int overlap, int cover) { return mosaic_axis(n, win, overlap, cover).count; }
int sifsrx_tile_origin(int k, int n, int win, int overlap, int cover) {
  return mosaic_origin(mosaic_axis(n, win, overlap, cover), k);
}
int sifsrx_tiles_prepare(const float* lst, const float* ndvi, float* x, int lst_h, int lst_w, int win, int overlap, int cover,
                         float mean_lst, float std_lst, float mean_ndvi, float std_ndvi, int clip_ndvi, void* stream) {
  if (!lst || !ndvi || !x) return SIFSR_ERR_ARG;
  return launch_mosaic_prepare(lst, ndvi, x, lst_h, lst_w, win, overlap, cover, mean_lst, std_lst, mean_ndvi, std_ndvi,
                               clip_ndvi, (hipStream_t)stream);
}
int sifsrx_tiles_blend(const float* sr, float* out, int lst_h, int lst_w, int win, int overlap, int cover, float mean_lst,
                       float std_lst, void* stream) {
  if (!sr || !out) return SIFSR_ERR_ARG;
  return launch_mosaic_blend(sr, out, lst_h, lst_w, win, overlap, cover, mean_lst, std_lst, (hipStream_t)stream);
}
