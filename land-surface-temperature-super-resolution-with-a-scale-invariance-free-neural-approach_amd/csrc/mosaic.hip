// Seamless whole-granule prediction (C ABI: include/sifsr_mosaic.h): the input pipeline for tiles laid at a
// stride smaller than the window with the last tile of each axis flush to the raster edge (layout: mosaic.h), and the merge of
// the per-tile predictions by a normalised feathered blend.
//
//  * mosaic_prepare_kernel: tiles_prepare_kernel (pipeline.hip) with the tile's position taken from the layout; the per-tile
//    body is the same device function, so a tile's network input does not depend on which of the two cut it.
//  * mosaic_blend_kernel: a GATHER.  Each output pixel is covered by at most 3 x 3 tiles whose indices follow from two integer
//    divisions per axis, so one thread sums its own pixels in a fixed order: no atomics, no accumulation raster and weight raster
//    to zero, fill and divide (three more passes over the output), and bit-reproducible results.  Bandwidth-bound: every
//    prediction element is read once per pixel it contributes to (16-byte loads, contiguous along x inside a tile), every
//    output element is written once (one 16-byte store per thread, 1 KiB per wave).
#include "../../include/sifsr_mosaic.h"

#include "mosaic.h"

namespace {

struct MosaicGeom {
  MosaicAxis ay, ax;
  int lst_w;   // raster row stride (LST pixels)
};

__global__ __launch_bounds__(256) void mosaic_prepare_kernel(const float* __restrict__ lst, const float* __restrict__ ndvi,
                                                             float* __restrict__ x, const MosaicGeom gm, int win,
                                                             float mean_lst, float istd_lst, float mean_ndvi,
                                                             float istd_ndvi, int clip_ndvi) {
  __shared__ float src[8][64 + 1];
  const int hr = 4 * win;
  const int t = blockIdx.x;
  const int ty = t / gm.ax.count, tx = t - ty * gm.ax.count;
  const int oy = mosaic_origin(gm.ay, ty), ox = mosaic_origin(gm.ax, tx);
  tile_prepare_rows(lst + (size_t)oy * gm.lst_w + ox, ndvi + (size_t)(4 * oy) * (4 * gm.lst_w) + 4 * ox, gm.lst_w, 4 * gm.lst_w,
                    x + ((size_t)t * 2 + 0) * hr * hr, x + ((size_t)t * 2 + 1) * hr * hr, src, win, blockIdx.y * 16, mean_lst,
                    istd_lst, mean_ndvi, istd_ndvi, clip_ndvi);
}

// t(q) of the header: the feather of a tile at local coordinate q in [0, W); R = 0: no feather
__device__ __forceinline__ float feather(int q, int W, float R) {
  if (R == 0.f) return 1.f;
  return fminf(1.f, fminf(((float)q + 0.5f) / R, ((float)(W - q) - 0.5f) / R));
}

// block = 64 x 4 threads: thread (i, j) owns output pixels [4*(64*blockIdx.x + i), +4) of row 4*blockIdx.y + j
__global__ __launch_bounds__(256) void mosaic_blend_kernel(const float* __restrict__ sr, float* __restrict__ out,
                                                           const MosaicGeom gm, float R, float mean, float std) {
  const int W = 4 * gm.ax.w;                    // tile side in output pixels
  const int out_w = 4 * gm.lst_w, out_h = 4 * gm.ay.n;
  const int X = 4 * (blockIdx.x * 64 + threadIdx.x), Y = blockIdx.y * 4 + threadIdx.y;
  if (X >= out_w || Y >= out_h) return;
  const MosaicCover cy = mosaic_cover(gm.ay, Y >> 2), cx = mosaic_cover(gm.ax, X >> 2);
  float4 num = make_float4(0.f, 0.f, 0.f, 0.f), den = num;
  for (int a = 0; a < cy.n; ++a) {
    const int ky = mosaic_cover_index(cy, a);
    const int qy = Y - 4 * mosaic_origin(gm.ay, ky);
    const float wy = feather(qy, W, R);
    for (int b = 0; b < cx.n; ++b) {
      const int kx = mosaic_cover_index(cx, b);
      const int qx = X - 4 * mosaic_origin(gm.ax, kx);         // a multiple of 4: the 4 pixels lie in the same tiles
      const float4 v = ld4(sr + ((size_t)(ky * gm.ax.count + kx) * W + qy) * W + qx);
      const float w0 = wy * feather(qx, W, R), w1 = wy * feather(qx + 1, W, R);
      const float w2 = wy * feather(qx + 2, W, R), w3 = wy * feather(qx + 3, W, R);
      num.x += w0 * v.x; num.y += w1 * v.y; num.z += w2 * v.z; num.w += w3 * v.w;
      den.x += w0; den.y += w1; den.z += w2; den.w += w3;
    }
  }
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);   // uncovered (cover = 0 only): the reference's np.zeros
  if (cy.n > 0 && cx.n > 0) {
    o.x = num.x / den.x * std + mean; o.y = num.y / den.y * std + mean;
    o.z = num.z / den.z * std + mean; o.w = num.w / den.w * std + mean;
  }
  st4(out + (size_t)Y * out_w + X, o);
}

// the shape rules the two launches share; false: SIFSR_ERR_SHAPE
bool mosaic_geom(int lst_h, int lst_w, int win, int overlap, int cover, MosaicGeom* gm) {
  if (win < 4 || win > 64 || win % 4) return false;
  gm->ay = mosaic_axis(lst_h, win, overlap, cover);
  gm->ax = mosaic_axis(lst_w, win, overlap, cover);
  gm->lst_w = lst_w;
  if (gm->ay.count < 1 || gm->ax.count < 1) return false;
  // tile counts and pixel offsets stay inside int / the grid limits (a raster of 16384^2 LST pixels is far above any granule)
  return lst_h <= 16384 && lst_w <= 16384;
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
