// Whole-granule prediction at any ratio (C ABI: include/sifsr_ratio.h): the bicubic resampler with an exact
// phase, the input pipeline of the tiles of a granule at ratio hr / win, and the merge of their predictions.
//
//  * ratio_upsample_kernel  (B, h, w) -> (B, H, W): one workgroup = 16 x 256 outputs of one image (ratio_resample_block of
//    ratio.h).  Bandwidth-bound: every source element a workgroup needs is read once into LDS, every output is written once,
//    256 consecutive floats per row.
//  * ratio_prepare_kernel   the same device function per tile, clamped at the tile, with the z-score applied while staging, and
//    the NDVI plane (clip, z-score) written beside it; over all tiles or over the compact list sifsrg_tiles_select left
//    (workgroups past n_active exit at once).
//  * ratio_blend_kernel     the feathered gather of mosaic.h one pixel at a time (a thread walks 8 rows of one column): the covering
//    tiles follow from mosaic_cover on the axes restated in HR pixels, so there is no group of pixels that must share their
//    tiles; with slot / valid the tile is looked up through `slot` and a pixel of an invalid LST cell reads nothing.  No atomics,
//    a fixed order, every element written.
#include "../../include/sifsr_ratio.h"

#include "ratio.h"

namespace {

__global__ __launch_bounds__(256) void ratio_upsample_kernel(const float* __restrict__ x, float* __restrict__ out, int h, int w,
                                                             int H, int W) {
  __shared__ float src[RATIO_SRC_ROWS][RATIO_SRC_COLS];
  const float* xi = x + (size_t)blockIdx.z * h * w;
  float* oi = out + (size_t)blockIdx.z * H * W;
  ratio_resample_block(xi, (size_t)w, h, w, H, W, blockIdx.y * RATIO_ROWS, blockIdx.x * RATIO_COLS, 0.f, 1.f, src,
                       [oi, W](int, int Y, int X, float v) { oi[(size_t)Y * W + X] = v; });
}

// grid = (T or cap, ceil(hr / 16)); hr <= 256: one workgroup spans the tile's width
__global__ __launch_bounds__(256) void ratio_prepare_kernel(const float* __restrict__ lst, const float* __restrict__ ndvi,
                                                            float* __restrict__ x, const int* __restrict__ active,
                                                            const int* __restrict__ n_active, const RatioGeom g, float mean_lst,
                                                            float istd_lst, float mean_ndvi, float istd_ndvi, int clip_ndvi) {
  __shared__ float src[RATIO_SRC_ROWS][RATIO_SRC_COLS];
  int t = blockIdx.x;
  if (active != nullptr) {
    if ((int)blockIdx.x >= *n_active) return;                            // (uniform over the workgroup)
    t = active[blockIdx.x];
    if (t < 0 || t >= g.ay.count * g.ax.count) return;                   // never written by sifsrg_tiles_select
  }
  const int hr = g.hr, win = g.ax.w;
  const int ty = t / g.ax.count, tx = t - ty * g.ax.count;
  const int oy = mosaic_origin(g.ay, ty), ox = mosaic_origin(g.ax, tx);
  const float* nt = ndvi + (size_t)(oy / g.q * g.p) * g.W + ox / g.q * g.p;
  const size_t ndvi_row = (size_t)g.W;
  float* o0 = x + (size_t)blockIdx.x * 2 * hr * hr;
  float* o1 = o0 + (size_t)hr * hr;
  const int Y0 = blockIdx.y * RATIO_ROWS;
  // the thread's 16 NDVI values first: their loads are in flight while the LST block is staged
  float nv[RATIO_ROWS];
#pragma unroll
  for (int dy = 0; dy < RATIO_ROWS; ++dy)
    nv[dy] = ((int)threadIdx.x < hr && Y0 + dy < hr) ? nt[(size_t)(Y0 + dy) * ndvi_row + threadIdx.x] : 0.f;
  ratio_resample_block(lst + (size_t)oy * g.lst_w + ox, (size_t)g.lst_w, win, win, hr, hr, Y0, 0, mean_lst, istd_lst, src,
                       [&](int dy, int Y, int X, float v) {
                         o0[(size_t)Y * hr + X] = v;
                         float n = nv[dy];
                         if (clip_ndvi) n = fminf(fmaxf(n, -1.f), 1.f);
                         o1[(size_t)Y * hr + X] = (n - mean_ndvi) * istd_ndvi;
                       });
}

// block = 256 threads along x, 8 rows each: thread i owns column 256 blockIdx.y + i of rows [8 blockIdx.x, + 8).  What depends on
// the column alone (its covering tiles, their weights, its LST cell) is found once per thread; what depends on the row alone is
// uniform over the workgroup.
constexpr int BLEND_ROWS = 8;
__global__ __launch_bounds__(256) void ratio_blend_kernel(const float* __restrict__ sr, const int* __restrict__ slot,
                                                          const unsigned char* __restrict__ valid, float* __restrict__ out,
                                                          const RatioGeom g, float R, float mean, float std, float fill_value) {
  const int X = blockIdx.y * 256 + threadIdx.x;
  if (X >= g.W) return;
  const int hr = g.hr;
  const MosaicAxis ay = ratio_hr_axis(g.ay, g.p, g.q, hr), ax = ratio_hr_axis(g.ax, g.p, g.q, hr);
  const MosaicCover cx = mosaic_cover(ax, X);
  int kx[3], qx[3];
  float wx[3];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    kx[b] = b < cx.n ? mosaic_cover_index(cx, b) : 0;
    qx[b] = X - mosaic_origin(ax, kx[b]);
    wx[b] = feather(qx[b], hr, R);
  }
  const int cell_x = X * g.q / g.p;
  const int Yend = min((int)(blockIdx.x + 1) * BLEND_ROWS, g.H);
  for (int Y = blockIdx.x * BLEND_ROWS; Y < Yend; ++Y) {
    float o = fill_value;
    if (valid == nullptr || valid[(size_t)(Y * g.q / g.p) * g.lst_w + cell_x] != 0) {
      const MosaicCover cy = mosaic_cover(ay, Y);
      float num = 0.f, den = 0.f;
      for (int a = 0; a < cy.n; ++a) {
        const int ky = mosaic_cover_index(cy, a);
        const int qy = Y - mosaic_origin(ay, ky);
        const float wy = feather(qy, hr, R);
#pragma unroll
        for (int b = 0; b < 3; ++b) {
          if (b >= cx.n) break;
          int k = ky * ax.count + kx[b];
          if (slot != nullptr) k = slot[k];
          if (k < 0) continue;
          const float wgt = wy * wx[b];
          num += wgt * sr[((size_t)k * hr + qy) * hr + qx[b]];
          den += wgt;
        }
      }
      o = (cy.n > 0 && cx.n > 0) ? num / den * std + mean : 0.f;
    }
    out[(size_t)Y * g.W + X] = o;
  }
}

}  // namespace

// ---- C ABI (include/sifsr_ratio.h) ----
int sifsrr_geometry(int lst_h, int lst_w, int win, int hr, int overlap, int cover, int* out6) {
  if (!out6) return SIFSR_ERR_ARG;
  RatioGeom g;
  if (!ratio_geom(lst_h, lst_w, win, hr, overlap, cover, &g)) return SIFSR_ERR_SHAPE;
  out6[0] = g.p; out6[1] = g.q; out6[2] = g.ay.count; out6[3] = g.ax.count; out6[4] = g.H; out6[5] = g.W;
  return SIFSR_OK;
}

int sifsrr_upsample(const float* x, float* out, int B, int h, int w, int H, int W, void* stream) {
  if (!x || !out) return SIFSR_ERR_ARG;
  if (B < 1 || B > 65535 || h < 1 || w < 1 || h > 16384 || w > 16384 || H < h || W < w || H > 32768 || W > 32768) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(ratio_upsample_kernel, dim3((W + RATIO_COLS - 1) / RATIO_COLS, (H + RATIO_ROWS - 1) / RATIO_ROWS, B), dim3(256),
                     0, (hipStream_t)stream, x, out, h, w, H, W);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrr_tiles_prepare(const float* lst, const float* ndvi, float* x, const int* active, const int* n_active, int cap, int lst_h,
                         int lst_w, int win, int hr, int overlap, int cover, float mean_lst, float std_lst, float mean_ndvi,
                         float std_ndvi, int clip_ndvi, void* stream) {
  if (!lst || !ndvi || !x || (active == nullptr) != (n_active == nullptr)) return SIFSR_ERR_ARG;
  RatioGeom g;
  if (!ratio_geom(lst_h, lst_w, win, hr, overlap, cover, &g) || std_lst == 0.f || std_ndvi == 0.f) return SIFSR_ERR_SHAPE;
  if (active && cap < 1) return SIFSR_ERR_SHAPE;
  const int n = active ? cap : g.ay.count * g.ax.count;
  hipLaunchKernelGGL(ratio_prepare_kernel, dim3(n, (hr + RATIO_ROWS - 1) / RATIO_ROWS), dim3(256), 0, (hipStream_t)stream, lst, ndvi,
                     x, active, n_active, g, mean_lst, 1.f / std_lst, mean_ndvi, 1.f / std_ndvi, clip_ndvi);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrr_tiles_blend(const float* sr, const int* slot, const unsigned char* valid, float* out, int lst_h, int lst_w, int win,
                       int hr, int overlap, int cover, float mean_lst, float std_lst, float fill_value, void* stream) {
  if (!sr || !out || (slot == nullptr) != (valid == nullptr)) return SIFSR_ERR_ARG;
  RatioGeom g;
  if (!ratio_geom(lst_h, lst_w, win, hr, overlap, cover, &g)) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(ratio_blend_kernel, dim3((g.H + BLEND_ROWS - 1) / BLEND_ROWS, (g.W + 255) / 256), dim3(256), 0, (hipStream_t)stream, sr, slot, valid,
                     out, g, (float)(overlap / g.q * g.p), mean_lst, std_lst, fill_value);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}
