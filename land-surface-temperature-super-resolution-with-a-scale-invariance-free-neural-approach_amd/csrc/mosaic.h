// Whole-granule mosaics: the ONE definition of the overlapped tile layout, shared by the host entry points,
// the kernels of mosaic.hip and (restated) pipeline.tile_origins, and the per-tile device body of the input pipeline that both
// tiles_prepare_kernel (pipeline.hip), mosaic_prepare_kernel (mosaic.hip) and gaps_prepare_kernel (gaps.hip) run; the feathered
// gather of the blend, shared by mosaic.hip and gaps.hip.
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------------
// Tile layout along one axis.  n = raster length in LST pixels, w = window, v = overlap (0 <= v <= w/2), stride s = w - v.
//   cover = 0: origins k*s for every k with k*s + w <= n                       (v = 0: the tiles of predict.py:84-95)
//   cover = 1: the same, plus one last tile at n - w when the regular tiles do not already end at n
// Origins are strictly increasing.  Invalid arguments (n < w, w < 1, w > 64, v < 0, 2v > w): count 0, origin -1.
// ---------------------------------------------------------------------------------------------
struct MosaicAxis {
  int n, w, s;   // raster length, window, stride (LST pixels)
  int reg;       // regular tiles (origins k*s)
  int count;     // reg + 1 when a flush tile at n - w follows them
};

__host__ __device__ inline MosaicAxis mosaic_axis(int n, int w, int v, int cover) {
  MosaicAxis a{n, w, 0, 0, 0};
  if (w < 1 || w > 64 || n < w || v < 0 || 2 * v > w) return a;
  a.s = w - v;
  a.reg = (n - w) / a.s + 1;
  a.count = a.reg + ((cover && (a.reg - 1) * a.s + w < n) ? 1 : 0);
  return a;
}

__host__ __device__ inline int mosaic_origin(const MosaicAxis& a, int k) {
  if (k < 0 || k >= a.count) return -1;
  return k < a.reg ? k * a.s : a.n - a.w;
}

// The tiles that cover LST pixel P (0 <= P < n): at most two regular ones (s >= w/2), indices lo .. lo + nreg - 1, and the
// flush tile (index reg); in increasing order the a-th of the n covering tiles is mosaic_cover_index(a).
struct MosaicCover {
  int lo, nreg, n, flush;
};

__host__ __device__ inline MosaicCover mosaic_cover(const MosaicAxis& a, int P) {
  int lo = P - a.w + 1;
  lo = lo <= 0 ? 0 : (lo + a.s - 1) / a.s;
  int hi = P / a.s;
  if (hi > a.reg - 1) hi = a.reg - 1;
  MosaicCover c;
  c.lo = lo;
  c.nreg = hi >= lo ? hi - lo + 1 : 0;
  c.flush = a.reg;
  c.n = c.nreg + ((a.count > a.reg && P >= a.n - a.w) ? 1 : 0);
  return c;
}

__host__ __device__ inline int mosaic_cover_index(const MosaicCover& c, int i) { return i < c.nreg ? c.lo + i : c.flush; }

// ---------------------------------------------------------------------------------------------
// bicubic x4 (ATen upsample_bicubic2d / OpenCV INTER_CUBIC coefficients, A = -0.75)
// ---------------------------------------------------------------------------------------------
static __device__ __forceinline__ float cc1(float x, float A) { return ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f; }
static __device__ __forceinline__ float cc2(float x, float A) { return ((A * x - 5.f * A) * x + 8.f * A) * x - 4.f * A; }
static __device__ __forceinline__ void cubic_coeffs(float t, float c[4]) {
  const float A = -0.75f;
  c[0] = cc2(t + 1.f, A); c[1] = cc1(t, A); c[2] = cc1(1.f - t, A); c[3] = cc2(2.f - t, A);
}

// One workgroup of 256 threads = 16 output rows (from Y0, a multiple of 16) x (4*win) columns of ONE tile; thread = output column.
// lt / nt: the tile's first LST / NDVI element, lst_row / ndvi_row their row strides (elements); o0 / o1: the tile's two output
// planes (4win x 4win each).  z-score, per-tile edge-clamped bicubic x4, NDVI clip + z-score, concatenation.
static __device__ __forceinline__ void tile_prepare_rows(const float* __restrict__ lt, const float* __restrict__ nt, int lst_row,
                                                         int ndvi_row, float* __restrict__ o0, float* __restrict__ o1,
                                                         float (*src)[64 + 1], int win, int Y0, float mean_lst, float istd_lst,
                                                         float mean_ndvi, float istd_ndvi, int clip_ndvi) {
  const int hr = 4 * win;
  const int X = threadIdx.x;
  const int sy0 = Y0 / 4 - 2;   // first of the 8 source rows the 16 output rows touch
  for (int e = threadIdx.x; e < 8 * win; e += 256) {
    const int r = e / win, cidx = e - r * win;
    const int gy = clampi(sy0 + r, 0, win - 1);
    src[r][cidx] = (lt[(size_t)gy * lst_row + cidx] - mean_lst) * istd_lst;
  }
  __syncthreads();
  if (X < hr) {
    // horizontal pass: source index of output column X (scale 1/4, half-pixel centres)
    const float sx = 0.25f * ((float)X + 0.5f) - 0.5f;
    const float fx = floorf(sx);
    const int ix = (int)fx;
    float cx[4];
    cubic_coeffs(sx - fx, cx);
    int xs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xs[j] = clampi(ix - 1 + j, 0, win - 1);
    float hrow[8];
#pragma unroll
    for (int r = 0; r < 8; ++r)
      hrow[r] = src[r][xs[0]] * cx[0] + src[r][xs[1]] * cx[1] + src[r][xs[2]] * cx[2] + src[r][xs[3]] * cx[3];
#pragma unroll
    for (int dy = 0; dy < 16; ++dy) {
      const int Y = Y0 + dy;
      const float sy = 0.25f * ((float)Y + 0.5f) - 0.5f;
      const float fy = floorf(sy);
      float cy[4];
      cubic_coeffs(sy - fy, cy);
      float v = 0.f;
      // staged row r <-> source row clamp(sy0 + r): the clamp is already applied; Y0 is a multiple of 16, so
      // iy - sy0 depends on dy alone (compile time): iy = Y0/4 + ((dy + 2) >> 2) - 1
      const int rb = ((dy + 2) >> 2) + 0;   // = iy - 1 - sy0
#pragma unroll
      for (int i = 0; i < 4; ++i) v = (i == 0) ? hrow[rb + i] * cy[0] : v + hrow[rb + i] * cy[i];
      o0[(size_t)Y * hr + X] = v;
      float nv = nt[(size_t)Y * ndvi_row + X];
      if (clip_ndvi) nv = fminf(fmaxf(nv, -1.f), 1.f);
      o1[(size_t)Y * hr + X] = (nv - mean_ndvi) * istd_ndvi;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// The raster's layout on both axes, and the shape rules every launch over it shares (mosaic.hip, gaps.hip)
// ---------------------------------------------------------------------------------------------
struct MosaicGeom {
  MosaicAxis ay, ax;
  int lst_w;   // raster row stride (LST pixels)
};

// false: SIFSR_ERR_SHAPE
inline bool mosaic_geom(int lst_h, int lst_w, int win, int overlap, int cover, MosaicGeom* gm) {
  if (win < 4 || win > 64 || win % 4) return false;
  gm->ay = mosaic_axis(lst_h, win, overlap, cover);
  gm->ax = mosaic_axis(lst_w, win, overlap, cover);
  gm->lst_w = lst_w;
  if (gm->ay.count < 1 || gm->ax.count < 1) return false;
  // tile counts and pixel offsets stay inside int / the grid limits (a raster of 16384^2 LST pixels is far above any granule)
  return lst_h <= 16384 && lst_w <= 16384;
}

// Tile t of the layout -> its network input xt (2 planes of 4win x 4win): the rows [Y0, Y0 + 16) of tile_prepare_rows at the
// tile's origin.  What mosaic_prepare_kernel (mosaic.hip) and gaps_prepare_kernel (gaps.hip) run.
static __device__ __forceinline__ void mosaic_prepare_tile(const float* __restrict__ lst, const float* __restrict__ ndvi,
                                                           float* __restrict__ xt, const MosaicGeom& gm, int t,
                                                           float (*src)[64 + 1], int win, int Y0, float mean_lst, float istd_lst,
                                                           float mean_ndvi, float istd_ndvi, int clip_ndvi) {
  const int hr = 4 * win;
  const int ty = t / gm.ax.count, tx = t - ty * gm.ax.count;
  const int oy = mosaic_origin(gm.ay, ty), ox = mosaic_origin(gm.ax, tx);
  tile_prepare_rows(lst + (size_t)oy * gm.lst_w + ox, ndvi + (size_t)(4 * oy) * (4 * gm.lst_w) + 4 * ox, gm.lst_w, 4 * gm.lst_w, xt,
                    xt + (size_t)hr * hr, src, win, Y0, mean_lst, istd_lst, mean_ndvi, istd_ndvi, clip_ndvi);
}

// t(q) of sifsr_mosaic.h: the feather of a tile at local coordinate q in [0, W); R = 0: no feather
static __device__ __forceinline__ float feather(int q, int W, float R) {
  if (R == 0.f) return 1.f;
  return fminf(1.f, fminf(((float)q + 0.5f) / R, ((float)(W - q) - 0.5f) / R));
}

// The feathered gather of the 4 output pixels [X, X + 4) of row Y (X a multiple of 4: the 4 pixels lie in the same tiles), the
// ONE body of mosaic_blend_kernel (mosaic.hip) and gaps_blend_kernel (gaps.hip).  Tiles are visited in increasing (ky, kx);
// slot_of(k) is the position of tile k in sr, a negative one skips the tile.  Uncovered (cover = 0 only): the reference's np.zeros.
template <class SlotOf>
static __device__ __forceinline__ float4 mosaic_blend4(const float* __restrict__ sr, const MosaicGeom& gm, float R, float mean,
                                                       float std, int X, int Y, SlotOf slot_of) {
  const int W = 4 * gm.ax.w;                    // tile side in output pixels
  const MosaicCover cy = mosaic_cover(gm.ay, Y >> 2), cx = mosaic_cover(gm.ax, X >> 2);
  float4 num = make_float4(0.f, 0.f, 0.f, 0.f), den = num;
  for (int a = 0; a < cy.n; ++a) {
    const int ky = mosaic_cover_index(cy, a);
    const int qy = Y - 4 * mosaic_origin(gm.ay, ky);
    const float wy = feather(qy, W, R);
    for (int b = 0; b < cx.n; ++b) {
      const int kx = mosaic_cover_index(cx, b);
      const int qx = X - 4 * mosaic_origin(gm.ax, kx);
      const int k = slot_of(ky * gm.ax.count + kx);
      if (k < 0) continue;
      const float4 v = ld4(sr + ((size_t)k * W + qy) * W + qx);
      const float w0 = wy * feather(qx, W, R), w1 = wy * feather(qx + 1, W, R);
      const float w2 = wy * feather(qx + 2, W, R), w3 = wy * feather(qx + 3, W, R);
      num.x += w0 * v.x; num.y += w1 * v.y; num.z += w2 * v.z; num.w += w3 * v.w;
      den.x += w0; den.y += w1; den.z += w2; den.w += w3;
    }
  }
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (cy.n > 0 && cx.n > 0) {
    o.x = num.x / den.x * std + mean; o.y = num.y / den.y * std + mean;
    o.z = num.z / den.z * std + mean; o.w = num.w / den.w * std + mean;
  }
  return o;
}

// ---- mosaic.hip ----
int launch_mosaic_prepare(const float* lst, const float* ndvi, float* x, int lst_h, int lst_w, int win, int overlap, int cover,
                          float mean_lst, float std_lst, float mean_ndvi, float std_ndvi, int clip_ndvi, hipStream_t s);
int launch_mosaic_blend(const float* sr, float* out, int lst_h, int lst_w, int win, int overlap, int cover, float mean_lst,
                        float std_lst, hipStream_t s);
