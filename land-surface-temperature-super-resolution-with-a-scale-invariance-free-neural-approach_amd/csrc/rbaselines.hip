// The sharpening baselines at any ratio p / q (C entry points and every definition: csrc/rbaselines_api.h):
// the passes of TsHARP, ATPRK, AATPRK and DMS that touch the FINE raster.  What reads coarse rasters alone stays in baselines.hip
// and dms.hip.  Evaluation operators: float64 arithmetic, one rounding at the float32 store, accuracy before rate.
//
//  * rb_aggregate_kernel   one thread per coarse cell: the <= 8 x 8 fine pixels of the cell in row-major order, twice (mean, then
//    the centred squares); neighbouring threads read neighbouring row segments, so the lines of a row are used in full.
//  * rb_sharpen_kernel     block = 64 x 4 threads = the fine rows of ONE coarse row over 256 fine columns: thread (i, j) owns the
//    4 consecutive fine pixels [X0 + 4 i, + 4) of the rows Ya + j, Ya + j + 4 (a coarse row holds at most 8).  Modes 1, 2: the
//    image's s^2 x 25 weights and the 5 residual rows over the columns of the workgroup's cells plus 2 either side are staged in
//    LDS, zero outside the raster; every staged element is written before the barrier and nothing else is read.
//    LDS banks (ds_read_b64: 32-lane groups, 32 distinct 8-byte slots per 256-byte row): a weight row is 25 doubles, an odd stride,
//    so the <= 8 rows the lanes of a group read for one tap lie on distinct slots; the residual tap of the lanes of a group
//    advances by 4 / s doubles per lane: conflict-free from s = 4, two lanes per slot at s = 2 and 3.
//  * rb_predict_kernel     the image's E leaf tables in LDS, a thread owns 4 consecutive pixels of the FLAT image, a block walks
//    4 x 1024 of them: no geometry, any (H, W).
//  * rb_correct_kernel     ratio_resample_block_t<double> of ratio.h -- the one body of the package's bicubic resampler, with
//    lst^4 - m4 as the loader and the fourth root as the emitter: 16 x 256 outputs per workgroup, 256 consecutive floats a row.
// The access width V (4, 2, 1 floats) of the fine raster is picked on the host per call from the alignment of the bases and of
// the row pitch (the way of rproducts.hip); what is computed from the loaded values does not depend on V.
// No atomics, no allocation, no host synchronisation.  Products and sums are kept apart (no contraction), so that every stage is
// the float64 arithmetic tests/rbaselines_reference.py writes down.
#include "rbaselines_api.h"

#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

#include "dms_dev.h"
#include "ratio.h"

namespace {

constexpr int HALO = 2;                 // radius of the 5 x 5 kriging block
constexpr int SH_COLS = 256;            // fine columns of one sharpening workgroup
constexpr int SH_CELLS = SH_COLS / 2 + 1 + 2 * HALO;     // modes 1, 2 (s >= 2): the cells under 256 fine columns, and the halo
constexpr int MAX_S = 8;
constexpr int MAXL = 30, MAXT = MAXL - 1;                // SIFSRD_MAX_LEAVES of include/sifsr_dms.h
constexpr int PRED_ITERS = 4;

struct Geom {
  int h, w, H, W, p, q;
};

// false: SIFSR_ERR_SHAPE (the rules of rbaselines_api.h)
bool geom(int B, int h, int w, int H, int W, Geom* g) {
  if (B < 1 || B > 65535 || h < 1 || w < 1 || h > 16384 || w > 16384 || H <= h || W <= w) return false;
  const int d = ratio_gcd(H, h);
  const int p = H / d, q = h / d;
  if (p > 8 * q || w % q || (long long)W != (long long)(w / q) * p) return false;
  *g = Geom{h, w, H, W, p, q};
  return true;
}

// first fine index of cell i along an axis: ceil(i p / q).  i <= h = g q and p = H / g, so i p <= H q <= 2^17 * 2^14: the product
// and the q - 1 added to it stay inside 32 unsigned bits, and a 32-bit division is a fraction of the cost of a 64-bit one
__device__ __forceinline__ int cell_begin(int i, int p, int q) { return (int)(((unsigned)i * (unsigned)p + (unsigned)(q - 1)) / (unsigned)q); }
// the cell of fine index Y: floor(Y q / p).  Y < H <= 2^17, q <= 2^14: Y q < 2^31
__device__ __forceinline__ int cell_of(int Y, int p, int q) { return (int)(((unsigned)Y * (unsigned)q) / (unsigned)p); }

// ---- cell statistics -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rb_aggregate_kernel(const float* __restrict__ fine, double* __restrict__ mean,
                                                           double* __restrict__ sd, const Geom g, size_t cells, int pow4) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= cells) return;
  const size_t per = (size_t)g.h * g.w;
  const size_t b = t / per, r = t - b * per;
  const int i = (int)(r / g.w), j = (int)(r - (size_t)i * g.w);
  const int Ya = cell_begin(i, g.p, g.q), Yb = cell_begin(i + 1, g.p, g.q);
  const int Xa = cell_begin(j, g.p, g.q), Xb = cell_begin(j + 1, g.p, g.q);
  const float* src = fine + b * (size_t)g.H * g.W;
  double s = 0.0, n = 0.0;
  for (int Y = Ya; Y < Yb; ++Y)
    for (int X = Xa; X < Xb; ++X) {
      double v = (double)src[(size_t)Y * g.W + X];
      if (pow4) v = pow4d(v);
      const bool ok = v == v;
      s = s + (ok ? v : 0.0);
      n = n + (ok ? 1.0 : 0.0);
    }
  const double m = s / n;
  mean[t] = m;
  if (sd != nullptr) {
    double qs = 0.0;
    for (int Y = Ya; Y < Yb; ++Y)
      for (int X = Xa; X < Xb; ++X) {
        double v = (double)src[(size_t)Y * g.W + X];
        if (pow4) v = pow4d(v);
        const double d = (v == v) ? v - m : 0.0;
        qs = qs + d * d;
      }
    sd[t] = sqrt(qs / n);
  }
}

// ---- four consecutive floats at p, of which the first n (1 .. 4) exist; V = the widest access the call's alignment allows ------
template <int V> __device__ __forceinline__ void load_quad(const float* p, int n, float v[4]) {
  if (V == 4) {                                        // n == 4: W % 4 == 0
    const float4 q = ld4(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else if (V == 2) {                                 // n is 2 or 4: W % 2 == 0
    const float2 a = *reinterpret_cast<const float2*>(p);
    v[0] = a.x; v[1] = a.y; v[2] = 0.f; v[3] = 0.f;
    if (n > 2) {
      const float2 c = *reinterpret_cast<const float2*>(p + 2);
      v[2] = c.x; v[3] = c.y;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = k < n ? p[k] : 0.f;
  }
}

template <int V> __device__ __forceinline__ void store_quad(float* p, int n, const float v[4]) {
  if (V == 4) {
    st4(p, make_float4(v[0], v[1], v[2], v[3]));
  } else if (V == 2) {
    *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
    if (n > 2) *reinterpret_cast<float2*>(p + 2) = make_float2(v[2], v[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) p[k] = v[k];
  }
}

// ---- the fused unmix + correction pass -----------------------------------------------------------------------------------------
// grid = (ceil(W / 256), h, B), block = (64, 4)
template <int MODE, int V>
__global__ __launch_bounds__(256) void rb_sharpen_kernel(const float* __restrict__ lst, const float* __restrict__ ndvi_f,
                                                         const double* __restrict__ coef, const double* __restrict__ delta,
                                                         const double* __restrict__ lambdas, float* __restrict__ out,
                                                         const Geom g) {
  __shared__ double lam[MODE != 0 ? MAX_S * MAX_S * 25 : 1];
  __shared__ double drow[MODE != 0 ? 5 : 1][MODE != 0 ? SH_CELLS : 1];
  const int b = blockIdx.z, r = blockIdx.y, X0 = blockIdx.x * SH_COLS;
  const int h = g.h, w = g.w, W = g.W, p = g.p, q = g.q;
  const int tid = threadIdx.y * 64 + threadIdx.x;
  const size_t cimg = (size_t)b * h * w;
  const double* d = delta + cimg;
  const int X1 = min(X0 + SH_COLS, W) - 1;
  const int c_lo = cell_of(X0, p, q);                  // the first cell under the workgroup
  if (MODE != 0) {
    const int s2 = p * p;                              // q == 1: s = p
    for (int e = tid; e < s2 * 25; e += 256) lam[e] = lambdas[(size_t)b * s2 * 25 + e];
    const int nc = cell_of(X1, p, q) - c_lo + 1 + 2 * HALO;      // <= 128 + 4 < SH_CELLS
    for (int e = tid; e < 5 * nc; e += 256) {
      const int y = e / nc, x = e - y * nc;
      const int rr = r - HALO + y, cc = c_lo - HALO + x;
      drow[y][x] = (rr >= 0 && rr < h && cc >= 0 && cc < w) ? d[(size_t)rr * w + cc] : 0.0;
    }
    __syncthreads();
  }
  const int X = X0 + 4 * threadIdx.x;
  if (X >= W) return;
  const int n = min(4, W - X);
  // what depends on the column alone: the cell of each of the 4 pixels, its lst mask or coefficients, its residual
  int cx[4];
  double a0[4], a1[4], m[4], dc[4];
  bool inner[4];
  const bool rin = r >= HALO && r < h - HALO;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    cx[k] = cell_of(min(X + k, W - 1), p, q);
    const size_t cpx = (size_t)r * w + cx[k];
    if (MODE == 2) {
      a0[k] = coef[2 * cimg + cpx];
      a1[k] = coef[2 * cimg + (size_t)h * w + cpx];
      m[k] = 1.0;
    } else {
      a0[k] = coef[(size_t)b * 2 + 0];
      a1[k] = coef[(size_t)b * 2 + 1];
      m[k] = lst[cimg + cpx] != 0.f ? 1.0 : 0.0;
    }
    dc[k] = MODE == 0 ? d[cpx] : 0.0;
    inner[k] = rin && cx[k] >= HALO && cx[k] < w - HALO;
  }
  const int Ya = cell_begin(r, p, q), Yb = cell_begin(r + 1, p, q);
  for (int Y = Ya + threadIdx.y; Y < Yb; Y += 4) {
    const size_t fpx = ((size_t)b * g.H + Y) * (size_t)W + X;
    float iv[4], ov[4];
    load_quad<V>(ndvi_f + fpx, n, iv);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double I = (double)iv[k];
      double u;
      if (MODE == 2) u = fabs(I) > 0.0 ? a0[k] + a1[k] * I : 0.0;
      else u = (a0[k] + a1[k] * I) * m[k];
      double o = u;
      if (MODE == 0) {
        o = u == 0.0 ? u : u + dc[k];
      } else if (k < n && inner[k]) {                  // a lane past the raster's last column forms no weight row
        const double* l = lam + ((Y - Ya) * p + (X + k - cx[k] * p)) * 25;      // q == 1: Y % s, X % s
        const int xo = cx[k] - c_lo;
        double s = 0.0;
#pragma unroll
        for (int t = 0; t < 25; ++t) s += l[t] * drow[t / 5][xo + t % 5];
        o = u == 0.0 ? u : u + s;
      }
      ov[k] = (float)o;
    }
    store_quad<V>(out + fpx, n, ov);
  }
}

// ---- the tree ensemble at any (H, W) -------------------------------------------------------------------------------------------
// grid = (ceil(npx / 4096), B), block = 256: thread t owns the flat pixels [4096 blockIdx.x + 1024 k + 4 t, + 4), k = 0 .. 3
template <int V>
__global__ __launch_bounds__(256) void rb_predict_kernel(const float* __restrict__ ndvi, const double* __restrict__ thresholds,
                                                         const int* __restrict__ nleaf, const double* __restrict__ leaves,
                                                         float* __restrict__ sr, int E, size_t npx) {
  extern __shared__ double tab[];                                  // thr [E][29], leaves [E][120], nleaf [E]
  double* thr = tab;
  double* lf = tab + (size_t)E * MAXT;
  int* nl = reinterpret_cast<int*>(lf + (size_t)E * MAXL * 4);
  const int tid = threadIdx.x, b = blockIdx.y;
  for (int k = tid; k < E * MAXT; k += 256) thr[k] = thresholds[(size_t)b * E * MAXT + k];
  for (int k = tid; k < E * MAXL * 4; k += 256) lf[k] = leaves[(size_t)b * E * MAXL * 4 + k];
  for (int k = tid; k < E; k += 256) nl[k] = nleaf[(size_t)b * E + k];
  __syncthreads();
  const bool model = nl[0] > 0;
  const float fnan = __uint_as_float(0x7FC00000u);
  for (int it = 0; it < PRED_ITERS; ++it) {
    const size_t e = ((size_t)blockIdx.x * PRED_ITERS + it) * 1024 + 4 * (size_t)tid;
    if (e >= npx) break;
    const int n = (int)min((size_t)4, npx - e);
    const size_t px = (size_t)b * npx + e;
    float in[4], o[4];
    load_quad<V>(ndvi + px, n, in);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool nan = in[u] != in[u];
      const double x = nan ? 0.0 : (double)in[u];
      double acc = 0.0;
      if (model)
        for (int k = 0; k < E; ++k) acc = acc + tree_value(thr + k * MAXT, lf + k * MAXL * 4, nl[k], x);
      o[u] = (nan || !model) ? fnan : (float)(acc / (double)E);
    }
    store_quad<V>(sr + px, n, o);
  }
}

// ---- the radiance residual correction ------------------------------------------------------------------------------------------
// grid = (ceil(W / 256), ceil(H / 16), B), block = 256
__global__ __launch_bounds__(256) void rb_correct_kernel(const float* __restrict__ lst, const float* __restrict__ sr,
                                                         const double* __restrict__ m4, float* __restrict__ out, int h, int w, int H,
                                                         int W) {
  __shared__ double src[RATIO_SRC_ROWS][RATIO_SRC_COLS];
  const float* T = lst + (size_t)blockIdx.z * h * w;
  const double* M = m4 + (size_t)blockIdx.z * h * w;
  const float* si = sr + (size_t)blockIdx.z * H * W;
  float* oi = out + (size_t)blockIdx.z * H * W;
  ratio_resample_block_t<double>(
      [=](int gy, int gx) {
        const size_t c = (size_t)gy * w + gx;
        return pow4d((double)T[c]) - M[c];
      },
      h, w, H, W, blockIdx.y * RATIO_ROWS, blockIdx.x * RATIO_COLS, src,
      [=](int, int Y, int X, double v) {
        const size_t e = (size_t)Y * W + X;
        oi[e] = (float)sqrt(sqrt(v + pow4d((double)si[e])));
      });
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// the widest access of a raster whose rows (or whose whole image) are `pitch` floats apart
int width_of(const void* in, const void* out, size_t pitch) {
  if (pitch % 4 == 0 && aligned(in, 16) && aligned(out, 16)) return 4;
  if (pitch % 2 == 0 && aligned(in, 8) && aligned(out, 8)) return 2;
  return 1;
}

template <int MODE>
void launch_sharpen(int V, dim3 grid, hipStream_t s, const float* lst, const float* ndvi_f, const double* coef,
                    const double* delta, const double* lambdas, float* out, const Geom& g) {
  const dim3 block(64, 4);
  if (V == 4) hipLaunchKernelGGL((rb_sharpen_kernel<MODE, 4>), grid, block, 0, s, lst, ndvi_f, coef, delta, lambdas, out, g);
  else if (V == 2) hipLaunchKernelGGL((rb_sharpen_kernel<MODE, 2>), grid, block, 0, s, lst, ndvi_f, coef, delta, lambdas, out, g);
  else hipLaunchKernelGGL((rb_sharpen_kernel<MODE, 1>), grid, block, 0, s, lst, ndvi_f, coef, delta, lambdas, out, g);
}

}  // namespace

// ---- C entry points (rbaselines_api.h) ----
int sifsrh_aggregate(const float* fine, double* mean, double* sd, int B, int h, int w, int H, int W, int pow4, void* stream) {
  if (!fine || !mean || !aligned(fine, 4) || !aligned(mean, 8) || !aligned(sd, 8)) return SIFSR_ERR_ARG;
  Geom g;
  if (!geom(B, h, w, H, W, &g)) return SIFSR_ERR_SHAPE;
  const size_t cells = (size_t)B * h * w;
  if (cells > ((size_t)1 << 31)) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(rb_aggregate_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream, fine, mean, sd,
                     g, cells, pow4 ? 1 : 0);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrh_sharpen(const float* lst, const float* ndvi_f, const double* coef, const double* delta, const double* lambdas,
                   float* out, int B, int h, int w, int H, int W, int mode, void* stream) {
  if (!lst || !ndvi_f || !coef || !delta || !out || (mode != 0 && !lambdas)) return SIFSR_ERR_ARG;
  if (mode < 0 || mode > 2) return SIFSR_ERR_ARG;
  if (!aligned(lst, 4) || !aligned(ndvi_f, 4) || !aligned(out, 4) || !aligned(coef, 8) || !aligned(delta, 8) || !aligned(lambdas, 8)) return SIFSR_ERR_ARG;
  Geom g;
  if (!geom(B, h, w, H, W, &g)) return SIFSR_ERR_SHAPE;
  if (mode != 0 && (g.q != 1 || g.p < 2 || g.p > MAX_S || h < 5 || w < 5)) return SIFSR_ERR_SHAPE;
  const dim3 grid((W + SH_COLS - 1) / SH_COLS, h, B);
  const int V = width_of(ndvi_f, out, (size_t)W);
  hipStream_t s = (hipStream_t)stream;
  if (mode == 0) launch_sharpen<0>(V, grid, s, lst, ndvi_f, coef, delta, lambdas, out, g);
  else if (mode == 1) launch_sharpen<1>(V, grid, s, lst, ndvi_f, coef, delta, lambdas, out, g);
  else launch_sharpen<2>(V, grid, s, lst, ndvi_f, coef, delta, lambdas, out, g);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrh_predict(const float* ndvi_f, const double* thresholds, const int* nleaf, const double* leaves, float* sr, int B, int E,
                   int H, int W, void* stream) {
  if (!ndvi_f || !thresholds || !nleaf || !leaves || !sr || !aligned(ndvi_f, 4) || !aligned(sr, 4) || !aligned(thresholds, 8) ||
      !aligned(leaves, 8) || !aligned(nleaf, 4))
    return SIFSR_ERR_ARG;
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > 131072 || W > 131072 || E < 1 || E > 32) return SIFSR_ERR_SHAPE;
  const size_t npx = (size_t)H * W;
  const size_t lds = (size_t)E * (MAXT + MAXL * 4) * sizeof(double) + (size_t)E * sizeof(int);
  const dim3 grid((unsigned)((npx + PRED_ITERS * 1024 - 1) / (PRED_ITERS * 1024)), B);
  hipStream_t s = (hipStream_t)stream;
  if (width_of(ndvi_f, sr, npx) == 4)
    hipLaunchKernelGGL(rb_predict_kernel<4>, grid, dim3(256), lds, s, ndvi_f, thresholds, nleaf, leaves, sr, E, npx);
  else
    hipLaunchKernelGGL(rb_predict_kernel<1>, grid, dim3(256), lds, s, ndvi_f, thresholds, nleaf, leaves, sr, E, npx);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrh_correct(const float* lst, const float* sr, const double* m4, float* out, int B, int h, int w, int H, int W,
                   void* stream) {
  if (!lst || !sr || !m4 || !out || !aligned(lst, 4) || !aligned(sr, 4) || !aligned(out, 4) || !aligned(m4, 8)) return SIFSR_ERR_ARG;
  Geom g;
  if (!geom(B, h, w, H, W, &g)) return SIFSR_ERR_SHAPE;
  // the resampler forms (2 d + 1) n - N in int (ratio.h)
  if ((long long)2 * H * h >= (1ll << 31) || (long long)2 * W * w >= (1ll << 31)) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(rb_correct_kernel, dim3((W + RATIO_COLS - 1) / RATIO_COLS, (H + RATIO_ROWS - 1) / RATIO_ROWS, B), dim3(256), 0,
                     (hipStream_t)stream, lst, sr, m4, out, h, w, H, W);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}
