// The classical sharpening baselines of the paper's comparison (C ABI: include/sifsr_baselines.h):
// TsHARP, ATPRK and AATPRK, reference utils.py:854-1606.  The reference computes them in float64 NumPy loops; the data-sized parts
// are regular stencil and reduction work and run here, in float64 with one rounding at the final float32 store (an evaluation
// operator: accuracy before rate, the choice of fourier.hip).  The variogram fits and the kriging system stay on the host.
//
//  * linfit_kernel            one workgroup per image, two passes (means, then centred sums), fixed-order reductions
//  * linfit_window_kernel     one thread per coarse pixel, the same regression over its window
//  * residual_kernel          delta = T - (a0 + a1 I), 0-model where !(T > 0)
//  * semivar_tile_kernel      16 x 16 windows per workgroup from a 20 x 20 LDS tile; a thread forms the 300 pair differences of
//    semivar_final_kernel     its window in registers; per-tile sums / counts, then added in tile order
//  * sharpen_kernel           unmix + correction fused: 16 bytes of the fine index in, 16 bytes out per thread
// No atomics anywhere: the results are bit-reproducible and a row of a batch equals its own single-image call.
#include "../../include/sifsr_baselines.h"

#include "common.h"

namespace {

constexpr int NCLASS = 15;       // distinct squared distances in a 5 x 5 block
constexpr int TILE = 16;         // windows per tile side
constexpr int HALO = 2;          // block radius
constexpr int TW = TILE + 2 * HALO;

// class index of the squared distance k = dr^2 + dc^2 (0 <= dr, dc <= 4): the rank of k among the 15 values that occur
constexpr int class_of(int k) {
  constexpr int ks[NCLASS] = {0, 1, 2, 4, 5, 8, 9, 10, 13, 16, 17, 18, 20, 25, 32};
  for (int i = 0; i < NCLASS; ++i)
    if (ks[i] == k) return i;
  return -1;
}
// pairs i < j of the 5 x 5 block at squared distance ks[c]
constexpr int npairs_of(int c) {
  int n = 0;
  for (int i = 0; i < 25; ++i)
    for (int j = i + 1; j < 25; ++j) {
      const int dr = i / 5 - j / 5, dc = i % 5 - j % 5;
      if (class_of(dr * dr + dc * dc) == c) ++n;
    }
  return n;
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// sum of v over the 256 threads of a workgroup, returned to every thread: shuffles inside a wave, then the four wave sums
// in wave order.  `red` holds 4 doubles, tid is the thread's linear index; the two barriers make it reusable by the next call.
__device__ __forceinline__ double block_sum(double v, double* red, int tid) {
  v = wave_sum(v);
  const int lane = tid & 63, wv = tid >> 6;
  if (lane == 0) red[wv] = v;
  __syncthreads();
  const double s = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();
  return s;
}

__device__ __forceinline__ bool fit_valid(float T, float I, float min_T) { return T > min_T && isfinite(I); }

__global__ __launch_bounds__(256) void linfit_kernel(const float* __restrict__ lst, const float* __restrict__ ndvi,
                                                     double* __restrict__ fit, int npx, float min_T) {
  __shared__ double red[4];
  const float* T = lst + (size_t)blockIdx.x * npx;
  const float* I = ndvi + (size_t)blockIdx.x * npx;
  double n = 0.0, sT = 0.0, sI = 0.0;
  for (int p = threadIdx.x; p < npx; p += 256) {
    const float t = T[p], i = I[p];
    if (fit_valid(t, i, min_T)) { n += 1.0; sT += (double)t; sI += (double)i; }
  }
  n = block_sum(n, red, threadIdx.x); sT = block_sum(sT, red, threadIdx.x); sI = block_sum(sI, red, threadIdx.x);
  const double mT = sT / n, mI = sI / n;
  double cov = 0.0, var = 0.0;
  for (int p = threadIdx.x; p < npx; p += 256) {
    const float t = T[p], i = I[p];
    if (fit_valid(t, i, min_T)) {
      const double di = (double)i - mI;
      cov += di * ((double)t - mT); var += di * di;
    }
  }
  cov = block_sum(cov, red, threadIdx.x); var = block_sum(var, red, threadIdx.x);
  if (threadIdx.x == 0) {
    const double a1 = cov / var;
    fit[(size_t)blockIdx.x * 2 + 0] = mT - a1 * mI;
    fit[(size_t)blockIdx.x * 2 + 1] = a1;
  }
}

__global__ __launch_bounds__(256) void linfit_window_kernel(const float* __restrict__ lst, const float* __restrict__ ndvi,
                                                            const double* __restrict__ fit, double* __restrict__ coef, int h,
                                                            int w, int rad, float min_T) {
  const int p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (p >= h * w) return;
  const int r = p / w, c = p - r * w;
  const float* T = lst + (size_t)b * h * w;
  const float* I = ndvi + (size_t)b * h * w;
  double a0 = fit[(size_t)b * 2 + 0], a1 = fit[(size_t)b * 2 + 1];
  if (r >= rad && r < h - rad && c >= rad && c < w - rad) {
    const int side = 2 * rad + 1;
    int n = 0;
    double sT = 0.0, sI = 0.0;
    for (int y = r - rad; y <= r + rad; ++y)
      for (int x = c - rad; x <= c + rad; ++x) {
        const float t = T[y * w + x], i = I[y * w + x];
        if (fit_valid(t, i, min_T)) { ++n; sT += (double)t; sI += (double)i; }
      }
    if (3 * n > 2 * side * side) {                       // len(Tw) > 2/3 (2 radius + 1)^2
      const double mT = sT / n, mI = sI / n;
      double cov = 0.0, var = 0.0;
      for (int y = r - rad; y <= r + rad; ++y)
        for (int x = c - rad; x <= c + rad; ++x) {
          const float t = T[y * w + x], i = I[y * w + x];
          if (fit_valid(t, i, min_T)) {
            const double di = (double)i - mI;
            cov += di * ((double)t - mT); var += di * di;
          }
        }
      a1 = cov / var;
      a0 = mT - a1 * mI;
    }
  }
  double* o = coef + (size_t)b * 2 * h * w;
  o[p] = a0;
  o[(size_t)h * w + p] = a1;
}

__global__ __launch_bounds__(256) void residual_kernel(const float* __restrict__ lst, const float* __restrict__ ndvi,
                                                       const double* __restrict__ coef, int per_pixel,
                                                       double* __restrict__ delta, int npx) {
  const int p = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (p >= npx) return;
  const size_t e = (size_t)b * npx + p;
  const double a0 = per_pixel ? coef[(size_t)b * 2 * npx + p] : coef[(size_t)b * 2 + 0];
  const double a1 = per_pixel ? coef[(size_t)b * 2 * npx + npx + p] : coef[(size_t)b * 2 + 1];
  const double T = (double)lst[e];
  const double m = T > 0.0 ? a0 + a1 * (double)ndvi[e] : 0.0;
  delta[e] = T - m;
}

// block = 16 x 16 threads, thread (tx, ty) owns the window centred on coarse pixel (2 + 16 blockIdx.y + ty, 2 + 16 blockIdx.x + tx)
// part (B, tiles, 2, 14): per tile the sums of the non-zero gamma_w(k) and their counts, k = 1 .. 14
__global__ __launch_bounds__(256) void semivar_tile_kernel(const double* __restrict__ delta, double* __restrict__ part, int h,
                                                           int w) {
  __shared__ double tile[TW][TW + 1];
  __shared__ double red[4];
  const int b = blockIdx.z;
  const int r0 = blockIdx.y * TILE, c0 = blockIdx.x * TILE;      // top-left of the staged tile (halo included)
  const double* d = delta + (size_t)b * h * w;
  const int tid = threadIdx.y * TILE + threadIdx.x;
  for (int e = tid; e < TW * TW; e += 256) {
    const int y = e / TW, x = e - y * TW;
    tile[y][x] = (r0 + y < h && c0 + x < w) ? d[(size_t)(r0 + y) * w + c0 + x] : 0.0;
  }
  __syncthreads();
  const bool live = r0 + threadIdx.y + 2 * HALO < h && c0 + threadIdx.x + 2 * HALO < w;     // the window's last row / column exists
  double acc[NCLASS];
#pragma unroll
  for (int k = 0; k < NCLASS; ++k) acc[k] = 0.0;
  if (live) {
    double v[25];
#pragma unroll
    for (int i = 0; i < 25; ++i) v[i] = tile[threadIdx.y + i / 5][threadIdx.x + i % 5];
#pragma unroll
    for (int i = 0; i < 25; ++i)
#pragma unroll
      for (int j = i + 1; j < 25; ++j) {                           // the reference's pair order (utils.py:1038-1042)
        const int dr = i / 5 - j / 5, dc = i % 5 - j % 5;
        const double df = v[i] - v[j];
        acc[class_of(dr * dr + dc * dc)] += df * df;
      }
  }
  const int ntiles = gridDim.x * gridDim.y, t = blockIdx.y * gridDim.x + blockIdx.x;
  double* o = part + ((size_t)b * ntiles + t) * 2 * (NCLASS - 1);
#pragma unroll
  for (int k = 1; k < NCLASS; ++k) {
    const double g = acc[k] / (double)(2 * npairs_of(k));
    const bool use = live && g != 0.0;                             // np.nonzero: NaN counts
    const double s = block_sum(use ? g : 0.0, red, tid);
    const double n = block_sum(use ? 1.0 : 0.0, red, tid);
    if (tid == 0) { o[k - 1] = s; o[(NCLASS - 1) + k - 1] = n; }
  }
}

__global__ void semivar_final_kernel(const double* __restrict__ part, double* __restrict__ gamma, int ntiles) {
  const int b = blockIdx.x, k = threadIdx.x;                       // 15 threads
  if (k >= NCLASS) return;
  double g = 0.0;
  if (k > 0) {
    double s = 0.0, n = 0.0;
    for (int t = 0; t < ntiles; ++t) {
      const double* p = part + ((size_t)b * ntiles + t) * 2 * (NCLASS - 1);
      s += p[k - 1]; n += p[(NCLASS - 1) + k - 1];
    }
    g = n > 0.0 ? s / n : 0.0;
    if (isnan(g)) g = 0.0;                                         // Gamma_coarse[np.isnan(Gamma_coarse)] = 0
  }
  gamma[(size_t)b * NCLASS + k] = g;
}

// block = 64 x 4 threads: thread (i, j) owns fine pixels [4 c, 4 c + 4) of fine row 4 blockIdx.y + j, c = 64 blockIdx.x + i
template <int MODE>
__global__ __launch_bounds__(256) void sharpen_kernel(const float* __restrict__ lst, const float* __restrict__ ndvi_f,
                                                      const double* __restrict__ coef, const double* __restrict__ delta,
                                                      const double* __restrict__ lambdas, float* __restrict__ out, int h, int w) {
  __shared__ double lam[16 * 25];
  __shared__ double drow[5][64 + 2 * HALO];
  const int b = blockIdx.z, r = blockIdx.y, cbase = blockIdx.x * 64;
  const int tid = threadIdx.y * 64 + threadIdx.x;
  const double* d = delta + (size_t)b * h * w;
  if (MODE != 0) {
    for (int e = tid; e < 16 * 25; e += 256) lam[e] = lambdas[(size_t)b * 400 + e];
    for (int e = tid; e < 5 * (64 + 2 * HALO); e += 256) {
      const int y = e / (64 + 2 * HALO), x = e - y * (64 + 2 * HALO);
      const int rr = r - HALO + y, cc = cbase - HALO + x;
      drow[y][x] = (rr >= 0 && rr < h && cc >= 0 && cc < w) ? d[(size_t)rr * w + cc] : 0.0;
    }
    __syncthreads();
  }
  const int c = cbase + threadIdx.x;
  if (c >= w) return;
  const int Y = 4 * r + threadIdx.y;
  const size_t cpx = (size_t)r * w + c;
  const size_t fpx = ((size_t)b * 4 * h + Y) * (4 * (size_t)w) + 4 * c;
  const float4 iv = ld4(ndvi_f + fpx);
  const double I[4] = {(double)iv.x, (double)iv.y, (double)iv.z, (double)iv.w};
  double u[4];
  if (MODE == 2) {
    const double a0 = coef[(size_t)b * 2 * h * w + cpx], a1 = coef[(size_t)b * 2 * h * w + (size_t)h * w + cpx];
#pragma unroll
    for (int q = 0; q < 4; ++q) u[q] = fabs(I[q]) > 0.0 ? a0 + a1 * I[q] : 0.0;
  } else {
    const double a0 = coef[(size_t)b * 2 + 0], a1 = coef[(size_t)b * 2 + 1];
    const double m = lst[(size_t)b * h * w + cpx] != 0.f ? 1.0 : 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) u[q] = (a0 + a1 * I[q]) * m;
  }
  double o[4];
  if (MODE == 0) {
    const double dc = d[cpx];
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = u[q] == 0.0 ? u[q] : u[q] + dc;
  } else if (r >= HALO && r < h - HALO && c >= HALO && c < w - HALO) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double* l = lam + (threadIdx.y * 4 + q) * 25;
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < 25; ++k) s += l[k] * drow[k / 5][threadIdx.x + k % 5];
      o[q] = u[q] == 0.0 ? u[q] : u[q] + s;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = u[q];
  }
  st4(out + fpx, make_float4((float)o[0], (float)o[1], (float)o[2], (float)o[3]));
}

// shapes every launch shares: pixel counts and offsets of one image stay inside int, the batch inside the grid limits
bool shape_ok(int B, int h, int w) { return B >= 1 && B <= 65535 && h >= 5 && w >= 5 && h <= 8192 && w <= 8192; }
int tiles_1d(int n) { return (n - 2 * HALO + TILE - 1) / TILE; }      // tiles covering the n - 4 window centres of an axis

}  // namespace

// ---- C ABI (include/sifsr_baselines.h) ----
int sifsrb_linfit(const float* lst, const float* ndvi_c, double* fit, int B, int h, int w, float min_T, void* stream) {
  if (!lst || !ndvi_c || !fit) return SIFSR_ERR_ARG;
  if (!shape_ok(B, h, w)) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(linfit_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, lst, ndvi_c, fit, h * w, min_T);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrb_linfit_window(const float* lst, const float* ndvi_c, const double* fit, double* coef, int B, int h, int w, int radius,
                         float min_T, void* stream) {
  if (!lst || !ndvi_c || !fit || !coef) return SIFSR_ERR_ARG;
  if (!shape_ok(B, h, w) || radius < 1 || radius > 8) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(linfit_window_kernel, dim3((h * w + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, lst, ndvi_c, fit, coef,
                     h, w, radius, min_T);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrb_residual(const float* lst, const float* ndvi_c, const double* coef, int per_pixel, double* delta, int B, int h, int w,
                    void* stream) {
  if (!lst || !ndvi_c || !coef || !delta) return SIFSR_ERR_ARG;
  if (!shape_ok(B, h, w)) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(residual_kernel, dim3((h * w + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, lst, ndvi_c, coef,
                     per_pixel != 0, delta, h * w);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

size_t sifsrb_semivariogram_scratch_bytes(int B, int h, int w) {
  if (!shape_ok(B, h, w)) return 0;
  return (size_t)B * tiles_1d(h) * tiles_1d(w) * 2 * (NCLASS - 1) * sizeof(double);
}

int sifsrb_semivariogram(const double* delta, double* scratch, double* gamma, int B, int h, int w, void* stream) {
  if (!delta || !scratch || !gamma) return SIFSR_ERR_ARG;
  if (!shape_ok(B, h, w)) return SIFSR_ERR_SHAPE;
  const int ty = tiles_1d(h), tx = tiles_1d(w);
  hipLaunchKernelGGL(semivar_tile_kernel, dim3(tx, ty, B), dim3(TILE, TILE), 0, (hipStream_t)stream, delta, scratch, h, w);
  hipLaunchKernelGGL(semivar_final_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, scratch, gamma, ty * tx);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrb_sharpen(const float* lst, const float* ndvi_f, const double* coef, const double* delta, const double* lambdas,
                   float* out, int B, int h, int w, int mode, void* stream) {
  if (!lst || !ndvi_f || !coef || !delta || !out || (mode != 0 && !lambdas)) return SIFSR_ERR_ARG;
  if (mode < 0 || mode > 2) return SIFSR_ERR_ARG;
  if (!shape_ok(B, h, w)) return SIFSR_ERR_SHAPE;
  const dim3 grid((w + 63) / 64, h, B), block(64, 4);
  hipStream_t s = (hipStream_t)stream;
  if (mode == 0) hipLaunchKernelGGL(sharpen_kernel<0>, grid, block, 0, s, lst, ndvi_f, coef, delta, lambdas, out, h, w);
  else if (mode == 1) hipLaunchKernelGGL(sharpen_kernel<1>, grid, block, 0, s, lst, ndvi_f, coef, delta, lambdas, out, h, w);
  else hipLaunchKernelGGL(sharpen_kernel<2>, grid, block, 0, s, lst, ndvi_f, coef, delta, lambdas, out, h, w);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}
