// Whole-granule prediction at any ratio hr / win (C ABI: include/sifsr_ratio.h): the ONE definition of the
// geometry, shared by the host entry points and the kernels of ratio.hip, and the ONE device body of the bicubic resampler that
// ratio_upsample_kernel and ratio_prepare_kernel run.  Tile origins are those of mosaic.h; nothing of the layout is restated.
#pragma once
#include "mosaic.h"

// ---------------------------------------------------------------------------------------------
// Geometry: p / q = hr / win in lowest terms; the LST axes are mosaic.h's, the HR raster is (H, W) = (lst_h, lst_w) * p / q.
// ---------------------------------------------------------------------------------------------
struct RatioGeom {
  MosaicAxis ay, ax;   // LST pixels
  int p, q, hr;
  int lst_w, H, W;
};

__host__ __device__ inline int ratio_gcd(int a, int b) {
  while (b) {
    const int t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// false: SIFSR_ERR_SHAPE (the rules of include/sifsr_ratio.h)
inline bool ratio_geom(int lst_h, int lst_w, int win, int hr, int overlap, int cover, RatioGeom* g) {
  if (win < 1 || win > 64 || hr % 8 || hr < 24 || hr > 256 || hr <= win || hr > 16 * win) return false;
  const int d = ratio_gcd(hr, win);
  g->p = hr / d;
  g->q = win / d;
  g->hr = hr;
  if (lst_h < win || lst_w < win || lst_h > 16384 || lst_w > 16384 || lst_h % g->q || lst_w % g->q) return false;
  if (overlap < 0 || 2 * overlap > win || overlap % g->q) return false;
  g->ay = mosaic_axis(lst_h, win, overlap, cover);
  g->ax = mosaic_axis(lst_w, win, overlap, cover);
  if (g->ay.count < 1 || g->ax.count < 1) return false;
  g->lst_w = lst_w;
  g->H = lst_h / g->q * g->p;
  g->W = lst_w / g->q * g->p;
  return true;
}

// The same axis in HR pixels: raster n p / q, window hr, stride s p / q -- whole pixels under the rules above -- so that
// mosaic_origin / mosaic_cover of mosaic.h answer in HR pixels: tile k covers HR pixel Y iff o_k p <= Y q < (o_k + win) p.
__host__ __device__ inline MosaicAxis ratio_hr_axis(const MosaicAxis& a, int p, int q, int hr) {
  return MosaicAxis{a.n / q * p, hr, a.s / q * p, a.reg, a.count};
}

// ---------------------------------------------------------------------------------------------
// The resampler: F.interpolate(mode="bicubic", align_corners=False) along an axis n -> N (N >= n) with an exact phase
// ---------------------------------------------------------------------------------------------
template <class T>
struct RatioPhaseT {
  int i;   // floor of the source coordinate ((2d + 1) n - N) / (2N): -1 .. n - 1
  T t;     // its fraction: remainder / (2N), both integers below 2^24 -> one rounding
};
typedef RatioPhaseT<float> RatioPhase;

template <class T>
static __device__ __forceinline__ RatioPhaseT<T> ratio_phase_t(int d, int n, int N) {
  const int num = (2 * d + 1) * n - N, den = 2 * N;   // num > -den
  const int i = num < 0 ? -1 : num / den;
  return RatioPhaseT<T>{i, (T)(num - i * den) / (T)den};
}
static __device__ __forceinline__ RatioPhase ratio_phase(int d, int n, int N) { return ratio_phase_t<float>(d, n, N); }

// the four weights at fraction t (A = -0.75), Horner forms in explicit fused multiply-adds: 0, 1, 0, 0 exactly at t = 0.  T is
// float (the network's input pipeline) or double (the evaluation operators of rbaselines.hip); the constants are exact in both.
static __device__ __forceinline__ float ratio_fma(float a, float b, float c) { return fmaf(a, b, c); }
static __device__ __forceinline__ double ratio_fma(double a, double b, double c) { return fma(a, b, c); }
template <class T> static __device__ __forceinline__ T ratio_w_near(T x) { return ratio_fma(ratio_fma((T)1.25, x, (T)-2.25) * x, x, (T)1); }
template <class T> static __device__ __forceinline__ T ratio_w_far(T x) {
  return ratio_fma(ratio_fma(ratio_fma((T)-0.75, x, (T)3.75), x, (T)-6), x, (T)3);
}
template <class T> static __device__ __forceinline__ void ratio_weights(T t, T c[4]) {
  c[0] = ratio_w_far(t + (T)1); c[1] = ratio_w_near(t); c[2] = ratio_w_near((T)1 - t); c[3] = ratio_w_far((T)2 - t);
}
template <class T> static __device__ __forceinline__ T ratio_dot4(T a0, T a1, T a2, T a3, const T c[4]) {
  return ratio_fma(a3, c[3], ratio_fma(a2, c[2], ratio_fma(a1, c[1], a0 * c[0])));
}

constexpr int RATIO_ROWS = 16;             // output rows of one workgroup
constexpr int RATIO_COLS = 256;            // output columns of one workgroup: thread = output column
constexpr int RATIO_SRC_ROWS = 20;         // N >= n: 16 output rows touch at most 15 + 4 source rows
constexpr int RATIO_SRC_COLS = 260 + 4;    // 256 output columns touch at most 255 + 4 source columns (+ padding)

// One workgroup of 256 threads = output rows [Y0, Y0 + 16) x columns [X0, X0 + 256) of ONE (H, W) image resampled from an
// (h, w) block, indices clamped to the block.  The source rows and columns the workgroup needs are staged in LDS as
// load(gy, gx) with the clamp applied; a thread then slides a window of four horizontally resampled rows down its column
// (N >= n: the source row advances by 0 or 1 per output row, uniformly over the workgroup) and hands every output to
// emit(dy, Y, X, v), dy = Y - Y0 a compile-time constant of the unrolled loop.  Stores by emit are coalesced along X.
// T is the type of the staged values, of the weights and of the arithmetic.
template <class T, class Load, class Emit>
static __device__ __forceinline__ void ratio_resample_block_t(Load load, int h, int w, int H, int W, int Y0, int X0,
                                                              T (*src)[RATIO_SRC_COLS], Emit emit) {
  const int Y1 = min(Y0 + RATIO_ROWS, H) - 1, X1 = min(X0 + RATIO_COLS, W) - 1;
  const int r0 = ratio_phase(Y0, h, H).i - 1, NR = ratio_phase(Y1, h, H).i + 3 - r0;   // <= 19
  const int c0 = ratio_phase(X0, w, W).i - 1, NC = ratio_phase(X1, w, W).i + 3 - c0;   // <= 259
  for (int e = threadIdx.x; e < NR * NC; e += 256) {
    const int r = e / NC, c = e - r * NC;
    const int gy = clampi(r0 + r, 0, h - 1), gx = clampi(c0 + c, 0, w - 1);
    src[r][c] = load(gy, gx);
  }
  __syncthreads();
  const int X = X0 + threadIdx.x;
  if (X > X1) return;
  const RatioPhaseT<T> px = ratio_phase_t<T>(X, w, W);
  T cx[4];
  ratio_weights(px.t, cx);
  const int xo = px.i - 1 - c0;
  auto hpass = [&](int r) { return ratio_dot4(src[r][xo], src[r][xo + 1], src[r][xo + 2], src[r][xo + 3], cx); };
  T w0 = hpass(0), w1 = hpass(1), w2 = hpass(2), w3 = hpass(3);
  int cur = 0;   // w0 .. w3 = staged rows cur .. cur + 3
#pragma unroll
  for (int dy = 0; dy < RATIO_ROWS; ++dy) {
    const int Y = Y0 + dy;
    if (Y > Y1) break;
    const RatioPhaseT<T> py = ratio_phase_t<T>(Y, h, H);
    if (cur < py.i - 1 - r0) {   // = cur + 1 <= NR - 4
      ++cur;
      w0 = w1; w1 = w2; w2 = w3;
      w3 = hpass(cur + 3);
    }
    T cy[4];
    ratio_weights(py.t, cy);
    emit(dy, Y, X, ratio_dot4(w0, w1, w2, w3, cy));
  }
}

// the float form every kernel of the network's pipeline runs: the (h, w) block at p (row stride `row` elements), staged as
// (v - mean) * istd
template <class Emit>
static __device__ __forceinline__ void ratio_resample_block(const float* __restrict__ p, size_t row, int h, int w, int H, int W,
                                                            int Y0, int X0, float mean, float istd,
                                                            float (*src)[RATIO_SRC_COLS], Emit emit) {
  ratio_resample_block_t<float>([=](int gy, int gx) { return (p[(size_t)gy * row + gx] - mean) * istd; }, h, w, H, W, Y0, X0, src,
                                emit);
}
