// From the raw integer rasters of a MODIS granule to training patches and their statistics (C ABI:
// include/sifsr_products.h): reference process_modis.py:38-335 and the statistics half of data_preparation.py.
//
//  * decode_lst_kernel / decode_ndvi_kernel   eight pixels per thread, 16-byte loads and stores (a scalar tail for LST)
//  * census_kernel    one workgroup of 16 waves per window of the reference's generator: bad LST pixels and zero denominators
//  * select_kernel    one wavefront: ballot + prefix population count, the accepted windows in the order of k
//  * gather_kernel    one workgroup per accepted window: both patches and one row of float64 moments
// All four are one pass over HBM.  No atomics: integer counts are exact whatever the route, the moments merge in a fixed order.
//
// The float32 algebra is numpy's, operation by operation (0.0001f * raw, then the difference, the sum and the quotient); contraction
// into FMAs is off in this file so that nir - red and nir + red round exactly as there.  The quotient is formed in float64 and
// rounded once: for binary32 operands that IS the correctly rounded float32 quotient (53 >= 2 * 24 + 2), whatever the division
// mode the file is compiled with.
#include "../../include/sifsr_products.h"

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int CENSUS_THREADS = 1024;     // 16 waves: a 256 x 256 fine window is 8 chunks of 16 bytes per thread and array
constexpr int NWAVE = CENSUS_THREADS / 64;
constexpr float LST_SCALE = 0.02f, REFL_SCALE = 0.0001f;

template <int V> struct Vec;
template <> struct Vec<8> { typedef __attribute__((ext_vector_type(8))) short type; };
template <> struct Vec<4> { typedef __attribute__((ext_vector_type(4))) short type; };
typedef __attribute__((ext_vector_type(8))) unsigned short u16x8;

__device__ __forceinline__ float den_of(short n, short r) { return REFL_SCALE * (float)n + REFL_SCALE * (float)r; }
__device__ __forceinline__ float ndvi_of(short n, short r) {
  const float nir = REFL_SCALE * (float)n, red = REFL_SCALE * (float)r;
  const float num = nir - red, den = nir + red;
  return (float)((double)num / (double)den);
}
__device__ __forceinline__ float clip1(float v) {       // ndvi[ndvi > 1] = 1; ndvi[ndvi < -1] = -1: NaN passes
  v = v > 1.f ? 1.f : v;
  return v < -1.f ? -1.f : v;
}

// ---- 1. decode ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void decode_lst_kernel(const unsigned short* __restrict__ raw, float* __restrict__ out, size_t n) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, n8 = n / 8;
  if (g < n8) {
    const u16x8 v = *reinterpret_cast<const u16x8*>(raw + 8 * g);
    st4(out + 8 * g, make_float4(LST_SCALE * (float)v[0], LST_SCALE * (float)v[1], LST_SCALE * (float)v[2], LST_SCALE * (float)v[3]));
    st4(out + 8 * g + 4, make_float4(LST_SCALE * (float)v[4], LST_SCALE * (float)v[5], LST_SCALE * (float)v[6], LST_SCALE * (float)v[7]));
  }
  const size_t t = 8 * n8 + g;                                        // the tail: fewer than 8 pixels, the first threads
  if (g < 8 && t < n) out[t] = LST_SCALE * (float)raw[t];
}

__global__ __launch_bounds__(256) void decode_ndvi_kernel(const short* __restrict__ nir, const short* __restrict__ red,
                                                          float* __restrict__ out, size_t n, int clip) {
  typedef Vec<8>::type V8;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, n8 = n / 8;       // n = 16 h w: no tail
  if (g < n8) {
    const V8 a = *reinterpret_cast<const V8*>(nir + 8 * g), b = *reinterpret_cast<const V8*>(red + 8 * g);
    float o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      o[i] = ndvi_of(a[i], b[i]);
      if (clip) o[i] = clip1(o[i]);
    }
    st4(out + 8 * g, make_float4(o[0], o[1], o[2], o[3]));
    st4(out + 8 * g + 4, make_float4(o[4], o[5], o[6], o[7]));
  }
}

// ---- the window of step k of us.split: outer loop col0 (bounded by h), inner loop row0 (bounded by w) -------------------------
struct Window { int row0, col0; bool full; };
__device__ __forceinline__ Window window_of(int k0, int n_inner, int window, int h, int w) {
  Window q;
  q.row0 = (k0 % n_inner) * window;
  q.col0 = (k0 / n_inner) * window;
  q.full = q.row0 + window <= h && q.col0 + window <= w;
  return q;
}

// ---- 2. census ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum_i(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

template <int V>
__global__ __launch_bounds__(CENSUS_THREADS) void census_kernel(const unsigned short* __restrict__ lst_raw,
                                                                const unsigned char* __restrict__ qc, const short* __restrict__ nir,
                                                                const short* __restrict__ red, int* __restrict__ counts, int h, int w,
                                                                int window, int n_inner, int qc_mode) {
  typedef typename Vec<V>::type VT;
  __shared__ int part[2][NWAVE];
  const int k0 = blockIdx.x, tid = threadIdx.x;
  const Window q = window_of(k0, n_inner, window, h, w);
  if (!q.full) {                                                      // (uniform over the workgroup)
    if (tid < 2) counts[2 * k0 + tid] = -1;
    return;
  }
  int bad = 0, zden = 0;
  for (int e = tid; e < window * window; e += CENSUS_THREADS) {
    const size_t p = (size_t)(q.row0 + e / window) * w + q.col0 + e % window;
    bool b = lst_raw[p] == 0;
    if (qc_mode == 1) b = b || (qc[p] & 1);
    bad += b ? 1 : 0;
  }
  const int fw = 4 * window, per_row = fw / V;
  const size_t fine_w = 4 * (size_t)w;
  for (int e = tid; e < fw * per_row; e += CENSUS_THREADS) {
    const size_t p = (size_t)(4 * q.row0 + e / per_row) * fine_w + 4 * q.col0 + (e % per_row) * V;
    const VT a = *reinterpret_cast<const VT*>(nir + p), b = *reinterpret_cast<const VT*>(red + p);
#pragma unroll
    for (int i = 0; i < V; ++i) zden += den_of(a[i], b[i]) == 0.0f ? 1 : 0;
  }
  bad = wave_sum_i(bad);
  zden = wave_sum_i(zden);
  if ((tid & 63) == 0) { part[0][tid >> 6] = bad; part[1][tid >> 6] = zden; }
  __syncthreads();
  if (tid < 2) {
    int s = 0;
    for (int i = 0; i < NWAVE; ++i) s += part[tid][i];
    counts[2 * k0 + tid] = s;
  }
}

// ---- 3. select ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void select_kernel(const int* __restrict__ counts, int* __restrict__ index,
                                                    int* __restrict__ n_accepted, int nwin, int n_inner, int window, int max_bad,
                                                    int cap) {
  const int lane = threadIdx.x;
  int running = 0;
  for (int base = 0; base < nwin; base += 64) {
    const int k0 = base + lane;
    bool acc = false;
    if (k0 < nwin) {
      const int bad = counts[2 * k0], zden = counts[2 * k0 + 1];
      acc = bad >= 0 && bad <= max_bad && zden == 0;
    }
    const unsigned long long m = __ballot(acc);
    const int pos = running + __popcll(m & ((1ull << lane) - 1ull));
    if (acc && pos < cap) {
      index[3 * pos] = k0 + 1;
      index[3 * pos + 1] = (k0 % n_inner) * window;
      index[3 * pos + 2] = (k0 / n_inner) * window;
    }
    running += __popcll(m);
  }
  if (lane == 0) *n_accepted = running < cap ? running : cap;
}

// ---- 4. gather ----------------------------------------------------------------------------------------------------------------
struct Mom { double n, mean, m2; };

// Chan, Golub & LeVeque: the moments of the union of two samples.  An empty side leaves the other untouched.
__device__ __forceinline__ Mom merge(Mom a, Mom b) {
  if (b.n == 0.0) return a;
  if (a.n == 0.0) return b;
  Mom r;
  r.n = a.n + b.n;
  const double d = b.mean - a.mean, f = b.n / r.n;
  r.mean = a.mean + d * f;
  r.m2 = a.m2 + b.m2 + d * d * a.n * f;
  return r;
}

template <int N> __device__ __forceinline__ Mom chunk_moments(const float (&x)[N]) {       // two passes in registers
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) s += (double)x[i];
  Mom c;
  c.n = (double)N;
  c.mean = s / (double)N;
  c.m2 = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) { const double d = (double)x[i] - c.mean; c.m2 += d * d; }
  return c;
}

__device__ __forceinline__ Mom wave_merge(Mom a) {                    // lane 0 gets the wave's moments, always in the same tree
  for (int o = 32; o > 0; o >>= 1) {
    Mom b;
    b.n = __shfl_down(a.n, o, 64);
    b.mean = __shfl_down(a.mean, o, 64);
    b.m2 = __shfl_down(a.m2, o, 64);
    a = merge(a, b);
  }
  return a;
}

template <int V>
__global__ __launch_bounds__(CENSUS_THREADS) void gather_kernel(const unsigned short* __restrict__ lst_raw, const short* __restrict__ nir,
                                                                const short* __restrict__ red, const int* __restrict__ index,
                                                                const int* __restrict__ n_accepted, float* __restrict__ lst,
                                                                float* __restrict__ ndvi, double* __restrict__ moments, int h, int w,
                                                                int window) {
  typedef typename Vec<V>::type VT;
  __shared__ Mom part[2][NWAVE];
  __shared__ float ext[2][NWAVE];
  const int i = blockIdx.x, tid = threadIdx.x;
  if (i >= *n_accepted) return;
  const int row0 = index[3 * i + 1], col0 = index[3 * i + 2];
  if (row0 < 0 || col0 < 0 || row0 + window > h || col0 + window > w) return;     // never written by sifsrp_select
  const int ww = window * window;

  Mom ml = {0.0, 0.0, 0.0};
  float lo = INFINITY, hi = -INFINITY;
  float* lout = lst + (size_t)i * ww;
  for (int e = tid; e < ww; e += CENSUS_THREADS) {
    const float v = LST_SCALE * (float)lst_raw[(size_t)(row0 + e / window) * w + col0 + e % window];
    lout[e] = v;
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
    const Mom one = {1.0, (double)v, 0.0};
    ml = merge(ml, one);
  }

  Mom mn = {0.0, 0.0, 0.0};
  const int fw = 4 * window, per_row = fw / V;
  const size_t fine_w = 4 * (size_t)w;
  float* nout = ndvi + (size_t)i * fw * fw;
  for (int e = tid; e < fw * per_row; e += CENSUS_THREADS) {
    const int r = e / per_row, c = (e % per_row) * V;
    const size_t p = (size_t)(4 * row0 + r) * fine_w + 4 * col0 + c;
    const VT a = *reinterpret_cast<const VT*>(nir + p), b = *reinterpret_cast<const VT*>(red + p);
    float x[V];
#pragma unroll
    for (int j = 0; j < V; ++j) x[j] = clip1(ndvi_of(a[j], b[j]));
#pragma unroll
    for (int j = 0; j < V; j += 4) st4(nout + (size_t)r * fw + c + j, make_float4(x[j], x[j + 1], x[j + 2], x[j + 3]));
    mn = merge(mn, chunk_moments<V>(x));
  }

  ml = wave_merge(ml);
  mn = wave_merge(mn);
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_down(lo, o, 64));
    hi = fmaxf(hi, __shfl_down(hi, o, 64));
  }
  if ((tid & 63) == 0) {
    part[0][tid >> 6] = ml; part[1][tid >> 6] = mn;
    ext[0][tid >> 6] = lo; ext[1][tid >> 6] = hi;
  }
  __syncthreads();
  if (tid == 0) {
    for (int v = 1; v < NWAVE; ++v) {                                 // in wave order
      ml = merge(ml, part[0][v]);
      mn = merge(mn, part[1][v]);
      lo = fminf(lo, ext[0][v]);
      hi = fmaxf(hi, ext[1][v]);
    }
    double* m = moments + 8 * (size_t)i;
    m[0] = ml.n; m[1] = ml.mean; m[2] = ml.m2; m[3] = (double)lo; m[4] = (double)hi;
    m[5] = mn.mean; m[6] = mn.m2; m[7] = 0.0;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
int ceil_div(int a, int b) { return (a + b - 1) / b; }
bool window_ok(int h, int w, int window) { return window >= 4 && window % 4 == 0 && h >= window && w >= window && h <= 16384 && w <= 16384; }
int n_full(int h, int w, int window) {
  const int no = ceil_div(h, window), ni = ceil_div(w, window);
  return (no < w / window ? no : w / window) * (ni < h / window ? ni : h / window);
}
// 8 int16 per access when both fine rasters and every window row start on 16 bytes, else 4; 0: not even 8-byte aligned
int fine_vec(const short* nir, const short* red, int w) {
  if (w % 2 == 0 && aligned(nir, 16) && aligned(red, 16)) return 8;
  return aligned(nir, 8) && aligned(red, 8) ? 4 : 0;
}

}  // namespace

int sifsrp_decode(const unsigned short* lst_raw, const short* nir, const short* red, float* lst_k, float* ndvi, int h, int w,
                  int clip, void* stream) {
  if (!lst_raw || !nir || !red || !lst_k || !ndvi || (clip != 0 && clip != 1)) return SIFSR_ERR_ARG;
  if (h < 1 || w < 1 || h > 16384 || w > 16384) return SIFSR_ERR_SHAPE;
  if (!aligned(lst_raw, 16) || !aligned(nir, 16) || !aligned(red, 16) || !aligned(lst_k, 16) || !aligned(ndvi, 16)) return SIFSR_ERR_ARG;
  const size_t n = (size_t)h * w, nf = 16 * n;
  hipLaunchKernelGGL(decode_lst_kernel, dim3((unsigned)((n / 8 + 256) / 256)), dim3(256), 0, (hipStream_t)stream, lst_raw, lst_k, n);
  SIFSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(decode_ndvi_kernel, dim3((unsigned)((nf / 8 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nir, red, ndvi, nf,
                     clip);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrp_census(const unsigned short* lst_raw, const unsigned char* qc, const short* nir, const short* red, int* counts, int h,
                  int w, int window, int qc_mode, void* stream) {
  if (!lst_raw || !nir || !red || !counts || (qc_mode != 0 && qc_mode != 1) || (qc_mode == 1 && !qc)) return SIFSR_ERR_ARG;
  if (!window_ok(h, w, window)) return SIFSR_ERR_SHAPE;
  const int v = fine_vec(nir, red, w);
  if (!v) return SIFSR_ERR_ARG;
  const int n_inner = ceil_div(w, window), nwin = ceil_div(h, window) * n_inner;
  if (v == 8)
    hipLaunchKernelGGL(census_kernel<8>, dim3(nwin), dim3(CENSUS_THREADS), 0, (hipStream_t)stream, lst_raw, qc, nir, red, counts, h,
                       w, window, n_inner, qc_mode);
  else
    hipLaunchKernelGGL(census_kernel<4>, dim3(nwin), dim3(CENSUS_THREADS), 0, (hipStream_t)stream, lst_raw, qc, nir, red, counts, h,
                       w, window, n_inner, qc_mode);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrp_select(const int* counts, int* index, int* n_accepted, int h, int w, int window, int max_bad, int cap, void* stream) {
  if (!counts || !index || !n_accepted || max_bad < 0) return SIFSR_ERR_ARG;
  if (!window_ok(h, w, window) || cap < n_full(h, w, window)) return SIFSR_ERR_SHAPE;
  const int n_inner = ceil_div(w, window), nwin = ceil_div(h, window) * n_inner;
  hipLaunchKernelGGL(select_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, counts, index, n_accepted, nwin, n_inner, window,
                     max_bad, cap);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrp_gather(const unsigned short* lst_raw, const short* nir, const short* red, const int* index, const int* n_accepted,
                  float* lst, float* ndvi, double* moments, int h, int w, int window, int cap, void* stream) {
  if (!lst_raw || !nir || !red || !index || !n_accepted || !lst || !ndvi || !moments) return SIFSR_ERR_ARG;
  if (!window_ok(h, w, window) || cap < n_full(h, w, window)) return SIFSR_ERR_SHAPE;
  const int v = fine_vec(nir, red, w);
  if (!v || !aligned(ndvi, 16)) return SIFSR_ERR_ARG;
  const int blocks = n_full(h, w, window);                            // n_accepted lives on the device: the rest exit at once
  if (v == 8)
    hipLaunchKernelGGL(gather_kernel<8>, dim3(blocks), dim3(CENSUS_THREADS), 0, (hipStream_t)stream, lst_raw, nir, red, index,
                       n_accepted, lst, ndvi, moments, h, w, window);
  else
    hipLaunchKernelGGL(gather_kernel<4>, dim3(blocks), dim3(CENSUS_THREADS), 0, (hipStream_t)stream, lst_raw, nir, red, index,
                       n_accepted, lst, ndvi, moments, h, w, window);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}
