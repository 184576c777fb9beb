// From the raw integer rasters of a MODIS granule to training patches and their statistics (C ABI:
// include/sifsr_products.h): reference process_modis.py:38-335 and the statistics half of data_preparation.py.
//
//  * decode_lst_kernel / decode_ndvi_kernel   eight pixels per thread, 16-byte loads and stores (a scalar tail for LST)
//  * census_kernel    one workgroup of 16 waves per window of the reference's generator: bad LST pixels and zero denominators
//  * select_kernel    one wavefront: ballot + prefix population count, the accepted windows in the order of k
//  * gather_kernel    one workgroup per accepted window: both patches and one row of float64 moments
// All four are one pass over HBM.  No atomics: integer counts are exact whatever the route, the moments merge in a fixed order.
// The float32 algebra, the window order and the moments are products_common.h, shared with rproducts.hip.
#include "../../include/sifsr_products.h"

#include "products_common.h"

namespace {

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

// ---- 2. census ----------------------------------------------------------------------------------------------------------------
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
bool window_ok(int h, int w, int window) { return window >= 4 && window % 4 == 0 && h >= window && w >= window && h <= 16384 && w <= 16384; }
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
