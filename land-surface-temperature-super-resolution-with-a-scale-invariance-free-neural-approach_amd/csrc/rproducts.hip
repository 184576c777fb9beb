// Patch mining at any ratio hr / window (C ABI and every definition: include/sifsr_rproducts.h): the kernels of
// products.hip with the fine window side as an argument, and the two mask helpers the epoch loop at a ratio needs.
//
//  * rdecode_lst_kernel / rdecode_ndvi_kernel   eight pixels per thread over the flat rasters, a scalar tail
//  * rcensus_kernel   one workgroup of 16 waves per window of the reference's generator: bad LST pixels, zero denominators of the
//                     hr x hr fine window
//  * rgather_kernel   one workgroup per accepted window: both patches and one row of float64 moments
//  * patch_counts_kernel   one workgroup per patch: {valid cells, HR pixels under them}, the row sifsrq_valid_counts gives
//  * expand_valid_kernel   the HR mask under an LR mask, four bytes per thread
// The selection between census and gather is sifsrp_select: it reads the counts and the LST geometry alone.
//
// A thread always works on 8 consecutive int16 of a fine row (hr % 8 == 0) and loads them as 1 x 16, 2 x 8 or 8 x 2 bytes
// (load8<V>, V picked on the host from the alignment of the bases and of the row pitch); everything after the load is the same
// code, and the moments merge in the order of products.hip's 16-byte path (products_common.h), so the three paths and, at
// hr == 4 window, the two families give the same bits.  No atomics.
#include "../../include/sifsr_rproducts.h"

#include "../../include/sifsr_degrade.h"
#include "../../include/sifsr_ratio.h"
#include "products_common.h"

namespace {

constexpr int MAX_LST_SIDE = 16384, MAX_RATIO = 16;
typedef Vec<8>::type S8;

template <int V> __device__ __forceinline__ S8 load8(const short* p);
template <> __device__ __forceinline__ S8 load8<8>(const short* p) { return *reinterpret_cast<const S8*>(p); }
template <> __device__ __forceinline__ S8 load8<4>(const short* p) {
  typedef Vec<4>::type S4;
  const S4 a = *reinterpret_cast<const S4*>(p), b = *reinterpret_cast<const S4*>(p + 4);
  S8 v;
  v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
  return v;
}
template <> __device__ __forceinline__ S8 load8<1>(const short* p) {
  S8 v;
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = p[i];
  return v;
}

// ---- 1. decode ------------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void rdecode_lst_kernel(const unsigned short* __restrict__ raw, float* __restrict__ out, size_t n) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, n8 = n / 8;
  if (g < n8) {
    const S8 v = load8<V>(reinterpret_cast<const short*>(raw) + 8 * g);
    float o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = LST_SCALE * (float)(unsigned short)v[i];
    st4(out + 8 * g, make_float4(o[0], o[1], o[2], o[3]));
    st4(out + 8 * g + 4, make_float4(o[4], o[5], o[6], o[7]));
  }
  const size_t t = 8 * n8 + g;                                        // the tail: fewer than 8 pixels, the first threads
  if (g < 8 && t < n) out[t] = LST_SCALE * (float)raw[t];
}

template <int V>
__global__ __launch_bounds__(256) void rdecode_ndvi_kernel(const short* __restrict__ nir, const short* __restrict__ red,
                                                           float* __restrict__ out, size_t n, int clip) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, n8 = n / 8;
  if (g < n8) {
    const S8 a = load8<V>(nir + 8 * g), b = load8<V>(red + 8 * g);
    float o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      o[i] = ndvi_of(a[i], b[i]);
      if (clip) o[i] = clip1(o[i]);
    }
    st4(out + 8 * g, make_float4(o[0], o[1], o[2], o[3]));
    st4(out + 8 * g + 4, make_float4(o[4], o[5], o[6], o[7]));
  }
  const size_t t = 8 * n8 + g;                                        // fh fw need not be a multiple of 8
  if (g < 8 && t < n) {
    const float v = ndvi_of(nir[t], red[t]);
    out[t] = clip ? clip1(v) : v;
  }
}

// ---- 2. census ----------------------------------------------------------------------------------------------------------------
// fw: the width of the fine rasters; the fine window of LST window (row0, col0) starts at ((row0 / window) hr, (col0 / window) hr)
template <int V>
__global__ __launch_bounds__(CENSUS_THREADS) void rcensus_kernel(const unsigned short* __restrict__ lst_raw,
                                                                 const unsigned char* __restrict__ qc, const short* __restrict__ nir,
                                                                 const short* __restrict__ red, int* __restrict__ counts, int h, int w,
                                                                 int fw, int window, int hr, int n_inner, int qc_mode) {
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
  const int per_row = hr / 8, fr0 = (q.row0 / window) * hr, fc0 = (q.col0 / window) * hr;
  for (int e = tid; e < hr * per_row; e += CENSUS_THREADS) {
    const size_t p = (size_t)(fr0 + e / per_row) * fw + fc0 + (e % per_row) * 8;
    const S8 a = load8<V>(nir + p), b = load8<V>(red + p);
#pragma unroll
    for (int i = 0; i < 8; ++i) zden += den_of(a[i], b[i]) == 0.0f ? 1 : 0;
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

// ---- 3. gather ----------------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(CENSUS_THREADS) void rgather_kernel(const unsigned short* __restrict__ lst_raw, const short* __restrict__ nir,
                                                                 const short* __restrict__ red, const int* __restrict__ index,
                                                                 const int* __restrict__ n_accepted, float* __restrict__ lst,
                                                                 float* __restrict__ ndvi, double* __restrict__ moments, int h, int w,
                                                                 int fw, int window, int hr) {
  __shared__ Mom part[2][NWAVE];
  __shared__ float ext[2][NWAVE];
  const int i = blockIdx.x, tid = threadIdx.x;
  if (i >= *n_accepted) return;
  const int row0 = index[3 * i + 1], col0 = index[3 * i + 2];
  if (row0 < 0 || col0 < 0 || row0 + window > h || col0 + window > w || row0 % window || col0 % window) return;   // never written by sifsrp_select
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
  const int per_row = hr / 8, fr0 = (row0 / window) * hr, fc0 = (col0 / window) * hr;
  float* nout = ndvi + (size_t)i * hr * hr;
  for (int e = tid; e < hr * per_row; e += CENSUS_THREADS) {
    const int r = e / per_row, c = (e % per_row) * 8;
    const size_t p = (size_t)(fr0 + r) * fw + fc0 + c;
    const S8 a = load8<V>(nir + p), b = load8<V>(red + p);
    float x[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = clip1(ndvi_of(a[j], b[j]));
#pragma unroll
    for (int j = 0; j < 8; j += 4) st4(nout + (size_t)r * hr + c + j, make_float4(x[j], x[j + 1], x[j + 2], x[j + 3]));
    mn = merge(mn, chunk_moments<8>(x));
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

// ---- 4. the counts of a patch -------------------------------------------------------------------------------------------------
// cell i of an axis holds the HR pixels Y with Y window / hr == i: ceil((i + 1) hr / window) - ceil(i hr / window) of them
__device__ __forceinline__ int cell_pixels(int i, int window, int hr) {
  return ((i + 1) * hr + window - 1) / window - (i * hr + window - 1) / window;
}

__global__ __launch_bounds__(256) void patch_counts_kernel(const unsigned char* __restrict__ valid, long long* __restrict__ counts,
                                                           int window, int hr) {
  __shared__ int part[2][4];
  const int tid = threadIdx.x, ww = window * window;
  const unsigned char* v = valid + (size_t)blockIdx.x * ww;
  int c1 = 0, c2 = 0;                                                 // at most hr * hr <= 2^28
  for (int e = tid; e < ww; e += 256) {
    if (v[e] == 0) continue;
    c1 += 1;
    c2 += cell_pixels(e / window, window, hr) * cell_pixels(e % window, window, hr);
  }
  c1 = wave_sum_i(c1);
  c2 = wave_sum_i(c2);
  if ((tid & 63) == 0) { part[0][tid >> 6] = c1; part[1][tid >> 6] = c2; }
  __syncthreads();
  if (tid < 2) {
    long long s = 0;
    for (int i = 0; i < 4; ++i) s += part[tid][i];
    counts[2 * (size_t)blockIdx.x + tid] = s;
  }
}

// ---- 5. the HR mask under an LR mask ------------------------------------------------------------------------------------------
// a thread owns 4 consecutive bytes of an output row; `wide`: W % 4 == 0 and out on 4 bytes, one 4-byte store
__global__ __launch_bounds__(256) void expand_valid_kernel(const unsigned char* __restrict__ valid, unsigned char* __restrict__ out,
                                                           int h, int w, int H, int W, long long n4, int wide) {
  const int per_row = (W + 3) / 4;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n4; t += (long long)gridDim.x * 256) {
    const long long row = t / per_row;                               // b * H + Y
    const int x0 = (int)(t % per_row) * 4, Y = (int)(row % H);
    const unsigned char* src = valid + ((row / H) * h + (long long)Y * h / H) * w;
    unsigned char* dst = out + row * W + x0;
    unsigned pack = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int X = x0 + k;
      if (X < W) {
        const unsigned b = src[(long long)X * w / W] != 0 ? 1u : 0u;
        if (wide) pack |= b << (8 * k); else dst[k] = (unsigned char)b;
      }
    }
    if (wide) *reinterpret_cast<unsigned*>(dst) = pack;
  }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
int gcd_of(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }

// the trainable-pair rule of the header
bool trainable(int window, int hr) {
  int g6[6], oh = 0, ow = 0;
  if (sifsrr_geometry(window, window, window, hr, 0, 0, g6) != SIFSR_OK) return false;
  if (hr > 8 * window) return false;
  if (sifsrs_out_shape(hr, hr, (double)hr / (double)window, 0, 1, &oh, &ow) != SIFSR_OK) return false;
  return oh == window && ow == window;
}

// the raster rules: -> the width of the fine rasters, or 0
int fine_width(int h, int w, int window, int hr) {
  if (!trainable(window, hr)) return 0;
  const int g = gcd_of(hr, window), p = hr / g, q = window / g;
  if (h < window || w < window || h > MAX_LST_SIDE || w > MAX_LST_SIDE || h % q || w % q) return 0;
  return w / q * p;
}

// int16 per access: 8 when both fine rasters and every row start on 16 bytes, 4 when on 8 bytes, else 1
int fine_vec(const short* nir, const short* red, int fw) {
  if (fw % 8 == 0 && aligned(nir, 16) && aligned(red, 16)) return 8;
  if (fw % 4 == 0 && aligned(nir, 8) && aligned(red, 8)) return 4;
  return 1;
}

}  // namespace

int sifsrn_decode(const unsigned short* lst_raw, const short* nir, const short* red, float* lst_k, float* ndvi, int h, int w, int fh,
                  int fw, int clip, void* stream) {
  if (!lst_raw || !nir || !red || !lst_k || !ndvi || (clip != 0 && clip != 1)) return SIFSR_ERR_ARG;
  if (h < 1 || w < 1 || h > MAX_LST_SIDE || w > MAX_LST_SIDE || fh < h || fw < w || (long long)fh * w != (long long)fw * h ||
      (long long)fh > (long long)MAX_RATIO * h)
    return SIFSR_ERR_SHAPE;
  if (!aligned(lst_raw, 2) || !aligned(nir, 2) || !aligned(red, 2) || !aligned(lst_k, 16) || !aligned(ndvi, 16)) return SIFSR_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)h * w, nf = (size_t)fh * fw;
  const dim3 gl((unsigned)((n / 8 + 256) / 256)), gf((unsigned)((nf / 8 + 256) / 256));
  const int vl = aligned(lst_raw, 16) ? 8 : aligned(lst_raw, 8) ? 4 : 1;
  if (vl == 8) hipLaunchKernelGGL(rdecode_lst_kernel<8>, gl, dim3(256), 0, s, lst_raw, lst_k, n);
  else if (vl == 4) hipLaunchKernelGGL(rdecode_lst_kernel<4>, gl, dim3(256), 0, s, lst_raw, lst_k, n);
  else hipLaunchKernelGGL(rdecode_lst_kernel<1>, gl, dim3(256), 0, s, lst_raw, lst_k, n);
  SIFSR_LAUNCH_CHECK();
  const int v = fine_vec(nir, red, 8);                               // flat: the bases alone
  if (v == 8) hipLaunchKernelGGL(rdecode_ndvi_kernel<8>, gf, dim3(256), 0, s, nir, red, ndvi, nf, clip);
  else if (v == 4) hipLaunchKernelGGL(rdecode_ndvi_kernel<4>, gf, dim3(256), 0, s, nir, red, ndvi, nf, clip);
  else hipLaunchKernelGGL(rdecode_ndvi_kernel<1>, gf, dim3(256), 0, s, nir, red, ndvi, nf, clip);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrn_census(const unsigned short* lst_raw, const unsigned char* qc, const short* nir, const short* red, int* counts, int h,
                  int w, int window, int hr, int qc_mode, void* stream) {
  if (!lst_raw || !nir || !red || !counts || (qc_mode != 0 && qc_mode != 1) || (qc_mode == 1 && !qc)) return SIFSR_ERR_ARG;
  const int fw = fine_width(h, w, window, hr);
  if (!fw) return SIFSR_ERR_SHAPE;
  if (!aligned(lst_raw, 2) || !aligned(nir, 2) || !aligned(red, 2) || !aligned(counts, 4)) return SIFSR_ERR_ARG;
  const int n_inner = ceil_div(w, window), nwin = ceil_div(h, window) * n_inner;
  const int v = fine_vec(nir, red, fw);
  const dim3 grid(nwin), block(CENSUS_THREADS);
  hipStream_t s = (hipStream_t)stream;
  if (v == 8) hipLaunchKernelGGL(rcensus_kernel<8>, grid, block, 0, s, lst_raw, qc, nir, red, counts, h, w, fw, window, hr, n_inner, qc_mode);
  else if (v == 4) hipLaunchKernelGGL(rcensus_kernel<4>, grid, block, 0, s, lst_raw, qc, nir, red, counts, h, w, fw, window, hr, n_inner, qc_mode);
  else hipLaunchKernelGGL(rcensus_kernel<1>, grid, block, 0, s, lst_raw, qc, nir, red, counts, h, w, fw, window, hr, n_inner, qc_mode);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrn_gather(const unsigned short* lst_raw, const short* nir, const short* red, const int* index, const int* n_accepted,
                  float* lst, float* ndvi, double* moments, int h, int w, int window, int hr, int cap, void* stream) {
  if (!lst_raw || !nir || !red || !index || !n_accepted || !lst || !ndvi || !moments) return SIFSR_ERR_ARG;
  const int fw = fine_width(h, w, window, hr);
  if (!fw || cap < n_full(h, w, window)) return SIFSR_ERR_SHAPE;
  if (!aligned(lst_raw, 2) || !aligned(nir, 2) || !aligned(red, 2) || !aligned(index, 4) || !aligned(n_accepted, 4) ||
      !aligned(lst, 16) || !aligned(ndvi, 16) || !aligned(moments, 8))
    return SIFSR_ERR_ARG;
  const int v = fine_vec(nir, red, fw);
  const dim3 grid(n_full(h, w, window)), block(CENSUS_THREADS);     // n_accepted lives on the device: the rest exit at once
  hipStream_t s = (hipStream_t)stream;
  if (v == 8) hipLaunchKernelGGL(rgather_kernel<8>, grid, block, 0, s, lst_raw, nir, red, index, n_accepted, lst, ndvi, moments, h, w, fw, window, hr);
  else if (v == 4) hipLaunchKernelGGL(rgather_kernel<4>, grid, block, 0, s, lst_raw, nir, red, index, n_accepted, lst, ndvi, moments, h, w, fw, window, hr);
  else hipLaunchKernelGGL(rgather_kernel<1>, grid, block, 0, s, lst_raw, nir, red, index, n_accepted, lst, ndvi, moments, h, w, fw, window, hr);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrn_patch_counts(const unsigned char* valid, long long* counts, int N, int window, int hr, void* stream) {
  if (!valid || !counts || !aligned(counts, 8)) return SIFSR_ERR_ARG;
  if (N < 1 || window < 1 || hr < window || hr > MAX_LST_SIDE) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(patch_counts_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, valid, counts, window, hr);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrn_expand_valid(const unsigned char* valid, unsigned char* out, int B, int h, int w, int H, int W, void* stream) {
  if (!valid || !out) return SIFSR_ERR_ARG;
  if (B < 1 || B > 65535 || h < 1 || w < 1 || h > H || w > W || H > MAX_LST_SIDE || W > MAX_LST_SIDE) return SIFSR_ERR_SHAPE;
  const long long n4 = (long long)B * H * ((W + 3) / 4), blocks = (n4 + 255) / 256;
  hipLaunchKernelGGL(expand_valid_kernel, dim3((unsigned)(blocks > (1 << 20) ? (1 << 20) : blocks)), dim3(256), 0, (hipStream_t)stream,
                     valid, out, h, w, H, W, n4, (W % 4 == 0 && aligned(out, 4)) ? 1 : 0);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}
