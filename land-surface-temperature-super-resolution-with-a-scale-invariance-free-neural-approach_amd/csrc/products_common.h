// What the two patch-mining families share (products.hip: x4, include/sifsr_products.h; rproducts.hip: any ratio,
// include/sifsr_rproducts.h): the float32 algebra of NDVI, the window of step k of the reference's generator, the moments of a
// patch and the fixed order in which they merge.  One definition, so that the two families give the same bits where they meet.
//
// The float32 algebra is numpy's, operation by operation (0.0001f * raw, then the difference, the sum and the quotient); contraction
// into FMAs is off in every file that includes this one so that nir - red and nir + red round exactly as there.  The quotient is
// formed in float64 and rounded once: for binary32 operands that IS the correctly rounded float32 quotient (53 >= 2 * 24 + 2),
// whatever the division mode the file is compiled with.
#pragma once
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

// ---- the window of step k of us.split: outer loop col0 (bounded by h), inner loop row0 (bounded by w) -------------------------
struct Window { int row0, col0; bool full; };
__device__ __forceinline__ Window window_of(int k0, int n_inner, int window, int h, int w) {
  Window q;
  q.row0 = (k0 % n_inner) * window;
  q.col0 = (k0 / n_inner) * window;
  q.full = q.row0 + window <= h && q.col0 + window <= w;
  return q;
}

__device__ __forceinline__ int wave_sum_i(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// ---- the moments of a patch ---------------------------------------------------------------------------------------------------
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

// ---- host side ----------------------------------------------------------------------------------------------------------------
bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
int ceil_div(int a, int b) { return (a + b - 1) / b; }
int n_full(int h, int w, int window) {
  const int no = ceil_div(h, window), ni = ceil_div(w, window);
  return (no < w / window ? no : w / window) * (ni < h / window ? ni : h / window);
}

}  // namespace
