// The weight tables of the sensor model, shared by csrc/degrade.hip (include/sifsr_degrade.h, include/sifsr_sensor.h) and
// csrc/rloss.hip (include/sifsr_rloss.h): ONE place forms the weights of R (degrade_table_kernel), of L (lowpass_table_kernel),
// the runs of outputs over an input pixel (range_kernel), the Gaussian taps (psf_of) and the geometry of an axis (axis_of).
// Every translation unit that includes this header gets its own copy of the kernels (anonymous namespace).
#pragma once
#include <math.h>

#include "common.h"

namespace {

constexpr int MAX_HW = 16;
constexpr int MAX_SIDE = 16384;
constexpr int MAX_BATCH = 65535;

struct Axis {
  int n, n_pad, count, cut;    // original length, padded length, outputs after the crop, outputs cut on each side
};

struct Psf {
  double g[2 * MAX_HW + 1];
  int hw;
  float scale;                 // (float)(1.0 / (1.0 / factor))
};

// the original pixels that the blurred entries q_lo .. q_hi read, after the reflection: [*lo, *hi]
__device__ __forceinline__ void fold_range(int q_lo, int q_hi, int hw, int n, int n_pad, int* lo, int* hi) {
  const int i_lo = max(q_lo - hw, 0) - hw;                // >= -hw, <= n - 1
  const int i_hi = min(q_hi + hw, n_pad - 1) - hw;        // >= 0,   <= n - 1 + hw
  int a = max(i_lo, 0), b = min(i_hi, n - 1);            // read directly: never empty
  if (i_lo < 0) { a = 0; b = max(b, -i_lo); }             // mirrored at the low edge: 1 .. -i_lo (hw <= n - 1)
  if (i_hi >= n) a = min(a, 2 * (n - 1) - i_hi);          // mirrored at the high edge: 2 (n - 1) - i_hi .. n - 2, and b = n - 1
  *lo = a;
  *hi = b;
}

__global__ __launch_bounds__(256) void degrade_table_kernel(const Psf p, const Axis ay, const Axis ax, double* __restrict__ wy,
                                                            double* __restrict__ wx, int4* __restrict__ my, int4* __restrict__ mx) {
#pragma clang fp contract(off)
  const bool rows = blockIdx.y == 0;
  const Axis A = rows ? ay : ax;
  const int hw = p.hw, K = 2 * hw + 4, n = A.n;
  const int e = blockIdx.x * 256 + threadIdx.x;           // the index of the weight in its table, either layout
  if (e >= A.count * K) return;
  const int o = rows ? e / K : e % A.count, k = rows ? e % K : e / A.count;
  // the source coordinate as upsample_bicubic2d forms it, every step rounded to fp32
  const float s = __fsub_rn(__fmul_rn(p.scale, __fadd_rn((float)(o + A.cut), 0.5f)), 0.5f);
  const float fl = floorf(s);
  const double t = (double)__fsub_rn(s, fl);
  const int f = (int)fl;
  const double a = -0.75, u = 1.0 - t;
  double c[4];
  c[0] = ((a * (t + 1.0) - 5.0 * a) * (t + 1.0) + 8.0 * a) * (t + 1.0) - 4.0 * a;
  c[1] = ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0;
  c[2] = ((a + 2.0) * u - (a + 3.0)) * u * u + 1.0;
  c[3] = ((a * (u + 1.0) - 5.0 * a) * (u + 1.0) + 8.0 * a) * (u + 1.0) - 4.0 * a;
  int q[4], q_lo = A.n_pad, q_hi = -1, ring = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    q[i] = clampi(f - 1 + i, 0, A.n_pad - 1);
    if (c[i] != 0.0) {
      q_lo = min(q_lo, q[i]);
      q_hi = max(q_hi, q[i]);
      ring |= (q[i] < hw || q[i] > A.n_pad - 1 - hw) ? 1 : 0;
    }
  }
  int start, last, lo, hi;
  fold_range(q[0], q[3], hw, n, A.n_pad, &start, &last);  // last - start < K: the window holds every weight
  fold_range(q_lo, q_hi, hw, n, A.n_pad, &lo, &hi);       // c[1] and c[2] are never both 0: q_lo <= q_hi
  (void)last;
  const int j = start + k;
  double w = 0.0;
  if (j < n) {
    // the padded entries that hold pixel j: itself, its mirror at the low edge, its mirror at the high edge
    const int cand[3] = {j + hw, hw - j, 2 * (n - 1) - j + hw};
    const bool use[3] = {true, j >= 1 && j <= hw, j <= n - 2 && n - 1 - j <= hw};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      if (!use[m]) continue;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int d = cand[m] - q[i];
        if (d >= -hw && d <= hw) w += c[i] * p.g[d + hw];
      }
    }
  }
  (rows ? wy : wx)[e] = w;
  if (k == 0) (rows ? my : mx)[o] = make_int4(start, lo, hi, ring);
}

// ---- the differentiable half (include/sifsr_sensor.h) ----
// one thread per weight of an axis, in the layouts of degrade_table_kernel with K = 2 hw + 1: row weights [output][tap], column
// weights [tap][output]; tap k of output o is pixel max(0, o - hw) + k.  A.count == A.n.
__global__ __launch_bounds__(256) void lowpass_table_kernel(const Psf p, const Axis ay, const Axis ax, double* __restrict__ wy,
                                                            double* __restrict__ wx, int4* __restrict__ my, int4* __restrict__ mx) {
#pragma clang fp contract(off)
  const bool rows = blockIdx.y == 0;
  const Axis A = rows ? ay : ax;
  const int hw = p.hw, K = 2 * hw + 1, n = A.n;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n * K) return;
  const int o = rows ? e / K : e % n, k = rows ? e % K : e / n;
  const int start = max(o - hw, 0), j = start + k;
  double w = 0.0;
  if (j < n) {
    // the reflected positions that hold pixel j: itself, its mirror at the low edge, its mirror at the high edge (hw <= n - 1)
    const int cand[3] = {j, -j, 2 * (n - 1) - j};
    const bool use[3] = {true, j >= 1, j <= n - 2};
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const int d = cand[m] - o;
      if (use[m] && d >= -hw && d <= hw) w += p.g[d + hw];
    }
  }
  (rows ? wy : wx)[e] = w;
  if (k == 0) (rows ? my : mx)[o] = make_int4(start, start, min(o + hw, n - 1), 0);
}

// one thread per input index of an axis (blockIdx.y: 0 rows, 1 columns): the outputs o with lo(o) <= i <= hi(o).  lo and hi are
// non-decreasing in o, so these are [first o with hi(o) >= i, last o with lo(o) <= i]; the run is empty when the first is past the
// last.  Whatever the table holds, 0 <= first <= count and -1 <= last <= count - 1.
__global__ __launch_bounds__(256) void range_kernel(const int4* __restrict__ my, const int4* __restrict__ mx, int2* __restrict__ ry,
                                                    int2* __restrict__ rx, int h, int w, int oh, int ow) {
  const bool rows = blockIdx.y == 0;
  const int n = rows ? h : w, count = rows ? oh : ow;
  const int4* m = rows ? my : mx;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int a = 0, b = count;                                    // first o in [0, count] with hi(o) >= i
  while (a < b) {
    const int c = (a + b) >> 1;
    if (m[c].z >= i) b = c; else a = c + 1;
  }
  const int first = a;
  a = 0, b = count;                                        // first o in [0, count] with lo(o) > i
  while (a < b) {
    const int c = (a + b) >> 1;
    if (m[c].y > i) b = c; else a = c + 1;
  }
  (rows ? ry : rx)[i] = make_int2(first, a - 1);
}

bool axis_of(int n, double factor, int hw, int crop, Axis* a) {
  if (n < hw + 1 || n > MAX_SIDE) return false;
  a->n = n;
  a->n_pad = n + 2 * hw;
  a->cut = crop ? (int)((double)hw / factor) : 0;
  a->count = (int)floor((double)a->n_pad * (1.0 / factor)) - 2 * a->cut;
  return a->count >= 1;
}

size_t up16(size_t v) { return (v + 15) & ~(size_t)15; }

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

Psf psf_of(double factor, double mtf, int hw) {
  Psf psf;
  const double pi = 3.14159265358979323846;
  const double sigma = sqrt(-log(mtf) / 2.0) / (pi * (0.5 / factor));
  double sum = 0.0;
  for (int k = -hw; k <= hw; ++k) sum += (psf.g[k + hw] = exp(-((double)k * k) / (2.0 * sigma * sigma)));
  for (int k = 0; k < 2 * MAX_HW + 1; ++k) psf.g[k] = k <= 2 * hw ? psf.g[k] / sum : 0.0;
  psf.hw = hw;
  psf.scale = (float)(1.0 / (1.0 / factor));
  return psf;
}

}  // namespace
