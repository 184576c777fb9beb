// Device helpers the DMS kernels of dms.hip (x4) and rbaselines.hip (any ratio) share: ONE definition of the fourth power and of
// a fitted tree's prediction, so that both families are the float64 arithmetic tests/dms_reference.py writes down.
// Products and sums are kept apart: the pragma below holds for the rest of the translation unit that includes this header, which
// is what both includers want (dms.hip states it itself as well).
#pragma once

#pragma clang fp contract(off)

static __device__ __forceinline__ double pow4d(double v) { return (v * v) * (v * v); }

// thr: the tree's ascending thresholds, lf: its leaf records [coef, intercept, lo, hi], L leaves: the leaf by `x <= threshold -> left`
static __device__ __forceinline__ double tree_value(const double* thr, const double* lf, int L, double x) {
  int a = 0, z = L - 1;
  while (a < z) {
    const int mid = (a + z) >> 1;
    if (thr[mid] < x) a = mid + 1; else z = mid;
  }
  const double* p = lf + 4 * a;
  return fmin(fmax(x * p[0] + p[1], p[2]), p[3]);
}
