// The sensor model at any ratio (C ABI and every definition: include/sifsr_degrade.h): reflect pad, Gaussian PSF
// with the reference's zero ring, bicubic resampling by a non-integer factor, as one banded operator per axis, out = Ry . x . Rx^T.
//
//  * degrade_table_kernel   one thread per weight of an axis (blockIdx.y: 0 rows, 1 columns).  From the fp32 source coordinate of
//    F.interpolate it forms, in float64, one of the K = 2 hw + 4 weights of its output over consecutive ORIGINAL pixels -- reflection
//    and zero ring folded in --; the thread of tap 0 also stores the first pixel of that window, the stencil [lo, hi] (the pixels a
//    non-zero coefficient reaches) and the "touches the ring" flag.  Row weights are stored [output][tap] (a wave of the row pass reads one output's taps: scalar
//    loads), column weights [tap][output] (the lanes of the column pass are consecutive outputs: coalesced).
//  * degrade_rows_kernel    the large pass, and the coalesced one: a wave owns 64 consecutive columns of ONE output row and walks the
//    K input rows of its window; weights and row indices are wave-uniform.  Only the rows some output samples are read: at factor
//    10.3 the reference blurs a hundred pixels for each one it keeps.  Writes the (B, oh, w) float64 intermediate and, with `valid`,
//    one byte per entry: the column of the stencil is all valid.
//  * degrade_cols_kernel    a lane owns one output; it walks K consecutive entries of the intermediate row, 1 / factor of the
//    first pass' data.  Validity, fill value and the single rounding to fp32 happen here.
// No LDS, no atomics, no allocation, no host synchronisation; nothing depends on the order in which workgroups run.
//
// The differentiable half (include/sifsr_sensor.h): dx = Ry^T . dout . Rx as a GATHER over the same tables, and
// the reflect-border low-pass of get_output_ftm at any half width through the same passes with another table.
//  * lowpass_table_kernel   the table of L: output o has 2 hw + 1 weights over [max(0, o - hw), ..], both reflections folded in.
//  * range_kernel           one thread per INPUT index of an axis: the run [o_lo, o_hi] of outputs whose stencil holds it, by
//    bisection of the stencil ends the table kernel stored (both are non-decreasing in o).  An empty run means a zero gradient.
//  * adjoint_cols_kernel    the small pass first: a lane owns input column j of one OUTPUT row and sums its run of output columns
//    (validity is applied here) into the (B, oh, w) float64 intermediate; writes are coalesced.
//  * adjoint_rows_kernel    the large pass: a wave owns 64 consecutive columns of ONE input row; its run of output rows and their
//    weights are wave-uniform (scalar loads), the intermediate is read coalesced.  Rounds to fp32 once.
// The runs have no compile-time bound (52 outputs over one pixel at factor 1.25 with hkw 16): both passes loop over the stored run.
#include "../../include/sifsr_degrade.h"
#include "../../include/sifsr_sensor.h"

#include <math.h>

#include "common.h"
#include "sensor_tables.h"

namespace {

constexpr int BX = 64;         // outputs (columns) per wave
constexpr int BY = 4;          // output rows per workgroup: one per wave

// (MAX_HW, MAX_SIDE, MAX_BATCH, Axis, Psf, the three table kernels, axis_of and psf_of: sensor_tables.h, shared with rloss.hip)
struct Plan {
  int hw, K, oh, ow;
  Axis ay, ax;
  size_t wy_off, wx_off, my_off, mx_off, tmp_off, tv_off, bytes;
};

// grid (ceil(w / BX), ceil(oh / BY), B), 256 threads: wave v of the workgroup owns output row blockIdx.y * BY + v
__global__ __launch_bounds__(256) void degrade_rows_kernel(const float* __restrict__ x, const unsigned char* __restrict__ valid,
                                                           const double* __restrict__ wy, const int4* __restrict__ my,
                                                           double* __restrict__ tmp, unsigned char* __restrict__ tv, int h, int w,
                                                           int oh, int K) {
  const int oy = __builtin_amdgcn_readfirstlane(blockIdx.y * BY + (threadIdx.x >> 6));
  const int col = blockIdx.x * BX + (threadIdx.x & 63);
  if (oy >= oh || col >= w) return;
  const int4 m = my[oy];
  const double* wk = wy + (size_t)oy * K;
  const size_t img = (size_t)blockIdx.z * h * w;
  const float* src = x + img + col;
  double acc = 0.0;
  // no branch in the loop, so that the loads of several taps are in flight together; a window that ends past the raster has zero
  // weights there and reads the last row instead, and what lies under a zero weight (a NaN of an invalid pixel) is not used
#pragma unroll 8
  for (int k = 0; k < K; ++k) {
    const double wgt = wk[k];
    const double v = (double)src[(size_t)min(m.x + k, h - 1) * w];
    acc = wgt != 0.0 ? fma(wgt, v, acc) : acc;
  }
  const size_t dst = ((size_t)blockIdx.z * oh + oy) * w + col;
  tmp[dst] = acc;
  if (valid != nullptr) {
    const unsigned char* v = valid + img + col;
    int ok = 1;
#pragma unroll 4
    for (int j = m.y; j <= m.z; ++j) ok &= v[(size_t)j * w] != 0 ? 1 : 0;
    tv[dst] = (unsigned char)ok;
  }
}

// grid (ceil(ow / BX), ceil(oh / BY), B), 256 threads: lane = output column, wave = output row
__global__ __launch_bounds__(256) void degrade_cols_kernel(const double* __restrict__ tmp, const unsigned char* __restrict__ tv,
                                                           const double* __restrict__ wx, const int4* __restrict__ my,
                                                           const int4* __restrict__ mx, float* __restrict__ out,
                                                           unsigned char* __restrict__ out_valid, int w, int oh, int ow, int K,
                                                           int with_valid, float fill_value) {
  const int oy = __builtin_amdgcn_readfirstlane(blockIdx.y * BY + (threadIdx.x >> 6));
  const int ox = blockIdx.x * BX + (threadIdx.x & 63);
  if (oy >= oh || ox >= ow) return;
  const int4 m = mx[ox];
  const size_t row = ((size_t)blockIdx.z * oh + oy) * w;
  const double* src = tmp + row;
  double acc = 0.0;
#pragma unroll 4
  for (int k = 0; k < K; ++k) {
    const double wgt = wx[(size_t)k * ow + ox];
    const double v = src[min(m.x + k, w - 1)];
    acc = wgt != 0.0 ? fma(wgt, v, acc) : acc;             // what lies under a zero weight (a NaN of an invalid pixel) is not used
  }
  int ok = (my[oy].w | m.w) == 0 ? 1 : 0;
  if (with_valid) {
    const unsigned char* v = tv + row;
    for (int j = m.y; j <= m.z; ++j) ok &= v[j];
  }
  const size_t dst = ((size_t)blockIdx.z * oh + oy) * ow + ox;
  out[dst] = (with_valid && !ok) ? fill_value : (float)acc;
  if (out_valid != nullptr) out_valid[dst] = (unsigned char)ok;
}

// grid (ceil(w / BX), ceil(oh / BY), B), 256 threads: lane = input column j, wave = output row oy.
// tmp[b, oy, j] = sum over ox in the run of j of wx[ox][j - start(ox)] * dout[b, oy, ox], ascending ox
__global__ __launch_bounds__(256) void adjoint_cols_kernel(const float* __restrict__ dout, const unsigned char* __restrict__ out_valid,
                                                           const double* __restrict__ wx, const int4* __restrict__ mx,
                                                           const int2* __restrict__ rx, double* __restrict__ tmp, int w, int oh,
                                                           int ow, int K) {
  const int oy = __builtin_amdgcn_readfirstlane(blockIdx.y * BY + (threadIdx.x >> 6));
  const int j = blockIdx.x * BX + (threadIdx.x & 63);
  if (oy >= oh || j >= w) return;
  const int2 r = rx[j];
  const size_t row = ((size_t)blockIdx.z * oh + oy) * ow;
  const float* src = dout + row;
  double acc = 0.0;
  for (int ox = r.x; ox <= r.y; ++ox) {
    const int k = j - mx[ox].x;                             // the tap of output ox that lies over pixel j
    if (k < 0 || k >= K) continue;                          // (never, while the stencil lies inside the window)
    const double wgt = wx[(size_t)k * ow + ox];
    const bool counted = out_valid == nullptr || out_valid[row + ox] != 0;
    const double v = (double)src[ox];
    acc = (counted && wgt != 0.0) ? fma(wgt, v, acc) : acc;  // what lies under a zero weight or an uncounted output is not used
  }
  tmp[((size_t)blockIdx.z * oh + oy) * w + j] = acc;
}

// grid (ceil(w / BX), ceil(h / BY), B), 256 threads: wave v of the workgroup owns INPUT row blockIdx.y * BY + v.
// dx[b, i, j] = sum over oy in the run of i of wy[oy][i - start(oy)] * tmp[b, oy, j], ascending oy
__global__ __launch_bounds__(256) void adjoint_rows_kernel(const double* __restrict__ tmp, const double* __restrict__ wy,
                                                           const int4* __restrict__ my, const int2* __restrict__ ry,
                                                           float* __restrict__ dx, int h, int w, int oh, int K) {
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.y * BY + (threadIdx.x >> 6));
  const int col = blockIdx.x * BX + (threadIdx.x & 63);
  if (i >= h || col >= w) return;
  const int2 r = ry[i];
  const double* src = tmp + (size_t)blockIdx.z * oh * w + col;
  double acc = 0.0;
#pragma unroll 4
  for (int oy = r.x; oy <= r.y; ++oy) {
    const int k = i - my[oy].x;
    if (k < 0 || k >= K) continue;                          // (never, while the stencil lies inside the window)
    const double wgt = wy[(size_t)oy * K + k];
    const double v = src[(size_t)oy * w];
    acc = wgt != 0.0 ? fma(wgt, v, acc) : acc;
  }
  dx[((size_t)blockIdx.z * h + i) * w + col] = (float)acc;
}

bool plan_of(int B, int h, int w, double factor, int hkw, int crop, Plan* p) {
  if (!(factor > 1.0 && factor <= 16.0) || hkw < 0 || B < 1 || B > MAX_BATCH || (crop != 0 && crop != 1)) return false;
  p->hw = hkw == 0 ? (int)ceil(factor) : hkw;
  if (p->hw < 1 || p->hw > MAX_HW) return false;
  if (!axis_of(h, factor, p->hw, crop, &p->ay) || !axis_of(w, factor, p->hw, crop, &p->ax)) return false;
  p->K = 2 * p->hw + 4;
  p->oh = p->ay.count;
  p->ow = p->ax.count;
  const size_t mid = (size_t)B * p->oh * w;
  p->wy_off = 0;
  p->wx_off = up16((size_t)p->oh * p->K * sizeof(double));
  p->my_off = p->wx_off + up16((size_t)p->ow * p->K * sizeof(double));
  p->mx_off = p->my_off + (size_t)p->oh * sizeof(int4);
  p->tmp_off = p->mx_off + (size_t)p->ow * sizeof(int4);
  p->tv_off = p->tmp_off + mid * sizeof(double);
  p->bytes = up16(p->tv_off + mid);
  return true;
}

// The adjoint's workspace: the forward's two weight tables and two stencil tables at the forward's offsets, then one run per input
// index of each axis and the (B, oh, w) float64 intermediate.  `lowpass`: oh = h, ow = w, K = 2 hw + 1, no crop.
struct AdjointPlan {
  int hw, K, oh, ow;
  Axis ay, ax;
  size_t wy_off, wx_off, my_off, mx_off, ry_off, rx_off, tmp_off, bytes;
};

bool adjoint_plan_of(int B, int h, int w, double factor, int hkw, int crop, bool lowpass, AdjointPlan* a) {
  if (lowpass) {                                           // the limits of plan_of but one: there is always an output
    if (!(factor > 1.0 && factor <= 16.0) || hkw < 0 || B < 1 || B > MAX_BATCH) return false;
    a->hw = hkw == 0 ? (int)ceil(factor) : hkw;
    if (a->hw < 1 || a->hw > MAX_HW || h < a->hw + 1 || w < a->hw + 1 || h > MAX_SIDE || w > MAX_SIDE) return false;
    a->ay = Axis{h, h + 2 * a->hw, h, 0};
    a->ax = Axis{w, w + 2 * a->hw, w, 0};
  } else {
    Plan p;
    if (!plan_of(B, h, w, factor, hkw, crop, &p)) return false;
    a->hw = p.hw;
    a->ay = p.ay;
    a->ax = p.ax;
  }
  a->K = lowpass ? 2 * a->hw + 1 : 2 * a->hw + 4;
  a->oh = a->ay.count;
  a->ow = a->ax.count;
  a->wy_off = 0;
  a->wx_off = up16((size_t)a->oh * a->K * sizeof(double));
  a->my_off = a->wx_off + up16((size_t)a->ow * a->K * sizeof(double));
  a->mx_off = a->my_off + (size_t)a->oh * sizeof(int4);
  a->ry_off = a->mx_off + (size_t)a->ow * sizeof(int4);
  a->rx_off = a->ry_off + (size_t)h * sizeof(int2);
  a->tmp_off = up16(a->rx_off + (size_t)w * sizeof(int2));
  a->bytes = up16(a->tmp_off + (size_t)B * a->oh * w * sizeof(double));
  return true;
}

struct AdjointBuffers {
  double *wy, *wx, *tmp;
  int4 *my, *mx;
  int2 *ry, *rx;
};

AdjointBuffers buffers_of(void* workspace, const AdjointPlan& a) {
  char* ws = static_cast<char*>(workspace);
  AdjointBuffers b;
  b.wy = reinterpret_cast<double*>(ws + a.wy_off);
  b.wx = reinterpret_cast<double*>(ws + a.wx_off);
  b.my = reinterpret_cast<int4*>(ws + a.my_off);
  b.mx = reinterpret_cast<int4*>(ws + a.mx_off);
  b.ry = reinterpret_cast<int2*>(ws + a.ry_off);
  b.rx = reinterpret_cast<int2*>(ws + a.rx_off);
  b.tmp = reinterpret_cast<double*>(ws + a.tmp_off);
  return b;
}

int launch_table(const AdjointPlan& a, const AdjointBuffers& b, const Psf& psf, bool lowpass, hipStream_t s) {
  const int most = (a.oh > a.ow ? a.oh : a.ow) * a.K;
  if (lowpass)
    hipLaunchKernelGGL(lowpass_table_kernel, dim3((most + 255) / 256, 2), dim3(256), 0, s, psf, a.ay, a.ax, b.wy, b.wx, b.my, b.mx);
  else
    hipLaunchKernelGGL(degrade_table_kernel, dim3((most + 255) / 256, 2), dim3(256), 0, s, psf, a.ay, a.ax, b.wy, b.wx, b.my, b.mx);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

// range kernel, adjoint column pass, adjoint row pass: dx (B, h, w) from dout (B, oh, ow) over the tables in `b`
int launch_adjoint(const AdjointPlan& a, const AdjointBuffers& b, const float* dout, const unsigned char* out_valid, float* dx, int B,
                   int h, int w, hipStream_t s) {
  hipLaunchKernelGGL(range_kernel, dim3(((h > w ? h : w) + 255) / 256, 2), dim3(256), 0, s, b.my, b.mx, b.ry, b.rx, h, w, a.oh, a.ow);
  SIFSR_LAUNCH_CHECK();
  const int gx = (w + BX - 1) / BX;
  hipLaunchKernelGGL(adjoint_cols_kernel, dim3(gx, (a.oh + BY - 1) / BY, B), dim3(256), 0, s, dout, out_valid, b.wx, b.mx, b.rx, b.tmp, w,
                     a.oh, a.ow, a.K);
  SIFSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(adjoint_rows_kernel, dim3(gx, (h + BY - 1) / BY, B), dim3(256), 0, s, b.tmp, b.wy, b.my, b.ry, dx, h, w, a.oh, a.K);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

}  // namespace

// ---- C ABI (include/sifsr_degrade.h) ----
int sifsrs_out_shape(int h, int w, double factor, int hkw, int crop, int* oh, int* ow) {
  if (!oh || !ow) return SIFSR_ERR_ARG;
  Plan p;
  if (!plan_of(1, h, w, factor, hkw, crop, &p)) return SIFSR_ERR_SHAPE;
  *oh = p.oh;
  *ow = p.ow;
  return SIFSR_OK;
}

size_t sifsrs_workspace_bytes(int B, int h, int w, double factor, int hkw, int crop) {
  Plan p;
  return plan_of(B, h, w, factor, hkw, crop, &p) ? p.bytes : 0;
}

int sifsrs_degrade(const float* x, const unsigned char* valid, float* out, unsigned char* out_valid, void* workspace,
                   size_t workspace_bytes, int B, int h, int w, double factor, double mtf, int hkw, int crop, float fill_value,
                   void* stream) {
  if (!x || !out || !workspace || !aligned(workspace, 16) || !aligned(x, 4) || !aligned(out, 4)) return SIFSR_ERR_ARG;
  Plan p;
  if (!plan_of(B, h, w, factor, hkw, crop, &p) || !(mtf > 0.0 && mtf < 1.0)) return SIFSR_ERR_SHAPE;
  if (workspace_bytes < p.bytes) return SIFSR_ERR_WORKSPACE;

  const Psf psf = psf_of(factor, mtf, p.hw);
  char* ws = static_cast<char*>(workspace);
  double* wy = reinterpret_cast<double*>(ws + p.wy_off);
  double* wx = reinterpret_cast<double*>(ws + p.wx_off);
  int4* my = reinterpret_cast<int4*>(ws + p.my_off);
  int4* mx = reinterpret_cast<int4*>(ws + p.mx_off);
  double* tmp = reinterpret_cast<double*>(ws + p.tmp_off);
  unsigned char* tv = reinterpret_cast<unsigned char*>(ws + p.tv_off);
  hipStream_t s = (hipStream_t)stream;
  const int most = (p.oh > p.ow ? p.oh : p.ow) * p.K;
  hipLaunchKernelGGL(degrade_table_kernel, dim3((most + 255) / 256, 2), dim3(256), 0, s, psf, p.ay, p.ax, wy, wx, my, mx);
  SIFSR_LAUNCH_CHECK();
  const int gy = (p.oh + BY - 1) / BY;
  hipLaunchKernelGGL(degrade_rows_kernel, dim3((w + BX - 1) / BX, gy, B), dim3(256), 0, s, x, valid, wy, my, tmp, tv, h, w, p.oh, p.K);
  SIFSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(degrade_cols_kernel, dim3((p.ow + BX - 1) / BX, gy, B), dim3(256), 0, s, tmp, tv, wx, my, mx, out, out_valid, w,
                     p.oh, p.ow, p.K, valid != nullptr ? 1 : 0, fill_value);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

// ---- C ABI (include/sifsr_sensor.h) ----
size_t sifsrt_degrade_bwd_workspace_bytes(int B, int h, int w, double factor, int hkw, int crop) {
  AdjointPlan a;
  return adjoint_plan_of(B, h, w, factor, hkw, crop, false, &a) ? a.bytes : 0;
}

int sifsrt_degrade_bwd(const float* dout, const unsigned char* out_valid, float* dx, void* workspace, size_t workspace_bytes, int B,
                       int h, int w, double factor, double mtf, int hkw, int crop, void* stream) {
  if (!dout || !dx || !workspace || !aligned(workspace, 16) || !aligned(dout, 4) || !aligned(dx, 4)) return SIFSR_ERR_ARG;
  AdjointPlan a;
  if (!adjoint_plan_of(B, h, w, factor, hkw, crop, false, &a) || !(mtf > 0.0 && mtf < 1.0)) return SIFSR_ERR_SHAPE;
  if (workspace_bytes < a.bytes) return SIFSR_ERR_WORKSPACE;
  const AdjointBuffers b = buffers_of(workspace, a);
  hipStream_t s = (hipStream_t)stream;
  const int rc = launch_table(a, b, psf_of(factor, mtf, a.hw), false, s);
  return rc != SIFSR_OK ? rc : launch_adjoint(a, b, dout, out_valid, dx, B, h, w, s);
}

size_t sifsrt_lowpass_workspace_bytes(int B, int h, int w, double factor, int hkw) {
  AdjointPlan a;
  return adjoint_plan_of(B, h, w, factor, hkw, 0, true, &a) ? a.bytes : 0;
}

int sifsrt_lowpass_fwd(const float* x, float* out, void* workspace, size_t workspace_bytes, int B, int h, int w, double factor,
                       double mtf, int hkw, void* stream) {
  if (!x || !out || !workspace || !aligned(workspace, 16) || !aligned(x, 4) || !aligned(out, 4)) return SIFSR_ERR_ARG;
  AdjointPlan a;
  if (!adjoint_plan_of(B, h, w, factor, hkw, 0, true, &a) || !(mtf > 0.0 && mtf < 1.0)) return SIFSR_ERR_SHAPE;
  if (workspace_bytes < a.bytes) return SIFSR_ERR_WORKSPACE;
  const AdjointBuffers b = buffers_of(workspace, a);
  hipStream_t s = (hipStream_t)stream;
  const int rc = launch_table(a, b, psf_of(factor, mtf, a.hw), true, s);
  if (rc != SIFSR_OK) return rc;
  const int gx = (w + BX - 1) / BX, gy = (h + BY - 1) / BY;
  hipLaunchKernelGGL(degrade_rows_kernel, dim3(gx, gy, B), dim3(256), 0, s, x, (const unsigned char*)nullptr, b.wy, b.my, b.tmp,
                     (unsigned char*)nullptr, h, w, h, a.K);
  SIFSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(degrade_cols_kernel, dim3(gx, gy, B), dim3(256), 0, s, b.tmp, (const unsigned char*)nullptr, b.wx, b.my, b.mx, out,
                     (unsigned char*)nullptr, w, h, w, a.K, 0, 0.0f);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrt_lowpass_bwd(const float* dout, float* dx, void* workspace, size_t workspace_bytes, int B, int h, int w, double factor,
                       double mtf, int hkw, void* stream) {
  if (!dout || !dx || !workspace || !aligned(workspace, 16) || !aligned(dout, 4) || !aligned(dx, 4)) return SIFSR_ERR_ARG;
  AdjointPlan a;
  if (!adjoint_plan_of(B, h, w, factor, hkw, 0, true, &a) || !(mtf > 0.0 && mtf < 1.0)) return SIFSR_ERR_SHAPE;
  if (workspace_bytes < a.bytes) return SIFSR_ERR_WORKSPACE;
  const AdjointBuffers b = buffers_of(workspace, a);
  hipStream_t s = (hipStream_t)stream;
  const int rc = launch_table(a, b, psf_of(factor, mtf, a.hw), true, s);
  return rc != SIFSR_OK ? rc : launch_adjoint(a, b, dout, nullptr, dx, B, h, w, s);
}
