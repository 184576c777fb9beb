// Conservation of the observed LST at any ratio (C ABI and every definition: include/sifsr_rconserve.h): the
// residual r = lst - D(sr) over the cells where it is defined, its statistics, and the correction sr += relax * U(r), with D the
// banded operator of the sensor model (sensor_tables.h: the table kernel of degrade.hip writes the weights and the stencils) and U
// the exact-phase bicubic of ratio.h.
//
//  * rconserve_residual_kernel   one workgroup per tile of tl x tl cells, tl <= 16 sized from the factor as pass A of rloss.hip sizes
//    its tile.  It stages, ONCE, the sr pixels of every cell the tile's stencils touch (whole cells: at most CAP x CAP fp32 in LDS),
//    a wave per staged row with all of a wave's loads in flight before the first is used, and decides the validity of those cells
//    from the values just loaded and from lst / mask.  Ry goes into a float64 LDS intermediate (a wave per output row: lane k loads
//    weight k once, every tap reads it wave-uniformly, a zero weight is one uniform branch), then one thread per cell tests the cells
//    under its stencil rectangle, applies Rx (its weights loaded together) and emits r, the cell's validity byte and -- through a
//    fixed tree over the workgroup -- four float64 partials (sum r, sum r^2, max |r|, count).
//  * rconserve_apply_kernel      ratio_resample_block of ratio.h over r -- the body of ratio_upsample_kernel, so U(r) has its bits --
//    with the step as the emitter: one read of sr, one write of out, 256 consecutive floats per row.  A pixel of a cell without c
//    keeps its bits.
//  * rconserve_finish_kernel     one workgroup per statistics row adds the partials in a fixed order.
// No atomics, no allocation, no host synchronisation; nothing depends on the order in which workgroups run.
#include "../../include/sifsr_rconserve.h"

#include "ratio.h"
#include "sensor_tables.h"

namespace {

constexpr int RC_MAX_HW = 8;                    // factor <= 8
constexpr double RC_MAX_FACTOR = 8.0;
constexpr int RC_CAP = 80;                      // most staged sr rows / columns of one tile, and most cells under them
constexpr int RC_LS = RC_CAP + 1;               // ... and the LDS row stride
constexpr int RC_TL = 16;                       // most cells per tile side: RC_TL^2 = one cell per thread
constexpr int RC_MAX_ITER = 64;
constexpr int RC_RPW = RC_CAP / 4;               // staged rows per wave
constexpr int RC_MAX_K = 2 * RC_MAX_HW + 4;     // most weights of a window

struct RcArgs {
  const float *sr, *lst;
  const unsigned char* mask;
  const double *wy, *wx;
  const int4 *my, *mx;
  float* r;
  unsigned char* cval;
  double* part;
  int H, W, h, w, K, tl;
};

__device__ __forceinline__ bool rc_good(float v) { return isfinite(v) && v != 0.f; }
// the cell of pixel P along an axis n <- N, and the first pixel of cell c (both below 2^28)
__device__ __forceinline__ int rc_cell(int P, int n, int N) { return P * n / N; }
__device__ __forceinline__ int rc_first(int c, int n, int N) { return (c * N + n - 1) / n; }

// grid (ceil(w / tl), ceil(h / tl)), 256 threads
__global__ __launch_bounds__(256) void rconserve_residual_kernel(const RcArgs a) {
  __shared__ float S[RC_CAP * RC_LS];
  __shared__ double T[RC_TL * RC_LS];
  __shared__ unsigned char bad[RC_CAP * RC_CAP];
  __shared__ double red[4][4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int H = a.H, W = a.W, h = a.h, w = a.w, K = a.K, tl = a.tl;
  const int i0 = blockIdx.y * tl, j0 = blockIdx.x * tl;
  const int ni = min(tl, h - i0), nj = min(tl, w - j0);

  // the cells the tile's stencil rectangles touch, with the tile's own; then the pixels of those cells
  int ylo = H - 1, yhi = 0, xlo = W - 1, xhi = 0;
  for (int i = 0; i < ni; ++i) {
    const int4 m = a.my[i0 + i];
    ylo = min(ylo, m.y);
    yhi = max(yhi, m.z);
  }
  for (int j = 0; j < nj; ++j) {
    const int4 m = a.mx[j0 + j];
    xlo = min(xlo, m.y);
    xhi = max(xhi, m.z);
  }
  // (the spans fit RC_CAP by the choice of tl: tests/test_rconserve_host.py holds it; the clamps keep every index inside its
  // array whatever the tables hold)
  ylo = clampi(ylo, 0, H - 1); yhi = clampi(yhi, 0, H - 1);
  xlo = clampi(xlo, 0, W - 1); xhi = clampi(xhi, 0, W - 1);
  const int cy0 = min(i0, rc_cell(ylo, h, H)), cy1 = max(i0 + ni - 1, rc_cell(yhi, h, H));
  const int cx0 = min(j0, rc_cell(xlo, w, W)), cx1 = max(j0 + nj - 1, rc_cell(xhi, w, W));
  const int ys = rc_first(cy0, h, H), xs = rc_first(cx0, w, W);
  const int nr = clampi(rc_first(cy1 + 1, h, H) - ys, 1, RC_CAP), nc = clampi(rc_first(cx1 + 1, w, W) - xs, 1, RC_CAP);
  const int ncy = min(cy1 - cy0 + 1, RC_CAP), ncx = min(cx1 - cx0 + 1, RC_CAP);   // a cell holds a pixel at least: ncy <= nr

  // the lst part of c
  for (int e = tid; e < ncy * ncx; e += 256) {
    const int ci = e / ncx, cj = e - ci * ncx;
    const size_t p = (size_t)min(cy0 + ci, h - 1) * w + min(cx0 + cj, w - 1);
    const bool ok = rc_good(a.lst[p]) && (a.mask == nullptr || a.mask[p] != 0);
    bad[e] = ok ? 0 : 1;
  }
  __syncthreads();
  // the pixels, a wave per row, and the sr part of c: any pixel of the cell that is not finite or is 0 (every writer stores 1)
  const int c_a = lane, c_b = lane + 64;
  const int cell_a = c_a < nc ? min(rc_cell(xs + c_a, w, W) - cx0, ncx - 1) : 0;
  const int cell_b = c_b < nc ? min(rc_cell(xs + c_b, w, W) - cx0, ncx - 1) : 0;
  // (all loads of a wave's rows are issued before the first value is used: the loop is bound by latency otherwise)
  float va[RC_RPW], vb[RC_RPW];
#pragma unroll
  for (int t = 0; t < RC_RPW; ++t) {
    const int r = wv + 4 * t;
    const float* row = a.sr + (size_t)min(ys + r, H - 1) * W + xs;
    va[t] = (r < nr && c_a < nc) ? row[c_a] : 1.f;
    vb[t] = (r < nr && c_b < nc) ? row[c_b] : 1.f;
  }
#pragma unroll
  for (int t = 0; t < RC_RPW; ++t) {
    const int r = wv + 4 * t;
    const int crow = min(rc_cell(min(ys + r, H - 1), h, H) - cy0, ncy - 1) * ncx;
    if (r < nr && c_a < nc) {
      S[r * RC_LS + c_a] = va[t];
      if (!rc_good(va[t])) bad[crow + cell_a] = 1;
    }
    if (r < nr && c_b < nc) {
      S[r * RC_LS + c_b] = vb[t];
      if (!rc_good(vb[t])) bad[crow + cell_b] = 1;
    }
  }
  __syncthreads();
  // Ry, a wave per output row: T[i][c] = sum_k wy[i][k] S[start + k][c]
  for (int i = wv; i < ni; i += 4) {
    const int start = a.my[i0 + i].x;
    // lane k holds weight k of the row (K <= 20): one load, then a wave-uniform read per tap
    const double wl = a.wy[(size_t)(i0 + i) * K + min(lane, K - 1)];
    const int ca = min(c_a, nc - 1), cb = min(c_b, nc - 1);
    double acc_a = 0.0, acc_b = 0.0;
    for (int k = 0; k < K; ++k) {
      const double wgt = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(wl), k), __builtin_amdgcn_readlane(__double2loint(wl), k));
      if (wgt != 0.0) {                                      // (wave-uniform)
        const int r = clampi(min(start + k, H - 1) - ys, 0, nr - 1);
        acc_a = fma(wgt, (double)S[r * RC_LS + ca], acc_a);
        acc_b = fma(wgt, (double)S[r * RC_LS + cb], acc_b);
      }
    }
    if (c_a < nc) T[i * RC_LS + c_a] = acc_a;
    if (c_b < nc) T[i * RC_LS + c_b] = acc_b;
  }
  __syncthreads();
  // Rx, the counted test, r, the validity byte and the partials: a thread per cell
  float res = 0.f;
  bool counted = false;
  if (tid < ni * nj) {
    const int i = tid / nj, j = tid - i * nj;
    const int4 m = a.my[i0 + i], n = a.mx[j0 + j];
    const size_t p = (size_t)(i0 + i) * w + j0 + j;
    const bool c = bad[min(i0 + i - cy0, ncy - 1) * ncx + min(j0 + j - cx0, ncx - 1)] == 0;
    counted = c && (m.w | n.w) == 0;
    if (counted) {
      const int a0 = clampi(rc_cell(clampi(m.y, 0, H - 1), h, H) - cy0, 0, ncy - 1), a1 = clampi(rc_cell(clampi(m.z, 0, H - 1), h, H) - cy0, 0, ncy - 1);
      const int b0 = clampi(rc_cell(clampi(n.y, 0, W - 1), w, W) - cx0, 0, ncx - 1), b1 = clampi(rc_cell(clampi(n.z, 0, W - 1), w, W) - cx0, 0, ncx - 1);
      int any = 0;
      for (int ci = a0; ci <= a1; ++ci)
        for (int cj = b0; cj <= b1; ++cj) any |= bad[ci * ncx + cj];
      counted = any == 0;
    }
    if (counted) {
      double acc = 0.0, wk[RC_MAX_K];
#pragma unroll
      for (int k = 0; k < RC_MAX_K; ++k) wk[k] = k < K ? a.wx[(size_t)k * w + j0 + j] : 0.0;   // in flight together
#pragma unroll
      for (int k = 0; k < RC_MAX_K; ++k) {
        const double wgt = wk[k];                            // 0 past K: skipped
        const int cc = clampi(min(n.x + k, W - 1) - xs, 0, nc - 1);
        acc = wgt != 0.0 ? fma(wgt, T[i * RC_LS + cc], acc) : acc;
      }
      res = (float)((double)a.lst[p] - acc);
    }
    a.r[p] = res;
    a.cval[p] = c ? 1 : 0;
  }
  double s1 = (double)res, s2 = (double)res * (double)res, mx = fabs((double)res), cnt = counted ? 1.0 : 0.0;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
    mx = fmax(mx, __shfl_xor(mx, o));
    cnt += __shfl_xor(cnt, o);
  }
  if (lane == 0) {
    red[0][wv] = s1; red[1][wv] = s2; red[2][wv] = mx; red[3][wv] = cnt;
  }
  __syncthreads();
  if (tid == 0) {
    double* o = a.part + 4 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
    o[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    o[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    o[2] = fmax(fmax(red[2][0], red[2][1]), fmax(red[2][2], red[2][3]));
    o[3] = (red[3][0] + red[3][1]) + (red[3][2] + red[3][3]);
  }
}

// grid (ceil(W / 256), ceil(H / 16)), 256 threads: thread = output column.  out may be sr itself: a pixel is read and written by
// one thread.
__global__ __launch_bounds__(256) void rconserve_apply_kernel(const float* sr, const float* __restrict__ r,
                                                              const unsigned char* __restrict__ cval, float* out, int h, int w, int H,
                                                              int W, float relax) {
  __shared__ float src[RATIO_SRC_ROWS][RATIO_SRC_COLS];
  ratio_resample_block(r, (size_t)w, h, w, H, W, blockIdx.y * RATIO_ROWS, blockIdx.x * RATIO_COLS, 0.f, 1.f, src,
                       [=](int, int Y, int X, float u) {
                         const size_t p = (size_t)Y * W + X;
                         const float s = sr[p];
                         const bool c = cval[(size_t)rc_cell(Y, h, H) * w + rc_cell(X, w, W)] != 0;
                         out[p] = c ? fmaf(relax, u, s) : s;
                       });
}

// one workgroup per statistics row: thread t adds the partials t, t + 256, ... in that order, then a fixed tree over the threads
__global__ __launch_bounds__(256) void rconserve_finish_kernel(const double* __restrict__ partial, double* __restrict__ stats, int nwg) {
  __shared__ double a[4][256];
  const int t = threadIdx.x;
  const double* src = partial + 4 * (size_t)blockIdx.x * nwg;
  double s1 = 0.0, s2 = 0.0, mx = 0.0, n = 0.0;
  for (int g = t; g < nwg; g += 256) {
    s1 += src[4 * (size_t)g];
    s2 += src[4 * (size_t)g + 1];
    mx = fmax(mx, src[4 * (size_t)g + 2]);
    n += src[4 * (size_t)g + 3];
  }
  a[0][t] = s1; a[1][t] = s2; a[2][t] = mx; a[3][t] = n;
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (t < o) {
      a[0][t] += a[0][t + o];
      a[1][t] += a[1][t + o];
      a[2][t] = fmax(a[2][t], a[2][t + o]);
      a[3][t] += a[3][t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    double* o = stats + 4 * (size_t)blockIdx.x;
    const double cnt = a[3][0], nan = __longlong_as_double(0x7FF8000000000000ll);
    o[0] = cnt;
    o[1] = cnt > 0.0 ? a[0][0] / cnt : nan;
    o[2] = cnt > 0.0 ? sqrt(a[1][0] / cnt) : nan;
    o[3] = cnt > 0.0 ? a[2][0] : nan;
  }
}

struct RcPlan {
  int hw, K, tl, gx, gy;
  double factor;
  Axis ay, ax;
  size_t wy, wx, my, mx, part, cval, bytes;                // r at 0
};

bool rc_plan_of(int h, int w, int H, int W, int n_iter, RcPlan* p) {
  if (h < 1 || w < 1 || H < 1 || W < 1 || h > MAX_SIDE || w > MAX_SIDE || H > MAX_SIDE || W > MAX_SIDE) return false;
  if (n_iter < 0 || n_iter > RC_MAX_ITER || (long long)H * w != (long long)W * h) return false;
  p->factor = (double)H / (double)h;
  if (!(p->factor > 1.0 && p->factor <= RC_MAX_FACTOR)) return false;
  p->hw = (int)ceil(p->factor);
  if (p->hw < 1 || p->hw > RC_MAX_HW) return false;
  if (!axis_of(H, p->factor, p->hw, 1, &p->ay) || !axis_of(W, p->factor, p->hw, 1, &p->ax)) return false;
  if (p->ay.count != h || p->ax.count != w) return false;
  p->K = 2 * p->hw + 4;
  // the stencils of tl consecutive outputs span at most factor (tl - 1) + K + 2 pixels of an axis (rloss.hip); completing the
  // first and the last cell adds at most hw - 1 pixels on each side
  const int tl = (int)floor((double)(RC_CAP - p->K - 2 * p->hw) / p->factor) + 1;
  p->tl = tl < 1 ? 1 : (tl > RC_TL ? RC_TL : tl);
  p->gx = (w + p->tl - 1) / p->tl;
  p->gy = (h + p->tl - 1) / p->tl;
  size_t off = 0;
  auto take = [&off](size_t bytes) { const size_t at = off; off = up16(off + bytes); return at; };
  take((size_t)h * w * sizeof(float));
  p->wy = take((size_t)h * p->K * sizeof(double));
  p->wx = take((size_t)w * p->K * sizeof(double));
  p->my = take((size_t)h * sizeof(int4));
  p->mx = take((size_t)w * sizeof(int4));
  p->part = take((size_t)(n_iter + 1) * p->gx * p->gy * 4 * sizeof(double));
  p->cval = take((size_t)h * w);
  p->bytes = off;
  return true;
}

}  // namespace

// ---- C ABI (include/sifsr_rconserve.h) ----
size_t sifsrc_workspace_bytes(int h, int w, int H, int W, int n_iter) {
  RcPlan p;
  return rc_plan_of(h, w, H, W, n_iter, &p) ? p.bytes : 0;
}

int sifsrc_conserve(const float* sr, const float* lst, const unsigned char* mask, float* out, double* stats, void* workspace,
                    size_t workspace_bytes, int h, int w, int H, int W, double mtf, float relax, int n_iter, void* stream) {
  if (!sr || !lst || !stats || !workspace || !aligned(workspace, 16) || !aligned(sr, 4) || !aligned(lst, 4) || !aligned(stats, 8))
    return SIFSR_ERR_ARG;
  RcPlan p;
  if (!rc_plan_of(h, w, H, W, n_iter, &p) || !(mtf > 0.0 && mtf < 1.0)) return SIFSR_ERR_SHAPE;
  if (n_iter > 0 && (!out || !aligned(out, 4))) return SIFSR_ERR_ARG;
  if (!(relax - relax == 0.f)) return SIFSR_ERR_ARG;              // NaN or inf
  if (workspace_bytes < p.bytes) return SIFSR_ERR_WORKSPACE;

  char* ws = static_cast<char*>(workspace);
  const int nwg = p.gx * p.gy;
  RcArgs a;
  a.lst = lst; a.mask = mask;
  double* wy = reinterpret_cast<double*>(ws + p.wy);
  double* wx = reinterpret_cast<double*>(ws + p.wx);
  int4* my = reinterpret_cast<int4*>(ws + p.my);
  int4* mx = reinterpret_cast<int4*>(ws + p.mx);
  a.wy = wy; a.wx = wx; a.my = my; a.mx = mx;
  a.r = reinterpret_cast<float*>(ws);
  a.cval = reinterpret_cast<unsigned char*>(ws + p.cval);
  double* partial = reinterpret_cast<double*>(ws + p.part);
  a.H = H; a.W = W; a.h = h; a.w = w; a.K = p.K; a.tl = p.tl;
  hipStream_t s = (hipStream_t)stream;

  hipLaunchKernelGGL(degrade_table_kernel, dim3(((h > w ? h : w) * p.K + 255) / 256, 2), dim3(256), 0, s, psf_of(p.factor, mtf, p.hw),
                     p.ay, p.ax, wy, wx, my, mx);
  SIFSR_LAUNCH_CHECK();
  const float* cur = sr;
  for (int it = 0; it <= n_iter; ++it) {
    a.sr = cur;
    a.part = partial + 4 * (size_t)it * nwg;
    hipLaunchKernelGGL(rconserve_residual_kernel, dim3(p.gx, p.gy), dim3(256), 0, s, a);
    SIFSR_LAUNCH_CHECK();
    if (it == n_iter) break;
    hipLaunchKernelGGL(rconserve_apply_kernel, dim3((W + RATIO_COLS - 1) / RATIO_COLS, (H + RATIO_ROWS - 1) / RATIO_ROWS), dim3(256), 0, s,
                       cur, a.r, a.cval, out, h, w, H, W, relax);
    SIFSR_LAUNCH_CHECK();
    cur = out;
  }
  hipLaunchKernelGGL(rconserve_finish_kernel, dim3(n_iter + 1), dim3(256), 0, s, partial, stats, nwg);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}
