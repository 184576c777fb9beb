// Conservation of the observed LST (C ABI and every definition: include/sifsr_conserve.h): the residual
// r = lst - D(sr) over the cells where it is defined, its statistics, and the correction sr += relax * U(r).
//
//  * conserve_residual_kernel   one workgroup per 32 x 32 HR tile = 8 x 8 cells, the reflect-padded 40 x 40 halo in LDS as
//    blurdec_fwd_kernel (loss.hip) has it.  sr is read ONCE, 16 bytes per load where the halo is not reflected; the validity of the
//    10 x 10 cells under the halo is decided from the values just loaded.  PSF and decimation are one 12-tap filter per axis
//    (q = k4 * taps9): a horizontal pass at the 8 cell columns only (40 x 8 dot products), a vertical pass at the 8 x 8 cells.  The
//    tile is held as deviations from c0, the lst of the tile's first valid cell, so the residual is not the difference of two rounded
//    300 K sums.  Wave 0 emits the 64 residuals, the cells' validity bytes and four float64 partials (sum r, sum r^2, max |r|, count).
//  * conserve_apply_kernel      one thread per row of a cell: 4 HR pixels, one 16-byte load, one 16-byte store (the access pattern
//    of gaps_blend_kernel); the 4 x 5 residuals around the cell come from L2, the four x4 phases from constants.  A cell without c
//    keeps its bits (in place: it is not touched at all).
//  * conserve_finish_kernel     one workgroup per statistics row adds the partials in a fixed order.
// No atomics, no allocation, no host synchronisation; nothing depends on the order in which workgroups run.
#include "../../include/sifsr_conserve.h"

#include "common.h"

namespace {

constexpr int T = 32;          // HR tile edge
constexpr int R = 4;           // PSF half width
constexpr int TP = T + 2 * R;  // 40
constexpr int LS = TP + 1;     // LDS row stride of the halo
constexpr int NC = T / 4;      // 8 cells per tile side
constexpr int CP = NC + 2;     // 10: with the ring of neighbours
constexpr int MS = 10;         // LDS row stride of the horizontal pass (8 cell columns)
constexpr int MAX_ITER = 64;

struct Filter {
  float q[12];  // k4 * taps9
  float eps;    // sum(taps9)^2 - 1
};

__device__ __forceinline__ int refl(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }
__device__ __forceinline__ bool good(float v) { return isfinite(v) && v != 0.f; }

__global__ __launch_bounds__(256) void conserve_residual_kernel(const float* __restrict__ sr, const float* __restrict__ lst,
                                                                const unsigned char* __restrict__ mask, float* __restrict__ r,
                                                                unsigned char* __restrict__ cval, double* __restrict__ partial,
                                                                const Filter k, int h, int w) {
  __shared__ float L[TP * LS], M[TP * MS], lv[CP * CP];
  __shared__ int ok[CP * CP], bad[CP * CP], first;
  const int tid = threadIdx.x, H = 4 * h, W = 4 * w;
  const int x0 = blockIdx.x * T, y0 = blockIdx.y * T, i0 = blockIdx.y * NC, j0 = blockIdx.x * NC;

  // the halo, 10 groups of 4 pixels per row, into registers first: the loads are in flight while the cells are set up
  float4 v[2];
  int cell[2];
  bool inside[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int g = tid + 256 * s;
    v[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    cell[s] = 0;
    inside[s] = false;
    if (g < TP * (TP / 4)) {
      const int py = g / (TP / 4), gx = g - py * (TP / 4);
      const int ry = y0 - R + py, rx = x0 - R + 4 * gx;
      // partial tiles reach past the raster: clamp to the last halo coordinate (n-1+R) before reflecting; the LDS entries beyond it
      // only feed cells that are never stored
      const float* row = sr + (size_t)refl(min(ry, H - 1 + R), H) * W;
      if (rx >= 0 && rx + 3 < W) {
        v[s] = ld4(row + rx);
      } else {
        v[s].x = row[refl(min(rx, W - 1 + R), W)];
        v[s].y = row[refl(min(rx + 1, W - 1 + R), W)];
        v[s].z = row[refl(min(rx + 2, W - 1 + R), W)];
        v[s].w = row[refl(min(rx + 3, W - 1 + R), W)];
      }
      cell[s] = (py >> 2) * CP + gx;                              // ry >> 2 = i0 - 1 + (py >> 2)
      inside[s] = ry >= 0 && ry < H && rx >= 0 && rx < W;         // not a reflected or clamped copy
    }
  }
  // the lst part of c for the 10 x 10 cells; a cell outside the raster is clipped from every neighbourhood: it passes
  if (tid < CP * CP) {
    const int ci = tid / CP, cj = tid - ci * CP;
    const int gi = i0 - 1 + ci, gj = j0 - 1 + cj;
    float f = 0.f;
    int o = 1;
    if (gi >= 0 && gi < h && gj >= 0 && gj < w) {
      const size_t p = (size_t)gi * w + gj;
      f = lst[p];
      o = (good(f) && (mask == nullptr || mask[p] != 0)) ? 1 : 0;
    }
    lv[tid] = f;
    ok[tid] = o;
    bad[tid] = 0;
  }
  __syncthreads();
  // the sr part: any pixel of the cell that is not finite or is 0 (every writer stores the same value)
#pragma unroll
  for (int s = 0; s < 2; ++s)
    if (inside[s] && !(good(v[s].x) && good(v[s].y) && good(v[s].z) && good(v[s].w))) bad[cell[s]] = 1;
  __syncthreads();
  const int ti = tid >> 3, tj = tid & 7;                          // wave 0: cell (ti, tj) of the tile
  const int own = (ti + 1) * CP + tj + 1;
  const bool in_raster = tid < 64 && i0 + ti < h && j0 + tj < w;
  bool c = false;
  if (tid < 64) {
    c = in_raster && ok[own] != 0 && bad[own] == 0;
    const unsigned long long m = __ballot(c);
    if (tid == 0) first = m ? (int)__ffsll((long long)m) - 1 : -1;
  }
  __syncthreads();
  const int f0 = first;
  const float c0 = f0 >= 0 ? lv[((f0 >> 3) + 1) * CP + (f0 & 7) + 1] : 0.f;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int g = tid + 256 * s;
    if (g < TP * (TP / 4)) {
      const int py = g / (TP / 4), gx = g - py * (TP / 4);
      float* d = L + py * LS + 4 * gx;
      d[0] = v[s].x - c0; d[1] = v[s].y - c0; d[2] = v[s].z - c0; d[3] = v[s].w - c0;
    }
  }
  __syncthreads();
  // horizontal: M[py][j] = sum_u q[u] L[py][4j + u]   (HR columns 4(j0 + j) - 4 .. + 7)
  for (int e = tid; e < TP * NC; e += 256) {
    const int py = e >> 3, j = e & 7;
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < 12; ++u) s = fmaf(k.q[u], L[py * LS + 4 * j + u], s);
    M[py * MS + j] = s;
  }
  __syncthreads();
  if (tid < 64) {
    float d = 0.f;
#pragma unroll
    for (int u = 0; u < 12; ++u) d = fmaf(k.q[u], M[(4 * ti + u) * MS + tj], d);
    bool counted = c;
#pragma unroll
    for (int a = -1; a <= 1; ++a)
#pragma unroll
      for (int b = -1; b <= 1; ++b) counted = counted && ok[own + a * CP + b] != 0 && bad[own + a * CP + b] == 0;
    // lst - D(sr) = (lst - c0) - D(sr - c0) - c0 (S^2 - 1)
    const float res = counted ? fmaf(-c0, k.eps, (lv[own] - c0) - d) : 0.f;
    if (in_raster) {
      const size_t p = (size_t)(i0 + ti) * w + j0 + tj;
      r[p] = res;
      cval[p] = c ? 1 : 0;
    }
    double s1 = (double)res, s2 = (double)res * (double)res, mx = fabs((double)res), n = counted ? 1.0 : 0.0;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      s1 += __shfl_down(s1, o);
      s2 += __shfl_down(s2, o);
      mx = fmax(mx, __shfl_down(mx, o));
      n += __shfl_down(n, o);
    }
    if (tid == 0) {
      double* o = partial + 4 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
      o[0] = s1; o[1] = s2; o[2] = mx; o[3] = n;
    }
  }
}

// cv2 INTER_CUBIC x4 (A = -0.75): the coefficients of t = 0.625, 0.875, 0.125, 0.375 for the output phases 0 .. 3
__device__ const float UP4[4][4] = {{-0.06591796875f, 0.42626953125f, 0.74951171875f, -0.10986328125f},
                                    {-0.01025390625f, 0.11474609375f, 0.96728515625f, -0.07177734375f},
                                    {-0.07177734375f, 0.96728515625f, 0.11474609375f, -0.01025390625f},
                                    {-0.10986328125f, 0.74951171875f, 0.42626953125f, -0.06591796875f}};

__device__ __forceinline__ float dot4(float a, float b, float c, float d, const float* k) {
  return fmaf(d, k[3], fmaf(c, k[2], fmaf(b, k[1], a * k[0])));
}

// block = 64 x 4 threads: thread (x, y) owns row y of cell (blockIdx.y, 64 blockIdx.x + x).  out may be sr itself.
__global__ __launch_bounds__(256) void conserve_apply_kernel(const float* sr, const float* __restrict__ r,
                                                             const unsigned char* __restrict__ cval, float* out, int h, int w,
                                                             float relax) {
  const int J = blockIdx.x * 64 + threadIdx.x, I = blockIdx.y, py = threadIdx.y;
  if (J >= w) return;
  const size_t p = (size_t)(4 * I + py) * (4 * (size_t)w) + 4 * (size_t)J;
  if (cval[(size_t)I * w + J] == 0) {
    if (out != sr) st4(out + p, ld4(sr + p));
    return;
  }
  const float4 s = ld4(sr + p);
  int cj[5];
#pragma unroll
  for (int b = 0; b < 5; ++b) cj[b] = clampi(J - 2 + b, 0, w - 1);
  const int rb = I - 2 + (py >> 1);                    // phases 0, 1 read rows I-2 .. I+1, phases 2, 3 rows I-1 .. I+2
  float hx[4][4];                                      // [source row][output phase]
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float* row = r + (size_t)clampi(rb + a, 0, h - 1) * w;
    const float e0 = row[cj[0]], e1 = row[cj[1]], e2 = row[cj[2]], e3 = row[cj[3]], e4 = row[cj[4]];
    hx[a][0] = dot4(e0, e1, e2, e3, UP4[0]);
    hx[a][1] = dot4(e0, e1, e2, e3, UP4[1]);
    hx[a][2] = dot4(e1, e2, e3, e4, UP4[2]);
    hx[a][3] = dot4(e1, e2, e3, e4, UP4[3]);
  }
  const float* ky = UP4[py];
  float4 o;
  o.x = fmaf(relax, dot4(hx[0][0], hx[1][0], hx[2][0], hx[3][0], ky), s.x);
  o.y = fmaf(relax, dot4(hx[0][1], hx[1][1], hx[2][1], hx[3][1], ky), s.y);
  o.z = fmaf(relax, dot4(hx[0][2], hx[1][2], hx[2][2], hx[3][2], ky), s.z);
  o.w = fmaf(relax, dot4(hx[0][3], hx[1][3], hx[2][3], hx[3][3], ky), s.w);
  st4(out + p, o);
}

// one workgroup per statistics row: thread t adds the partials t, t + 256, ... in that order, then a fixed tree over the threads
__global__ __launch_bounds__(256) void conserve_finish_kernel(const double* __restrict__ partial, double* __restrict__ stats, int nwg) {
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

struct Plan {
  int gx, gy;                              // residual grid
  size_t part_off, cval_off, bytes;        // r at 0
};

bool plan_of(int h, int w, int n_iter, Plan* p) {
  if (h < 3 || w < 3 || h > 16384 || w > 16384 || n_iter < 0 || n_iter > MAX_ITER) return false;
  p->gx = (w + NC - 1) / NC;
  p->gy = (h + NC - 1) / NC;
  const size_t cells = (size_t)h * w;
  p->part_off = (cells * sizeof(float) + 7) & ~(size_t)7;
  p->cval_off = p->part_off + (size_t)(n_iter + 1) * p->gx * p->gy * 4 * sizeof(double);
  p->bytes = p->cval_off + cells;
  return true;
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

// ---- C ABI (include/sifsr_conserve.h) ----
size_t sifsrk_workspace_bytes(int h, int w, int n_iter) {
  Plan p;
  return plan_of(h, w, n_iter, &p) ? p.bytes : 0;
}

int sifsrk_conserve(const float* sr, const float* lst, const unsigned char* mask, float* out, double* stats, void* workspace,
                    size_t workspace_bytes, int h, int w, const float* taps9, float relax, int n_iter, void* stream) {
  if (!sr || !lst || !stats || !workspace || !taps9 || !aligned(workspace, 8) || !aligned(sr, 16) || !aligned(stats, 8))
    return SIFSR_ERR_ARG;
  Plan p;
  if (!plan_of(h, w, n_iter, &p)) return SIFSR_ERR_SHAPE;
  if (n_iter > 0 && (!out || !aligned(out, 16))) return SIFSR_ERR_ARG;
  if (!(relax - relax == 0.f)) return SIFSR_ERR_ARG;              // NaN or inf
  if (workspace_bytes < p.bytes) return SIFSR_ERR_WORKSPACE;

  Filter k;
  const double k4[4] = {-0.09375, 0.59375, 0.59375, -0.09375};
  double S = 0.0;
  for (int t = 0; t < 9; ++t) S += (double)taps9[t];
  for (int u = 0; u < 12; ++u) {
    double q = 0.0;
    for (int a = 0; a < 4; ++a)
      if (u - a >= 0 && u - a < 9) q += k4[a] * (double)taps9[u - a];
    k.q[u] = (float)q;
  }
  k.eps = (float)(S * S - 1.0);

  char* ws = static_cast<char*>(workspace);
  float* r = reinterpret_cast<float*>(ws);
  double* partial = reinterpret_cast<double*>(ws + p.part_off);
  unsigned char* cval = reinterpret_cast<unsigned char*>(ws + p.cval_off);
  const int nwg = p.gx * p.gy;
  hipStream_t s = (hipStream_t)stream;
  const float* cur = sr;
  for (int it = 0; it <= n_iter; ++it) {
    hipLaunchKernelGGL(conserve_residual_kernel, dim3(p.gx, p.gy), dim3(256), 0, s, cur, lst, mask, r, cval,
                       partial + 4 * (size_t)it * nwg, k, h, w);
    SIFSR_LAUNCH_CHECK();
    if (it == n_iter) break;
    hipLaunchKernelGGL(conserve_apply_kernel, dim3((w + 63) / 64, h), dim3(64, 4), 0, s, cur, r, cval, out, h, w, relax);
    SIFSR_LAUNCH_CHECK();
    cur = out;
  }
  hipLaunchKernelGGL(conserve_finish_kernel, dim3(n_iter + 1), dim3(256), 0, s, partial, stats, nwg);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}
