// The scale-invariance-free loss at any ratio, masked, with its gradient (C ABI and every definition:
// include/sifsr_rloss.h).  The two-pass shape of sif_loss_fwd_kernel / sif_loss_bwd_kernel (loss.hip) over the tables of the sensor
// model (sensor_tables.h: the table kernels of degrade.hip write the weights of R and L and the runs of the adjoint).
//
//  * rloss_counts_kernel   n1 = valid cells, n2 = HR pixels under them (cell i of an axis holds ceil((i + 1) N / n) - ceil(i N / n)
//    pixels): per-thread int64 sums, a fixed tree per workgroup, one integer atomic add per workgroup and counter, onto the zeros
//    rloss_counts_zero_kernel left.
//  * rloss_fwd_kernel      pass A, one workgroup per (image, LR tile of tl x tl cells, tl <= 16 sized from the factor).  Stages the
//    HR pixels the tile's windows of R reach (at most CAP x CAP fp32) in LDS, applies Ry into a float64 LDS intermediate, then one
//    thread per cell applies Rx: e1, r1 = alpha / n1 clamp(e1) (0 and lst unread under an invalid cell).  Then the tile's OWN HR
//    pixels (those whose cell lies in the tile) in chunks of 32 x 32: kind 2 stages d = sr - gamma ndvi with a halo of hw in float64,
//    applies Ly then Lx, e2 = d - L d; kind 1 forms the Sobel bank from global memory.  r2 = (1 - alpha) / (F n2) clamp(e2), 0 under
//    an invalid cell.  The Huber sums leave as two float64 partials per workgroup.
//  * rloss_bwd_kernel      pass B, one workgroup per (image, 32 x 32 HR tile), a thread owns 4 pixels.  dsr = Ry^T r1 Rx gathered over
//    the runs of range_kernel (a few outputs per axis) from global memory, plus r2 - L^T r2 through an LDS tile with a halo of hw
//    (Ly^T into a float64 intermediate, then Lx^T), or the Sobel adjoint.  Workgroup (0, 0, 0) finalises the three loss values.
//  * rloss_finalize_kernel the same finalisation alone, when no gradient is asked for.
// Weights that are zero are skipped, not multiplied: what lies under them (an unstaged LDS entry) is not used.  No float atomics.
#include "../../include/sifsr_rloss.h"

#include "sensor_tables.h"

namespace {

constexpr int RL_MAX_HW = 8;                    // factor <= 8
constexpr double RL_MAX_FACTOR = 8.0;
constexpr int RL_CAP = 80;                      // pass A: most staged HR rows / columns of one LR tile
constexpr int RL_LS = RL_CAP + 1;               // ... and their LDS row stride
constexpr int RL_TL = 16;                       // most LR cells per tile side: RL_TL^2 = one cell per thread
constexpr int RL_CH = 32;                       // side of an HR chunk (pass A) / HR tile (pass B)
constexpr int RL_CS = RL_CH + 2 * RL_MAX_HW;    // ... with its halo: 48
constexpr int RL_CLS = RL_CS + 1;
// LDS of pass A, in doubles: phase 1 S fp32 [CAP][LS] + T f64 [TL][LS]; phase 2 D f64 [CS][CLS] + U f64 [CH][CLS]
constexpr int RL_S_DOUBLES = RL_CAP * RL_LS / 2;
constexpr int RL_A_DOUBLES = RL_S_DOUBLES + RL_TL * RL_LS;
static_assert(RL_CAP * RL_LS % 2 == 0 && RL_CS * RL_CLS + RL_CH * RL_CLS <= RL_A_DOUBLES, "pass A: phase 2 reuses phase 1's LDS");

struct RlArgs {
  const float *sr, *lst, *ndvi;
  const unsigned char* valid;
  const long long* counts;
  const double *wy, *wx, *lwy, *lwx;
  const int4 *my, *mx;
  const int2 *ry, *rx;
  float *r1, *r2;
  double* part;
  float *losses, *dsr;
  long long n1, n2, nblk;       // the unmasked counts B h w and B H W; workgroups of pass A
  int H, W, h, w, K, KL, hw, tl;
  float mean, std, alpha, gamma;
};

__device__ __forceinline__ double huber_d(double e) { const double a = fabs(e); return a < 1.0 ? 0.5 * e * e : a - 0.5; }
__device__ __forceinline__ double clamp_d(double e) { return e < -1.0 ? -1.0 : (e > 1.0 ? 1.0 : e); }   // (a NaN residual stays NaN, as in loss.hip)
__host__ __device__ __forceinline__ long long cdiv_ll(long long a, long long b) { return (a + b - 1) / b; }

// s1 = 1 / n1, s2 = 1 / (F n2) from the counts on the device (or the unmasked ones, by the same expressions); a count <= 0: both 0
__device__ __forceinline__ void rl_scales(const RlArgs& a, int F, double* s1, double* s2) {
  const long long n1 = a.counts != nullptr ? a.counts[0] : a.n1, n2 = a.counts != nullptr ? a.counts[1] : a.n2;
  const bool ok = n1 > 0 && n2 > 0;
  *s1 = ok ? 1.0 / (double)n1 : 0.0;
  *s2 = ok ? 1.0 / ((double)F * (double)n2) : 0.0;
}

// sum over the 256 threads, fixed order; valid in every thread
__device__ __forceinline__ double rl_block_sum(double v, double* sh) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// losses3 from the partials of pass A; called by all 256 threads of ONE workgroup
__device__ __forceinline__ void rl_finalize(const RlArgs& a, int F, double* sh) {
  double s0 = 0.0, s1 = 0.0;
  for (long long k = threadIdx.x; k < a.nblk; k += 256) {
    s0 += a.part[2 * k];
    s1 += a.part[2 * k + 1];
  }
  s0 = rl_block_sum(s0, sh);
  s1 = rl_block_sum(s1, sh);
  if (threadIdx.x == 0) {
    double c1, c2;
    rl_scales(a, F, &c1, &c2);
    const float ds = (float)(s0 * c1), pl = (float)(s1 * c2);
    a.losses[0] = ds;
    a.losses[1] = pl;
    a.losses[2] = a.alpha * ds + (1.f - a.alpha) * pl;
  }
}

__global__ void rloss_counts_zero_kernel(unsigned long long* __restrict__ counts) {
  if (threadIdx.x < 2) counts[threadIdx.x] = 0ull;
}

__global__ __launch_bounds__(256) void rloss_counts_kernel(const unsigned char* __restrict__ valid, int h, int w, int H, int W,
                                                           long long n, unsigned long long* __restrict__ counts) {
  __shared__ long long sh[2][256];
  long long c1 = 0, c2 = 0;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    if (valid[e] == 0) continue;
    const long long j = e % w, i = (e / w) % h;
    c1 += 1;
    c2 += (cdiv_ll((i + 1) * H, h) - cdiv_ll(i * H, h)) * (cdiv_ll((j + 1) * W, w) - cdiv_ll(j * W, w));
  }
  sh[0][threadIdx.x] = c1;
  sh[1][threadIdx.x] = c2;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      sh[0][threadIdx.x] += sh[0][threadIdx.x + st];
      sh[1][threadIdx.x] += sh[1][threadIdx.x + st];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    atomicAdd(counts, (unsigned long long)sh[0][0]);
    atomicAdd(counts + 1, (unsigned long long)sh[1][0]);
  }
}

__device__ __forceinline__ void sobel4_d(const float* __restrict__ img, int H, int W, int y, int x, double o[4]) {
  double n[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
    n[t] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? (double)img[(size_t)yy * W + xx] : 0.0;
  }
  o[0] = (n[0] + 2.0 * n[1] + n[2]) - (n[6] + 2.0 * n[7] + n[8]);
  o[1] = (n[0] + 2.0 * n[3] + n[6]) - (n[2] + 2.0 * n[5] + n[8]);
  o[2] = (2.0 * n[0] + n[1] + n[3]) - (n[5] + n[7] + 2.0 * n[8]);
  o[3] = (n[1] + 2.0 * n[2] + n[5]) - (n[3] + 2.0 * n[6] + n[7]);
}

// pass A.  grid (ceil(w / tl), ceil(h / tl), B), 256 threads
template <int KIND>
__global__ __launch_bounds__(256) void rloss_fwd_kernel(const RlArgs a) {
  __shared__ double lds[RL_A_DOUBLES];
  __shared__ double red[4];
  constexpr int F = KIND == 1 ? 4 : 1;
  const int tid = threadIdx.x, b = blockIdx.z;
  const int H = a.H, W = a.W, h = a.h, w = a.w, K = a.K, tl = a.tl;
  const int i0 = blockIdx.y * tl, j0 = blockIdx.x * tl;
  const int ni = min(tl, h - i0), nj = min(tl, w - j0);
  const size_t img = (size_t)b * H * W;
  double s1, s2;
  rl_scales(a, F, &s1, &s2);
  const double w1 = (double)a.alpha * s1, w2 = (1.0 - (double)a.alpha) * s2;

  // ---- consistency term: R over the pixels the tile's windows reach ----
  int ys = H, ye = -1, xs = W, xe = -1;
  for (int i = 0; i < ni; ++i) {
    const int s = a.my[i0 + i].x;
    ys = min(ys, s);
    ye = max(ye, min(s + K - 1, H - 1));
  }
  for (int j = 0; j < nj; ++j) {
    const int s = a.mx[j0 + j].x;
    xs = min(xs, s);
    xe = max(xe, min(s + K - 1, W - 1));
  }
  // (the spans fit RL_CAP by the choice of tl: tests/test_rloss_host.py holds it; the clamps keep every LDS index inside whatever
  // the tables hold)
  ys = clampi(ys, 0, H - 1);
  xs = clampi(xs, 0, W - 1);
  const int nr = clampi(ye - ys + 1, 1, RL_CAP), nc = clampi(xe - xs + 1, 1, RL_CAP);
  float* S = reinterpret_cast<float*>(lds);
  double* T = lds + RL_S_DOUBLES;
  for (int e = tid; e < nr * nc; e += 256) {
    const int r = e / nc, c = e - r * nc;
    S[r * RL_LS + c] = a.sr[img + (size_t)min(ys + r, H - 1) * W + min(xs + c, W - 1)];
  }
  __syncthreads();
  for (int e = tid; e < ni * nc; e += 256) {
    const int i = e / nc, c = e - i * nc;
    const int start = a.my[i0 + i].x;
    const double* wk = a.wy + (size_t)(i0 + i) * K;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
      const double wgt = wk[k];
      const int r = clampi(min(start + k, H - 1) - ys, 0, RL_CAP - 1);
      acc = wgt != 0.0 ? fma(wgt, (double)S[r * RL_LS + c], acc) : acc;
    }
    T[i * RL_LS + c] = acc;
  }
  __syncthreads();
  double h1 = 0.0, h2 = 0.0;
  if (tid < ni * nj) {
    const int i = tid / nj, j = tid - i * nj;
    const size_t o = ((size_t)b * h + i0 + i) * w + j0 + j;
    float rv = 0.f;
    if (a.valid == nullptr || a.valid[o] != 0) {
      const int start = a.mx[j0 + j].x;
      const double* wk = a.wy + (size_t)(i0 + i) * K;
      double acc = 0.0, sx = 0.0, sy = 0.0;
      for (int k = 0; k < K; ++k) {
        const double wgt = a.wx[(size_t)k * w + j0 + j];
        const int c = clampi(min(start + k, W - 1) - xs, 0, RL_CAP - 1);
        acc = wgt != 0.0 ? fma(wgt, T[i * RL_LS + c], acc) : acc;
        sx += wgt;
        sy += wk[k];
      }
      // R (sr std + mean) = std R sr + mean rowsum(Ry) rowsum(Rx): nothing is rounded at the 300 K scale
      const double dn = acc + ((double)a.mean / (double)a.std) * (sy * sx - 1.0);
      const double e = dn - (double)a.lst[o];
      h1 = huber_d(e);
      rv = (float)(w1 * clamp_d(e));
    }
    a.r1[o] = rv;
  }

  // ---- high-frequency term over the tile's own HR pixels ----
  const int Y0 = (int)cdiv_ll((long long)i0 * H, h), Y1 = (int)cdiv_ll((long long)(i0 + ni) * H, h);
  const int X0 = (int)cdiv_ll((long long)j0 * W, w), X1 = (int)cdiv_ll((long long)(j0 + nj) * W, w);
  const unsigned char* vimg = a.valid != nullptr ? a.valid + (size_t)b * h * w : nullptr;
  if (KIND == 2) {
    const int hw = a.hw, KL = a.KL;
    const double g = (double)a.gamma;
    double* D = lds;
    double* U = lds + RL_CS * RL_CLS;
    for (int cy = Y0; cy < Y1; cy += RL_CH) {
      for (int cx = X0; cx < X1; cx += RL_CH) {
        const int ch = min(RL_CH, Y1 - cy), cw = min(RL_CH, X1 - cx);
        const int sy0 = max(cy - hw, 0), sx0 = max(cx - hw, 0);
        const int sr_n = min(cy + ch - 1 + hw, H - 1) - sy0 + 1, sc_n = min(cx + cw - 1 + hw, W - 1) - sx0 + 1;   // <= RL_CS
        __syncthreads();                                       // the LDS of the phase (or chunk) before is free
        for (int e = tid; e < sr_n * sc_n; e += 256) {
          const int r = e / sc_n, c = e - r * sc_n;
          const size_t p = img + (size_t)(sy0 + r) * W + sx0 + c;
          D[r * RL_CLS + c] = (double)a.sr[p] - g * (double)a.ndvi[p];
        }
        __syncthreads();
        for (int e = tid; e < ch * sc_n; e += 256) {
          const int y = e / sc_n, c = e - y * sc_n;
          const int o = cy + y, start = max(o - hw, 0);
          const double* wk = a.lwy + (size_t)o * KL;
          double acc = 0.0;
          for (int k = 0; k < KL; ++k) {
            const double wgt = wk[k];
            const int r = clampi(min(start + k, H - 1) - sy0, 0, RL_CS - 1);
            acc = wgt != 0.0 ? fma(wgt, D[r * RL_CLS + c], acc) : acc;
          }
          U[y * RL_CLS + c] = acc;
        }
        __syncthreads();
        for (int e = tid; e < ch * cw; e += 256) {
          const int y = e / cw, x = e - y * cw;
          const int Y = cy + y, X = cx + x, start = max(X - hw, 0);
          double acc = 0.0;
          for (int k = 0; k < KL; ++k) {
            const double wgt = a.lwx[(size_t)k * W + X];
            const int c = clampi(min(start + k, W - 1) - sx0, 0, RL_CS - 1);
            acc = wgt != 0.0 ? fma(wgt, U[y * RL_CLS + c], acc) : acc;
          }
          const double e2 = D[(Y - sy0) * RL_CLS + (X - sx0)] - acc;
          const bool ok = vimg == nullptr || vimg[(size_t)((long long)Y * h / H) * w + (size_t)((long long)X * w / W)] != 0;
          h2 += ok ? huber_d(e2) : 0.0;
          a.r2[img + (size_t)Y * W + X] = ok ? (float)(w2 * clamp_d(e2)) : 0.f;
        }
      }
    }
  } else {
    const int oh_ = Y1 - Y0, ow_ = X1 - X0;
    const double g = (double)a.gamma;
    for (int e = tid; e < oh_ * ow_; e += 256) {
      const int y = e / ow_, Y = Y0 + y, X = X0 + (e - y * ow_);
      const bool ok = vimg == nullptr || vimg[(size_t)((long long)Y * h / H) * w + (size_t)((long long)X * w / W)] != 0;
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (ok) {
        double s[4], n[4], r[4];
        sobel4_d(a.sr + img, H, W, Y, X, s);
        sobel4_d(a.ndvi + img, H, W, Y, X, n);
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          const double e2 = s[f] - g * n[f];
          h2 += huber_d(e2);
          r[f] = w2 * clamp_d(e2);
        }
        o = make_float4((float)r[0], (float)r[1], (float)r[2], (float)r[3]);
      }
      st4(a.r2 + (img + (size_t)Y * W + X) * 4, o);
    }
  }
  h1 = rl_block_sum(h1, red);
  h2 = rl_block_sum(h2, red);
  if (tid == 0) {
    const size_t blk = ((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    a.part[2 * blk] = h1;
    a.part[2 * blk + 1] = h2;
  }
}

// pass B.  grid (ceil(W / 32), ceil(H / 32), B), 256 threads: thread (tx, ty) owns pixels (y0 + ty + 8 r, x0 + tx), r < 4
template <int KIND>
__global__ __launch_bounds__(256) void rloss_bwd_kernel(const RlArgs a) {
  __shared__ float V[RL_CS * RL_CLS];
  __shared__ double U[RL_CH * RL_CLS];
  __shared__ double red[4];
  constexpr int F = KIND == 1 ? 4 : 1;
  const int tid = threadIdx.x, b = blockIdx.z, tx = tid & 31, ty = tid >> 5;
  const int H = a.H, W = a.W, h = a.h, w = a.w, K = a.K;
  const int x0 = blockIdx.x * RL_CH, y0 = blockIdx.y * RL_CH;
  const size_t img = (size_t)b * H * W;
  const float* r1 = a.r1 + (size_t)b * h * w;
  double acc[4];
  // Ry^T r1 Rx over the runs of outputs whose stencil holds the pixel
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int Y = y0 + ty + 8 * r, X = x0 + tx;
    double s = 0.0;
    if (Y < H && X < W) {
      const int2 ry = a.ry[Y], rx = a.rx[X];
      for (int i = ry.x; i <= ry.y; ++i) {
        const int ky = Y - a.my[i].x;
        if (ky < 0 || ky >= K) continue;
        const double wyv = a.wy[(size_t)i * K + ky];
        if (wyv == 0.0) continue;
        double inner = 0.0;
        for (int j = rx.x; j <= rx.y; ++j) {
          const int kx = X - a.mx[j].x;
          if (kx < 0 || kx >= K) continue;
          const double wxv = a.wx[(size_t)kx * w + j];
          inner = wxv != 0.0 ? fma(wxv, (double)r1[(size_t)i * w + j], inner) : inner;
        }
        s = fma(wyv, inner, s);
      }
    }
    acc[r] = s;
  }
  if (KIND == 2) {
    const int hw = a.hw, KL = a.KL;
    const int ch = min(RL_CH, H - y0), cw = min(RL_CH, W - x0);
    const int sy0 = max(y0 - hw, 0), sx0 = max(x0 - hw, 0);
    const int sr_n = min(y0 + ch - 1 + hw, H - 1) - sy0 + 1, sc_n = min(x0 + cw - 1 + hw, W - 1) - sx0 + 1;       // <= RL_CS
    for (int e = tid; e < sr_n * sc_n; e += 256) {
      const int r = e / sc_n, c = e - r * sc_n;
      V[r * RL_CLS + c] = a.r2[img + (size_t)(sy0 + r) * W + sx0 + c];
    }
    __syncthreads();
    // U[y][c] = sum over rows o of L that read row Y = y0 + y: Ly[o][Y] V[o][c]
    for (int e = tid; e < ch * sc_n; e += 256) {
      const int y = e / sc_n, c = e - y * sc_n, Y = y0 + y;
      double s = 0.0;
      for (int o = max(Y - hw, 0); o <= min(Y + hw, H - 1); ++o) {
        const double wgt = a.lwy[(size_t)o * KL + (Y - max(o - hw, 0))];
        s = wgt != 0.0 ? fma(wgt, (double)V[(o - sy0) * RL_CLS + c], s) : s;
      }
      U[y * RL_CLS + c] = s;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int y = ty + 8 * r, Y = y0 + y, X = x0 + tx;
      if (Y >= H || X >= W) continue;
      double s = 0.0;
      for (int p = max(X - hw, 0); p <= min(X + hw, W - 1); ++p) {
        const double wgt = a.lwx[(size_t)(X - max(p - hw, 0)) * W + p];
        s = wgt != 0.0 ? fma(wgt, U[y * RL_CLS + (p - sx0)], s) : s;
      }
      acc[r] += (double)V[(Y - sy0) * RL_CLS + (X - sx0)] - s;
    }
  } else {
    const double Fk[4][9] = {{1, 2, 1, 0, 0, 0, -1, -2, -1}, {1, 0, -1, 2, 0, -2, 1, 0, -1},
                             {2, 1, 0, 1, 0, -1, 0, -1, -2}, {0, 1, 2, -1, 0, 1, -2, -1, 0}};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int Y = y0 + ty + 8 * r, X = x0 + tx;
      if (Y >= H || X >= W) continue;
      double s = 0.0;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int yy = Y - (t / 3 - 1), xx = X - (t % 3 - 1);
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
          const float4 g = ld4(a.r2 + (img + (size_t)yy * W + xx) * 4);
          s += Fk[0][t] * (double)g.x + Fk[1][t] * (double)g.y + Fk[2][t] * (double)g.z + Fk[3][t] * (double)g.w;
        }
      }
      acc[r] += s;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int Y = y0 + ty + 8 * r, X = x0 + tx;
    if (Y < H && X < W) a.dsr[img + (size_t)Y * W + X] = (float)acc[r];
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) rl_finalize(a, F, red);   // (workgroup-uniform)
}

__global__ __launch_bounds__(256) void rloss_finalize_kernel(const RlArgs a, int F) {
  __shared__ double red[4];
  rl_finalize(a, F, red);
}

struct RlPlan {
  int hw, K, KL, h, w, tl, ty, tx;
  Axis ay, ax;
  size_t wy, wx, my, mx, ry, rx, lwy, lwx, lmy, lmx, r1, r2, part, bytes;
  long long nblk;
};

bool rl_plan_of(int kind, int B, int H, int W, double factor, RlPlan* p) {
  if ((kind != 1 && kind != 2) || !(factor > 1.0 && factor <= RL_MAX_FACTOR) || B < 1 || B > MAX_BATCH) return false;
  p->hw = (int)ceil(factor);
  if (p->hw < 1 || p->hw > RL_MAX_HW) return false;
  if (!axis_of(H, factor, p->hw, 1, &p->ay) || !axis_of(W, factor, p->hw, 1, &p->ax)) return false;
  p->K = 2 * p->hw + 4;
  p->KL = 2 * p->hw + 1;
  p->h = p->ay.count;
  p->w = p->ax.count;
  // the windows of tl consecutive outputs span at most factor (tl - 1) + K + 2 pixels of an axis
  int tl = (int)floor((double)(RL_CAP - p->K - 2) / factor) + 1;
  p->tl = tl < 1 ? 1 : (tl > RL_TL ? RL_TL : tl);
  p->ty = (p->h + p->tl - 1) / p->tl;
  p->tx = (p->w + p->tl - 1) / p->tl;
  p->nblk = (long long)B * p->ty * p->tx;
  const size_t hr = (size_t)B * H * W, lr = (size_t)B * p->h * p->w;
  size_t off = 0;
  auto take = [&off](size_t bytes) { const size_t at = off; off = up16(off + bytes); return at; };
  p->wy = take((size_t)p->h * p->K * sizeof(double));
  p->wx = take((size_t)p->w * p->K * sizeof(double));
  p->my = take((size_t)p->h * sizeof(int4));
  p->mx = take((size_t)p->w * sizeof(int4));
  p->ry = take((size_t)H * sizeof(int2));
  p->rx = take((size_t)W * sizeof(int2));
  p->lwy = take(kind == 2 ? (size_t)H * p->KL * sizeof(double) : 0);
  p->lwx = take(kind == 2 ? (size_t)W * p->KL * sizeof(double) : 0);
  p->lmy = take(kind == 2 ? (size_t)H * sizeof(int4) : 0);
  p->lmx = take(kind == 2 ? (size_t)W * sizeof(int4) : 0);
  p->r1 = take(lr * sizeof(float));
  p->r2 = take((kind == 1 ? 4 : 1) * hr * sizeof(float));
  p->part = take((size_t)p->nblk * 2 * sizeof(double));
  p->bytes = off;
  return true;
}

}  // namespace

// ---- C ABI (include/sifsr_rloss.h) ----
size_t sifsrq_sif_loss_workspace_bytes(int kind, int B, int H, int W, double factor) {
  RlPlan p;
  return rl_plan_of(kind, B, H, W, factor, &p) ? p.bytes : 0;
}

int sifsrq_valid_counts(const unsigned char* valid, int B, int h, int w, int H, int W, long long* counts2, void* stream) {
  if (!valid || !counts2 || !aligned(counts2, 8)) return SIFSR_ERR_ARG;
  if (B < 1 || B > MAX_BATCH || h < 1 || w < 1 || h > H || w > W || H > MAX_SIDE || W > MAX_SIDE) return SIFSR_ERR_SHAPE;
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts2);
  hipLaunchKernelGGL(rloss_counts_zero_kernel, dim3(1), dim3(64), 0, s, counts);   // (a kernel, not a memset node: the chain stays kernels)
  SIFSR_LAUNCH_CHECK();
  const long long n = (long long)B * h * w;
  const long long blocks = (n + 4095) / 4096;                // 16 cells per thread, at most 1024 workgroups
  hipLaunchKernelGGL(rloss_counts_kernel, dim3((unsigned)(blocks > 1024 ? 1024 : blocks)), dim3(256), 0, s, valid, h, w, H, W, n,
                     counts);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrq_sif_loss(int kind, const float* sr, const float* lst, const unsigned char* valid, const long long* counts2,
                    const float* ndvi, int B, int H, int W, double factor, float mean, float std, float alpha, float gamma,
                    void* workspace, size_t workspace_bytes, float* losses3, float* dsr, void* stream) {
  if (!sr || !lst || !ndvi || !workspace || !losses3 || (valid == nullptr) != (counts2 == nullptr) || (kind != 1 && kind != 2) ||
      !aligned(workspace, 16) || !aligned(sr, 4) || !aligned(lst, 4) || !aligned(ndvi, 4) || !aligned(losses3, 4) || !aligned(dsr, 4) ||
      !aligned(counts2, 8))
    return SIFSR_ERR_ARG;
  RlPlan p;
  if (!rl_plan_of(kind, B, H, W, factor, &p)) return SIFSR_ERR_SHAPE;
  if (workspace_bytes < p.bytes) return SIFSR_ERR_WORKSPACE;

  char* ws = static_cast<char*>(workspace);
  double* wy = reinterpret_cast<double*>(ws + p.wy);
  double* wx = reinterpret_cast<double*>(ws + p.wx);
  int4* my = reinterpret_cast<int4*>(ws + p.my);
  int4* mx = reinterpret_cast<int4*>(ws + p.mx);
  int2* ry = reinterpret_cast<int2*>(ws + p.ry);
  int2* rx = reinterpret_cast<int2*>(ws + p.rx);
  double* lwy = reinterpret_cast<double*>(ws + p.lwy);
  double* lwx = reinterpret_cast<double*>(ws + p.lwx);
  hipStream_t s = (hipStream_t)stream;

  hipLaunchKernelGGL(degrade_table_kernel, dim3(((p.h > p.w ? p.h : p.w) * p.K + 255) / 256, 2), dim3(256), 0, s, psf_of(factor, 0.1, p.hw),
                     p.ay, p.ax, wy, wx, my, mx);
  SIFSR_LAUNCH_CHECK();
  if (kind == 2) {
    const Axis ly = Axis{H, H + 2 * p.hw, H, 0}, lx = Axis{W, W + 2 * p.hw, W, 0};
    hipLaunchKernelGGL(lowpass_table_kernel, dim3(((H > W ? H : W) * p.KL + 255) / 256, 2), dim3(256), 0, s, psf_of(factor, 0.25, p.hw), ly,
                       lx, lwy, lwx, reinterpret_cast<int4*>(ws + p.lmy), reinterpret_cast<int4*>(ws + p.lmx));
    SIFSR_LAUNCH_CHECK();
  }
  if (dsr != nullptr) {
    hipLaunchKernelGGL(range_kernel, dim3(((H > W ? H : W) + 255) / 256, 2), dim3(256), 0, s, my, mx, ry, rx, H, W, p.h, p.w);
    SIFSR_LAUNCH_CHECK();
  }
  RlArgs a;
  a.sr = sr; a.lst = lst; a.ndvi = ndvi; a.valid = valid; a.counts = counts2;
  a.wy = wy; a.wx = wx; a.lwy = lwy; a.lwx = lwx; a.my = my; a.mx = mx; a.ry = ry; a.rx = rx;
  a.r1 = reinterpret_cast<float*>(ws + p.r1);
  a.r2 = reinterpret_cast<float*>(ws + p.r2);
  a.part = reinterpret_cast<double*>(ws + p.part);
  a.losses = losses3; a.dsr = dsr;
  a.n1 = (long long)B * p.h * p.w; a.n2 = (long long)B * H * W; a.nblk = p.nblk;
  a.H = H; a.W = W; a.h = p.h; a.w = p.w; a.K = p.K; a.KL = p.KL; a.hw = p.hw; a.tl = p.tl;
  a.mean = mean; a.std = std; a.alpha = alpha; a.gamma = gamma;
  const dim3 ga(p.tx, p.ty, B), gb((W + RL_CH - 1) / RL_CH, (H + RL_CH - 1) / RL_CH, B);
  if (kind == 2) hipLaunchKernelGGL(rloss_fwd_kernel<2>, ga, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(rloss_fwd_kernel<1>, ga, dim3(256), 0, s, a);
  SIFSR_LAUNCH_CHECK();
  if (dsr == nullptr) hipLaunchKernelGGL(rloss_finalize_kernel, dim3(1), dim3(256), 0, s, a, kind == 1 ? 4 : 1);
  else if (kind == 2) hipLaunchKernelGGL(rloss_bwd_kernel<2>, gb, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(rloss_bwd_kernel<1>, gb, dim3(256), 0, s, a);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}
