// Fine-tuning a trained model on the granule it is about to predict (C ABI: include/sifsr_adapt.h).
//
//  * bn_frozen_stats_kernel   mean / invstd of the 17 BatchNorm layers from the running statistics, for the backward's reductions
//    (scale / shift are bn_eval_coeffs_kernel's: the frozen forward IS the eval-mode forward, in the training workspace).
//  * conv_in_dgrad_kernel     the 16 -> 2 input gradient of inbloc.bloc.0 under replicate padding.  Two phases per tile:
//      1. every pixel q of a 32 x 16 halo tile forms dy[q][16] from (g, y) and the float64 coefficients -- the expression of
//         conv_in_wgrad_fused, edge_conv.hip -- and T[q][ci*9+t] = sum_co w[co][ci][t] * dy[q][co]: 18 numbers, 288 FMAs with the
//         weights at uniform, compile-time offsets (scalar loads; dy never goes to LDS).  T of a pixel outside the image is 0.
//      2. every pixel p of the 30 x 14 interior gathers dX[p][ci] = sum_t sum_{q : clamp(q + d_t) = p} T[q][ci*9+t]: q = p - d_t,
//         and for a p on the image border also the q whose tap fell outside the image and was clamped onto p (p itself on that
//         axis; both axes at a corner).  18 LDS reads per pixel (19-float pixel stride: conflict-free), fixed order, no atomics.
//  * tile_targets_kernel / tile_count_kernel   the loss targets of `count` active tiles, cyclic over the active list, and their
//    number of valid cells (one workgroup, integer sum: order-free).
#include "../../include/sifsr_adapt.h"

#include "engine.h"
#include "mosaic.h"

namespace {

struct BnRunTable { int run_off[SIFSR_NUM_BN_LAYERS], ch_off[SIFSR_NUM_BN_LAYERS], cout[SIFSR_NUM_BN_LAYERS]; };

__global__ void bn_frozen_stats_kernel(const float* __restrict__ running, float eps, float* __restrict__ mean,
                                       float* __restrict__ invstd, const BnRunTable tb) {
  const int l = blockIdx.x, c = threadIdx.x;
  if (c >= tb.cout[l]) return;
  mean[tb.ch_off[l] + c] = running[tb.run_off[l] + c];
  invstd[tb.ch_off[l] + c] = 1.f / sqrtf(running[tb.run_off[l] + tb.cout[l] + c] + eps);
}

constexpr int DG_HW = 32, DG_HH = 16;            // halo tile: 512 pixels, two per thread
constexpr int DG_TW = DG_HW - 2, DG_TH = DG_HH - 2;   // the pixels it completes
constexpr int DG_PS = 19;                        // LDS pixel stride in floats (18 values; odd: consecutive pixels, distinct banks)

__global__ __launch_bounds__(256) void conv_in_dgrad_kernel(const float* __restrict__ g, const float* __restrict__ y,
                                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                                            const double* __restrict__ coef, const float* __restrict__ w,
                                                            float* __restrict__ dx, int H, int W, int tiles_x, int tiles_y) {
  SIFSR_CHAIN_PRIO();
  __shared__ float T[DG_HW * DG_HH * DG_PS];
  const int tid = threadIdx.x;
  const int tl = blockIdx.x;
  const int tx = tl % tiles_x, ty = (tl / tiles_x) % tiles_y, b = tl / (tiles_x * tiles_y);
  const int x0 = tx * DG_TW, y0 = ty * DG_TH;

  // ---- phase 1: halo pixels tid and tid + 256 (rows hy and hy + 8) ----
  f32x2 dyv[16];                                   // .x: pixel tid, .y: pixel tid + 256 -- one packed FMA serves both
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int q = tid + 256 * k;
    const int gy = y0 - 1 + q / DG_HW, gx = x0 - 1 + q % DG_HW;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    const size_t off = in ? ((size_t)(b * H + gy) * W + gx) * 16 : 0;
#pragma unroll
    for (int c4 = 0; c4 < 4; ++c4) {
      float4 gv = make_float4(0.f, 0.f, 0.f, 0.f), yv = gv;
      if (in) { gv = ld4(g + off + 4 * c4); yv = ld4(y + off + 4 * c4); }
      const float gg[4] = {gv.x, gv.y, gv.z, gv.w}, yy[4] = {yv.x, yv.y, yv.z, yv.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = 4 * c4 + j;
        const float dz = fmaf(yy[j], scale[c], shift[c]) > 0.f ? gg[j] : 0.f;
        const float v = (float)fma(coef[c], (double)dz, fma(coef[16 + c], (double)yy[j], coef[32 + c]));
        dyv[c][k] = in ? v : 0.f;
      }
    }
  }
  f32x2 acc[18];
#pragma unroll
  for (int n = 0; n < 18; ++n) acc[n] = (f32x2){0.f, 0.f};
#pragma unroll
  for (int co = 0; co < 16; ++co) {
#pragma unroll
    for (int n = 0; n < 18; ++n) {
      const float wv = w[co * 18 + n];             // OIHW (16,2,3,3): n = ci * 9 + tap
      acc[n] = __builtin_elementwise_fma((f32x2){wv, wv}, dyv[co], acc[n]);
    }
  }
#pragma unroll
  for (int k = 0; k < 2; ++k)
#pragma unroll
    for (int n = 0; n < 18; ++n) T[(tid + 256 * k) * DG_PS + n] = acc[n][k];
  __syncthreads();

  // ---- phase 2: gather ----
  for (int o = tid; o < DG_TW * DG_TH; o += 256) {
    const int ly = o / DG_TW, lx = o - ly * DG_TW;
    const int py = y0 + ly, px = x0 + lx;
    if (py >= H || px >= W) continue;
    const int hy = ly + 1, hx = lx + 1;            // p in halo coordinates
#pragma unroll
    for (int ci = 0; ci < 2; ++ci) {
      float s = 0.f;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        // the tap (ky, kx) of q reads clamp(q + (ky - 1, kx - 1)): q = p - d, and q = p on an axis where q + d left the image
        const bool fy = (py == 0 && ky == 0) || (py == H - 1 && ky == 2);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
          const bool fx = (px == 0 && kx == 0) || (px == W - 1 && kx == 2);
          const int n = ci * 9 + ky * 3 + kx;
          const int qy = hy - (ky - 1), qx = hx - (kx - 1);
          float v = T[(qy * DG_HW + qx) * DG_PS + n];
          if (fy) v += T[(hy * DG_HW + qx) * DG_PS + n];
          if (fx) v += T[(qy * DG_HW + hx) * DG_PS + n];
          if (fy && fx) v += T[(hy * DG_HW + hx) * DG_PS + n];
          s += v;
        }
      }
      dx[((size_t)(b * 2 + ci) * H + py) * W + px] = s;
    }
  }
}

// ---- tile targets ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tile_targets_kernel(const float* __restrict__ filled, const unsigned char* __restrict__ valid,
                                                           const int* __restrict__ active, const int* __restrict__ n_active, int first,
                                                           const MosaicGeom gm, float mean_lst, float istd_lst,
                                                           float* __restrict__ lst_out, unsigned char* __restrict__ valid_out) {
  const int win = gm.ax.w, n = min(*n_active, gm.ay.count * gm.ax.count);   // (never past the list sifsrg_tiles_select wrote)
  int t = -1;
  if (n > 0) t = active[(int)(((long long)first + blockIdx.x) % n)];
  const bool ok = t >= 0 && t < gm.ay.count * gm.ax.count;                  // (uniform over the workgroup)
  const int ty = ok ? t / gm.ax.count : 0, tx = ok ? t - ty * gm.ax.count : 0;
  const size_t org = ok ? (size_t)mosaic_origin(gm.ay, ty) * gm.lst_w + mosaic_origin(gm.ax, tx) : 0;
  float* lo = lst_out + (size_t)blockIdx.x * win * win;
  unsigned char* vo = valid_out + (size_t)blockIdx.x * win * win;
  for (int e = threadIdx.x; e < win * win; e += 256) {
    const int r = e / win, c = e - r * win;
    const size_t p = org + (size_t)r * gm.lst_w + c;
    lo[e] = ok ? (filled[p] - mean_lst) * istd_lst : 0.f;                   // the value tile_prepare_rows (mosaic.h) upsamples
    vo[e] = ok && valid[p] != 0 ? 1 : 0;
  }
}

__global__ __launch_bounds__(1024) void tile_count_kernel(const unsigned char* __restrict__ valid_out, size_t n, long long* __restrict__ n_valid) {
  __shared__ int wsum[16];
  int s = 0;
  for (size_t e = threadIdx.x; e < n; e += 1024) s += valid_out[e] != 0 ? 1 : 0;
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long tot = 0;
    for (int k = 0; k < 16; ++k) tot += wsum[k];
    *n_valid = tot;
  }
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

int launch_bn_frozen_stats(const float* running, float eps, float* mean, float* invstd, hipStream_t s) {
  const NetTable& nt = sifsr_net();
  BnRunTable tb;
  for (int l = 0; l < SIFSR_NUM_BN_LAYERS; ++l) { tb.run_off[l] = nt.L[l].run_off; tb.ch_off[l] = nt.L[l].ch_off; tb.cout[l] = nt.L[l].cout; }
  hipLaunchKernelGGL(bn_frozen_stats_kernel, dim3(SIFSR_NUM_BN_LAYERS), dim3(64), 0, s, running, eps, mean, invstd, tb);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int launch_conv_in_dgrad(const float* g, const float* y, const float* scale, const float* shift, const double* coef, const float* w,
                         float* dx, int B, int H, int W, hipStream_t s) {
  if (B < 1 || H < 3 || W < 3) return SIFSR_ERR_SHAPE;
  const int tiles_x = (W + DG_TW - 1) / DG_TW, tiles_y = (H + DG_TH - 1) / DG_TH;
  const long long ntiles = (long long)B * tiles_x * tiles_y;
  if (ntiles > 0x7fffffffLL || (long long)B * H > 0x7fffffffLL) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(conv_in_dgrad_kernel, dim3((unsigned)ntiles), dim3(256), 0, s, g, y, scale, shift, coef, w, dx, H, W, tiles_x, tiles_y);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

// ---- C ABI (include/sifsr_adapt.h) ----
#define S(stream) ((hipStream_t)(stream))

size_t sifsra_model_workspace_bytes(int B, int H, int W) {
  WsLayout l;
  if (sifsr_layout(B, H, W, 1, &l) != SIFSR_OK) return 0;
  return l.total * sizeof(float);
}

int sifsra_model_forward(const float* x, float* sr, const float* params, const float* running, void* workspace, size_t workspace_bytes,
                         int B, int H, int W, float eps, void* stream) {
  if (!x || !sr || !params || !running || !workspace) return SIFSR_ERR_ARG;
  return sifsr_engine_forward_frozen(x, sr, params, running, (float*)workspace, workspace_bytes / sizeof(float), B, H, W, eps, S(stream));
}

int sifsra_model_backward(const float* x, const float* dsr, const float* params, float* grads, float* dx, void* workspace,
                          size_t workspace_bytes, int B, int H, int W, int frozen, void* stream) {
  if (frozen < 0 || frozen > 1) return SIFSR_ERR_ARG;
  return sifsr_engine_backward(x, dsr, params, grads, (float*)workspace, workspace_bytes / sizeof(float), B, H, W, S(stream), 0, frozen,
                               dx);
}

int sifsra_conv_in_dgrad(const float* g, const float* y, const float* scale, const float* shift, const double* coef, const float* w,
                         float* dx, int B, int H, int W, void* stream) {
  if (!g || !y || !scale || !shift || !coef || !w || !dx || !aligned(g, 16) || !aligned(y, 16) || !aligned(coef, 8)) return SIFSR_ERR_ARG;
  return launch_conv_in_dgrad(g, y, scale, shift, coef, w, dx, B, H, W, S(stream));
}

int sifsra_tile_targets(const float* filled, const unsigned char* valid, const int* active, const int* n_active, int first, int count,
                        int h, int w, int window, int overlap, int cover_edges, float mean_lst, float std_lst, float* lst_out,
                        unsigned char* valid_out, long long* n_valid_out, void* stream) {
  if (!filled || !valid || !active || !n_active || !lst_out || !valid_out || !n_valid_out || !aligned(n_valid_out, 8)) return SIFSR_ERR_ARG;
  MosaicGeom gm;
  if (!mosaic_geom(h, w, window, overlap, cover_edges, &gm) || first < 0 || count < 1 || count > 65535 || std_lst == 0.f) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(tile_targets_kernel, dim3(count), dim3(256), 0, S(stream), filled, valid, active, n_active, first, gm, mean_lst,
                     1.f / std_lst, lst_out, valid_out);
  SIFSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(tile_count_kernel, dim3(1), dim3(1024), 0, S(stream), valid_out, (size_t)count * window * window, n_valid_out);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}
