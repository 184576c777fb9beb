// Training on partly valid patches (C ABI: include/sifsr_masked.h): the per-patch form of the gap fill of
// gaps.hip with the moments of the valid pixels, and the C entry points of the masked SIF loss (its kernels are the MASKED
// instantiations of loss.hip).
//
//  * patches_fill_kernel   one workgroup = one patch of w x w pixels, 4 <= w <= 64.  A thread owns up to four 2 x 2 blocks of the
//    patch (its level-1 cells) and keeps their 16 pixels in registers; the pyramid above (levels 1 .. top, at most 1365 cells of a
//    float64 sum and an int count) lives in LDS.  Reduce level by level, then push in closed form (an invalid pixel walks up its
//    ancestors to the first cell with a count), then the moments: the mean from the top cell, M2 / min / max by a fixed tree.
//    The sums are formed in the order gaps_reduce_kernel forms them, so `filled` agrees with sifsrg_fill for any values.
// No atomics; nothing is shared between workgroups.
#include "../../include/sifsr_masked.h"

#include <math.h>

#include "loss.h"

namespace {

constexpr int PF_MAX_W = 64;
constexpr int PF_MAX_CELLS = 1365;   // 32^2 + 16^2 + 8^2 + 4^2 + 2^2 + 1
constexpr int PF_MAX_LEVELS = 8;     // level 0 .. 6 for w = 64

// wave-then-LDS reductions over the 256 threads, fixed order; the result is valid in every thread
__device__ __forceinline__ double pf_block_sum(double v, double* sh) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
__device__ __forceinline__ float pf_block_min(float v, float* sh) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = fminf(v, __shfl_xor(v, m));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fminf(fminf(sh[0], sh[1]), fminf(sh[2], sh[3]));
}
__device__ __forceinline__ float pf_block_max(float v, float* sh) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

__global__ __launch_bounds__(256) void patches_fill_kernel(const float* __restrict__ lst, float* __restrict__ filled,
                                                           unsigned char* __restrict__ valid, double* __restrict__ moments,
                                                           int w) {
  __shared__ double S[PF_MAX_CELLS];
  __shared__ int C[PF_MAX_CELLS];
  __shared__ double shd[4];
  __shared__ float shf[4];
  const int tid = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * w * w;
  // the pyramid: side n[l] and first cell off[l] of level l >= 1 (ceil halving down to 1 x 1)
  int n[PF_MAX_LEVELS], off[PF_MAX_LEVELS], top = 0;
  n[0] = w;
  off[0] = 0;
  {
    int cells = 0;
#pragma unroll
    for (int l = 1; l < PF_MAX_LEVELS; ++l) {
      n[l] = (n[l - 1] + 1) / 2;
      off[l] = cells;
      cells += n[l] * n[l];
      if (top == 0 && n[l] == 1) top = l;
    }
  }
  const int n1 = n[1];   // w / 2: w is even, every level-1 cell has its four pixels

  // ---- level 0 -> 1: a thread's 2 x 2 blocks, pixels kept in registers ----
  float px[4][4];
  bool ok[4][4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int cell = tid + 256 * c;
    if (cell >= n1 * n1) break;
    const int i = cell / n1, j = cell - i * n1;
    double s = 0.0;
    int cnt = 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const size_t p = base + (size_t)(2 * i + r) * w + 2 * j;
      const float2 v = *reinterpret_cast<const float2*>(lst + p);   // (p is even: 8-byte aligned)
      px[c][2 * r] = v.x;
      px[c][2 * r + 1] = v.y;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const float f = px[c][2 * r + k];
        const bool good = isfinite(f) && f != 0.f;
        ok[c][2 * r + k] = good;
        valid[p + k] = good ? 1 : 0;
        s = s + (good ? (double)f : 0.0);          // (the order of gaps_reduce_kernel: row-major within the 2 x 2 block)
        cnt += good ? 1 : 0;
      }
    }
    S[cell] = s;
    C[cell] = cnt;
  }
  // ---- levels 2 .. top in LDS: (a + b) + (c + d), children past the ragged edge contribute nothing ----
#pragma unroll
  for (int l = 2; l < PF_MAX_LEVELS; ++l) {
    if (l > top) break;                            // (uniform over the workgroup)
    __syncthreads();
    const int nl = n[l], ns = n[l - 1];
    const double* Ss = S + off[l - 1];
    const int* Cs = C + off[l - 1];
    for (int cell = tid; cell < nl * nl; cell += 256) {
      const int i = cell / nl, j = cell - i * nl;
      double s[4];
      int cn[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int y = 2 * i + (q >> 1), x = 2 * j + (q & 1);
        const bool in = y < ns && x < ns;
        s[q] = in ? Ss[y * ns + x] : 0.0;
        cn[q] = in ? Cs[y * ns + x] : 0;
      }
      S[off[l] + cell] = (s[0] + s[1]) + (s[2] + s[3]);
      C[off[l] + cell] = (cn[0] + cn[1]) + (cn[2] + cn[3]);
    }
  }
  __syncthreads();
  const double total = S[off[top]];
  const int count = C[off[top]];
  const double mean = count > 0 ? total / (double)count : 0.0;

  // ---- push (closed form) and the per-thread moments ----
  double m2 = 0.0;
  float lo = INFINITY, hi = -INFINITY;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int cell = tid + 256 * c;
    if (cell >= n1 * n1) break;
    const int i = cell / n1, j = cell - i * n1;
    // the value an invalid pixel of this block takes: the first ancestor with a count (all four pixels share their ancestors)
    float fillv = 0.f;
#pragma unroll
    for (int l = 1; l < PF_MAX_LEVELS; ++l) {
      if (l > top) break;
      const int e = off[l] + ((2 * i) >> l) * n[l] + ((2 * j) >> l);
      const int cc = C[e];
      if (cc > 0) {
        fillv = (float)(S[e] / (double)cc);
        break;
      }
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const size_t p = base + (size_t)(2 * i + r) * w + 2 * j;
      float2 o;
      o.x = ok[c][2 * r] ? px[c][2 * r] : fillv;
      o.y = ok[c][2 * r + 1] ? px[c][2 * r + 1] : fillv;
      *reinterpret_cast<float2*>(filled + p) = o;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (ok[c][2 * r + k]) {
          const float f = px[c][2 * r + k];
          const double d = (double)f - mean;
          m2 += d * d;
          lo = fminf(lo, f);
          hi = fmaxf(hi, f);
        }
      }
    }
  }
  m2 = pf_block_sum(m2, shd);
  lo = pf_block_min(lo, shf);
  hi = pf_block_max(hi, shf);
  if (tid == 0) {
    double* row = moments + (size_t)blockIdx.x * 5;
    row[0] = (double)count;
    row[1] = mean;
    row[2] = m2;
    row[3] = (double)lo;
    row[4] = (double)hi;
  }
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

// ---- C ABI (include/sifsr_masked.h) ----
int sifsrm_patches_fill(const float* lst, float* filled, unsigned char* valid, double* moments, int N, int w, void* stream) {
  if (!lst || !filled || !valid || !moments || !aligned(lst, 8) || !aligned(filled, 8) || !aligned(moments, 8)) return SIFSR_ERR_ARG;
  if (N < 1 || w < 4 || w > PF_MAX_W || w % 4) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(patches_fill_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, lst, filled, valid, moments, w);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

size_t sifsrm_sif_loss_workspace_bytes(int kind, int B, int H, int W) { return sif_loss_workspace_floats(kind, B, H, W) * sizeof(float); }

int sifsrm_sif_loss(int kind, const float* sr, const float* lst, const unsigned char* valid, const long long* n_valid,
                    const float* ndvi, int B, int H, int W, float mean, float std, float alpha, float gamma, const float* taps_ds9,
                    const float* taps_ftm9, void* workspace, size_t workspace_bytes, float* losses3, float* dsr, void* stream) {
  if (!sr || !lst || !valid || !n_valid || !ndvi || !taps_ds9 || !taps_ftm9 || !workspace || !losses3 || !aligned(workspace, 4) ||
      !aligned(n_valid, 8))
    return SIFSR_ERR_ARG;
  if (kind != 1 && kind != 2) return SIFSR_ERR_ARG;
  if (B < 1 || B > 65535 || H < 10 || W < 10 || H % 4 || W % 4) return SIFSR_ERR_SHAPE;
  if (workspace_bytes < sifsrm_sif_loss_workspace_bytes(kind, B, H, W)) return SIFSR_ERR_WORKSPACE;
  return launch_sif_loss_masked(kind, sr, lst, valid, n_valid, ndvi, B, H, W, mean, std, alpha, gamma, taps_ds9, taps_ftm9,
                                (float*)workspace, losses3, dsr, (hipStream_t)stream);
}
