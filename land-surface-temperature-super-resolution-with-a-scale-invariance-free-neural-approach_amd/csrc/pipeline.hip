// The step before the hot path and the per-batch metrics after it (f1), on the device.
//
//  * tiles_prepare: what ModisDatasetB.__getitem__ (dataset.py:134-142) / predict.py:84-100 do on the host per
//    tile -- z-score of the 64x64 LST tile, bicubic x4 upsample (us.upsampling = cv2.resize INTER_CUBIC,
//    utils.py:163-180: A = -0.75, half-pixel centres, edge-clamped), NDVI clip to [-1,1] + z-score,
//    torch.cat((lst_up, ndvi), 1) -- fused into one kernel that reads tiles straight out of a granule (or a
//    batch) and writes the model input (T,2,4w,4w).
//  * tiles_paste: predict.py:101-103, `* std + mean` and the write into the 4x granule.
//  * psnr / ssim: us.psnr_skimage / us.ssim_skimage (utils.py:548-578; scikit-image 0.22 defaults: 7x7 uniform
//    window, sample covariance, K1 = 0.01, K2 = 0.03, data_range = max - min of the TARGET BATCH, mean over
//    the window-valid interior), batch means as two device scalars -- no D2H of the images, no host stall.
//    MASKED instantiations (include/sifsr_scores.h; entry points in scores.hip): validity is the byte of
//    the pixel's LR cell, the range is taken over the valid target pixels, the squared error is summed over the valid
//    pixels and the SSIM map over the pixels whose 7x7 window is all valid (separable byte counts in LDS, 3-pixel halo);
//    selection by predicate, so that an all-valid mask adds the same values in the same order as the unmasked kernels.
#include "edge_conv.h"
#include "mosaic.h"   // tile_prepare_rows: the per-tile body shared with the overlapped layout

namespace {

struct TileGeom {
  int tiles_x;                        // tile t -> (ty, tx) = (t / tiles_x, t % tiles_x)
  long long lst_step_y, lst_step_x;   // element offset of tile (ty, tx) = ty*step_y + tx*step_x
  int lst_row;                        // row stride inside a tile (elements)
  long long ndvi_step_y, ndvi_step_x;
  int ndvi_row;
};

// one workgroup = 16 output rows x (4*win) columns of one tile; thread = output column (win = 64 -> 256 threads); body: mosaic.h
__global__ __launch_bounds__(256) void tiles_prepare_kernel(const float* __restrict__ lst, const float* __restrict__ ndvi,
                                                            float* __restrict__ x, const TileGeom gm, int win,
                                                            float mean_lst, float istd_lst, float mean_ndvi,
                                                            float istd_ndvi, int clip_ndvi) {
  __shared__ float src[8][64 + 1];
  const int hr = 4 * win;
  const int t = blockIdx.x;
  const int ty = t / gm.tiles_x, tx = t - ty * gm.tiles_x;
  tile_prepare_rows(lst + ty * gm.lst_step_y + tx * gm.lst_step_x, ndvi + ty * gm.ndvi_step_y + tx * gm.ndvi_step_x, gm.lst_row,
                    gm.ndvi_row, x + ((size_t)t * 2 + 0) * hr * hr, x + ((size_t)t * 2 + 1) * hr * hr, src, win, blockIdx.y * 16,
                    mean_lst, istd_lst, mean_ndvi, istd_ndvi, clip_ndvi);
}

__global__ __launch_bounds__(256) void tiles_paste_kernel(const float* __restrict__ sr, float* __restrict__ out, int T,
                                                          int tiles_x, int hr, long long out_row, float mean, float std) {
  const size_t n = (size_t)T * hr * hr;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    const int X = (int)(e % hr);
    const size_t r = e / hr;
    const int Y = (int)(r % hr), t = (int)(r / hr);
    const int ty = t / tiles_x, tx = t - ty * tiles_x;
    out[((size_t)ty * hr + Y) * out_row + (size_t)tx * hr + X] = sr[e] * std + mean;
  }
}

// us.downsampling (utils.py:183-213), the 'norm-L4' decimation: (mean of x^4 over each 4x4 block)^(1/4)
__global__ __launch_bounds__(256) void l4pool4_kernel(const float* __restrict__ x, float* __restrict__ out, int B, int H, int W) {
  const int Ho = H / 4, Wo = W / 4;
  const size_t n = (size_t)B * Ho * Wo;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    const int ox = (int)(e % Wo);
    const size_t r = e / Wo;
    const int oy = (int)(r % Ho), b = (int)(r / Ho);
    const float* src = x + ((size_t)b * H + 4 * oy) * W + 4 * ox;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float4 v = ld4(src + (size_t)i * W);
      s += v.x * v.x * v.x * v.x; s += v.y * v.y * v.y * v.y; s += v.z * v.z * v.z * v.z; s += v.w * v.w * v.w * v.w;
    }
    out[e] = powf(s / 16.f, 0.25f);
  }
}

// ---------------------------------------------------------------------------------------------
// PSNR / SSIM
// ---------------------------------------------------------------------------------------------
// min / max that keep a NaN (fminf / fmaxf drop it): numpy's, which skimage's data range is taken with.  The MASKED instantiation
// keeps fminf / fmaxf: what a valid NaN pixel does there is the scores family's contract (include/sifsr_scores.h).
template <bool MASKED> __device__ __forceinline__ float mm_min(float a, float b) {
  if constexpr (MASKED) return fminf(a, b); else return (a != a || b != b) ? a + b : fminf(a, b);
}
template <bool MASKED> __device__ __forceinline__ float mm_max(float a, float b) {
  if constexpr (MASKED) return fmaxf(a, b); else return (a != a || b != b) ? a + b : fmaxf(a, b);
}

template <bool MASKED>
__global__ __launch_bounds__(256) void minmax_partial_kernel(const float* __restrict__ t, size_t n, float* __restrict__ part,
                                                             const unsigned char* __restrict__ valid, int H, int W, int scale) {
  __shared__ float smin[256], smax[256];
  float lo = INFINITY, hi = -INFINITY;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    if constexpr (MASKED) {
      const int x = (int)(e % W);
      const size_t r = e / W;
      const int y = (int)(r % H);
      if (!valid[((r / H) * (H / scale) + y / scale) * (W / scale) + x / scale]) continue;
    }
    const float v = t[e];
    lo = mm_min<MASKED>(lo, v); hi = mm_max<MASKED>(hi, v);
  }
  smin[threadIdx.x] = lo; smax[threadIdx.x] = hi;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      smin[threadIdx.x] = mm_min<MASKED>(smin[threadIdx.x], smin[threadIdx.x + st]);
      smax[threadIdx.x] = mm_max<MASKED>(smax[threadIdx.x], smax[threadIdx.x + st]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = smin[0]; part[2 * blockIdx.x + 1] = smax[0]; }
}

template <bool MASKED>
__global__ void minmax_final_kernel(float* __restrict__ part, int n) {
  if (threadIdx.x == 0) {
    float lo = INFINITY, hi = -INFINITY;
    for (int i = 0; i < n; ++i) { lo = mm_min<MASKED>(lo, part[2 * i]); hi = mm_max<MASKED>(hi, part[2 * i + 1]); }
    part[512] = lo; part[513] = hi;
  }
}

constexpr int MT = 32;          // SSIM output tile
constexpr int MH = MT + 6;      // + 3-pixel halo of the 7x7 window

// per (image, 32x32 tile): sum of the SSIM map over the window-valid pixels of the tile, and sum of squared error
// MASKED: vb = the validity byte of every pixel of the 38 x 38 LDS tile (0 outside the image), hv = its horizontal 7-counts;
// pcnt = per tile the number of valid pixels and of all-valid windows.  6.7 KB on top of 64.6 KB: two workgroups per CU as before.
template <bool MASKED>
__global__ __launch_bounds__(256) void psnr_ssim_tile_kernel(const float* __restrict__ pred, const float* __restrict__ targ,
                                                             const float* __restrict__ mm, int H, int W,
                                                             double* __restrict__ part, const unsigned char* __restrict__ valid,
                                                             int scale, int* __restrict__ pcnt) {
  __shared__ float a[MH][MH + 1], b[MH][MH + 1];   // a = target (im1 in skimage's call), b = prediction
  __shared__ double hs[5][MH][MT];                  // horizontal 7-sums of a, b, a*a, b*b, a*b
  __shared__ double red[256][2];
  __shared__ unsigned char vb[MASKED ? MH : 1][MASKED ? MH : 1], hv[MASKED ? MH : 1][MASKED ? MT : 1];
  __shared__ int redi[MASKED ? 256 : 1][2];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * MT, y0 = blockIdx.y * MT, img = blockIdx.z;
  const float R = mm[513] - mm[512];
  const float C1 = (0.01f * R) * (0.01f * R), C2 = (0.03f * R) * (0.03f * R);
  const float* tp = targ + (size_t)img * H * W;
  const float* pp = pred + (size_t)img * H * W;
  for (int e = tid; e < MH * MH; e += 256) {
    const int r = e / MH, c = e - r * MH;
    const int gy = y0 - 3 + r, gx = x0 - 3 + c;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    a[r][c] = in ? tp[(size_t)gy * W + gx] : 0.f;
    b[r][c] = in ? pp[(size_t)gy * W + gx] : 0.f;
    if constexpr (MASKED)
      vb[r][c] = in && valid[((size_t)img * (H / scale) + gy / scale) * (W / scale) + gx / scale] != 0 ? 1 : 0;
  }
  __syncthreads();
  for (int e = tid; e < MH * MT; e += 256) {
    const int r = e / MT, c = e - r * MT;
    if constexpr (MASKED) {
      int n = 0;
#pragma unroll
      for (int k = 0; k < 7; ++k) n += vb[r][c + k];
      hv[r][c] = (unsigned char)n;
    }
    double s[5] = {0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const float u = a[r][c + k], v = b[r][c + k];
      s[0] += (double)u; s[1] += (double)v; s[2] += (double)(u * u); s[3] += (double)(v * v); s[4] += (double)(u * v);
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) hs[q][r][c] = s[q];
  }
  __syncthreads();
  double ssum = 0.0, esum = 0.0;
  int n0 = 0, n3 = 0;
  for (int e = tid; e < MT * MT; e += 256) {
    const int r = e / MT, c = e - r * MT;
    const int gy = y0 + r, gx = x0 + c;
    bool in0 = gy < H && gx < W, in3 = gy >= 3 && gy < H - 3 && gx >= 3 && gx < W - 3;
    if constexpr (MASKED) {
      int n = 0;
#pragma unroll
      for (int k = 0; k < 7; ++k) n += hv[r + k][c];
      in0 = vb[r + 3][c + 3] != 0; in3 = n == 49;     // (both imply the unmasked conditions: vb is 0 outside the image)
      n0 += in0; n3 += in3;
    }
    if (in0) {
      const float d = a[r + 3][c + 3] - b[r + 3][c + 3];   // skimage: float32 difference, squared, float64 mean
      esum += (double)(d * d);
    }
    if (in3) {
      double s[5] = {0, 0, 0, 0, 0};
#pragma unroll
      for (int k = 0; k < 7; ++k)
#pragma unroll
        for (int q = 0; q < 5; ++q) s[q] += hs[q][r + k][c];
      // scipy.ndimage.uniform_filter: float64 accumulation, float32 result; the rest in float32 like skimage
      const float ux = (float)(s[0] / 49.0), uy = (float)(s[1] / 49.0);
      const float uxx = (float)(s[2] / 49.0), uyy = (float)(s[3] / 49.0), uxy = (float)(s[4] / 49.0);
      const float cov_norm = 49.f / 48.f;
      const float vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
      const float A1 = 2.f * ux * uy + C1, A2 = 2.f * vxy + C2;
      const float B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
      ssum += (double)((A1 * A2) / (B1 * B2));
    }
  }
  red[tid][0] = ssum; red[tid][1] = esum;
  if constexpr (MASKED) { redi[tid][0] = n3; redi[tid][1] = n0; }
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if (tid < st) {
      red[tid][0] += red[tid + st][0]; red[tid][1] += red[tid + st][1];
      if constexpr (MASKED) { redi[tid][0] += redi[tid + st][0]; redi[tid][1] += redi[tid + st][1]; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const size_t blk = ((size_t)img * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    part[2 * blk] = red[0][0]; part[2 * blk + 1] = red[0][1];
    if constexpr (MASKED) { pcnt[2 * blk] = redi[0][0]; pcnt[2 * blk + 1] = redi[0][1]; }
  }
}

// out[0] = mean_i 10*log10(R^2 / mse_i), out[1] = mean_i mean(SSIM map_i over the valid interior)
// MASKED: an image contributes its PSNR iff it has a valid pixel and its SSIM iff it has an all-valid window; the means are taken
// over the contributing images (counts2), NaN where there is none.
template <bool MASKED>
__global__ __launch_bounds__(256) void psnr_ssim_final_kernel(const double* __restrict__ part, int tiles_per_img, int B,
                                                              int H, int W, const float* __restrict__ mm,
                                                              float* __restrict__ out, const int* __restrict__ pcnt,
                                                              int* __restrict__ counts2) {
  __shared__ double r1[256], r2[256];
  __shared__ int c1[MASKED ? 256 : 1], c2[MASKED ? 256 : 1];
  const double R = (double)(mm[513] - mm[512]);
  double ps = 0.0, ss = 0.0;
  int np = 0, ns = 0;
  for (int img = threadIdx.x; img < B; img += 256) {
    double s = 0.0, e = 0.0;
    for (int k = 0; k < tiles_per_img; ++k) { s += part[2 * ((size_t)img * tiles_per_img + k)]; e += part[2 * ((size_t)img * tiles_per_img + k) + 1]; }
    if constexpr (MASKED) {
      long long n3 = 0, n0 = 0;
      for (int k = 0; k < tiles_per_img; ++k) { n3 += pcnt[2 * ((size_t)img * tiles_per_img + k)]; n0 += pcnt[2 * ((size_t)img * tiles_per_img + k) + 1]; }
      if (n0 > 0) {
        const double mse = e / (double)n0;
        ps += 10.0 * log10(R * R / mse);
        ++np;
      }
      if (n3 > 0) {
        ss += s / (double)n3;
        ++ns;
      }
    } else {
      const double mse = e / ((double)H * W);
      ps += 10.0 * log10(R * R / mse);
      ss += s / ((double)(H - 6) * (W - 6));
    }
  }
  r1[threadIdx.x] = ps; r2[threadIdx.x] = ss;
  if constexpr (MASKED) { c1[threadIdx.x] = np; c2[threadIdx.x] = ns; }
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) {
      r1[threadIdx.x] += r1[threadIdx.x + st]; r2[threadIdx.x] += r2[threadIdx.x + st];
      if constexpr (MASKED) { c1[threadIdx.x] += c1[threadIdx.x + st]; c2[threadIdx.x] += c2[threadIdx.x + st]; }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if constexpr (MASKED) {
      out[0] = c1[0] > 0 ? (float)(r1[0] / c1[0]) : __uint_as_float(0x7FC00000u);
      out[1] = c2[0] > 0 ? (float)(r2[0] / c2[0]) : __uint_as_float(0x7FC00000u);
      counts2[0] = c1[0]; counts2[1] = c2[0];
    } else {
      out[0] = (float)(r1[0] / B); out[1] = (float)(r2[0] / B);
    }
  }
}

}  // namespace

int launch_tiles_prepare(const float* lst, const float* ndvi, float* x, int T, int tiles_x, int win, long long lst_step_y,
                         long long lst_step_x, int lst_row, long long ndvi_step_y, long long ndvi_step_x, int ndvi_row,
                         float mean_lst, float std_lst, float mean_ndvi, float std_ndvi, int clip_ndvi, hipStream_t s) {
  if (T < 1 || tiles_x < 1 || win < 4 || win > 64 || win % 4 || std_lst == 0.f || std_ndvi == 0.f) return SIFSR_ERR_SHAPE;
  TileGeom gm{tiles_x, lst_step_y, lst_step_x, lst_row, ndvi_step_y, ndvi_step_x, ndvi_row};
  hipLaunchKernelGGL(tiles_prepare_kernel, dim3(T, (4 * win) / 16), dim3(256), 0, s, lst, ndvi, x, gm, win, mean_lst,
                     1.f / std_lst, mean_ndvi, 1.f / std_ndvi, clip_ndvi);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int launch_tiles_paste(const float* sr, float* out, int T, int tiles_x, int hr, long long out_row, float mean, float std,
                       hipStream_t s) {
  if (T < 1 || tiles_x < 1 || hr < 1) return SIFSR_ERR_SHAPE;
  const size_t n = (size_t)T * hr * hr;
  size_t blocks = (n + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(tiles_paste_kernel, dim3((int)blocks), dim3(256), 0, s, sr, out, T, tiles_x, hr, out_row, mean, std);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

size_t psnr_ssim_scratch_bytes(int B, int H, int W) {
  const size_t tiles = (size_t)((W + MT - 1) / MT) * ((H + MT - 1) / MT);
  return 528 * sizeof(float) + (size_t)B * tiles * 2 * sizeof(double) + 64;
}

int launch_psnr_ssim(const float* pred, const float* targ, int B, int H, int W, void* scratch, float* out2, hipStream_t s) {
  if (B < 1 || H < 7 || W < 7) return SIFSR_ERR_SHAPE;
  float* mm = reinterpret_cast<float*>(scratch);
  double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(scratch) + 528 * sizeof(float));
  const size_t n = (size_t)B * H * W;
  int mmb = (int)((n + 256 * 64 - 1) / (256 * 64));
  if (mmb > 256) mmb = 256;
  if (mmb < 1) mmb = 1;
  const dim3 grid((W + MT - 1) / MT, (H + MT - 1) / MT, B);
  hipLaunchKernelGGL(minmax_partial_kernel<false>, dim3(mmb), dim3(256), 0, s, targ, n, mm, (const unsigned char*)nullptr, H, W, 1);
  hipLaunchKernelGGL(minmax_final_kernel<false>, dim3(1), dim3(64), 0, s, mm, mmb);
  hipLaunchKernelGGL(psnr_ssim_tile_kernel<false>, grid, dim3(256), 0, s, pred, targ, mm, H, W, part,
                     (const unsigned char*)nullptr, 1, (int*)nullptr);
  hipLaunchKernelGGL(psnr_ssim_final_kernel<false>, dim3(1), dim3(256), 0, s, part, (int)(grid.x * grid.y), B, H, W, mm, out2,
                     (const int*)nullptr, (int*)nullptr);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

// scratch: the unmasked layout [528 floats: min / max partials][per-tile double pairs], then the per-tile count pairs
size_t psnr_ssim_masked_scratch_bytes(int B, int H, int W) {
  const size_t tiles = (size_t)((W + MT - 1) / MT) * ((H + MT - 1) / MT);
  return 528 * sizeof(float) + (size_t)B * tiles * 2 * sizeof(double) + (size_t)B * tiles * 2 * sizeof(int) + 64;
}

int launch_psnr_ssim_masked(const float* pred, const float* targ, const unsigned char* valid, int scale, int B, int H, int W,
                            void* scratch, float* out2, int* counts2, hipStream_t s) {
  if (B < 1 || B > 65535 || H < 7 || W < 7 || (long long)H * W >= (1LL << 31) || (H + MT - 1) / MT > 65535) return SIFSR_ERR_SHAPE;
  if ((scale != 1 && scale != 4) || H % scale || W % scale) return SIFSR_ERR_SHAPE;
  const dim3 grid((W + MT - 1) / MT, (H + MT - 1) / MT, B);
  const size_t tiles = (size_t)grid.x * grid.y;
  float* mm = reinterpret_cast<float*>(scratch);
  double* part = reinterpret_cast<double*>(reinterpret_cast<char*>(scratch) + 528 * sizeof(float));
  int* pcnt = reinterpret_cast<int*>(part + (size_t)B * tiles * 2);
  const size_t n = (size_t)B * H * W;
  int mmb = (int)((n + 256 * 64 - 1) / (256 * 64));
  if (mmb > 256) mmb = 256;
  if (mmb < 1) mmb = 1;
  hipLaunchKernelGGL(minmax_partial_kernel<true>, dim3(mmb), dim3(256), 0, s, targ, n, mm, valid, H, W, scale);
  hipLaunchKernelGGL(minmax_final_kernel<true>, dim3(1), dim3(64), 0, s, mm, mmb);
  hipLaunchKernelGGL(psnr_ssim_tile_kernel<true>, grid, dim3(256), 0, s, pred, targ, (const float*)mm, H, W, part, valid, scale, pcnt);
  hipLaunchKernelGGL(psnr_ssim_final_kernel<true>, dim3(1), dim3(256), 0, s, (const double*)part, (int)tiles, B, H, W,
                     (const float*)mm, out2, (const int*)pcnt, counts2);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int launch_l4pool4(const float* x, float* out, int B, int H, int W, hipStream_t s) {
  if (B < 1 || H < 4 || W < 4 || H % 4 || W % 4) return SIFSR_ERR_SHAPE;
  const size_t n = (size_t)B * (H / 4) * (W / 4);
  size_t blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(l4pool4_kernel, dim3((int)blocks), dim3(256), 0, s, x, out, B, H, W);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}
