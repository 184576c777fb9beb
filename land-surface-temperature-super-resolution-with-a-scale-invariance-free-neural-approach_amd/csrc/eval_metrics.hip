// Per-pair ASTER evaluation metrics: the table of model_perf_aster_formatds.py:371-437, columns
// named at :507 without LPIPS, for B pairs (a = ASTER reference, im1 / overlap_11; b = prediction, im2 / overlap_22):
//
//   0 PSNR       skimage peak_signal_noise_ratio(a, b, data_range=R), R = max(a u b) - min(a u b) in float32 (:373-374)
//   1 SSIM       skimage structural_similarity(a, b, data_range=R), 0.22 defaults on float32 images
//   2 RMSE       sqrt(mean((a-b)^2))
//   3-5 RMSE_low / RMSE_mean / RMSE_high  (:379-404): g = |a - get_output_ftm(a)|, q25 / q75 = np.percentile(g, 25 / 75)
//                ('linear', float32 as numpy 2.x computes it), sqrt(sum of e over the stratum / N) -- the divisor is N
//                because the reference's filter((0.0).__ne__, ...) removes nothing from a list of np.float32
//   6 GSSIM      us.gssim(a, b, data_range=R), utils.py:1904-2005, float64
//   7 RMSE_grad  sqrt(mean((|grad b|_4 - |grad a|_4)^2)), the 4-kernel Sobel bank, convolve2d 'valid' (:414-437); scipy
//                promotes float32 images x int kernels to float64, so the magnitudes are float64 here too
//
// Launch sequence (all per image, so every image of a batch equals its own B = 1 result bit for bit):
//   1. the get_output_ftm forward (launch_blur_fwd, the same kernel as sif_ops.get_output_ftm) into the g buffer;
//   2. prep: g = |a - ftm| in place, R per pair (one workgroup per image);
//   3. tiles: 16x16 output tile + 4-pixel LDS halo -> per-tile float64 partials of the SSIM map, the GSSIM map and the
//      squared gradient-magnitude difference;
//   4. select: exact radix selection (11 + 11 + 10 bits of the uint32 patterns of g >= 0, LDS histograms, integer LDS
//      atomics) of the four order statistics numpy's percentile interpolates, the numpy lerp, the strata pass, the
//      fixed-order reduction of the tile partials and the (B, 8) float64 row (one workgroup per image).
// No float atomics, no allocation, no host synchronisation: capturable in a hipGraph.
//
// MASKED instantiations (DESIGN.md §9 f10, C ABI include/sifsr_scores.h, entry points csrc/scores.hip): a term is counted iff
// every pixel its stencil reads is valid.  prep writes one validity byte per pixel, the tile pass loads those bytes with the
// pixels' halo and forms the 3x3 / 7x7 / 9x9 all-valid predicates (and the image-clipped 9x9 one of the strata) from
// separable integer window sums in LDS, marks the pixels outside the strata set in g with a bit pattern above every finite
// value, and the selection takes its ranks from the number of eligible pixels.  Terms are SELECTED by the predicates, never
// weighted: with every pixel valid the predicates are the interiors of the unmasked kernels and the same values are added
// in the same order.
//
// The float32 algebra is written in numpy's evaluation order; contraction into FMAs is off in this file so that the
// percentile lerp and the SSIM terms round exactly where numpy rounds.
#include "loss.h"

#pragma clang fp contract(off)

namespace {

constexpr int ET = 16;            // output tile edge of the tile pass (256 threads, one pixel each)
constexpr int EH = 4;             // halo: 3 (7x7 window) + 1 (3x3 Sobel)
constexpr int EA = ET + 2 * EH;   // 24: a / b rows and columns in LDS
constexpr int EM = ET + 6;        // 22: Sobel magnitudes feeding the 7x7 GSSIM window
constexpr int NPART = 3;          // per-tile partials: SSIM sum, GSSIM sum, squared gradient difference sum
constexpr int SEL_THREADS = 512;  // selection / strata workgroup (8 waves)
constexpr int NQ = 10;            // horizontal window sums kept in LDS
constexpr int NCNT = 4;           // MASKED per-tile counts: n1 (3x3), n3 (7x7), n4 (9x9), ns (image-clipped 9x9)
constexpr unsigned G_OUT = 0xFFFFFFFFu;   // MASKED: g of a pixel outside the strata set (a NaN pattern above every finite value)

__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}

// ---- 2. g = |a - ftm(a)| in place, R = max(a u b) - min(a u b) ------------------------------------------------
// MASKED: vmap[p] = isfinite(a) && a != 0 && isfinite(b) && b != 0 && (mask == NULL || mask != 0); R over the valid pixels,
// at rng[4 * image] (the row holds R, q25, q75 and one unused float).
template <bool MASKED>
__global__ __launch_bounds__(1024) void eval_prep_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                         float* __restrict__ g, int N, float* __restrict__ rng,
                                                         const unsigned char* __restrict__ mask,
                                                         unsigned char* __restrict__ vmap) {
  __shared__ float smin[16], smax[16];
  const size_t off = (size_t)blockIdx.x * N;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < N; i += 1024) {
    const float u = a[off + i];
    g[off + i] = fabsf(u - g[off + i]);
    if constexpr (MASKED) {
      const float v = b[off + i];
      const bool ok = isfinite(u) && u != 0.f && isfinite(v) && v != 0.f && (!mask || mask[off + i] != 0);
      vmap[off + i] = ok ? 1 : 0;
      if (ok) { lo = fminf(lo, u); hi = fmaxf(hi, u); lo = fminf(lo, v); hi = fmaxf(hi, v); }
    } else {
      lo = fminf(lo, u); hi = fmaxf(hi, u);
      if (b) { const float v = b[off + i]; lo = fminf(lo, v); hi = fmaxf(hi, v); }
    }
  }
  if (!rng) return;
  for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_down(lo, o, 64)); hi = fmaxf(hi, __shfl_down(hi, o, 64)); }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { smin[w] = lo; smax[w] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 16; ++k) { lo = fminf(lo, smin[k]); hi = fmaxf(hi, smax[k]); }
    rng[(MASKED ? 4 : 1) * blockIdx.x] = hi - lo;
  }
}

// ---- 3. tile pass ------------------------------------------------------------------------------------------------
// LDS A / Bm hold a and b at original rows y0-4 .. y0+19 (zero outside the image: those entries only feed masked
// outputs).  Magnitude M[p][q] is centred at original (y0-3+p, x0-3+q).  Horizontal sums HS[k][r][c] cover original row
// y0-3+r and columns x0-3+c .. x0+3+c; the vertical pass of thread (yy, xx) adds rows yy .. yy+6.
//
// MASKED: VB holds the validity bytes of the same 24 x 24 pixels (1 valid, 0 invalid, 2 outside the image); HV[k][r][c] are the
// horizontal counts of row r over the columns c+3..c+5 (k = 0), c+1..c+7 (k = 1), c..c+8 (k = 2) of bytes equal to 1, and
// over c..c+8 of non-zero bytes (k = 3: a pixel outside the image does not spoil the reflect border's window).  About 2 KB on
// top of 40.7 KB: three workgroups per CU (160 KB) as before.
template <bool MASKED>
__global__ __launch_bounds__(256) void eval_tile_kernel(const float* __restrict__ a, const float* __restrict__ b, int H,
                                                        int W, const float* __restrict__ rng, float data_range,
                                                        double* __restrict__ part, const unsigned char* __restrict__ vmap,
                                                        unsigned* __restrict__ gu, int* __restrict__ pcnt) {
  __shared__ float A[EA][EA + 1], Bm[EA][EA + 1];
  __shared__ double FM[EM][EM], GM[EM][EM];
  __shared__ double HS[NQ][EM][ET];
  __shared__ unsigned char VB[MASKED ? EA : 1][MASKED ? EA : 1];
  __shared__ unsigned char HV[NCNT][MASKED ? EA : 1][MASKED ? ET : 1];
  __shared__ int ired[4][NCNT];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * ET, y0 = blockIdx.y * ET, img = blockIdx.z;
  const size_t off = (size_t)img * H * W;
  for (int e = tid; e < EA * EA; e += 256) {
    const int r = e / EA, c = e - r * EA;
    const int gy = y0 - EH + r, gx = x0 - EH + c;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    A[r][c] = in ? a[off + (size_t)gy * W + gx] : 0.f;
    Bm[r][c] = in ? b[off + (size_t)gy * W + gx] : 0.f;
    if constexpr (MASKED) VB[r][c] = in ? vmap[off + (size_t)gy * W + gx] : (unsigned char)2;
  }
  __syncthreads();
  if constexpr (MASKED) {
    for (int e = tid; e < EA * ET; e += 256) {
      const int r = e / ET, c = e - r * ET;
      int n3 = 0, n7 = 0, n9 = 0, s9 = 0;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const int v = VB[r][c + k];
        const int one = v == 1 ? 1 : 0;
        n9 += one; s9 += v != 0 ? 1 : 0;
        if (k >= 1 && k <= 7) n7 += one;
        if (k >= 3 && k <= 5) n3 += one;
      }
      HV[0][r][c] = (unsigned char)n3; HV[1][r][c] = (unsigned char)n7; HV[2][r][c] = (unsigned char)n9; HV[3][r][c] = (unsigned char)s9;
    }
  }
  // gssim's two Sobel kernels in float64 (exact sums of float32 values with weights 1, 2), f_mag = sqrt(f0^2 + f1^2)
  for (int e = tid; e < EM * EM; e += 256) {
    const int p = e / EM, q = e - p * EM;
    const int r = p + 1, c = q + 1;   // centre in A
    double u[3][3], v[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) { u[i][j] = (double)A[r - 1 + i][c - 1 + j]; v[i][j] = (double)Bm[r - 1 + i][c - 1 + j]; }
    const double f0 = (u[0][2] + 2.0 * u[1][2] + u[2][2]) - (u[0][0] + 2.0 * u[1][0] + u[2][0]);
    const double f1 = (u[2][0] + 2.0 * u[2][1] + u[2][2]) - (u[0][0] + 2.0 * u[0][1] + u[0][2]);
    const double g0 = (v[0][2] + 2.0 * v[1][2] + v[2][2]) - (v[0][0] + 2.0 * v[1][0] + v[2][0]);
    const double g1 = (v[2][0] + 2.0 * v[2][1] + v[2][2]) - (v[0][0] + 2.0 * v[0][1] + v[0][2]);
    FM[p][q] = sqrt(f0 * f0 + f1 * f1);
    GM[p][q] = sqrt(g0 * g0 + g1 * g1);
  }
  __syncthreads();
  for (int e = tid; e < EM * ET; e += 256) {
    const int r = e / ET, c = e - r * ET;
    double s[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k) s[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
      const float u = A[r + 1][c + 1 + k], v = Bm[r + 1][c + 1 + k];
      const double fm = FM[r][c + k], gm = GM[r][c + k];
      s[0] += (double)u; s[1] += (double)v;
      s[2] += (double)(u * u); s[3] += (double)(v * v); s[4] += (double)(u * v);   // float32 products (skimage)
      s[5] += fm; s[6] += gm; s[7] += fm * fm; s[8] += gm * gm; s[9] += fm * gm;    // float64 (gssim)
    }
#pragma unroll
    for (int k = 0; k < NQ; ++k) HS[k][r][c] = s[k];
  }
  __syncthreads();
  const float R = data_range >= 0.f ? data_range : rng[(MASKED ? 4 : 1) * img];
  const float C1 = (0.01f * R) * (0.01f * R), C2 = (0.03f * R) * (0.03f * R);   // float32, as numpy 2 evaluates K * R
  const int yy = tid >> 4, xx = tid & 15;
  const int y = y0 + yy, x = x0 + xx;
  double ssim = 0.0, gssim = 0.0, gd = 0.0;
  int cnt[NCNT] = {0, 0, 0, 0};
  if (y < H && x < W) {
    // which terms this pixel contributes: the interiors, or (MASKED) the all-valid windows, which lie inside them
    bool in1 = y >= 1 && y < H - 1 && x >= 1 && x < W - 1, in3 = y >= 3 && y < H - 3 && x >= 3 && x < W - 3;
    bool in4 = y >= 4 && y < H - 4 && x >= 4 && x < W - 4;
    if constexpr (MASKED) {
      int n3 = 0, n7 = 0, n9 = 0, s9 = 0;
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        n9 += HV[2][yy + j][xx]; s9 += HV[3][yy + j][xx];
        if (j >= 1 && j <= 7) n7 += HV[1][yy + j][xx];
        if (j >= 3 && j <= 5) n3 += HV[0][yy + j][xx];
      }
      in1 = n3 == 9; in3 = n7 == 49; in4 = n9 == 81;
      const bool ins = s9 == 81;
      cnt[0] = in1; cnt[1] = in3; cnt[2] = in4; cnt[3] = ins;
      if (!ins) gu[off + (size_t)y * W + x] = G_OUT;
    }
    double s[NQ];
#pragma unroll
    for (int k = 0; k < NQ; ++k) s[k] = 0.0;
#pragma unroll
    for (int j = 0; j < 7; ++j)
#pragma unroll
      for (int k = 0; k < NQ; ++k) s[k] += HS[k][yy + j][xx];
    if (in3) {
      // structural_similarity: uniform_filter (float64 sums, float32 result), float32 algebra
      const float ux = (float)(s[0] / 49.0), uy = (float)(s[1] / 49.0);
      const float uxx = (float)(s[2] / 49.0), uyy = (float)(s[3] / 49.0), uxy = (float)(s[4] / 49.0);
      const float cov_norm = 49.f / 48.f;
      const float vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
      const float A1 = 2.f * ux * uy + C1, A2 = 2.f * vxy + C2;
      const float B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
      ssim = (double)((A1 * A2) / (B1 * B2));
    }
    if (in4) {
      // gssim: luminance from the images, contrast / structure from the magnitudes, the reference's own C and S terms
      const double ux = s[0] / 49.0, uy = s[1] / 49.0;
      const double mf = s[5] / 49.0, mg = s[6] / 49.0;
      const double uxx = s[7] / 49.0, uyy = s[8] / 49.0, uxy = s[9] / 49.0;
      const double cov_norm = 49.0 / 48.0;
      const double vx = cov_norm * (uxx - mf * mf), vy = cov_norm * (uyy - mg * mg), vxy = cov_norm * (uxy - mf * mg);
      const double c1 = (double)C1, c2 = (double)C2;
      const double A1 = 2.0 * ux * uy + c1, B1 = ux * ux + uy * uy + c1, B2 = vx + vy + c2;
      const double L = A1 / B1;
      const double C = (2.0 * sqrt(vx) * sqrt(vy) + c2) / B2;
      const double S = (vxy + c2) / (sqrt(vx) * sqrt(vy) + c2 / 2.0);
      gssim = L * C * S;
    }
    if (in1) {
      // the 4-kernel bank of :414-419 in float64 (signs do not matter: every flipped kernel is +- the original)
      const int r = yy + EH, c = xx + EH;
      double m2[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        double u[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) u[i][j] = (double)(t ? Bm[r - 1 + i][c - 1 + j] : A[r - 1 + i][c - 1 + j]);
        const double k0 = (u[0][0] + 2.0 * u[0][1] + u[0][2]) - (u[2][0] + 2.0 * u[2][1] + u[2][2]);
        const double k1 = (u[0][0] + 2.0 * u[1][0] + u[2][0]) - (u[0][2] + 2.0 * u[1][2] + u[2][2]);
        const double k2 = (2.0 * u[0][0] + u[0][1] + u[1][0]) - (u[1][2] + u[2][1] + 2.0 * u[2][2]);
        const double k3 = (u[0][1] + 2.0 * u[0][2] + u[1][2]) - (u[1][0] + 2.0 * u[2][0] + u[2][1]);
        m2[t] = sqrt(k0 * k0 + k1 * k1 + k2 * k2 + k3 * k3);
      }
      const double d = m2[1] - m2[0];
      gd = d * d;
    }
  }
  // fixed-order block reduction: wave shuffles, then the four wave sums in order
  __syncthreads();                          // HS is reused below
  double* red = &HS[0][0][0];
  const double v0 = wave_sum(ssim), v1 = wave_sum(gssim), v2 = wave_sum(gd);
  if ((tid & 63) == 0) { red[3 * (tid >> 6)] = v0; red[3 * (tid >> 6) + 1] = v1; red[3 * (tid >> 6) + 2] = v2; }
  if constexpr (MASKED) {
#pragma unroll
    for (int k = 0; k < NCNT; ++k) {
      const int c = wave_sum_i(cnt[k]);
      if ((tid & 63) == 0) ired[tid >> 6][k] = c;
    }
  }
  __syncthreads();
  const size_t blk = ((size_t)img * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
  if (tid < NPART) {
    const double t = ((red[tid] + red[3 + tid]) + red[6 + tid]) + red[9 + tid];
    part[NPART * blk + tid] = t;
  }
  if constexpr (MASKED) {
    if (tid >= 64 && tid < 64 + NCNT) {
      const int k = tid - 64;
      pcnt[NCNT * blk + k] = ired[0][k] + ired[1][k] + ired[2][k] + ired[3][k];
    }
  }
}

// numpy 2.x _lerp in float32: a + (b-a)*t, or b - (b-a)*(1-t) where t >= 0.5
__device__ __forceinline__ float np_lerp(float a, float b, float t) {
  const float d = b - a;
  return t >= 0.5f ? b - d * (1.f - t) : a + d * t;
}

// ---- 4. selection, strata, finalize ----------------------------------------------------------------------------
// One workgroup per image.  Targets 0..3 are the ranks floor(vi25), floor(vi25)+1, floor(vi75), floor(vi75)+1 with
// vi = (N-1) * q in float32 (numpy: python int times the float32 quantile).  Each pass fixes the next digit of every
// target's bit pattern from a histogram of the elements that share the target's already fixed high bits; targets
// with equal prefixes share one histogram.
//
// MASKED: the population of the selection is the ns pixels of the strata set (g != G_OUT), ns being the sum of the tiles'
// counts; the upper ranks are clamped to ns - 1 (numpy's percentile of one value is that value).  The squared error is summed
// over the valid pixels (vmap), the strata over the strata set; each mean divides by its own count, a column whose count is 0
// is NaN.  rq = the (B, 4) rows of prep: R is read from them, q25 / q75 are left in them; cnt_out = (B, 5): n0, n1, n3, n4, ns.
template <bool MASKED>
__global__ __launch_bounds__(SEL_THREADS) void eval_select_kernel(
    const float* __restrict__ g, const float* __restrict__ a, const float* __restrict__ b, int H, int W,
    const float* __restrict__ rng, float data_range, const double* __restrict__ part, int tiles_per_img,
    float* __restrict__ q_out, int* __restrict__ cnt_out, double* __restrict__ out8,
    const unsigned char* __restrict__ vmap, const int* __restrict__ pcnt) {
  __shared__ unsigned hist[4][2048];
  __shared__ unsigned prefix[4], rank[4];
  __shared__ int slot[4];
  __shared__ double wred[SEL_THREADS / 64][8];
  __shared__ float qs[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = H * W;
  const size_t off = (size_t)blockIdx.x * N;
  const unsigned* gu = reinterpret_cast<const unsigned*>(g + off);
  __shared__ int tcw[SEL_THREADS / 64][NCNT], tcnt[NCNT];
  int last = N - 1;               // the largest rank of the population
  if constexpr (MASKED) {
    int c[NCNT] = {0, 0, 0, 0};
    const int* pc = pcnt + (size_t)blockIdx.x * tiles_per_img * NCNT;
#pragma unroll 1
    for (int k = tid; k < tiles_per_img; k += SEL_THREADS)
#pragma unroll
      for (int j = 0; j < NCNT; ++j) c[j] += pc[NCNT * k + j];
#pragma unroll
    for (int j = 0; j < NCNT; ++j) {
      const int v = wave_sum_i(c[j]);
      if (lane == 0) tcw[wave][j] = v;
    }
    __syncthreads();
    if (tid < NCNT) {
      int n = 0;
      for (int w = 0; w < SEL_THREADS / 64; ++w) n += tcw[w][tid];
      tcnt[tid] = n;
    }
    __syncthreads();
    last = tcnt[3] > 0 ? tcnt[3] - 1 : 0;
  }
  const float vi25 = (float)last * 0.25f, vi75 = (float)last * 0.75f;
  const float p25 = floorf(vi25), p75 = floorf(vi75);
  if (tid < 4) {
    const float p = tid < 2 ? p25 : p75;
    unsigned r = (unsigned)p + (tid & 1);
    if constexpr (MASKED) r = r > (unsigned)last ? (unsigned)last : r;
    rank[tid] = r;
    prefix[tid] = 0u;
  }
  __syncthreads();
#pragma unroll 1
  for (int pass = 0; pass < 3; ++pass) {
    const int width = pass == 2 ? 10 : 11, sh = pass == 0 ? 21 : (pass == 1 ? 10 : 0), nb = 1 << width;
    const unsigned hi_mask = pass == 0 ? 0u : ~((1u << (sh + width)) - 1u);
#pragma unroll 1
    for (int e = tid; e < 4 * 2048; e += SEL_THREADS) (&hist[0][0])[e] = 0u;
    if (tid < 4) {
      int s = tid;
      for (int t = 0; t < tid; ++t)
        if (prefix[t] == prefix[tid]) { s = t; break; }
      slot[tid] = s;
    }
    __syncthreads();
    unsigned pf[4];
    bool own[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) { pf[t] = prefix[t]; own[t] = slot[t] == t; }
#pragma unroll 1
    for (int i = tid; i < N; i += SEL_THREADS) {
      const unsigned u = gu[i], hb = u & hi_mask, d = (u >> sh) & (unsigned)(nb - 1);
      if constexpr (MASKED) {
        if (u == G_OUT) continue;
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (own[t] && hb == pf[t]) atomicAdd(&hist[t][d], 1u);
    }
    __syncthreads();
    if (wave < 4) {               // wave t resolves target t: lane l owns bins [l*per, (l+1)*per)
      const int t = wave, h = slot[t], per = nb >> 6;
      const unsigned k = rank[t];
      unsigned sum = 0;
#pragma unroll 1
      for (int j = 0; j < per; ++j) sum += hist[h][lane * per + j];
      unsigned incl = sum;        // inclusive scan over the 64 lanes
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      unsigned cum = incl - sum;
      if (cum <= k && k < incl) {   // exactly one lane holds rank k
        int d = lane * per;
#pragma unroll 1
        for (int j = 0; j < per; ++j) {
          const unsigned c = hist[h][lane * per + j];
          if (cum + c > k) { d = lane * per + j; break; }
          cum += c;
        }
        rank[t] = k - cum;
        prefix[t] |= (unsigned)d << sh;
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    const float v0 = __uint_as_float(prefix[0]), v1 = __uint_as_float(prefix[1]);
    const float v2 = __uint_as_float(prefix[2]), v3 = __uint_as_float(prefix[3]);
    qs[0] = np_lerp(v0, v1, vi25 - p25);
    qs[1] = np_lerp(v2, v3, vi75 - p75);
    if constexpr (MASKED) {
      q_out[4 * blockIdx.x + 1] = qs[0]; q_out[4 * blockIdx.x + 2] = qs[1];
    } else {
      if (q_out) { q_out[2 * blockIdx.x] = qs[0]; q_out[2 * blockIdx.x + 1] = qs[1]; }
    }
  }
  __syncthreads();
  const float q25 = qs[0], q75 = qs[1];
  // strata: e = (a-b)^2 in float32, sums in float64 (thread-strided, then wave shuffles and the waves in order)
  double s_lo = 0.0, s_mid = 0.0, s_hi = 0.0, s_all = 0.0;
  int n_lo = 0, n_mid = 0, n_hi = 0, n_all = 0;
  #pragma unroll 1
  for (int i = tid; i < N; i += SEL_THREADS) {
    const float gv = g[off + i];
    float e = 0.f;
    bool lo = gv < q25, mid = gv >= q25 && gv <= q75, hi = gv >= q75;
    if constexpr (MASKED) {
      const bool in = gu[i] != G_OUT;
      lo = lo && in; mid = mid && in; hi = hi && in;
      if (vmap[off + i]) {
        const float d = a[off + i] - b[off + i];
        e = d * d;
        s_all += (double)e;
        ++n_all;
      }
    } else {
      if (b) { const float d = a[off + i] - b[off + i]; e = d * d; }
      s_all += (double)e;
    }
    if (lo) { s_lo += (double)e; ++n_lo; }
    if (mid) { s_mid += (double)e; ++n_mid; }
    if (hi) { s_hi += (double)e; ++n_hi; }
  }
  // tile partials of this image, strided over the block (fixed assignment, fixed order)
  double p_ssim = 0.0, p_gssim = 0.0, p_gd = 0.0;
  if (part) {
    const double* pp = part + (size_t)blockIdx.x * tiles_per_img * NPART;
    #pragma unroll 1
    for (int k = tid; k < tiles_per_img; k += SEL_THREADS) {
      p_ssim += pp[NPART * k]; p_gssim += pp[NPART * k + 1]; p_gd += pp[NPART * k + 2];
    }
  }
  double v[7] = {s_lo, s_mid, s_hi, s_all, p_ssim, p_gssim, p_gd};
  int c[4] = {n_lo, n_mid, n_hi, n_all};
#pragma unroll
  for (int k = 0; k < 7; ++k) v[k] = wave_sum(v[k]);
#pragma unroll
  for (int k = 0; k < 4; ++k) c[k] = wave_sum_i(c[k]);
  __shared__ int cred[SEL_THREADS / 64][4];
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < 7; ++k) wred[wave][k] = v[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) cred[wave][k] = c[k];
  }
  __syncthreads();
  // wave sums in wave order: thread k < 7 folds value k, threads 7..10 the counts
  __shared__ double fin[7];
  __shared__ int nfin[4];
  if (tid < 11) {
    double t = 0.0;
    int n = 0;
#pragma unroll 1
    for (int w = 0; w < SEL_THREADS / 64; ++w) {
      if (tid < 7) t += wred[w][tid]; else n += cred[w][tid - 7];
    }
    if (tid < 7) fin[tid] = t; else nfin[tid - 7] = n;
  }
  __syncthreads();
  if (tid == 0) {
    const double* t = fin;
    const int* n = nfin;
    if constexpr (MASKED) {
      const float R = data_range >= 0.f ? data_range : rng[4 * blockIdx.x];
      const int n0 = n[3], n1 = tcnt[0], n3 = tcnt[1], n4 = tcnt[2], ns = tcnt[3];
      int* co = cnt_out + 5 * (size_t)blockIdx.x;
      co[0] = n0; co[1] = n1; co[2] = n3; co[3] = n4; co[4] = ns;
      const double nan = (double)__uint_as_float(0x7FC00000u);
      const double mse = t[3] / (double)n0, dS = (double)ns;
      double* o = out8 + 8 * (size_t)blockIdx.x;
      o[0] = n0 > 0 ? 10.0 * log10((double)(R * R) / mse) : nan;
      o[1] = n3 > 0 ? t[4] / (double)n3 : nan;
      o[2] = n0 > 0 ? sqrt(mse) : nan;
      o[3] = ns > 0 ? sqrt(t[0] / dS) : nan;
      o[4] = ns > 0 ? sqrt(t[1] / dS) : nan;
      o[5] = ns > 0 ? sqrt(t[2] / dS) : nan;
      o[6] = n4 > 0 ? t[5] / (double)n4 : nan;
      o[7] = n1 > 0 ? sqrt(t[6] / (double)n1) : nan;
      return;
    }
    if (cnt_out) for (int k = 0; k < 3; ++k) cnt_out[3 * blockIdx.x + k] = n[k];
    if (out8) {
      const float R = data_range >= 0.f ? data_range : rng[blockIdx.x];
      const double dN = (double)N, mse = t[3] / dN;
      double* o = out8 + 8 * (size_t)blockIdx.x;
      o[0] = 10.0 * log10((double)(R * R) / mse);      // skimage: data_range ** 2 in float32, / float64 mse
      o[1] = t[4] / ((double)(H - 6) * (W - 6));
      o[2] = sqrt(mse);
      o[3] = sqrt(t[0] / dN);
      o[4] = sqrt(t[1] / dN);
      o[5] = sqrt(t[2] / dN);
      o[6] = t[5] / ((double)(H - 8) * (W - 8));
      o[7] = sqrt(t[6] / ((double)(H - 2) * (W - 2)));
    }
  }
}

constexpr size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

// scratch: [g map B*H*W floats][R per pair][per-tile partials]
size_t eval_metrics_scratch_bytes(int B, int H, int W) {
  if (B < 1 || H < 16 || W < 16) return 0;
  const size_t tiles = (size_t)((W + ET - 1) / ET) * ((H + ET - 1) / ET);
  return align256((size_t)B * H * W * sizeof(float)) + align256((size_t)B * sizeof(float)) +
         (size_t)B * tiles * NPART * sizeof(double);
}

static bool eval_shape_ok(int B, int H, int W) {
  return B >= 1 && B <= 65535 && H >= 16 && W >= 16 && (long long)H * W < (1LL << 31) && (H + ET - 1) / ET <= 65535;
}

int launch_eval_metrics(const float* a, const float* b, int B, int H, int W, const float* taps9, float data_range,
                        void* scratch, double* out8, hipStream_t s) {
  if (!eval_shape_ok(B, H, W)) return SIFSR_ERR_SHAPE;
  const int N = H * W;
  char* p = reinterpret_cast<char*>(scratch);
  float* g = reinterpret_cast<float*>(p);
  float* rng = reinterpret_cast<float*>(p + align256((size_t)B * N * sizeof(float)));
  double* part = reinterpret_cast<double*>(p + align256((size_t)B * N * sizeof(float)) + align256((size_t)B * sizeof(float)));
  const dim3 tg((W + ET - 1) / ET, (H + ET - 1) / ET, B);
  int rc = launch_blur_fwd(a, taps9, g, B, H, W, s);
  if (rc != SIFSR_OK) return rc;
  hipLaunchKernelGGL(eval_prep_kernel<false>, dim3(B), dim3(1024), 0, s, a, b, g, N, rng, (const unsigned char*)nullptr,
                     (unsigned char*)nullptr);
  hipLaunchKernelGGL(eval_tile_kernel<false>, tg, dim3(256), 0, s, a, b, H, W, rng, data_range, part,
                     (const unsigned char*)nullptr, (unsigned*)nullptr, (int*)nullptr);
  hipLaunchKernelGGL(eval_select_kernel<false>, dim3(B), dim3(SEL_THREADS), 0, s, g, a, b, H, W, rng, data_range, part,
                     (int)(tg.x * tg.y), nullptr, nullptr, out8, (const unsigned char*)nullptr, (const int*)nullptr);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

// scratch: [g map B*H*W floats, G_OUT outside the strata set][B rows of R, q25, q75, -][validity bytes B*H*W]
//          [per-tile partials][per-tile counts]; the first two regions are documented in include/sifsr_scores.h
size_t eval_metrics_masked_scratch_bytes(int B, int H, int W) {
  if (!eval_shape_ok(B, H, W)) return 0;
  const size_t tiles = (size_t)((W + ET - 1) / ET) * ((H + ET - 1) / ET), n = (size_t)B * H * W;
  return align256(n * sizeof(float)) + align256((size_t)B * 4 * sizeof(float)) + align256(n) +
         align256((size_t)B * tiles * NPART * sizeof(double)) + (size_t)B * tiles * NCNT * sizeof(int);
}

int launch_eval_metrics_masked(const float* a, const float* b, const unsigned char* mask, int B, int H, int W,
                               const float* taps9, float data_range, void* scratch, double* out8, int* counts5, hipStream_t s) {
  if (!eval_shape_ok(B, H, W)) return SIFSR_ERR_SHAPE;
  const int N = H * W;
  const dim3 tg((W + ET - 1) / ET, (H + ET - 1) / ET, B);
  const size_t tiles = (size_t)tg.x * tg.y, n = (size_t)B * N;
  char* p = reinterpret_cast<char*>(scratch);
  float* g = reinterpret_cast<float*>(p);
  p += align256(n * sizeof(float));
  float* rq = reinterpret_cast<float*>(p);
  p += align256((size_t)B * 4 * sizeof(float));
  unsigned char* vmap = reinterpret_cast<unsigned char*>(p);
  p += align256(n);
  double* part = reinterpret_cast<double*>(p);
  p += align256((size_t)B * tiles * NPART * sizeof(double));
  int* pcnt = reinterpret_cast<int*>(p);
  int rc = launch_blur_fwd(a, taps9, g, B, H, W, s);   // on the raw reference: a NaN spreads 4 pixels, none of them in the strata set
  if (rc != SIFSR_OK) return rc;
  hipLaunchKernelGGL(eval_prep_kernel<true>, dim3(B), dim3(1024), 0, s, a, b, g, N, rq, mask, vmap);
  hipLaunchKernelGGL(eval_tile_kernel<true>, tg, dim3(256), 0, s, a, b, H, W, rq, data_range, part,
                     (const unsigned char*)vmap, reinterpret_cast<unsigned*>(g), pcnt);
  hipLaunchKernelGGL(eval_select_kernel<true>, dim3(B), dim3(SEL_THREADS), 0, s, g, a, b, H, W, rq, data_range,
                     (const double*)part, (int)tiles, rq, counts5, out8, (const unsigned char*)vmap, (const int*)pcnt);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int launch_gradient_strata(const float* a, int B, int H, int W, const float* taps9, float* g, float* q2, int* counts3,
                           hipStream_t s) {
  if (!eval_shape_ok(B, H, W)) return SIFSR_ERR_SHAPE;
  const int N = H * W;
  int rc = launch_blur_fwd(a, taps9, g, B, H, W, s);
  if (rc != SIFSR_OK) return rc;
  hipLaunchKernelGGL(eval_prep_kernel<false>, dim3(B), dim3(1024), 0, s, a, (const float*)nullptr, g, N, (float*)nullptr,
                     (const unsigned char*)nullptr, (unsigned char*)nullptr);
  hipLaunchKernelGGL(eval_select_kernel<false>, dim3(B), dim3(SEL_THREADS), 0, s, g, a, (const float*)nullptr, H, W,
                     (const float*)nullptr, -1.f, (const double*)nullptr, 0, q2, counts3, (double*)nullptr,
                     (const unsigned char*)nullptr, (const int*)nullptr);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}
