// LPIPS-VGG16 on the device (include/sifsr_lpips.h): the ninth column of the per-pair ASTER table.
//
// Replaces what the reference runs on the CPU through torchvision's vgg16().features and lpips.py:226-292 (ContentLoss.forward,
// normalize_features = True, distance = 'mse'), as called at model_perf_aster_formatds.py:134, :405-410.
//
// Both images of every pair travel as ONE batch of 2N NHWC tensors (x_i = image i, y_i = image N + i), so every launch serves both:
//   prepare   scan (per pair: min / max, the non-finite flag) and convert (standardise or min/max-normalise, NCHW -> NHWC, the 3
//             channels padded to 16 with zeros);
//   13 x      conv3x3 with zero padding on the fp32 matrix cores (launch_conv3x3_mfma, tap-domain kernel, output channels beyond
//             128 in slices of 128: the weight pack is [cout block][cin block]..., a slice is a pointer offset) -- or, for a feature
//             map with min(H, W) < 16 (thinner than one tile of that kernel), the plain direct kernel below -- into a RAW tensor,
//             then bias + ReLU as a pass of its own (the conv's staging path would turn zero padding into relu(bias), see
//             launch_layer), with the 2 x 2 floor max-pool fused in where a pool follows;
//   5 x       distance: one wave per pixel reduces the two channel norms and the lin-weighted squared difference over up to 512
//             contiguous channels; the spatial sum is accumulated in float64 per wave, per block, and written per block;
//   finish    one thread per pair adds the block partials in index order, divides by the pixel count, sums the layers, and
//             writes NaN rows for the flagged pairs.
// No atomics, no allocation, no synchronisation: one linear chain of launches.  Per-pixel arithmetic never depends on N or on the
// position of the pair in the batch, which is what makes row i bit-identical to its own N = 1 call.
#include "../../include/sifsr_lpips.h"

#include "conv.h"

namespace {

constexpr int NL = 13;
constexpr int CIN[NL] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int COUT[NL] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int TAP[NL] = {-1, 0, -1, 1, -1, -1, 2, -1, -1, 3, -1, -1, 4};   // the tap a layer's ReLU output is; a pool follows taps 0..3
constexpr int NBIAS = 4224, NLIN = 1472;
constexpr int PMAX = 128;          // block partials per (layer, pair) at most
constexpr int DIRECT_BELOW = 16;   // feature maps with min(H, W) below this go through the direct kernel (sifsr_lpips.h)
constexpr int DPIX = 4;            // pixels per wave of the direct kernel

struct PackTab {
  int w_src[NL], b_src[NL];   // offsets in vgg_params
  int w_pk[NL], b_pk[NL];     // offsets in packed (b_pk relative to bias0)
  int cin[NL], cout[NL];
  int bias0, lin0, total;
  int lin_off[5];
};

const PackTab& tab() {
  static const PackTab t = [] {
    PackTab r{};
    int src = 0, pk = 0, b = 0;
    for (int l = 0; l < NL; ++l) {
      const int cinp = CIN[l] < 16 ? 16 : CIN[l];
      r.w_src[l] = src; src += 9 * CIN[l] * COUT[l];
      r.b_src[l] = src; src += COUT[l];
      r.w_pk[l] = pk; pk += 9 * cinp * COUT[l];
      r.b_pk[l] = b; b += COUT[l];
      r.cin[l] = CIN[l]; r.cout[l] = COUT[l];
    }
    r.bias0 = pk; r.lin0 = pk + NBIAS; r.total = pk + NBIAS + NLIN;
    int lo = 0;
    for (int l = 0; l < NL; ++l)
      if (TAP[l] >= 0) { r.lin_off[TAP[l]] = lo; lo += COUT[l]; }
    return r;
  }();
  return t;
}

// ---- pack: OIHW -> wf[nb][q][tap][lane][j] (the forward layout documented above pack_weights_kernel), biases, lin -----------
__global__ void lpips_pack_kernel(const float* __restrict__ vgg, const float* __restrict__ lin, float* __restrict__ packed, const PackTab t) {
  const int l = blockIdx.y;
  const int i0 = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
  if (l == NL) {
    for (int i = i0; i < NBIAS + NLIN; i += step) {
      if (i < NBIAS) {
        int k = 0;
        while (k + 1 < NL && t.b_pk[k + 1] <= i) ++k;
        packed[t.bias0 + i] = vgg[t.b_src[k] + (i - t.b_pk[k])];
      } else {
        packed[t.lin0 + (i - NBIAS)] = lin[i - NBIAS];
      }
    }
    return;
  }
  const int cin = t.cin[l], cout = t.cout[l];
  const int cinp = cin < 16 ? 16 : cin, NQ = cinp / 16;
  const int n = 9 * cinp * cout;
  const float* W = vgg + t.w_src[l];
  for (int e = i0; e < n; e += step) {
    const int j = e & 3, lane = (e >> 2) & 63;
    const int rest = e >> 8;
    const int tap = rest % 9, r2 = rest / 9;
    const int q = r2 % NQ, nb = r2 / NQ;
    const int co = 16 * nb + (lane & 15), ci = 16 * q + 4 * (lane >> 4) + j;
    packed[t.w_pk[l] + e] = ci < cin ? W[(co * cin + ci) * 9 + tap] : 0.f;
  }
}

// ---- prepare -------------------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// one block per pair: min / max over both images and the flag (a non-finite pixel; pairs mode: also maxi == mini)
__global__ __launch_bounds__(256) void lpips_scan_kernel(const float* __restrict__ x, const float* __restrict__ y, const size_t n,
                                                         const int pairs_mode, float* __restrict__ mm, int* __restrict__ flag) {
  __shared__ float slo[4], shi[4];
  __shared__ int sbad[4];
  const int i = blockIdx.x, tid = threadIdx.x;
  const float* px = x + (size_t)i * n;
  const float* py = y + (size_t)i * n;
  float lo = INFINITY, hi = -INFINITY;
  int bad = 0;
  for (size_t k = tid; k < n; k += 256) {
    const float a = px[k], b = py[k];
    bad |= (int)!finite_bits(a) | (int)!finite_bits(b);
    lo = fminf(lo, fminf(a, b));
    hi = fmaxf(hi, fmaxf(a, b));
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    lo = fminf(lo, __shfl_xor(lo, m));
    hi = fmaxf(hi, __shfl_xor(hi, m));
    bad |= __shfl_xor(bad, m);
  }
  if ((tid & 63) == 0) { slo[tid >> 6] = lo; shi[tid >> 6] = hi; sbad[tid >> 6] = bad; }
  __syncthreads();
  if (tid == 0) {
    lo = fminf(fminf(slo[0], slo[1]), fminf(slo[2], slo[3]));
    hi = fmaxf(fmaxf(shi[0], shi[1]), fmaxf(shi[2], shi[3]));
    bad = sbad[0] | sbad[1] | sbad[2] | sbad[3];
    mm[2 * i] = lo; mm[2 * i + 1] = hi;
    flag[i] = (bad || (pairs_mode && !(hi > lo))) ? 1 : 0;
  }
}

// one thread per pixel of the 2N batch: (t - mean) / std per channel, NHWC with 16 channels (3 used).  pairs mode: the single
// channel is first normalised to t = (v - mini) / (maxi - mini) and repeated.
__global__ __launch_bounds__(256) void lpips_convert_kernel(const float* __restrict__ x, const float* __restrict__ y, const int N, const int HW,
                                                            const int pairs_mode, const float* __restrict__ mm, const float m0, const float m1,
                                                            const float m2, const float s0, const float s1, const float s2,
                                                            float* __restrict__ out) {
  const size_t total = (size_t)2 * N * HW;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int b = (int)(idx / HW), p = (int)(idx - (size_t)b * HW);
    const int i = b < N ? b : b - N;
    const float* src = b < N ? x : y;
    float v0, v1, v2;
    if (pairs_mode) {
      const float lo = mm[2 * i], hi = mm[2 * i + 1];
      v0 = v1 = v2 = (src[(size_t)i * HW + p] - lo) / (hi - lo);
    } else {
      const float* s = src + (size_t)i * 3 * HW + p;
      v0 = s[0]; v1 = s[HW]; v2 = s[2 * (size_t)HW];
    }
    float* o = out + idx * 16;
    st4(o, make_float4((v0 - m0) / s0, (v1 - m1) / s1, (v2 - m2) / s2, 0.f));
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    st4(o + 4, z); st4(o + 8, z); st4(o + 12, z);
  }
}

// ---- bias + ReLU (+ 2 x 2 floor max-pool) ---------------------------------------------------------------------------------------
static __device__ __forceinline__ float4 bias_relu4(float4 v, float4 b) {
  return make_float4(fmaxf(v.x + b.x, 0.f), fmaxf(v.y + b.y, 0.f), fmaxf(v.z + b.z, 0.f), fmaxf(v.w + b.w, 0.f));
}

// POOL: one thread per (2 x 2 cell, channel quad): writes the activated pixels of its cell that exist (odd H / W: the last row /
// column has cells of one or two pixels) and, for a complete cell, their maximum (MaxPool2d(2, 2) drops the incomplete cells).
template <bool POOL>
__global__ __launch_bounds__(256) void lpips_bias_relu_kernel(const float* __restrict__ raw, const float* __restrict__ bias, float* __restrict__ act,
                                                              float* __restrict__ pooled, const int B, const int H, const int W, const int C) {
  const int C4 = C / 4;
  if (!POOL) {
    const size_t total = (size_t)B * H * W * C4;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
      const int c4 = (int)(idx % C4);
      st4(act + idx * 4, bias_relu4(ld4(raw + idx * 4), ld4(bias + 4 * c4)));
    }
  } else {
    const int Hc = (H + 1) / 2, Wc = (W + 1) / 2, Hp = H / 2, Wp = W / 2;
    const size_t total = (size_t)B * Hc * Wc * C4;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
      const int c4 = (int)(idx % C4);
      size_t r = idx / C4;
      const int cx = (int)(r % Wc); r /= Wc;
      const int cy = (int)(r % Hc);
      const int b = (int)(r / Hc);
      const float4 bv = ld4(bias + 4 * c4);
      float4 m = make_float4(0.f, 0.f, 0.f, 0.f);   // ReLU outputs are >= 0
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        const int yy = 2 * cy + (d >> 1), xx = 2 * cx + (d & 1);
        if (yy < H && xx < W) {
          const size_t o = (((size_t)b * H + yy) * W + xx) * C + 4 * c4;
          const float4 v = bias_relu4(ld4(raw + o), bv);
          st4(act + o, v);
          m = make_float4(fmaxf(m.x, v.x), fmaxf(m.y, v.y), fmaxf(m.z, v.z), fmaxf(m.w, v.w));
        }
      }
      if (cy < Hp && cx < Wp) st4(pooled + (((size_t)b * Hp + cy) * Wp + cx) * C + 4 * c4, m);
    }
  }
}

// ---- direct 3x3 conv, zero padding, for feature maps thinner than one MFMA tile ------------------------------------------------
// One wave per (DPIX consecutive pixels, 16 output channels), reading the same fragment pack as the MFMA kernel: lane (i = lane & 15,
// kq = lane >> 4) holds W[co = 16 nb + i][ci = 16 q + 4 kq .. + 3][tap] -- one coalesced 1 KiB read per (q, tap) per wave -- and
// contracts its four input channels; the four kq partial sums of an output channel are added by two shuffles.  Raw output (no
// bias): the bias + ReLU pass is shared with the MFMA path.
__global__ __launch_bounds__(256) void lpips_conv_direct_kernel(const float* __restrict__ in, const float* __restrict__ wpk, float* __restrict__ out,
                                                                const int B, const int H, const int W, const int Cin, const int Cout) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int NQ = Cin / 16, NBt = Cout / 16;
  const int npix = B * H * W, ngrp = (npix + DPIX - 1) / DPIX;
  const long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= (long long)ngrp * NBt) return;
  const int nb = (int)(item % NBt), grp = (int)(item / NBt);
  const int kq = lane >> 4;
  int pb[DPIX], py[DPIX], px[DPIX];
  bool pv[DPIX];
  float acc[DPIX];
#pragma unroll
  for (int p = 0; p < DPIX; ++p) {
    const int pix = grp * DPIX + p;
    pv[p] = pix < npix;
    const int pc = pv[p] ? pix : 0;
    px[p] = pc % W; py[p] = (pc / W) % H; pb[p] = pc / (W * H);
    acc[p] = 0.f;
  }
  for (int tap = 0; tap < 9; ++tap) {
    const int dy = tap / 3 - 1, dx = tap - 3 * (tap / 3) - 1;
    bool ok[DPIX];
    const float* ip[DPIX];
#pragma unroll
    for (int p = 0; p < DPIX; ++p) {
      const int yy = py[p] + dy, xx = px[p] + dx;
      ok[p] = pv[p] && yy >= 0 && yy < H && xx >= 0 && xx < W;
      ip[p] = in + (((size_t)pb[p] * H + (ok[p] ? yy : 0)) * W + (ok[p] ? xx : 0)) * Cin + 4 * kq;
    }
    for (int q = 0; q < NQ; ++q) {
      const float4 w = ld4(wpk + ((size_t)(nb * NQ + q) * 9 + tap) * 256 + lane * 4);
#pragma unroll
      for (int p = 0; p < DPIX; ++p) {
        if (ok[p]) {
          const float4 a = ld4(ip[p] + 16 * q);
          acc[p] = fmaf(w.x, a.x, acc[p]); acc[p] = fmaf(w.y, a.y, acc[p]);
          acc[p] = fmaf(w.z, a.z, acc[p]); acc[p] = fmaf(w.w, a.w, acc[p]);
        }
      }
    }
  }
#pragma unroll
  for (int p = 0; p < DPIX; ++p) {
    float v = acc[p];
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    if (lane < 16 && pv[p]) out[(size_t)(grp * DPIX + p) * Cout + 16 * nb + lane] = v;
  }
}

// ---- distance: one wave per pixel, K = C / 64 channels per lane (c = lane + 64 k: every load instruction reads 256 contiguous bytes)
template <int K>
__global__ __launch_bounds__(256) void lpips_distance_kernel(const float* __restrict__ act, const float* __restrict__ lin, double* __restrict__ partial,
                                                             const int N, const int HW) {
  constexpr int C = 64 * K;
  __shared__ double sh[4];
  const int i = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* fx = act + (size_t)i * HW * C;
  const float* fy = act + (size_t)(N + i) * HW * C;
  float lw[K];
#pragma unroll
  for (int k = 0; k < K; ++k) lw[k] = lin[lane + 64 * k];
  double accd = 0.0;
  for (int p = blockIdx.x * 4 + wave; p < HW; p += gridDim.x * 4) {
    float vx[K], vy[K];
    float sx = 0.f, sy = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      vx[k] = fx[(size_t)p * C + lane + 64 * k];
      vy[k] = fy[(size_t)p * C + lane + 64 * k];
      sx = fmaf(vx[k], vx[k], sx);
      sy = fmaf(vy[k], vy[k], sy);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) { sx += __shfl_xor(sx, m); sy += __shfl_xor(sy, m); }
    const float nx = sqrtf(sx) + 1e-10f, ny = sqrtf(sy) + 1e-10f;
    float d = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float t = vx[k] / nx - vy[k] / ny;
      d = fmaf(lw[k], t * t, d);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) d += __shfl_xor(d, m);
    accd += (double)d;
  }
  if (lane == 0) sh[wave] = accd;
  __syncthreads();
  if (threadIdx.x == 0) partial[(size_t)i * gridDim.x + blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

struct FinishTab { int nblk[5], hw[5]; };

__global__ void lpips_finish_kernel(const double* __restrict__ partial, const int* __restrict__ flag, double* __restrict__ out6, const int N,
                                    const FinishTab t) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  double total = 0.0, d[5];
  for (int l = 0; l < 5; ++l) {
    const double* p = partial + (size_t)l * N * PMAX + (size_t)i * t.nblk[l];
    double s = 0.0;
    for (int k = 0; k < t.nblk[l]; ++k) s += p[k];
    d[l] = s / (double)t.hw[l];
    total += d[l];
  }
  const bool bad = flag[i] != 0;
  const double nan = __longlong_as_double(0x7FF8000000000000LL);
  for (int l = 0; l < 5; ++l) out6[6 * (size_t)i + l] = bad ? nan : d[l];
  out6[6 * (size_t)i + 5] = bad ? nan : total;
}

// ---- host side --------------------------------------------------------------------------------------------------------------
size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct WsLayout { size_t flag, mm, partial, buf[3], total; };

bool ws_layout(int N, int H, int W, WsLayout& w) {
  if (N < 1 || H < DIRECT_BELOW || W < DIRECT_BELOW) return false;
  const unsigned long long npix = 2ull * (unsigned long long)N * (unsigned long long)H * (unsigned long long)W;
  if (H > (1 << 20) || W > (1 << 20) || npix * 64ull * 4ull >= (1ull << 32) - 4096ull) return false;
  size_t o = 0;
  w.flag = o; o = up256(o + (size_t)N * sizeof(int));
  w.mm = o; o = up256(o + (size_t)N * 2 * sizeof(float));
  w.partial = o; o = up256(o + (size_t)5 * N * PMAX * sizeof(double));
  for (int k = 0; k < 3; ++k) { w.buf[k] = o; o = up256(o + (size_t)npix * 64 * sizeof(float)); }
  w.total = o;
  return true;
}

int grid_for(size_t total) {
  const size_t g = (total + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 16384 ? 16384 : g));
}

// conv of layer l on the B x h x w batch: in (activated, stored) -> raw (no bias).
// The bias does NOT go through ConvSrc.scale/shift: the staging path applies relu(x * scale + shift) to what it loaded, and with
// zero padding the out-of-image lanes loaded 0, so the padding would become relu(bias).  Every conv reads a stored, activated input.
int launch_layer(int l, const float* in, float* raw, const float* packed, int B, int h, int w, hipStream_t s) {
  const int cinp = CIN[l] < 16 ? 16 : CIN[l], cout = COUT[l], NQ = cinp / 16;
  const float* wpk = packed + tab().w_pk[l];
  if (h < DIRECT_BELOW || w < DIRECT_BELOW) {
    const long long items = (long long)((B * h * w + DPIX - 1) / DPIX) * (cout / 16);
    hipLaunchKernelGGL(lpips_conv_direct_kernel, dim3((unsigned)((items + 3) / 4)), dim3(256), 0, s, in, wpk, raw, B, h, w, cinp, cout);
    SIFSR_LAUNCH_CHECK();
    return SIFSR_OK;
  }
  const int sl = cout > 128 ? 128 : cout;
  for (int k = 0; k < cout / sl; ++k) {
    ConvArgs a{};
    a.src[0] = ConvSrc{in, nullptr, nullptr, cinp, 0, NQ};
    a.src[1] = ConvSrc{nullptr, nullptr, nullptr, 0, 0, 0};
    a.dst[0] = ConvDst{raw, cout, k * sl};
    a.dst[1] = a.dst[0];
    a.wpack = wpk + (size_t)k * (sl / 16) * NQ * 9 * 256;
    a.wpack_wino = nullptr;
    a.addend = nullptr; a.stat_partials = nullptr; a.addC = 0;
    a.dst_split = sl / 16;
    a.B = B; a.H = h; a.W = w; a.NQ = NQ;
    const int rc = launch_conv3x3_mfma(a, sl, 1, s);
    if (rc != SIFSR_OK) return rc;
  }
  return SIFSR_OK;
}

int launch_distance(const float* act, const float* lin, double* partial, int N, int hw, int C, int nblk, hipStream_t s) {
  const dim3 grid(nblk, N), block(256);
  switch (C) {
    case 64: hipLaunchKernelGGL(lpips_distance_kernel<1>, grid, block, 0, s, act, lin, partial, N, hw); break;
    case 128: hipLaunchKernelGGL(lpips_distance_kernel<2>, grid, block, 0, s, act, lin, partial, N, hw); break;
    case 256: hipLaunchKernelGGL(lpips_distance_kernel<4>, grid, block, 0, s, act, lin, partial, N, hw); break;
    case 512: hipLaunchKernelGGL(lpips_distance_kernel<8>, grid, block, 0, s, act, lin, partial, N, hw); break;
    default: return SIFSR_ERR_SHAPE;
  }
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int run_lpips(const float* x, const float* y, int pairs_mode, int N, int H, int W, const float* mean3, const float* std3, const float* packed,
              void* workspace, size_t workspace_bytes, double* out6, hipStream_t s) {
  WsLayout L;
  if (!ws_layout(N, H, W, L)) return SIFSR_ERR_SHAPE;
  if (!x || !y || !packed || !workspace || !out6 || (!pairs_mode && (!mean3 || !std3))) return SIFSR_ERR_ARG;
  if (((uintptr_t)workspace & 255) != 0) return SIFSR_ERR_ARG;
  if (N > 65535) return SIFSR_ERR_SHAPE;   // (grid.y of the distance kernel; unreachable below the 4 GiB limit with H, W >= 16)
  if (workspace_bytes < L.total) return SIFSR_ERR_WORKSPACE;
  char* ws = static_cast<char*>(workspace);
  int* flag = reinterpret_cast<int*>(ws + L.flag);
  float* mm = reinterpret_cast<float*>(ws + L.mm);
  double* partial = reinterpret_cast<double*>(ws + L.partial);
  float* raw = reinterpret_cast<float*>(ws + L.buf[0]);
  float* cur = reinterpret_cast<float*>(ws + L.buf[1]);
  float* other = reinterpret_cast<float*>(ws + L.buf[2]);
  const PackTab& t = tab();
  const float* bias = packed + t.bias0;
  const float* lin = packed + t.lin0;
  const int B = 2 * N;
  const float m[3] = {pairs_mode ? 0.f : mean3[0], pairs_mode ? 0.f : mean3[1], pairs_mode ? 0.f : mean3[2]};
  const float sd[3] = {pairs_mode ? 1.f : std3[0], pairs_mode ? 1.f : std3[1], pairs_mode ? 1.f : std3[2]};

  hipLaunchKernelGGL(lpips_scan_kernel, dim3(N), dim3(256), 0, s, x, y, (size_t)(pairs_mode ? 1 : 3) * H * W, pairs_mode, mm, flag);
  SIFSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(lpips_convert_kernel, dim3(grid_for((size_t)B * H * W)), dim3(256), 0, s, x, y, N, H * W, pairs_mode, mm, m[0], m[1], m[2],
                     sd[0], sd[1], sd[2], cur);
  SIFSR_LAUNCH_CHECK();

  FinishTab ft{};
  int h = H, w = W;
  for (int l = 0; l < NL; ++l) {
    int rc = launch_layer(l, cur, raw, packed, B, h, w, s);
    if (rc != SIFSR_OK) return rc;
    const int C = COUT[l];
    const float* bl = bias + t.b_pk[l];
    const int tp = TAP[l];
    if (tp < 0) {
      hipLaunchKernelGGL(lpips_bias_relu_kernel<false>, dim3(grid_for((size_t)B * h * w * (C / 4))), dim3(256), 0, s, raw, bl, other,
                         (float*)nullptr, B, h, w, C);
      SIFSR_LAUNCH_CHECK();
      float* sw = cur; cur = other; other = sw;
      continue;
    }
    const bool pool = tp < 4;
    if (pool) {   // the tap goes to `other`, the pooled tensor over the conv's input (the conv has finished: stream order)
      hipLaunchKernelGGL(lpips_bias_relu_kernel<true>, dim3(grid_for((size_t)B * ((h + 1) / 2) * ((w + 1) / 2) * (C / 4))), dim3(256), 0, s, raw,
                         bl, other, cur, B, h, w, C);
    } else {
      hipLaunchKernelGGL(lpips_bias_relu_kernel<false>, dim3(grid_for((size_t)B * h * w * (C / 4))), dim3(256), 0, s, raw, bl, other,
                         (float*)nullptr, B, h, w, C);
    }
    SIFSR_LAUNCH_CHECK();
    const int hw = h * w;
    int nblk = (hw + 3) / 4;
    nblk = nblk > PMAX ? PMAX : nblk;
    ft.nblk[tp] = nblk; ft.hw[tp] = hw;
    rc = launch_distance(other, lin + t.lin_off[tp], partial + (size_t)tp * N * PMAX, N, hw, C, nblk, s);
    if (rc != SIFSR_OK) return rc;
    if (pool) { h /= 2; w /= 2; }
  }
  hipLaunchKernelGGL(lpips_finish_kernel, dim3((N + 63) / 64), dim3(64), 0, s, partial, flag, out6, N, ft);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

}  // namespace

SIFSR_API size_t sifsrl_pack_floats(void) { return (size_t)tab().total; }

SIFSR_API int sifsrl_pack(const float* vgg_params, const float* lin, float* packed, void* stream) {
  if (!vgg_params || !lin || !packed) return SIFSR_ERR_ARG;
  hipLaunchKernelGGL(lpips_pack_kernel, dim3(256, NL + 1), dim3(256), 0, (hipStream_t)stream, vgg_params, lin, packed, tab());
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

SIFSR_API size_t sifsrl_workspace_bytes(int N, int H, int W) {
  WsLayout L;
  return ws_layout(N, H, W, L) ? L.total : 0;
}

SIFSR_API int sifsrl_lpips(const float* x, const float* y, int N, int H, int W, const float* mean3, const float* std3, const float* packed,
                           void* workspace, size_t workspace_bytes, double* out6, void* stream) {
  return run_lpips(x, y, 0, N, H, W, mean3, std3, packed, workspace, workspace_bytes, out6, (hipStream_t)stream);
}

SIFSR_API int sifsrl_lpips_pairs(const float* a, const float* b, int N, int H, int W, const float* packed, void* workspace, size_t workspace_bytes,
                                 double* out6, void* stream) {
  return run_lpips(a, b, 1, N, H, W, nullptr, nullptr, packed, workspace, workspace_bytes, out6, (hipStream_t)stream);
}
