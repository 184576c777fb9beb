// Gap-aware whole-granule prediction (C ABI: include/sifsr_gaps.h): cloud, ocean and fill pixels of a granule
// are marked, given a neutral local mean before the network sees the raster, tiles without a valid pixel are skipped, and the
// output is masked.  Tile layout and the two per-tile bodies (input pipeline, feathered gather) are those of mosaic.h.
//
//  * gaps_reduce_kernel   one workgroup reduces a 64 x 64 block of one pyramid level through six levels -- two in registers (a
//    thread owns 4 x 4 cells), four in LDS -- and writes all six.  Applied to the raster (where it also writes `valid`), then to
//    level 6, then to level 12: a 1200 x 1200 granule takes two launches, the largest raster three.  A cell is a float64 sum and
//    an integer count; a cell is written once, by the workgroup that owns it.
//  * gaps_fill_kernel     one thread per pixel: a valid pixel is copied, an invalid one walks up its ancestors to the first cell
//    with a count (the push of the header in closed form; the counts of a level are 4 bytes per cell and stay in L2).
//  * gaps_tile_any_kernel / gaps_order_kernel   one workgroup per tile ORs its window's bytes into slot[t]; one wavefront then
//    turns the flags into positions by ballot + prefix population count (select_kernel of products.hip).
//  * gaps_prepare_kernel  mosaic_prepare_kernel over the compact list: workgroups past n_active exit at once.
//  * gaps_blend_kernel    mosaic_blend_kernel with the tile looked up through `slot` and one byte of `valid` per thread.
// All of them small and latency-bound except the last two, which keep the access pattern of the kernels they restate.  No atomics;
// nothing depends on the order in which workgroups run.
#include "../../include/sifsr_gaps.h"

#include "mosaic.h"

namespace {

constexpr int MAX_LEVELS = 16;      // 16384 = 2^14: levels 0 .. 14
constexpr int LEVELS_PER_PASS = 6;  // a 64 x 64 block ends in one cell

struct Pyramid {
  int top;                          // the 1 x 1 level
  int h[MAX_LEVELS], w[MAX_LEVELS];
  unsigned off[MAX_LEVELS];         // first cell of level l >= 1 in the sum / count arrays
  unsigned cells;                   // cells of levels 1 .. top
};

bool pyramid_of(int lst_h, int lst_w, Pyramid* p) {
  if (lst_h < 1 || lst_w < 1 || lst_h > 16384 || lst_w > 16384) return false;
  *p = Pyramid{};
  p->h[0] = lst_h;
  p->w[0] = lst_w;
  int l = 0;
  do {
    ++l;
    p->h[l] = (p->h[l - 1] + 1) / 2;
    p->w[l] = (p->w[l - 1] + 1) / 2;
    p->off[l] = p->cells;
    p->cells += (unsigned)(p->h[l] * p->w[l]);
  } while (p->h[l] > 1 || p->w[l] > 1);
  p->top = l;
  return true;
}
size_t pyramid_bytes(const Pyramid& p) { return (size_t)p.cells * (sizeof(double) + sizeof(int)); }

__device__ __forceinline__ bool gap_valid(float v, const unsigned char* __restrict__ mask, size_t p) {
  return isfinite(v) && v != 0.f && (mask == nullptr || mask[p] != 0);
}

struct Cell { double s; int c; };
__device__ __forceinline__ Cell operator+(Cell a, Cell b) { return Cell{a.s + b.s, a.c + b.c}; }

// cell (i, j) of level l, if the pyramid has it
__device__ __forceinline__ void emit(double* __restrict__ S, int* __restrict__ C, const Pyramid& py, int l, int i, int j, Cell v) {
  if (l <= py.top && i < py.h[l] && j < py.w[l]) {
    const unsigned e = py.off[l] + (unsigned)(i * py.w[l] + j);
    S[e] = v.s;
    C[e] = v.c;
  }
}

// 2 x 2 -> 1 inside a workgroup's block: n = side of the level being formed
template <int N>
__device__ __forceinline__ void reduce_lds(Cell (*src)[2 * N], Cell (*dst)[N], double* __restrict__ S, int* __restrict__ C,
                                           const Pyramid& py, int l) {
  __syncthreads();
  const int t = threadIdx.x;
  if (t < N * N) {
    const int i = t / N, j = t % N;
    const Cell v = (src[2 * i][2 * j] + src[2 * i][2 * j + 1]) + (src[2 * i + 1][2 * j] + src[2 * i + 1][2 * j + 1]);
    dst[i][j] = v;
    emit(S, C, py, l, N * blockIdx.y + i, N * blockIdx.x + j, v);
  }
}

// RAW: level L = 0 is the raster itself (lst, mask -> valid); else level L of the pyramid
template <bool RAW>
__global__ __launch_bounds__(256) void gaps_reduce_kernel(const float* __restrict__ lst, const unsigned char* __restrict__ mask,
                                                          unsigned char* __restrict__ valid, double* __restrict__ S,
                                                          int* __restrict__ C, const Pyramid py, int L) {
  __shared__ Cell l2[16][16], l3[8][8], l4[4][4], l5[2][2], l6[1][1];
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int hin = py.h[L], win = py.w[L];
  const int y0 = 64 * blockIdx.y + 4 * ty, x0 = 64 * blockIdx.x + 4 * tx;
  Cell q[2][2] = {};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int y = y0 + r, x = x0 + k;
      Cell v{0.0, 0};
      if (y < hin && x < win) {          // children past the ragged edge contribute nothing
        if constexpr (RAW) {
          const size_t p = (size_t)y * win + x;
          const float f = lst[p];
          const bool ok = gap_valid(f, mask, p);
          valid[p] = ok ? 1 : 0;
          if (ok) v = Cell{(double)f, 1};
        } else {
          const unsigned e = py.off[L] + (unsigned)(y * win + x);
          v = Cell{S[e], C[e]};
        }
      }
      q[r >> 1][k >> 1] = q[r >> 1][k >> 1] + v;
    }
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) emit(S, C, py, L + 1, 32 * blockIdx.y + 2 * ty + a, 32 * blockIdx.x + 2 * tx + b, q[a][b]);
  const Cell v2 = (q[0][0] + q[0][1]) + (q[1][0] + q[1][1]);
  l2[ty][tx] = v2;
  emit(S, C, py, L + 2, 16 * blockIdx.y + ty, 16 * blockIdx.x + tx, v2);
  reduce_lds<8>(l2, l3, S, C, py, L + 3);
  reduce_lds<4>(l3, l4, S, C, py, L + 4);
  reduce_lds<2>(l4, l5, S, C, py, L + 5);
  reduce_lds<1>(l5, l6, S, C, py, L + 6);
}

__global__ __launch_bounds__(256) void gaps_fill_kernel(const float* __restrict__ lst, const unsigned char* __restrict__ mask,
                                                        float* __restrict__ filled, const double* __restrict__ S,
                                                        const int* __restrict__ C, const Pyramid py) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)py.h[0] * py.w[0]) return;
  const float f = lst[p];
  float o = f;
  if (!gap_valid(f, mask, p)) {
    const int y = (int)(p / py.w[0]), x = (int)(p - (size_t)y * py.w[0]);
    o = 0.f;                                                   // no valid pixel anywhere
    for (int l = 1; l <= py.top; ++l) {
      const unsigned e = py.off[l] + (unsigned)((y >> l) * py.w[l] + (x >> l));
      const int c = C[e];
      if (c > 0) {
        o = (float)(S[e] / (double)c);
        break;
      }
    }
  }
  filled[p] = o;
}

// ---- select -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gaps_tile_any_kernel(const unsigned char* __restrict__ valid, int* __restrict__ slot,
                                                            const MosaicGeom gm) {
  const int t = blockIdx.x, win = gm.ax.w;
  const int ty = t / gm.ax.count, tx = t - ty * gm.ax.count;
  const unsigned char* v = valid + (size_t)mosaic_origin(gm.ay, ty) * gm.lst_w + mosaic_origin(gm.ax, tx);
  int any = 0;
  for (int e = threadIdx.x; e < win * win; e += 256) {
    const int r = e / win, c = e - r * win;
    any |= v[(size_t)r * gm.lst_w + c] != 0 ? 1 : 0;
  }
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) slot[t] = any ? 1 : 0;
}

// slot[t]: the flag gaps_tile_any_kernel left -> the tile's position among the active ones, or -1
__global__ __launch_bounds__(64) void gaps_order_kernel(int* __restrict__ slot, int* __restrict__ active, int* __restrict__ n_active,
                                                        int T) {
  const int lane = threadIdx.x;
  int running = 0;
  for (int base = 0; base < T; base += 64) {
    const int t = base + lane;
    const bool on = t < T && slot[t] != 0;
    const unsigned long long m = __ballot(on);
    const int pos = running + __popcll(m & ((1ull << lane) - 1ull));
    if (t < T) slot[t] = on ? pos : -1;
    if (on) active[pos] = t;
    running += __popcll(m);
  }
  if (lane == 0) *n_active = running;
}

// ---- compact prepare, masked blend --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gaps_prepare_kernel(const float* __restrict__ filled, const float* __restrict__ ndvi,
                                                           float* __restrict__ x, const int* __restrict__ active,
                                                           const int* __restrict__ n_active, const MosaicGeom gm, int win,
                                                           float mean_lst, float istd_lst, float mean_ndvi, float istd_ndvi,
                                                           int clip_ndvi) {
  __shared__ float src[8][64 + 1];
  const int i = blockIdx.x;
  if (i >= *n_active) return;                                         // (uniform over the workgroup)
  const int t = active[i];
  if (t < 0 || t >= gm.ay.count * gm.ax.count) return;                // never written by sifsrg_tiles_select
  mosaic_prepare_tile(filled, ndvi, x + (size_t)i * 2 * (4 * win) * (4 * win), gm, t, src, win, blockIdx.y * 16, mean_lst,
                      istd_lst, mean_ndvi, istd_ndvi, clip_ndvi);
}

// block = 64 x 4 threads, as mosaic_blend_kernel: the 4 output pixels of a thread belong to ONE LST pixel
__global__ __launch_bounds__(256) void gaps_blend_kernel(const float* __restrict__ sr, const int* __restrict__ slot,
                                                         const unsigned char* __restrict__ valid, float* __restrict__ out,
                                                         const MosaicGeom gm, float R, float mean, float std, float fill_value) {
  const int out_w = 4 * gm.lst_w, out_h = 4 * gm.ay.n;
  const int X = 4 * (blockIdx.x * 64 + threadIdx.x), Y = blockIdx.y * 4 + threadIdx.y;
  if (X >= out_w || Y >= out_h) return;
  float4 o = make_float4(fill_value, fill_value, fill_value, fill_value);
  if (valid[(size_t)(Y >> 2) * gm.lst_w + (X >> 2)] != 0)
    o = mosaic_blend4(sr, gm, R, mean, std, X, Y, [slot](int k) { return slot[k]; });
  st4(out + (size_t)Y * out_w + X, o);
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

}  // namespace

// ---- C ABI (include/sifsr_gaps.h) ----
size_t sifsrg_fill_workspace_bytes(int lst_h, int lst_w) {
  Pyramid py;
  return pyramid_of(lst_h, lst_w, &py) ? pyramid_bytes(py) : 0;
}

int sifsrg_fill(const float* lst, const unsigned char* mask, float* filled, unsigned char* valid, void* workspace,
                size_t workspace_bytes, int lst_h, int lst_w, void* stream) {
  if (!lst || !filled || !valid || !workspace || !aligned(workspace, 8)) return SIFSR_ERR_ARG;
  Pyramid py;
  if (!pyramid_of(lst_h, lst_w, &py)) return SIFSR_ERR_SHAPE;
  if (workspace_bytes < pyramid_bytes(py)) return SIFSR_ERR_WORKSPACE;
  double* S = static_cast<double*>(workspace);
  int* C = reinterpret_cast<int*>(S + py.cells);
  hipStream_t s = (hipStream_t)stream;
  for (int L = 0; L < py.top; L += LEVELS_PER_PASS) {
    const dim3 grid((py.w[L] + 63) / 64, (py.h[L] + 63) / 64);
    if (L == 0)
      hipLaunchKernelGGL(gaps_reduce_kernel<true>, grid, dim3(256), 0, s, lst, mask, valid, S, C, py, L);
    else
      hipLaunchKernelGGL(gaps_reduce_kernel<false>, grid, dim3(256), 0, s, lst, mask, valid, S, C, py, L);
    SIFSR_LAUNCH_CHECK();
  }
  const size_t n = (size_t)lst_h * lst_w;
  hipLaunchKernelGGL(gaps_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lst, mask, filled, S, C, py);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrg_tiles_select(const unsigned char* valid, int* slot, int* active, int* n_active, int lst_h, int lst_w, int win,
                        int overlap, int cover, void* stream) {
  if (!valid || !slot || !active || !n_active) return SIFSR_ERR_ARG;
  MosaicGeom gm;
  if (!mosaic_geom(lst_h, lst_w, win, overlap, cover, &gm)) return SIFSR_ERR_SHAPE;
  const int T = gm.ay.count * gm.ax.count;
  hipLaunchKernelGGL(gaps_tile_any_kernel, dim3(T), dim3(256), 0, (hipStream_t)stream, valid, slot, gm);
  SIFSR_LAUNCH_CHECK();
  hipLaunchKernelGGL(gaps_order_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, slot, active, n_active, T);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrg_tiles_prepare(const float* filled, const float* ndvi, float* x, const int* active, const int* n_active, int cap,
                         int lst_h, int lst_w, int win, int overlap, int cover, float mean_lst, float std_lst, float mean_ndvi,
                         float std_ndvi, int clip_ndvi, void* stream) {
  if (!filled || !ndvi || !x || !active || !n_active) return SIFSR_ERR_ARG;
  MosaicGeom gm;
  if (!mosaic_geom(lst_h, lst_w, win, overlap, cover, &gm) || cap < 1 || std_lst == 0.f || std_ndvi == 0.f) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(gaps_prepare_kernel, dim3(cap, (4 * win) / 16), dim3(256), 0, (hipStream_t)stream, filled, ndvi, x, active,
                     n_active, gm, win, mean_lst, 1.f / std_lst, mean_ndvi, 1.f / std_ndvi, clip_ndvi);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrg_tiles_blend(const float* sr, const int* slot, const unsigned char* valid, float* out, int lst_h, int lst_w, int win,
                       int overlap, int cover, float mean_lst, float std_lst, float fill_value, void* stream) {
  if (!sr || !slot || !valid || !out || !aligned(sr, 16) || !aligned(out, 16)) return SIFSR_ERR_ARG;
  MosaicGeom gm;
  if (!mosaic_geom(lst_h, lst_w, win, overlap, cover, &gm)) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(gaps_blend_kernel, dim3((lst_w + 63) / 64, lst_h), dim3(64, 4), 0, (hipStream_t)stream, sr, slot, valid, out,
                     gm, (float)(4 * overlap), mean_lst, std_lst, fill_value);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}
