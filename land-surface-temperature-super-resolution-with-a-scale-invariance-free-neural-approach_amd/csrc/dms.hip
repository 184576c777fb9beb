// DMS, the Data Mining Sharpener (C ABI and every definition: include/sifsr_dms.h).
//
//  * dms_aggregate_kernel   one thread per coarse cell: four 16-byte loads, the NaN-ignoring mean and population std in float64.
//  * dms_trainset_kernel, dms_weights_kernel   one thread per cell: the feature, its coefficient of variation, the sample weight.
//  * dms_fit_kernel         one workgroup per (image, estimator).  Thread t owns the t-th chunk of the sorted samples: the chunk
//    sums are scanned over the threads in index order, then every thread writes the compacted feature and the prefix sums of its
//    chunk.  The node table (<= 59 nodes) lives in LDS; the arg-max of the split proxy over a node is a strided scan per thread, a
//    wavefront shuffle and an LDS step, the lowest position winning ties.  One wavefront per leaf then does the two-pass ridge sums.
//  * dms_predict_kernel     the image's E leaf tables in LDS, one thread per 4 fine pixels, a block walks 4 coarse rows.
//  * dms_correct_kernel     one thread per row of a cell (the access pattern of conserve_apply_kernel): the 4 x 5 radiance residuals
//    around the cell are formed on the fly, upsampled in float64 and the fourth root taken in the same pass.
// No atomics, no allocation, no host synchronisation.  Products and sums are kept apart (no contraction) so that every stage is
// the float64 arithmetic tests/dms_reference.py writes down.
#include "../../include/sifsr_dms.h"

#include <float.h>
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

#include "dms_dev.h"      // pow4d, tree_value: shared with rbaselines.hip

namespace {

constexpr int MAXL = SIFSRD_MAX_LEAVES;      // 30
constexpr int MAXT = MAXL - 1;               // 29 thresholds
constexpr int MAXN = 2 * MAXL - 1;           // 59 nodes
constexpr int MINLEAF = 10;
constexpr int NT = 256;

__device__ __forceinline__ double dinf() { return __longlong_as_double(0x7FF0000000000000ll); }

__global__ __launch_bounds__(256) void dms_aggregate_kernel(const float* __restrict__ fine, double* __restrict__ mean,
                                                            double* __restrict__ sd, int h, int w, size_t cells, int pow4) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= cells) return;
  const size_t per = (size_t)h * w;
  const size_t b = g / per, r = g - b * per;
  const int i = (int)(r / w), j = (int)(r - (size_t)i * w);
  const float* src = fine + b * per * 16 + (size_t)(4 * i) * (4 * (size_t)w) + 4 * (size_t)j;
  double v[16];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const float4 q = ld4(src + (size_t)a * 4 * w);
    v[4 * a] = q.x; v[4 * a + 1] = q.y; v[4 * a + 2] = q.z; v[4 * a + 3] = q.w;
  }
  double s = 0.0, n = 0.0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (pow4) v[k] = pow4d(v[k]);
    const bool ok = v[k] == v[k];
    s = s + (ok ? v[k] : 0.0);
    n = n + (ok ? 1.0 : 0.0);
  }
  const double m = s / n;
  mean[g] = m;
  if (sd != nullptr) {
    double q = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const double d = (v[k] == v[k]) ? v[k] - m : 0.0;
      q = q + d * d;
    }
    sd[g] = sqrt(q / n);
  }
}

__global__ __launch_bounds__(256) void dms_trainset_kernel(const float* __restrict__ lst, const double* __restrict__ mean,
                                                           const double* __restrict__ sd, double* __restrict__ x,
                                                           double* __restrict__ cv, unsigned char* __restrict__ good, size_t cells) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= cells) return;
  const double m = mean[g];
  const double xv = (m == 0.0) ? 1e-6 : m;
  double c = sd[g] / xv;
  if (c != c) c = 1000.0;
  const float t = lst[g];
  x[g] = xv;
  cv[g] = c;
  good[g] = (isfinite(t) && t > 0.f && isfinite(xv) && c > 0.0 && c < 1000.0) ? 1 : 0;
}

__global__ __launch_bounds__(256) void dms_weights_kernel(const double* __restrict__ cv, const unsigned char* __restrict__ good,
                                                          const double* __restrict__ stats, double* __restrict__ weight, int N,
                                                          size_t cells) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= cells) return;
  const double* st = stats + 3 * (g / (size_t)N);
  double wv = 0.0;
  if (good[g]) {
    const double c = cv[g], wmin = 1.0 / st[2], wmax = 1.0 / st[1];
    wv = (1.0 / c - wmin) / (wmax - wmin);
    if (!(c < st[0])) wv = wv / 2.0;
  }
  weight[g] = wv;
}

// ---- stage 3 ----------------------------------------------------------------------------------------------------------------
struct FitScratch {
  float* xz;            // [N]      the compacted float32 feature
  double *P0, *P1, *P2; // [N + 1]  prefix sums of w c, w c y, w c y^2 over the compacted samples
};

__host__ __device__ inline size_t fit_stride(int N) { return (((size_t)N * 4 + 7) & ~(size_t)7) + 3 * ((size_t)N + 1) * 8; }

struct Nodes {
  int s[MAXN], e[MAXN], pos[MAXN];
  double imp[MAXN], prio[MAXN], il[MAXN], ir[MAXN];
  unsigned char leaf[MAXN], open[MAXN];
};

// the best split of node `id`, by all threads of the workgroup; thread 0 files the result
__device__ void evaluate(Nodes& nd, int id, const FitScratch& S, double Wtot, double* rp, int* rq) {
  const int tid = threadIdx.x;
  const int s = nd.s[id], e = nd.e[id];
  const double imp = nd.imp[id];
  const bool leaf = (e - s < 2 * MINLEAF) || (imp <= DBL_EPSILON);       // uniform
  if (leaf) {
    if (tid == 0) { nd.leaf[id] = 1; nd.prio[id] = 0.0; nd.pos[id] = -1; }
    __syncthreads();
    return;
  }
  const double b0 = S.P0[s], b1 = S.P1[s], e0 = S.P0[e], e1 = S.P1[e];
  double bp = -dinf();
  int bq = -1;
  for (int p = s + MINLEAF + tid; p <= e - MINLEAF; p += NT) {
    const float xa = S.xz[p - 1], xb = S.xz[p];
    if (xb <= xa + 1e-7f) continue;
    const double sl = S.P1[p] - b1, wl = S.P0[p] - b0, sr = e1 - S.P1[p], wr = e0 - S.P0[p];
    const double proxy = sl * sl / wl + sr * sr / wr;
    if (proxy > bp) { bp = proxy; bq = p; }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double op = __shfl_down(bp, o);
    const int oq = __shfl_down(bq, o);
    if (oq >= 0 && (bq < 0 || op > bp || (op == bp && oq < bq))) { bp = op; bq = oq; }
  }
  if ((tid & 63) == 0) { rp[tid >> 6] = bp; rq[tid >> 6] = bq; }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < NT / 64; ++k)
      if (rq[k] >= 0 && (bq < 0 || rp[k] > bp || (rp[k] == bp && rq[k] < bq))) { bp = rp[k]; bq = rq[k]; }
    bool lf = bq < 0;
    if (!lf) {
      const double wn = e0 - b0, wl = S.P0[bq] - b0, wr = e0 - S.P0[bq];
      const double ml = (S.P1[bq] - b1) / wl, mr = (e1 - S.P1[bq]) / wr;
      const double il = (S.P2[bq] - S.P2[s]) / wl - ml * ml, ir = (S.P2[e] - S.P2[bq]) / wr - mr * mr;
      const double prio = wn / Wtot * (imp - wr / wn * ir - wl / wn * il);
      if (!(prio + DBL_EPSILON >= 0.0)) lf = true;
      nd.il[id] = il; nd.ir[id] = ir; nd.prio[id] = prio;
    }
    nd.leaf[id] = lf ? 1 : 0;
    nd.pos[id] = lf ? -1 : bq;
    if (lf) nd.prio[id] = 0.0;
  }
  __syncthreads();
}

__device__ __forceinline__ double split_threshold(const float* xz, int p) {
  const double a = (double)xz[p - 1], b = (double)xz[p];
  const double t = a / 2.0 + b / 2.0;
  return (t == b || isinf(t)) ? a : t;
}

__global__ __launch_bounds__(NT) void dms_fit_kernel(const double* __restrict__ xs, const double* __restrict__ ys,
                                                     const double* __restrict__ ws, const int* __restrict__ cs,
                                                     const int* __restrict__ n_train, char* __restrict__ scratch,
                                                     double* __restrict__ thresholds, int* __restrict__ nleaf,
                                                     double* __restrict__ leaves, int E, int N) {
  __shared__ Nodes nd;
  __shared__ double c0[NT], c1[NT], c2[NT], rp[NT / 64], thr[MAXT];
  __shared__ int ck[NT], rq[NT / 64], lstart[MAXL + 1], fb[MAXL + 1], sh_m, sh_pick, sh_nodes, sh_L;
  const int tid = threadIdx.x, b = blockIdx.y, est = blockIdx.x;
  const size_t be = (size_t)b * E + est;
  int n = n_train[b];
  n = n < 0 ? 0 : (n > N ? N : n);
  const double* x = xs + (size_t)b * N;
  const double* y = ys + (size_t)b * N;
  const double* w = ws + (size_t)b * N;
  const int* c = cs + be * N;
  double* thr_o = thresholds + be * MAXT;
  double* leaf_o = leaves + be * (MAXL * 4);

  if (n == 0) {                                                    // no model: padding only
    if (tid < MAXT) thr_o[tid] = dinf();
    if (tid < MAXL * 4) leaf_o[tid] = 0.0;
    if (tid == 0) nleaf[be] = 0;
    return;
  }

  char* base = scratch + be * fit_stride(N);
  FitScratch S;
  S.xz = reinterpret_cast<float*>(base);
  S.P0 = reinterpret_cast<double*>(base + (((size_t)N * 4 + 7) & ~(size_t)7));
  S.P1 = S.P0 + (N + 1);
  S.P2 = S.P1 + (N + 1);

  // compaction and prefix sums: chunk sums, a scan over the threads in index order, then the chunk again
  const int chunk = (n + NT - 1) / NT;
  const int lo = min(tid * chunk, n), hi = min(lo + chunk, n);
  {
    int k = 0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int i = lo; i < hi; ++i) {
      const double sw = w[i] * (double)c[i];
      if (sw != 0.0) {
        const double yi = y[i];
        ++k; a0 = a0 + sw; a1 = a1 + sw * yi; a2 = a2 + sw * yi * yi;
      }
    }
    ck[tid] = k; c0[tid] = a0; c1[tid] = a1; c2[tid] = a2;
  }
  __syncthreads();
  if (tid == 0) {
    int k = 0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int t = 0; t < NT; ++t) {
      const int kk = ck[t];
      const double t0 = c0[t], t1 = c1[t], t2 = c2[t];
      ck[t] = k; c0[t] = a0; c1[t] = a1; c2[t] = a2;
      k += kk; a0 = a0 + t0; a1 = a1 + t1; a2 = a2 + t2;
    }
    sh_m = k;
    S.P0[0] = 0.0; S.P1[0] = 0.0; S.P2[0] = 0.0;
  }
  __syncthreads();
  {
    int o = ck[tid];
    double a0 = c0[tid], a1 = c1[tid], a2 = c2[tid];
    for (int i = lo; i < hi; ++i) {
      const double sw = w[i] * (double)c[i];
      if (sw != 0.0) {
        const double yi = y[i];
        a0 = a0 + sw; a1 = a1 + sw * yi; a2 = a2 + sw * yi * yi;
        S.xz[o] = (float)x[i];
        ++o;                                                       // o <= (samples before the chunk) + (its own) <= n <= N
        S.P0[o] = a0; S.P1[o] = a1; S.P2[o] = a2;
      }
    }
  }
  __syncthreads();
  const int m = sh_m;
  const double Wtot = S.P0[m];

  // best-first growth
  if (tid == 0) {
    nd.s[0] = 0; nd.e[0] = m;
    const double mu = S.P1[m] / Wtot;
    nd.imp[0] = (m > 0 && Wtot != 0.0) ? S.P2[m] / Wtot - mu * mu : 0.0;
    nd.open[0] = 1;
    sh_nodes = 1;
  }
  __syncthreads();
  evaluate(nd, 0, S, Wtot, rp, rq);
  for (int splits = 0; splits < MAXL - 1; ++splits) {
    if (tid == 0) {
      int pick = -1;
      double best = 0.0;
      for (int k = 0; k < sh_nodes; ++k)
        if (nd.open[k] && !nd.leaf[k] && (pick < 0 || nd.prio[k] > best)) { pick = k; best = nd.prio[k]; }
      sh_pick = pick;
      if (pick >= 0) {
        const int l = sh_nodes, r = sh_nodes + 1;                  // <= 2 * 28 + 2 = 58 < MAXN
        nd.s[l] = nd.s[pick]; nd.e[l] = nd.pos[pick]; nd.imp[l] = nd.il[pick];
        nd.s[r] = nd.pos[pick]; nd.e[r] = nd.e[pick]; nd.imp[r] = nd.ir[pick];
        nd.open[pick] = 0; nd.open[l] = 1; nd.open[r] = 1;
        sh_nodes += 2;
      }
    }
    __syncthreads();
    if (sh_pick < 0) break;                                        // uniform
    const int l = sh_nodes - 2;
    evaluate(nd, l, S, Wtot, rp, rq);
    evaluate(nd, l + 1, S, Wtot, rp, rq);
  }
  __syncthreads();

  // the leaves in ascending order of their interval, the thresholds between them
  if (tid == 0) {
    int L = 0;
    for (int k = 0; k < sh_nodes; ++k) {
      if (!nd.open[k]) continue;
      int q = L++;
      while (q > 0 && lstart[q - 1] > nd.s[k]) { lstart[q] = lstart[q - 1]; --q; }
      lstart[q] = nd.s[k];
    }
    lstart[L] = m;
    sh_L = L;                                                      // 1 <= L <= 30
    for (int k = 1; k < L; ++k) thr[k - 1] = split_threshold(S.xz, lstart[k]);
    nleaf[be] = L;
  }
  __syncthreads();
  const int L = sh_L;
  if (tid < MAXT) thr_o[tid] = tid < L - 1 ? thr[tid] : dinf();
  // where the leaves begin among ALL the n samples: the first one whose float32 feature exceeds the threshold
  if (tid < L - 1) {
    const double t = thr[tid];
    int a = 0, z = n;
    while (a < z) {
      const int mid = (a + z) >> 1;
      if ((double)(float)x[mid] <= t) a = mid + 1; else z = mid;
    }
    fb[tid + 1] = a;
  }
  if (tid == 0) { fb[0] = 0; fb[L] = n; }
  __syncthreads();
  // one wavefront per leaf: the centred two-pass sums of the ridge, the range of y
  const int lane = tid & 63;
  for (int k = tid >> 6; k < MAXL; k += NT / 64) {
    double coef = 0.0, icpt = 0.0, lo_y = 0.0, hi_y = 0.0;
    if (k < L) {
      const int a = fb[k], z = fb[k + 1];
      double sx = 0.0, sy = 0.0, mn = dinf(), mx = -dinf();
      for (int i = a + lane; i < z; i += 64) {
        const double yi = y[i];
        sx = sx + x[i]; sy = sy + yi; mn = fmin(mn, yi); mx = fmax(mx, yi);
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        sx = sx + __shfl_down(sx, o); sy = sy + __shfl_down(sy, o);
        mn = fmin(mn, __shfl_down(mn, o)); mx = fmax(mx, __shfl_down(mx, o));
      }
      const double cnt = (double)(z - a);
      const double xm = __shfl(sx, 0) / cnt, ym = __shfl(sy, 0) / cnt;
      double sxx = 0.0, sxy = 0.0;
      for (int i = a + lane; i < z; i += 64) {
        const double dx = x[i] - xm;
        sxx = sxx + dx * dx; sxy = sxy + dx * (y[i] - ym);
      }
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) { sxx = sxx + __shfl_down(sxx, o); sxy = sxy + __shfl_down(sxy, o); }
      if (z > a) {
        coef = sxy / (sxx + 1.0);
        icpt = ym - coef * xm;
        const double rg = mx - mn;
        lo_y = mn - 0.25 * rg; hi_y = mx + 0.25 * rg;
      }
    }
    if (lane == 0) { leaf_o[4 * k] = coef; leaf_o[4 * k + 1] = icpt; leaf_o[4 * k + 2] = lo_y; leaf_o[4 * k + 3] = hi_y; }
  }
}

// ---- stage 4 ----------------------------------------------------------------------------------------------------------------
constexpr int ROWS = 4;      // coarse rows per workgroup

__global__ __launch_bounds__(256) void dms_predict_kernel(const float* __restrict__ ndvi, const double* __restrict__ thresholds,
                                                          const int* __restrict__ nleaf, const double* __restrict__ leaves,
                                                          float* __restrict__ sr, int E, int h, int w) {
  extern __shared__ double tab[];                                  // thr [E][29], leaves [E][120], nleaf [E]
  double* thr = tab;
  double* lf = tab + (size_t)E * MAXT;
  int* nl = reinterpret_cast<int*>(lf + (size_t)E * MAXL * 4);
  const int tid = threadIdx.y * 64 + threadIdx.x, b = blockIdx.z;
  for (int k = tid; k < E * MAXT; k += 256) thr[k] = thresholds[(size_t)b * E * MAXT + k];
  for (int k = tid; k < E * MAXL * 4; k += 256) lf[k] = leaves[(size_t)b * E * MAXL * 4 + k];
  for (int k = tid; k < E; k += 256) nl[k] = nleaf[(size_t)b * E + k];
  __syncthreads();
  const int J = blockIdx.x * 64 + threadIdx.x;
  if (J >= w) return;
  const bool model = nl[0] > 0;
  const float fnan = __uint_as_float(0x7FC00000u);
  for (int cr = 0; cr < ROWS; ++cr) {
    const int I = blockIdx.y * ROWS + cr;
    if (I >= h) break;
    const size_t p = (size_t)b * 16 * h * w + (size_t)(4 * I + threadIdx.y) * (4 * (size_t)w) + 4 * (size_t)J;
    const float4 q = ld4(ndvi + p);
    const float in[4] = {q.x, q.y, q.z, q.w};
    float o[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool nan = in[u] != in[u];
      const double x = nan ? 0.0 : (double)in[u];
      double acc = 0.0;
      if (model)
        for (int e = 0; e < E; ++e) acc = acc + tree_value(thr + e * MAXT, lf + e * MAXL * 4, nl[e], x);
      o[u] = (nan || !model) ? fnan : (float)(acc / (double)E);
    }
    st4(sr + p, make_float4(o[0], o[1], o[2], o[3]));
  }
}

// ---- stage 5 ----------------------------------------------------------------------------------------------------------------
// cv2 INTER_CUBIC x4 (A = -0.75): the coefficients of t = 0.625, 0.875, 0.125, 0.375 for the output phases 0 .. 3 (exact)
__device__ const double UP4D[4][4] = {{-0.06591796875, 0.42626953125, 0.74951171875, -0.10986328125},
                                      {-0.01025390625, 0.11474609375, 0.96728515625, -0.07177734375},
                                      {-0.07177734375, 0.96728515625, 0.11474609375, -0.01025390625},
                                      {-0.10986328125, 0.74951171875, 0.42626953125, -0.06591796875}};

__device__ __forceinline__ double dot4d(double a, double b, double c, double d, const double* k) {
  return a * k[0] + b * k[1] + c * k[2] + d * k[3];
}

// block = 64 x 4 threads: thread (x, y) owns row y of cell (blockIdx.y, 64 blockIdx.x + x) of image blockIdx.z
__global__ __launch_bounds__(256) void dms_correct_kernel(const float* __restrict__ lst, const float* __restrict__ sr,
                                                          const double* __restrict__ m4, float* __restrict__ out, int h, int w) {
  const int J = blockIdx.x * 64 + threadIdx.x, I = blockIdx.y, py = threadIdx.y;
  if (J >= w) return;
  const size_t cb = (size_t)blockIdx.z * h * w;
  const size_t p = cb * 16 + (size_t)(4 * I + py) * (4 * (size_t)w) + 4 * (size_t)J;
  const float4 s = ld4(sr + p);
  int cj[5];
#pragma unroll
  for (int b = 0; b < 5; ++b) cj[b] = clampi(J - 2 + b, 0, w - 1);
  const int rb = I - 2 + (py >> 1);                    // phases 0, 1 read rows I-2 .. I+1, phases 2, 3 rows I-1 .. I+2
  double hx[4][4];                                     // [source row][output phase]
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const size_t ro = cb + (size_t)clampi(rb + a, 0, h - 1) * w;
    double e[5];
#pragma unroll
    for (int b = 0; b < 5; ++b) e[b] = pow4d((double)lst[ro + cj[b]]) - m4[ro + cj[b]];
    hx[a][0] = dot4d(e[0], e[1], e[2], e[3], UP4D[0]);
    hx[a][1] = dot4d(e[0], e[1], e[2], e[3], UP4D[1]);
    hx[a][2] = dot4d(e[1], e[2], e[3], e[4], UP4D[2]);
    hx[a][3] = dot4d(e[1], e[2], e[3], e[4], UP4D[3]);
  }
  const double* ky = UP4D[py];
  const float in[4] = {s.x, s.y, s.z, s.w};
  float o[4];
#pragma unroll
  for (int u = 0; u < 4; ++u)
    o[u] = (float)sqrt(sqrt(dot4d(hx[0][u], hx[1][u], hx[2][u], hx[3][u], ky) + pow4d((double)in[u])));
  st4(out + p, make_float4(o[0], o[1], o[2], o[3]));
}

bool aligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
bool shape_ok(int B, int h, int w) { return B >= 1 && h >= 1 && w >= 1 && h <= 16384 && w <= 16384 && (size_t)B * h * w <= ((size_t)1 << 31); }
unsigned blocks_of(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

// ---- C ABI (include/sifsr_dms.h) ----
int sifsrd_aggregate(const float* fine, double* mean, double* sd, int B, int h, int w, int pow4, void* stream) {
  if (!fine || !mean || !aligned(fine, 16) || !aligned(mean, 8) || !aligned(sd, 8)) return SIFSR_ERR_ARG;
  if (!shape_ok(B, h, w)) return SIFSR_ERR_SHAPE;
  const size_t cells = (size_t)B * h * w;
  hipLaunchKernelGGL(dms_aggregate_kernel, dim3(blocks_of(cells)), dim3(256), 0, (hipStream_t)stream, fine, mean, sd, h, w, cells,
                     pow4 ? 1 : 0);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrd_trainset(const float* lst, const double* mean, const double* sd, double* x, double* cv, unsigned char* good, int B,
                    int h, int w, void* stream) {
  if (!lst || !mean || !sd || !x || !cv || !good || !aligned(mean, 8) || !aligned(sd, 8) || !aligned(x, 8) || !aligned(cv, 8))
    return SIFSR_ERR_ARG;
  if (!shape_ok(B, h, w)) return SIFSR_ERR_SHAPE;
  const size_t cells = (size_t)B * h * w;
  hipLaunchKernelGGL(dms_trainset_kernel, dim3(blocks_of(cells)), dim3(256), 0, (hipStream_t)stream, lst, mean, sd, x, cv, good,
                     cells);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrd_weights(const double* cv, const unsigned char* good, const double* stats, double* weight, int B, int N, void* stream) {
  if (!cv || !good || !stats || !weight || !aligned(cv, 8) || !aligned(stats, 8) || !aligned(weight, 8)) return SIFSR_ERR_ARG;
  if (B < 1 || N < 1 || (size_t)B * N > ((size_t)1 << 31)) return SIFSR_ERR_SHAPE;
  const size_t cells = (size_t)B * N;
  hipLaunchKernelGGL(dms_weights_kernel, dim3(blocks_of(cells)), dim3(256), 0, (hipStream_t)stream, cv, good, stats, weight, N,
                     cells);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

size_t sifsrd_fit_scratch_bytes(int B, int E, int N) {
  if (B < 1 || E < 1 || E > SIFSRD_MAX_ESTIMATORS || N < 1 || B > 65535 || (size_t)N > ((size_t)1 << 28)) return 0;
  return (size_t)B * E * fit_stride(N);
}

int sifsrd_fit(const double* xs, const double* ys, const double* ws, const int* cs, const int* n_train, void* scratch,
               double* thresholds, int* nleaf, double* leaves, int B, int E, int N, void* stream) {
  if (!xs || !ys || !ws || !cs || !n_train || !scratch || !thresholds || !nleaf || !leaves) return SIFSR_ERR_ARG;
  if (!aligned(xs, 8) || !aligned(ys, 8) || !aligned(ws, 8) || !aligned(cs, 4) || !aligned(n_train, 4) || !aligned(scratch, 8) ||
      !aligned(thresholds, 8) || !aligned(nleaf, 4) || !aligned(leaves, 8))
    return SIFSR_ERR_ARG;
  if (sifsrd_fit_scratch_bytes(B, E, N) == 0) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(dms_fit_kernel, dim3(E, B), dim3(NT), 0, (hipStream_t)stream, xs, ys, ws, cs, n_train,
                     static_cast<char*>(scratch), thresholds, nleaf, leaves, E, N);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrd_predict(const float* ndvi_f, const double* thresholds, const int* nleaf, const double* leaves, float* sr, int B, int E,
                   int h, int w, void* stream) {
  if (!ndvi_f || !thresholds || !nleaf || !leaves || !sr || !aligned(ndvi_f, 16) || !aligned(sr, 16) || !aligned(thresholds, 8) ||
      !aligned(leaves, 8) || !aligned(nleaf, 4))
    return SIFSR_ERR_ARG;
  if (!shape_ok(B, h, w) || B > 65535 || E < 1 || E > SIFSRD_MAX_ESTIMATORS) return SIFSR_ERR_SHAPE;
  const size_t lds = (size_t)E * (MAXT + MAXL * 4) * sizeof(double) + (size_t)E * sizeof(int);
  hipLaunchKernelGGL(dms_predict_kernel, dim3((w + 63) / 64, (h + ROWS - 1) / ROWS, B), dim3(64, 4), lds, (hipStream_t)stream, ndvi_f,
                     thresholds, nleaf, leaves, sr, E, h, w);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}

int sifsrd_correct(const float* lst, const float* sr, const double* m4, float* out, int B, int h, int w, void* stream) {
  if (!lst || !sr || !m4 || !out || !aligned(sr, 16) || !aligned(out, 16) || !aligned(m4, 8)) return SIFSR_ERR_ARG;
  if (!shape_ok(B, h, w) || B > 65535 || h > 65535) return SIFSR_ERR_SHAPE;
  hipLaunchKernelGGL(dms_correct_kernel, dim3((w + 63) / 64, h, B), dim3(64, 4), 0, (hipStream_t)stream, lst, sr, m4, out, h, w);
  SIFSR_LAUNCH_CHECK();
  return SIFSR_OK;
}
