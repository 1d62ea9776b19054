// Polynomial trend with marginalised coefficients: the trend's share of the streamed statistics and its query rows.
//
//   k_scatter_trend   C[m][p] += sum_i wa_i w(x_i) h(x_i)^T,   G[p][p] += sum_i wa_i h_i h_i^T (upper triangle),   g[p] += sum_i wby_i h_i
//   k_trend_rows      R*[n][p] = h(x*) - sum_t w_t(x*) S[idx_t][:]   (and, optionally, H*[n][p] = h(x*))
//
// h(x) holds the monomials of total degree <= deg in t_k = (x_k - c_k) / s_k, graded lexicographic: 1, t_1 .. t_d, t_1^2, t_1 t_2, ...
//
// Shape of the scatter.  p <= 15, so a point has T p = 4^d p increments for C -- 4 (d = 1, constant) to 3840 (d = 4, quadratic) --
// far fewer than a probe point's T S, and a workgroup per point would leave most of its lanes without work.  A workgroup therefore
// takes TREND_PTS points at a time: their per-dim stencils, bases and weights are staged in LDS in fp64, then the lanes run over
// (point, tap, j) with j fastest.  C is trend-minor, so consecutive lanes of a point cover the p reals of a tap and then the next tap of
// the innermost dim, whose node is the next one: runs of 4 p contiguous reals per (point, outer taps), the longest runs this layout has
// (240 B in fp32 for the quadratic trend in d >= 2; a constant trend in d = 1 has 16-B runs and 4 atomics per point: nothing to shape).
// G and g are the sums of p (p + 1) / 2 + p <= 135 products per point: thread e owns entry e, adds the staged points' products from
// LDS in fp64 in point order and keeps its sum in a register across the workgroup's batches; one set of fp64 atomics per workgroup
// at the end.  The grid is capped (TREND_MAX_BLOCKS workgroups, batch-strided) so that at most that many sets meet on G's addresses.
//
// No fused multiply-adds in this file: as for the probes (sample_paths.hip), every increment is DEFINED by its IEEE fp64 operation
// sequence (include/wiski.h), so that a host reference reproduces it, and the cubic's weights near their zeros are differences of
// O(1) intermediates.
#pragma clang fp contract(off)
#include "wiski_common.h"

namespace {

constexpr int TREND_THREADS = 256;
constexpr int TREND_PTS = 16;            // points staged per workgroup batch
constexpr int TREND_MAX_BLOCKS = 1024;

__host__ __device__ constexpr int trend_p(int d, int deg) { return deg == 0 ? 1 : (deg == 1 ? d + 1 : (d + 1) * (d + 2) / 2); }

// the basis of one point, from its raw coordinates (the working type, widened)
template <typename real, int D, int DEG>
__device__ __forceinline__ void trend_basis(const real* __restrict__ xp, const double* __restrict__ center, const double* __restrict__ scale, double* h) {
  h[0] = 1.0;
  if constexpr (DEG >= 1) {
    double t[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      t[k] = ((double)xp[k] - center[k]) / scale[k];
      h[1 + k] = t[k];
    }
    if constexpr (DEG >= 2) {
      int c = 1 + D;
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = a; b < D; ++b) h[c++] = t[a] * t[b];
    }
  }
}

// Stage the per-dim stencils of the points [p0, p0 + cnt) in LDS: thread (point, dim).  The inside / outside verdict is the absorb's, taken
// in the working precision against the grid as GridDev<real> rounds it (sample_paths.hip); the weights are taken in fp64, a point the
// verdict accepts within an ulp outside the fp64 grid moved onto the edge.  s_ok must have been set to 1 (and synchronised) before.
template <typename real, int D>
__device__ __forceinline__ void stage_stencils(const GridDev<double>& G, const GridDev<real>& Gr, const real* __restrict__ x, int64_t p0, int cnt,
                                               double (*s_w)[D][4], int (*s_j0)[D], int* s_ok) {
  const int tid = threadIdx.x;
  if (tid < cnt * D) {
    const int pt = tid / D, q = tid - pt * D;
    double w[4];
    const real xr = x[(p0 + pt) * D + q];
    const bool inside = xr >= Gr.g0[q] && xr <= Gr.hi[q];
    double xd = (double)xr;
    xd = xd < G.g0[q] ? G.g0[q] : (xd > G.hi[q] ? G.hi[q] : xd);
    const int j = dim_stencil<double>(xd, G.g0[q], G.h[q], G.hi[q], G.g[q], w);
    if (!inside || j < 0) s_ok[pt] = 0;              // (several dims of a point may write the same 0)
    s_j0[pt][q] = j < 0 ? 0 : j;
#pragma unroll
    for (int c = 0; c < 4; ++c) s_w[pt][q][c] = w[c];
  }
}

template <int D>
__device__ __forceinline__ void tap_of(const GridDev<double>& G, const double (*s_w)[4], const int* s_j0, int t, double* w_out, int* idx_out) {
  double w = 1.0;
  int idx = 0;
#pragma unroll
  for (int q = 0; q < D; ++q) {
    const int c = (t >> (2 * (D - 1 - q))) & 3;
    w *= s_w[q][c];
    idx += (s_j0[q] + c) * G.stride[q];
  }
  *w_out = w;
  *idx_out = idx;
}

template <typename real, int D, int DEG>
__global__ __launch_bounds__(TREND_THREADS) void k_scatter_trend(GridDev<double> G, GridDev<real> Gr, const real* __restrict__ x, const real* __restrict__ wa,
                                                                 const real* __restrict__ wby, int64_t n, const double* __restrict__ center,
                                                                 const double* __restrict__ scale, real* __restrict__ C, double* __restrict__ Gm,
                                                                 double* __restrict__ gv, int32_t* __restrict__ err) {
  constexpr int T = 1 << (2 * D);
  constexpr int P = trend_p(D, DEG);
  constexpr int NPAIR = P * (P + 1) / 2;
  static_assert(NPAIR + P <= TREND_THREADS && TREND_PTS * WISKI_MAX_DIM <= TREND_THREADS, "one thread per entry of G and g, one per (point, dim)");
  __shared__ double s_w[TREND_PTS][D][4];
  __shared__ int s_j0[TREND_PTS][D];
  __shared__ int s_ok[TREND_PTS];
  __shared__ double s_h[TREND_PTS][P];
  __shared__ double s_wa[TREND_PTS];
  __shared__ double s_wby[TREND_PTS];
  const int tid = threadIdx.x;
  // the entry of G (a <= b, row-major upper triangle) or of g this thread owns
  int ea = -1, eb = -1;
  if (tid < NPAIR) {
    int e = tid, a = 0;
    while (e >= P - a) { e -= P - a; ++a; }
    ea = a;
    eb = a + e;
  } else if (tid < NPAIR + P) {
    ea = tid - NPAIR;
  }
  double acc = 0.0;
  const int64_t nbatch = (n + TREND_PTS - 1) / TREND_PTS;
  for (int64_t bt = blockIdx.x; bt < nbatch; bt += gridDim.x) {
    const int64_t p0 = bt * TREND_PTS;
    const int cnt = (int)(n - p0 < TREND_PTS ? n - p0 : TREND_PTS);
    if (tid < TREND_PTS) s_ok[tid] = 1;
    __syncthreads();
    stage_stencils<real, D>(G, Gr, x, p0, cnt, s_w, s_j0, s_ok);
    if (tid >= TREND_THREADS - cnt) {                // (the other end of the workgroup: the stencil threads are busy)
      const int pt = TREND_THREADS - 1 - tid;
      double h[P];
      trend_basis<real, D, DEG>(x + (p0 + pt) * D, center, scale, h);
#pragma unroll
      for (int j = 0; j < P; ++j) s_h[pt][j] = h[j];
      s_wa[pt] = wa ? (double)wa[p0 + pt] : 1.0;
      s_wby[pt] = (double)wby[p0 + pt];
    }
    __syncthreads();
    if (tid < cnt && !s_ok[tid]) atomicOr(err, 1);   // outside the grid: the point contributes nothing anywhere (the absorb counts it)
    // C: lanes over (point, tap, j), j fastest
    const int total = cnt * T * P;
    for (int e = tid; e < total; e += TREND_THREADS) {
      const int pt = e / (T * P), r = e - pt * (T * P);
      const int t = r / P, j = r - t * P;
      if (!s_ok[pt]) continue;
      double w;
      int idx;
      tap_of<D>(G, s_w[pt], s_j0[pt], t, &w, &idx);
      if (w != 0.0) atomic_add_real(C + (int64_t)idx * P + j, (real)((s_wa[pt] * w) * s_h[pt][j]));
    }
    // G, g: this thread's entry over the staged points, in point order
    if (ea >= 0) {
      for (int pt = 0; pt < cnt; ++pt) {
        if (!s_ok[pt]) continue;
        acc += eb >= 0 ? (s_wa[pt] * s_h[pt][ea]) * s_h[pt][eb] : s_wby[pt] * s_h[pt][ea];
      }
    }
    __syncthreads();
  }
  if (ea >= 0 && acc != 0.0) {
    if (eb >= 0) unsafeAtomicAdd(Gm + ea * P + eb, acc);
    else unsafeAtomicAdd(gv + ea, acc);
  }
}

template <typename real, int D, int DEG>
__global__ __launch_bounds__(TREND_THREADS) void k_trend_rows(GridDev<double> G, GridDev<real> Gr, const real* __restrict__ x, int64_t n,
                                                              const double* __restrict__ center, const double* __restrict__ scale,
                                                              const real* __restrict__ S, real* __restrict__ R, real* __restrict__ H,
                                                              int32_t* __restrict__ err) {
  constexpr int T = 1 << (2 * D);
  constexpr int P = trend_p(D, DEG);
  static_assert(TREND_PTS * P <= TREND_THREADS, "one thread per (point, j)");
  __shared__ double s_w[TREND_PTS][D][4];
  __shared__ int s_j0[TREND_PTS][D];
  __shared__ int s_ok[TREND_PTS];
  __shared__ double s_h[TREND_PTS][P];
  const int tid = threadIdx.x;
  const int64_t nbatch = (n + TREND_PTS - 1) / TREND_PTS;
  for (int64_t bt = blockIdx.x; bt < nbatch; bt += gridDim.x) {
    const int64_t p0 = bt * TREND_PTS;
    const int cnt = (int)(n - p0 < TREND_PTS ? n - p0 : TREND_PTS);
    if (tid < TREND_PTS) s_ok[tid] = 1;
    __syncthreads();
    stage_stencils<real, D>(G, Gr, x, p0, cnt, s_w, s_j0, s_ok);
    if (tid >= TREND_THREADS - cnt) {
      const int pt = TREND_THREADS - 1 - tid;
      double h[P];
      trend_basis<real, D, DEG>(x + (p0 + pt) * D, center, scale, h);
#pragma unroll
      for (int j = 0; j < P; ++j) s_h[pt][j] = h[j];
    }
    __syncthreads();
    if (tid < cnt && !s_ok[tid]) atomicOr(err, 1);   // outside the grid: the row is h(x*)
    if (tid < cnt * P) {
      const int pt = tid / P, j = tid - pt * P;
      const double h = s_h[pt][j];
      double acc = 0.0;
      if (S && s_ok[pt]) {
        for (int t = 0; t < T; ++t) {
          double w;
          int idx;
          tap_of<D>(G, s_w[pt], s_j0[pt], t, &w, &idx);
          if (w != 0.0) acc += w * (double)S[(int64_t)idx * P + j];
        }
      }
      R[(p0 + pt) * P + j] = (real)(h - acc);
      if (H) H[(p0 + pt) * P + j] = (real)h;
    }
    __syncthreads();
  }
}

template <typename real>
int trend_grids(const wiski_grid* grid, GridDev<double>* G, GridDev<real>* Gr) {
  int rc = make_grid_dev<double>(grid, G);
  if (rc != WISKI_OK) return rc;
  return make_grid_dev<real>(grid, Gr);
}

#define TREND_DISPATCH_DEG(deg, DD, CALL) \
  switch (deg) {                          \
    case 0: { CALL(DD, 0); break; }       \
    case 1: { CALL(DD, 1); break; }       \
    default: { CALL(DD, 2); break; }      \
  }

template <typename real>
int scatter_trend_impl(const wiski_grid* grid, const real* d_x, const real* d_wa, const real* d_wby, int64_t n, int32_t deg, const double* d_center,
                       const double* d_scale, real* d_C, double* d_G, double* d_g, int32_t* d_err, void* stream) {
  GridDev<double> G;
  GridDev<real> Gr;
  const int rc = trend_grids<real>(grid, &G, &Gr);
  if (rc != WISKI_OK) return rc;
  if (deg < 0 || deg > 2 || n < 0 || !d_center || !d_scale || !d_C || !d_G || !d_g || !d_err) return WISKI_E_BADARG;
  if (n == 0) return WISKI_OK;                       // (an empty batch has no points and no weights to point at)
  if (!d_x || !d_wby) return WISKI_E_BADARG;
  const int64_t nbatch = (n + TREND_PTS - 1) / TREND_PTS;
  const unsigned blocks = (unsigned)(nbatch < TREND_MAX_BLOCKS ? nbatch : TREND_MAX_BLOCKS);
#define CALL2(DD, DG) \
  hipLaunchKernelGGL((k_scatter_trend<real, DD, DG>), dim3(blocks), dim3(TREND_THREADS), 0, (hipStream_t)stream, G, Gr, d_x, d_wa, d_wby, n, d_center, d_scale, d_C, d_G, d_g, d_err)
#define CALL(DD) TREND_DISPATCH_DEG(deg, DD, CALL2)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
#undef CALL2
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

template <typename real>
int trend_rows_impl(const wiski_grid* grid, const real* d_x, int64_t n, int32_t deg, const double* d_center, const double* d_scale, const real* d_S,
                    real* d_R, real* d_H, int32_t* d_err, void* stream) {
  GridDev<double> G;
  GridDev<real> Gr;
  const int rc = trend_grids<real>(grid, &G, &Gr);
  if (rc != WISKI_OK) return rc;
  if (deg < 0 || deg > 2 || n < 0 || !d_center || !d_scale || !d_err) return WISKI_E_BADARG;
  if (n == 0) return WISKI_OK;                       // (no points, no rows)
  if (!d_x || !d_R) return WISKI_E_BADARG;
  const int64_t nbatch = (n + TREND_PTS - 1) / TREND_PTS;
  const unsigned blocks = (unsigned)(nbatch < (int64_t)1 << 20 ? nbatch : (int64_t)1 << 20);
#define CALL2(DD, DG) \
  hipLaunchKernelGGL((k_trend_rows<real, DD, DG>), dim3(blocks), dim3(TREND_THREADS), 0, (hipStream_t)stream, G, Gr, d_x, n, d_center, d_scale, d_S, d_R, d_H, d_err)
#define CALL(DD) TREND_DISPATCH_DEG(deg, DD, CALL2)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
#undef CALL2
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

}  // namespace

extern "C" {
int wiski_scatter_trend_f32(const wiski_grid* grid, const float* d_x, const float* d_wa, const float* d_wby, int64_t n, int32_t deg, const double* d_center,
                            const double* d_scale, float* d_C, double* d_G, double* d_g, int32_t* d_err, void* stream) {
  return scatter_trend_impl<float>(grid, d_x, d_wa, d_wby, n, deg, d_center, d_scale, d_C, d_G, d_g, d_err, stream);
}
int wiski_scatter_trend_f64(const wiski_grid* grid, const double* d_x, const double* d_wa, const double* d_wby, int64_t n, int32_t deg, const double* d_center,
                            const double* d_scale, double* d_C, double* d_G, double* d_g, int32_t* d_err, void* stream) {
  return scatter_trend_impl<double>(grid, d_x, d_wa, d_wby, n, deg, d_center, d_scale, d_C, d_G, d_g, d_err, stream);
}
int wiski_trend_rows_f32(const wiski_grid* grid, const float* d_x, int64_t n, int32_t deg, const double* d_center, const double* d_scale, const float* d_S,
                         float* d_R, float* d_H, int32_t* d_err, void* stream) {
  return trend_rows_impl<float>(grid, d_x, n, deg, d_center, d_scale, d_S, d_R, d_H, d_err, stream);
}
int wiski_trend_rows_f64(const wiski_grid* grid, const double* d_x, int64_t n, int32_t deg, const double* d_center, const double* d_scale, const double* d_S,
                         double* d_R, double* d_H, int32_t* d_err, void* stream) {
  return trend_rows_impl<double>(grid, d_x, n, deg, d_center, d_scale, d_S, d_R, d_H, d_err, stream);
}
}
