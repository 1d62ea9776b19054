// Jet rows J(x) = [w(x); d_1 w(x); ...; d_D w(x)] (C = D + 1 channels) and the three kernels on them:
//   k_jet_quadform     out[p][c][c'] = J_c(x_p)^T M J_c'(x_p) from the 4^D x 4^D sub-block of a dense M (dense regime),
//   k_wt_columns_jet   the C rows of a point as dense m-columns (right-hand sides of the matrix-free solves),
//   k_gather_jet       out[p][j][c] = J_c(x_p) . V[row(p, j)]: value and gradient gather in one pass.
// Included from interp_gather.hip.  Channel order and boundary convention are those of k_gather_grad: channel 1 + q has dim q's
// four weights replaced by k'(s) / h_q, identically zero where dim q's cell is a one-hot boundary cell; a point outside the grid has
// all C rows zero and raises bit 0 of err.
#pragma once
#include "wiski_common.h"

// The cubic and its derivative in the operation order of their definition ((t + 1) - c, Horner), every operation rounded on its
// own: no fused multiply-add.  The quadratic form and the gather accumulate in fp64, so with these weights their fp64 error is
// that of the accumulation alone -- a contracted evaluation moves an outer tap next to a node (k(1) = k(2) = 0 by cancellation
// of terms of size 2 .. 24) by a few eps of the TERMS, which a table with entries of very different magnitude multiplies up.
template <typename real>
__device__ __forceinline__ real jet_keys(real s) {
#pragma clang fp contract(off)
  const real a = s < (real)0 ? -s : s;
  const real near = (((real)1.5 * a - (real)2.5) * a) * a + (real)1;
  const real far = (((real)-0.5 * a + (real)2.5) * a - (real)4) * a + (real)2;
  return a <= (real)1 ? near : (a < (real)2 ? far : (real)0);
}
template <typename real>
__device__ __forceinline__ real jet_keys_deriv(real s) {
#pragma clang fp contract(off)
  const real a = s < (real)0 ? -s : s;
  const real sg = s < (real)0 ? (real)-1 : (real)1;
  const real near = ((real)4.5 * a - (real)5) * a;
  const real far = ((real)-1.5 * a + (real)5) * a - (real)4;
  return a <= (real)1 ? sg * near : (a < (real)2 ? sg * far : (real)0);
}

// Tap c of one coordinate: lowest tap index *j0 (0 outside the grid), value weight *w and derivative weight *dw.
// Returns false for a coordinate outside the grid (both weights zero).
template <typename real>
__device__ __forceinline__ bool jet_dim_tap(real x, real g0, real h, real hi, int g, int c, int* j0, real* w, real* dw) {
#pragma clang fp contract(off)
  *j0 = 0;
  *w = (real)0;
  *dw = (real)0;
  if (!(x >= g0 && x <= hi)) return false;
  const real u = (x - g0) / h;
  const real fl = floor(u);
  const real t = u - fl;
  const int j = (int)fl - 1;
  if (j < 0 || j > g - 4) {                       // one-hot boundary cell: weight 1 on the nearest of the first / last four nodes
    const int base = j < 0 ? 0 : g - 4;
    int best = 0;
    real bd = (real)3.0e38;
    for (int cc = 0; cc < 4; ++cc) {
      real dd = g0 + h * (real)(base + cc) - x;
      dd = dd < (real)0 ? -dd : dd;
      if (dd < bd) { bd = dd; best = cc; }
    }
    *j0 = base;
    *w = c == best ? (real)1 : (real)0;
    return true;
  }
  const real s = (t + (real)1) - (real)c;
  *j0 = j;
  *w = jet_keys<real>(s);
  *dw = jet_keys_deriv<real>(s) / h;
  return true;
}

// Tap a of point xp: flat grid index and the C = D + 1 channel weights val[0..D] (val[0] the value weight).  The four taps of
// the last dim are consecutive grid indices, always (a boundary cell keeps its four nodes, with a one-hot weight).
template <typename real, int D>
__device__ __forceinline__ bool jet_tap(const GridDev<real>& G, const real* __restrict__ xp, int a, int* flat, real val[D + 1]) {
  real wv[D], dv[D];
  bool ok = true;
  int f = 0;
#pragma unroll
  for (int q = 0; q < D; ++q) {
    int j0;
    ok = jet_dim_tap<real>(xp[q], G.g0[q], G.h[q], G.hi[q], G.g[q], (a >> (2 * (D - 1 - q))) & 3, &j0, &wv[q], &dv[q]) && ok;
    f += (j0 + ((a >> (2 * (D - 1 - q))) & 3)) * G.stride[q];
  }
  real v = wv[0];
#pragma unroll
  for (int q = 1; q < D; ++q) v *= wv[q];
  val[0] = ok ? v : (real)0;
#pragma unroll
  for (int q = 0; q < D; ++q) {
    real t = q == 0 ? dv[0] : wv[0];
#pragma unroll
    for (int o = 1; o < D; ++o) t *= (o == q ? dv[o] : wv[o]);
    val[1 + q] = ok ? t : (real)0;
  }
  *flat = f;
  return ok;
}

template <typename real>
struct JetVec4 {
  typedef real type __attribute__((ext_vector_type(4), aligned(sizeof(real))));
};

// ------------------------------------------------------------------------------------------------------ quadratic forms
// One point per block: one wave at D <= 3 (4 / 16 / 64 of its lanes own a tap), four waves at D = 4 (256 taps).  The tap table is
// channel-minor in LDS, as k_scatter_stats_grad keeps it.  Phase 1: the lane of tap a forms t_c[a] = sum_b M[idx_a][idx_b] J_c[b]
// for the C channels, reading row idx_a of M four consecutive entries (the last dim's taps) per load.  Phase 2: out[c][c'] =
// sum_a J_c[a] t_c'[a] by a wave reduction, upper triangle only; both triangles are written from it.  fp64 accumulators.
template <typename real, int D>
__global__ __launch_bounds__(D == 4 ? 256 : 64) void k_jet_quadform(GridDev<real> G, const real* __restrict__ x, int64_t n,
                                                                   const real* __restrict__ M, int64_t ldm, real* __restrict__ out,
                                                                   int32_t* __restrict__ err) {
  constexpr int T = 1 << (2 * D), C = D + 1, NW = D == 4 ? 4 : 1, NP = C * (C + 1) / 2;
  __shared__ int s_idx[T];
  __shared__ real s_val[T][C];
  __shared__ double s_red[NW][NP];
  const int64_t p = blockIdx.x;
  const int a = threadIdx.x;
  real xp[D];
#pragma unroll
  for (int q = 0; q < D; ++q) xp[q] = x[p * D + q];
  real mine[C];
  int flat = 0;
#pragma unroll
  for (int c = 0; c < C; ++c) mine[c] = (real)0;
  if (a < T) {
    const bool ok = jet_tap<real, D>(G, xp, a, &flat, mine);
    s_idx[a] = flat;
#pragma unroll
    for (int c = 0; c < C; ++c) s_val[a][c] = mine[c];
    if (!ok && a == 0) atomicOr(err, 1);
  }
  __syncthreads();
  double t[C];
#pragma unroll
  for (int c = 0; c < C; ++c) t[c] = 0.0;
  if (a < T) {
    const real* __restrict__ row = M + (int64_t)flat * ldm;
#pragma unroll 4
    for (int b = 0; b < T; b += 4) {
      const typename JetVec4<real>::type r = *reinterpret_cast<const typename JetVec4<real>::type*>(row + s_idx[b]);
#pragma unroll
      for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int c = 0; c < C; ++c) t[c] += (double)r[k] * (double)s_val[b + k][c];
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  int e = 0;
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int c2 = c; c2 < C; ++c2) {
      const double s = wave_reduce_sum<double>((double)mine[c] * t[c2]);
      if (lane == 0) s_red[wid][e] = s;
      ++e;
    }
  __syncthreads();
  if (threadIdx.x < C * C) {
    const int c = threadIdx.x / C, c2 = threadIdx.x % C;
    const int lo = c < c2 ? c : c2, hi = c < c2 ? c2 : c;
    const int pe = lo * C - lo * (lo - 1) / 2 + (hi - lo);
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < NW; ++w) s += s_red[w][pe];
    out[p * (C * C) + threadIdx.x] = (real)s;
  }
}

template <typename real>
static int jet_quadform_impl(const wiski_grid* grid, const real* d_x, int64_t n, const real* d_M, int64_t ldm, real* d_out, int32_t* d_err,
                             void* stream) {
  GridDev<real> G;
  int rc = make_grid_dev<real>(grid, &G);
  if (rc) return rc;
  if (n < 0 || ldm < G.m) return WISKI_E_BADARG;
  if (n == 0) return WISKI_OK;
  if (!d_x || !d_M || !d_out || !d_err) return WISKI_E_BADARG;
  dim3 grd((unsigned)n);
#define CALL(DD) hipLaunchKernelGGL((k_jet_quadform<real, DD>), grd, dim3(DD == 4 ? 256 : 64), 0, (hipStream_t)stream, G, d_x, n, d_M, ldm, d_out, d_err)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

// ----------------------------------------------------------------------------------------------------- W^T jet columns
// out[(p C + c)][idx_a] = J_c(x_p)[a]: one thread per (point, tap), C plain stores (the taps of one row are distinct; the caller
// zeroes the buffer).  The value weights are dim_stencil's, multiplied in k_wt_columns' order: row p C is bit for bit the
// column wiski_wt_columns writes; the derivative weights are k_gather_grad's.
template <typename real, int D>
__global__ __launch_bounds__(256) void k_wt_columns_jet(GridDev<real> G, const real* __restrict__ x, int64_t n, real* __restrict__ out,
                                                        int32_t* __restrict__ err) {
  constexpr int T = 1 << (2 * D), C = D + 1;
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n * T) return;
  const int64_t p = e / T;
  const int a = (int)(e - p * T);
  int flat = 0;
  real v = (real)1, wv[D], dv[D];
  bool ok = true;
#pragma unroll
  for (int q = 0; q < D; ++q) {
    real w[4];
    const real xv = x[p * D + q];
    int j0 = dim_stencil<real>(xv, G.g0[q], G.h[q], G.hi[q], G.g[q], w);
    const int c = (a >> (2 * (D - 1 - q))) & 3;
    const real u = (xv - G.g0[q]) / G.h[q];
    const real fl = floor(u);
    const int jj = (int)fl - 1;
    const bool interior = j0 >= 0 && !(jj < 0 || jj > G.g[q] - 4);
    if (j0 < 0) { ok = false; j0 = 0; w[c] = (real)0; }
    flat += (j0 + c) * G.stride[q];
    v *= w[c];
    wv[q] = w[c];
    dv[q] = interior ? keys_cubic_deriv<real>(u - fl + (real)1 - (real)c) / G.h[q] : (real)0;
  }
  real* __restrict__ o = out + (p * C) * (int64_t)G.m + flat;
  o[0] = v;
#pragma unroll
  for (int q = 0; q < D; ++q) {
    real t = dv[q];
#pragma unroll
    for (int r = 0; r < D; ++r)
      if (r != q) t *= wv[r];
    o[(int64_t)(1 + q) * G.m] = ok ? t : (real)0;
  }
  if (!ok && a == 0) atomicOr(err, 1);
}

template <typename real>
static int wt_columns_jet_impl(const wiski_grid* grid, const real* d_x, int64_t n, real* d_out, int32_t* d_err, void* stream) {
  GridDev<real> G;
  int rc = make_grid_dev<real>(grid, &G);
  if (rc) return rc;
  if (n < 0) return WISKI_E_BADARG;
  if (n == 0) return WISKI_OK;
  if (!d_x || !d_out || !d_err) return WISKI_E_BADARG;
  const int64_t total = n * G.T;
  dim3 grd((unsigned)((total + 255) / 256));
#define CALL(DD) hipLaunchKernelGGL((k_wt_columns_jet<real, DD>), grd, dim3(256), 0, (hipStream_t)stream, G, d_x, n, d_out, d_err)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

// ---------------------------------------------------------------------------------------------------------- jet gather
// One point per block of four waves; the tap table is built once and serves every row and channel.  A row is read by L = 4^D / 4
// lanes, four consecutive entries (the last dim's taps) per lane in one load, so a wave works on 64 / L rows at a time; the C
// fp64 channel sums meet by xor shuffles inside the L-lane group.  rows_per_point = 0: the k rows of V are shared by all points;
// B >= 1: point p reads rows p B .. p B + B - 1.
template <typename real, int D>
__global__ __launch_bounds__(256) void k_gather_jet(GridDev<real> G, const real* __restrict__ x, int64_t n, const real* __restrict__ V, int k,
                                                    int per_point, real* __restrict__ out, int32_t* __restrict__ err) {
  constexpr int T = 1 << (2 * D), C = D + 1, L = T / 4, RPW = 64 / L, RPB = 4 * RPW;
  __shared__ int s_idx[T];
  __shared__ real s_val[T][C];
  const int64_t p = blockIdx.x;
  if (threadIdx.x < T) {
    real xp[D], val[C];
#pragma unroll
    for (int q = 0; q < D; ++q) xp[q] = x[p * D + q];
    int flat;
    const bool ok = jet_tap<real, D>(G, xp, threadIdx.x, &flat, val);
    s_idx[threadIdx.x] = flat;
#pragma unroll
    for (int c = 0; c < C; ++c) s_val[threadIdx.x][c] = val[c];
    if (!ok && threadIdx.x == 0) atomicOr(err, 1);
  }
  __syncthreads();
  const int sub = threadIdx.x % L, rloc = threadIdx.x / L;
  const int base = s_idx[4 * sub];
  real w[4][C];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < C; ++c) w[i][c] = s_val[4 * sub + i][c];
  const real* __restrict__ Vp = V + (per_point ? p * (int64_t)k * G.m : (int64_t)0);
  for (int j0 = 0; j0 < k; j0 += RPB) {
    const int j = j0 + rloc;
    const bool live = j < k;
    const typename JetVec4<real>::type r = *reinterpret_cast<const typename JetVec4<real>::type*>(Vp + (int64_t)(live ? j : 0) * G.m + base);
    double acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      acc[c] = 0.0;
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[c] += (double)r[i] * (double)w[i][c];
    }
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1)
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += __shfl_xor(acc[c], o, 64);
    if (sub == 0 && live) {
#pragma unroll
      for (int c = 0; c < C; ++c) out[(p * k + j) * C + c] = (real)acc[c];
    }
  }
}

template <typename real>
static int gather_jet_impl(const wiski_grid* grid, const real* d_x, int64_t n, const real* d_V, int32_t k, int32_t rows_per_point, real* d_out,
                           int32_t* d_err, void* stream) {
  GridDev<real> G;
  int rc = make_grid_dev<real>(grid, &G);
  if (rc) return rc;
  if (n < 0 || k < 1 || rows_per_point < 0) return WISKI_E_BADARG;
  if (n == 0) return WISKI_OK;
  if (!d_x || !d_V || !d_out || !d_err) return WISKI_E_BADARG;
  const int rows = rows_per_point > 0 ? rows_per_point : k;
  dim3 grd((unsigned)n);
#define CALL(DD) hipLaunchKernelGGL((k_gather_jet<real, DD>), grd, dim3(256), 0, (hipStream_t)stream, G, d_x, n, d_V, rows, rows_per_point > 0, d_out, d_err)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

extern "C" {
int wiski_jet_quadform_f32(const wiski_grid* g, const float* x, int64_t n, const float* M, int64_t ldm, float* out, int32_t* err, void* s) { return jet_quadform_impl<float>(g, x, n, M, ldm, out, err, s); }
int wiski_jet_quadform_f64(const wiski_grid* g, const double* x, int64_t n, const double* M, int64_t ldm, double* out, int32_t* err, void* s) { return jet_quadform_impl<double>(g, x, n, M, ldm, out, err, s); }
int wiski_wt_columns_jet_f32(const wiski_grid* g, const float* x, int64_t n, float* out, int32_t* err, void* s) { return wt_columns_jet_impl<float>(g, x, n, out, err, s); }
int wiski_wt_columns_jet_f64(const wiski_grid* g, const double* x, int64_t n, double* out, int32_t* err, void* s) { return wt_columns_jet_impl<double>(g, x, n, out, err, s); }
int wiski_gather_jet_f32(const wiski_grid* g, const float* x, int64_t n, const float* V, int32_t k, int32_t rows_per_point, float* out, int32_t* err, void* s) { return gather_jet_impl<float>(g, x, n, V, k, rows_per_point, out, err, s); }
int wiski_gather_jet_f64(const wiski_grid* g, const double* x, int64_t n, const double* V, int32_t k, int32_t rows_per_point, double* out, int32_t* err, void* s) { return gather_jet_impl<double>(g, x, n, V, k, rows_per_point, out, err, s); }
}
