// Interpolated bilinear forms out[s][a][b] = w(xL[s,a])^T A w(xR[s,b]) of a dense symmetric m x m table A, and their input
// gradient: the blocks W_j M W_j^T, W_j H W_j^T and W* M W_j^T of the look-ahead acquisitions in the dense regime,
// without ever forming an interpolation row [m].
//
// Layout (both kernels): one 256-thread workgroup per "self" point (batch s, row a).  The self point's 4^D taps -- flat index, value
// weight and, for the VJP, the D derivative weights k'(s)/h times the other dims' cubic weights (zero in one-hot boundary cells, as
// k_gather_rows_vjp) -- are staged in LDS.  The "other" points are then visited in one of two forms, chosen per call on the host:
//   pair  every (other point, tap) pair is a thread: sum_ta wS[ta] A[iS[ta], iO[tb]], then the T partials of one other point are
//         summed in LDS in a fixed order.  Cost T^2 reads of A per other point; used while nO * T <= m.
//   row   the self point's interpolated row r = wS^T A (or the D derivative rows) is formed over all m columns in LDS -- coalesced
//         row segments of A -- and each other point gathers its taps from LDS (gather_one).  Cost T m reads of A once, then LDS only;
//         used when nO * T > m (the qKG cross block: q rows against J = 256 fantasy points) and the rows fit in 32 KiB of LDS.
// A is read-mostly (6.5 MB at m = 900 in fp64) and stays in L2 / MALL.  Every result is written by exactly one thread with a plain
// store; the VJP reduces in fp64 in a fixed order, so it is deterministic and needs neither float atomics nor workspace.
#include "wiski_common.h"

namespace {

constexpr int kRowLdsBytes = 32768;

// Tap `a` of point xp: flat grid index, value weight and (WANT_D) the D derivative weights.  False when the point is outside the grid
// (zero weights then).
template <typename real, int D, bool WANT_D>
__device__ __forceinline__ bool tap_weights(const GridDev<real>& G, const real* __restrict__ xp, int a, int& flat, real& val, real dval[D]) {
  bool ok = true;
  real wv[D], dv[D];
  flat = 0;
#pragma unroll
  for (int q = 0; q < D; ++q) {
    real w[4];
    const real xv = xp[q];
    int j0 = dim_stencil<real>(xv, G.g0[q], G.h[q], G.hi[q], G.g[q], w);
    const int c = (a >> (2 * (D - 1 - q))) & 3;
    if (j0 < 0) { ok = false; j0 = 0; w[c] = (real)0; }
    flat += (j0 + c) * G.stride[q];
    wv[q] = w[c];
    if constexpr (WANT_D) {
      const real u = (xv - G.g0[q]) / G.h[q];
      const real fl = floor(u);
      const int jj = (int)fl - 1;
      const bool interior = !(jj < 0 || jj > G.g[q] - 4);
      dv[q] = interior ? keys_cubic_deriv<real>(u - fl + (real)1 - (real)c) / G.h[q] : (real)0;
    }
  }
  val = (real)1;
#pragma unroll
  for (int q = 0; q < D; ++q) val *= wv[q];
  if constexpr (WANT_D) {
#pragma unroll
    for (int q = 0; q < D; ++q) {
      real t = dv[q];
#pragma unroll
      for (int o = 0; o < D; ++o)
        if (o != q) t *= wv[o];
      dval[q] = t;
    }
  }
  return ok;
}

// ---------------------------------------------------------------------------------------------------------------- forward ---
template <typename real, int D, bool ROW>
__global__ __launch_bounds__(256) void k_bilinear(GridDev<real> G, const real* __restrict__ A, int64_t lda, const real* __restrict__ xL, int qL,
                                                  const real* __restrict__ xR, int qR, int sym, real* __restrict__ out, int32_t* __restrict__ err) {
  constexpr int T = 1 << (2 * D);
  __shared__ int s_idx[T];
  __shared__ real s_val[T];
  extern __shared__ unsigned char s_dyn[];
  real* s_buf = reinterpret_cast<real*>(s_dyn);
  const int64_t blk = blockIdx.x;
  const int64_t s = blk / qL;
  const int a = (int)(blk - s * qL);
  for (int ta = threadIdx.x; ta < T; ta += blockDim.x) {
    int flat;
    real v;
    const bool ok = tap_weights<real, D, false>(G, xL + blk * D, ta, flat, v, nullptr);
    s_idx[ta] = flat;
    s_val[ta] = v;
    if (!ok && ta == 0) atomicOr(err, 1);
  }
  __syncthreads();
  const real* xo = xR + s * (int64_t)qR * D;
  real* orow = out + blk * qR;
  real* obase = out + s * (int64_t)qL * qR;
  const int b0 = sym ? a : 0;
  if constexpr (ROW) {
    for (int c = threadIdx.x; c < G.m; c += blockDim.x) {
      real acc = (real)0;
      for (int ta = 0; ta < T; ++ta) acc += s_val[ta] * A[(int64_t)s_idx[ta] * lda + c];
      s_buf[c] = acc;
    }
    __syncthreads();
    for (int b = b0 + threadIdx.x; b < qR; b += blockDim.x) {
      int j0[D];
      real w[D][4];
      if (!point_stencil<real, D>(G, xo + (int64_t)b * D, j0, w)) atomicOr(err, 1);
      const real v = gather_one<real, D>(G, j0, w, s_buf);
      orow[b] = v;
      if (sym && b != a) obase[(int64_t)b * qR + a] = v;
    }
  } else {
    constexpr int per = 256 / T;                       // other points per tile (T divides 256 for D <= 4)
    const int e = threadIdx.x, tb = e % T;
    for (int bt = b0; bt < qR; bt += per) {
      const int b = bt + e / T;
      real part = (real)0;
      if (b < qR) {
        int flat;
        real v;
        const bool ok = tap_weights<real, D, false>(G, xo + (int64_t)b * D, tb, flat, v, nullptr);
        if (!ok && tb == 0) atomicOr(err, 1);
        real acc = (real)0;
        for (int ta = 0; ta < T; ++ta) acc += s_val[ta] * A[(int64_t)s_idx[ta] * lda + flat];
        part = v * acc;
      }
      s_buf[e] = part;
      __syncthreads();
      if (e < per && bt + e < qR) {
        real v = (real)0;
        for (int t = 0; t < T; ++t) v += s_buf[e * T + t];
        const int bb = bt + e;
        orow[bb] = v;
        if (sym && bb != a) obase[(int64_t)bb * qR + a] = v;
      }
      __syncthreads();
    }
  }
}

// -------------------------------------------------------------------------------------------------------------------- VJP ---
// gx[s][p][k] = sum_o Gf(p, o) * d/dx_pk ( w(x_p)^T A w(y_o) ) over the other points y_o of batch s (A symmetric), with
// Gf(p, o) = Gm[s][p*gsS + o*gsO] (+ Gm[s][o*gsS + p*gsO] in the symmetric mode, where the self and other points are the same set).
template <typename real, int D, bool ROW>
__global__ __launch_bounds__(256) void k_bilinear_vjp(GridDev<real> G, const real* __restrict__ A, int64_t lda, const real* __restrict__ xS, int nS,
                                                      const real* __restrict__ xO, int nO, const real* __restrict__ Gm, int64_t gsB, int gsS, int gsO,
                                                      int sym, real* __restrict__ gx) {
  constexpr int T = 1 << (2 * D);
  __shared__ int s_idx[T];
  __shared__ real s_dval[D][T];
  __shared__ double s_red[4][D];
  extern __shared__ unsigned char s_dyn[];
  real* s_row = reinterpret_cast<real*>(s_dyn);
  const int64_t blk = blockIdx.x;
  const int64_t s = blk / nS;
  const int p = (int)(blk - s * nS);
  for (int ta = threadIdx.x; ta < T; ta += blockDim.x) {
    int flat;
    real v, dv[D];
    tap_weights<real, D, true>(G, xS + blk * D, ta, flat, v, dv);
    s_idx[ta] = flat;
#pragma unroll
    for (int k = 0; k < D; ++k) s_dval[k][ta] = dv[k];
  }
  __syncthreads();
  const real* xo = xO + s * (int64_t)nO * D;
  const real* Gs = Gm + s * gsB;
  double acc[D];
#pragma unroll
  for (int k = 0; k < D; ++k) acc[k] = 0.0;
  if constexpr (ROW) {
    for (int c = threadIdx.x; c < G.m; c += blockDim.x) {
      real r[D];
#pragma unroll
      for (int k = 0; k < D; ++k) r[k] = (real)0;
      for (int ta = 0; ta < T; ++ta) {
        const real av = A[(int64_t)s_idx[ta] * lda + c];
#pragma unroll
        for (int k = 0; k < D; ++k) r[k] += s_dval[k][ta] * av;
      }
#pragma unroll
      for (int k = 0; k < D; ++k) s_row[(int64_t)k * G.m + c] = r[k];
    }
    __syncthreads();
    for (int o = threadIdx.x; o < nO; o += blockDim.x) {
      int j0[D];
      real w[D][4];
      point_stencil<real, D>(G, xo + (int64_t)o * D, j0, w);
      double gf = (double)Gs[(int64_t)p * gsS + (int64_t)o * gsO];
      if (sym) gf += (double)Gs[(int64_t)o * gsS + (int64_t)p * gsO];
#pragma unroll
      for (int k = 0; k < D; ++k) acc[k] += gf * (double)gather_one<real, D>(G, j0, w, s_row + (int64_t)k * G.m);
    }
  } else {
    for (int e = threadIdx.x; e < nO * T; e += blockDim.x) {
      const int o = e / T, tb = e - (e / T) * T;
      int flat;
      real v;
      tap_weights<real, D, false>(G, xo + (int64_t)o * D, tb, flat, v, nullptr);
      double gf = (double)Gs[(int64_t)p * gsS + (int64_t)o * gsO];
      if (sym) gf += (double)Gs[(int64_t)o * gsS + (int64_t)p * gsO];
      real r[D];
#pragma unroll
      for (int k = 0; k < D; ++k) r[k] = (real)0;
      for (int ta = 0; ta < T; ++ta) {
        const real av = A[(int64_t)s_idx[ta] * lda + flat];
#pragma unroll
        for (int k = 0; k < D; ++k) r[k] += s_dval[k][ta] * av;
      }
      const double gv = gf * (double)v;
#pragma unroll
      for (int k = 0; k < D; ++k) acc[k] += gv * (double)r[k];
    }
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    const double t = wave_reduce_sum<double>(acc[k]);
    if (lane == 0) s_red[wid][k] = t;
  }
  __syncthreads();
  if (threadIdx.x < D) {
    double t = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += s_red[w][threadIdx.x];
    gx[blk * D + threadIdx.x] = (real)t;
  }
}

// The row form pays T m reads of A once per self point instead of T^2 per other point; it also needs its K rows in LDS.
template <typename real>
bool use_row_form(const GridDev<real>& G, int64_t nOther, int K) {
  return nOther * (int64_t)G.T > (int64_t)G.m && (int64_t)K * G.m * (int64_t)sizeof(real) <= kRowLdsBytes;
}

template <typename real>
int bilinear_impl(const wiski_grid* grid, const real* d_A, int64_t lda, const real* d_xL, int32_t qL, const real* d_xR, int32_t qR, int64_t nbatch,
                  real* d_out, int32_t* d_err, void* stream) {
  GridDev<real> G;
  int rc = make_grid_dev<real>(grid, &G);
  if (rc) return rc;
  if (nbatch < 0 || qL < 0 || qR < 0 || lda < G.m) return WISKI_E_BADARG;
  if (nbatch == 0 || qL == 0 || qR == 0) return WISKI_OK;
  const bool sym = d_xR == nullptr;                     // explicit: an xR that aliases xL is the general mode (two inputs)
  if (sym && qR != qL) return WISKI_E_BADARG;
  if (sym) d_xR = d_xL;
  if (!d_A || !d_xL || !d_out || !d_err) return WISKI_E_BADARG;
  if (nbatch * (int64_t)qL > (int64_t)INT32_MAX) return WISKI_E_BADARG;
  dim3 grd((unsigned)(nbatch * qL));
  const bool row = use_row_form<real>(G, qR, 1);
  const size_t lds = row ? (size_t)G.m * sizeof(real) : 256 * sizeof(real);
#define CALL(DD)                                                                                                                          \
  if (row) hipLaunchKernelGGL((k_bilinear<real, DD, true>), grd, dim3(256), lds, (hipStream_t)stream, G, d_A, lda, d_xL, qL, d_xR, qR, (int)sym, d_out, d_err); \
  else hipLaunchKernelGGL((k_bilinear<real, DD, false>), grd, dim3(256), lds, (hipStream_t)stream, G, d_A, lda, d_xL, qL, d_xR, qR, (int)sym, d_out, d_err)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

template <typename real>
int launch_vjp(const GridDev<real>& G, const real* A, int64_t lda, const real* xS, int nS, const real* xO, int nO, int64_t nbatch, const real* Gm,
               int64_t gsB, int gsS, int gsO, bool sym, real* gx, hipStream_t stream) {
  if (nbatch * (int64_t)nS > (int64_t)INT32_MAX) return WISKI_E_BADARG;
  dim3 grd((unsigned)(nbatch * nS));
  const bool row = use_row_form<real>(G, nO, G.d);
  const size_t lds = row ? (size_t)G.d * G.m * sizeof(real) : 0;
#define CALL(DD)                                                                                                                                \
  if (row) hipLaunchKernelGGL((k_bilinear_vjp<real, DD, true>), grd, dim3(256), lds, stream, G, A, lda, xS, nS, xO, nO, Gm, gsB, gsS, gsO, (int)sym, gx); \
  else hipLaunchKernelGGL((k_bilinear_vjp<real, DD, false>), grd, dim3(256), lds, stream, G, A, lda, xS, nS, xO, nO, Gm, gsB, gsS, gsO, (int)sym, gx)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

template <typename real>
int bilinear_vjp_impl(const wiski_grid* grid, const real* d_A, int64_t lda, const real* d_xL, int32_t qL, const real* d_xR, int32_t qR, int64_t nbatch,
                      const real* d_G, real* d_gxL, real* d_gxR, void* stream) {
  GridDev<real> G;
  int rc = make_grid_dev<real>(grid, &G);
  if (rc) return rc;
  if (nbatch < 0 || qL < 0 || qR < 0 || lda < G.m) return WISKI_E_BADARG;
  const bool sym = d_xR == nullptr;                     // explicit: an xR that aliases xL is the general mode (two inputs)
  if (sym && (qR != qL || d_gxR)) return WISKI_E_BADARG;  // the symmetric mode returns the whole gradient in d_gxL
  if (nbatch == 0 || (qL == 0 && qR == 0)) return WISKI_OK;
  if (sym) d_xR = d_xL;
  if (!d_A || !d_xL || !d_G || (!d_gxL && !d_gxR)) return WISKI_E_BADARG;
  const int64_t gsB = (int64_t)qL * qR;
  hipStream_t st = (hipStream_t)stream;
  if (d_gxL && qL > 0) {
    rc = launch_vjp<real>(G, d_A, lda, d_xL, qL, d_xR, qR, nbatch, d_G, gsB, qR, 1, sym, d_gxL, st);
    if (rc) return rc;
  }
  if (d_gxR && qR > 0) {
    rc = launch_vjp<real>(G, d_A, lda, d_xR, qR, d_xL, qL, nbatch, d_G, gsB, 1, qR, false, d_gxR, st);
    if (rc) return rc;
  }
  return WISKI_OK;
}

}  // namespace

extern "C" {
int wiski_interp_bilinear_f32(const wiski_grid* g, const float* A, int64_t lda, const float* xL, int32_t qL, const float* xR, int32_t qR, int64_t nbatch,
                              float* out, int32_t* err, void* s) { return bilinear_impl<float>(g, A, lda, xL, qL, xR, qR, nbatch, out, err, s); }
int wiski_interp_bilinear_f64(const wiski_grid* g, const double* A, int64_t lda, const double* xL, int32_t qL, const double* xR, int32_t qR, int64_t nbatch,
                              double* out, int32_t* err, void* s) { return bilinear_impl<double>(g, A, lda, xL, qL, xR, qR, nbatch, out, err, s); }
int wiski_interp_bilinear_vjp_f32(const wiski_grid* g, const float* A, int64_t lda, const float* xL, int32_t qL, const float* xR, int32_t qR, int64_t nbatch,
                                  const float* G, float* gxL, float* gxR, void* s) { return bilinear_vjp_impl<float>(g, A, lda, xL, qL, xR, qR, nbatch, G, gxL, gxR, s); }
int wiski_interp_bilinear_vjp_f64(const wiski_grid* g, const double* A, int64_t lda, const double* xL, int32_t qL, const double* xR, int32_t qR, int64_t nbatch,
                                  const double* G, double* gxL, double* gxR, void* s) { return bilinear_vjp_impl<double>(g, A, lda, xL, qL, xR, qR, nbatch, G, gxL, gxR, s); }
}
