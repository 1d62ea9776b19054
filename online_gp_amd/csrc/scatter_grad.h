// Absorb of derivative observations (AbsorbArgs::channels = d + 1).  Included by scatter_stats.hip.
//
// A point carries C = d + 1 scalar observations: channel 0 is f(x_p), channel 1 + q is df/dx_q (x_p).  Under the SKI model each is
// one linear observation of the grid values; its row v_c of W is the value row with dim q's four weights replaced by
// keys_cubic_deriv / h_q (zero in a dim whose cell is a one-hot boundary cell: the convention of wiski_gather_grad).  All C rows
// sit on the same 4^d taps, so per point
//   A[a, b] += sum_c wa_c v_c[a] v_c[b]
// is formed in registers from the C-channel tap tables in LDS and leaves as ONE atomic per tap pair: a point with a full gradient
// costs the memory side what a point with a value costs (T (T + 1) / 2 tap-pair atomics), not C times that.
// An absent channel is wa = wb = 0, noise = 1 and contributes nothing anywhere; channels with wa_c = 0 are skipped wave-uniformly.
#pragma once

// point_stencil plus the derivative weights dw[q][c] = k'(t + 1 - c) / h_q (zero in a boundary cell of dim q, and everywhere for a
// point outside the grid)
template <typename real, int D>
__device__ __forceinline__ bool point_stencil_grad(const GridDev<real>& G, const real* __restrict__ xp, int j0[D], real w[D][4], real dw[D][4]) {
  bool ok = true;
#pragma unroll
  for (int q = 0; q < D; ++q) {
    int j = dim_stencil<real>(xp[q], G.g0[q], G.h[q], G.hi[q], G.g[q], w[q]);
    const real uu = (xp[q] - G.g0[q]) / G.h[q];
    const real fl = floor(uu);
    const int jj = (int)fl - 1;
    const bool interior = !(jj < 0 || jj > G.g[q] - 4);
#pragma unroll
    for (int c = 0; c < 4; ++c) dw[q][c] = interior ? keys_cubic_deriv<real>(uu - fl + (real)1 - (real)c) / G.h[q] : (real)0;
    if (j < 0) {
      ok = false;
      j = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) w[q][c] = dw[q][c] = (real)0;
    }
    j0[q] = j;
  }
  return ok;
}

// The point sweep is that of k_scatter_stats_sym (scatter_half.h) with C = d + 1 channels.  The per-point tap table is channel-minor,
// s_val[point][tap][C], so that the C values of a tap are one contiguous LDS read (a ds_read_b128 at d = 3 in fp32): per tap-pair
// atomic the inner loop reads two such vectors and spends C multiply-adds.  LDS at d = 4 in fp64: 4 x 256 x 5 x 8 B = 40 KB of
// tables + 4 KB of row indices + 8 KB of pairs.  y / wa / wb / noise / mean_out are [n][C].
template <typename real, int D>
__global__ __launch_bounds__(256) void k_scatter_stats_grad(GridDev<real> G, const real* __restrict__ x, const real* __restrict__ y,
                                                            const real* __restrict__ wa, const real* __restrict__ wb,
                                                            const real* __restrict__ noise, int64_t n, real* __restrict__ b,
                                                            real* __restrict__ A, double* __restrict__ stats, int32_t* __restrict__ err,
                                                            real* __restrict__ cnt, const real* __restrict__ u, real* __restrict__ res,
                                                            real* __restrict__ mean_out) {
  constexpr int C = D + 1;
  using H = HalfTaps<D>;
  __shared__ __align__(16) real s_val[4][H::T][C];
  __shared__ int s_idx[4][H::T];
  __shared__ int s_pair[H::NPAIR];
  __shared__ double s_red[16];
  const int lane = threadIdx.x & 63, loc = threadIdx.x >> 6;
  half_pair_list<D>(s_pair, reinterpret_cast<int*>(s_red), 0, 1 << 30);         // the whole stencil: H::NPAIR pairs
  bool bad = false;
  for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {
    const int64_t p = base + loc;
    const bool valid = p < n;
    int j0[D], flat_t[H::TPL];
    real w[D][4], dw[D][4], val_t[H::TPL][C], wu[C], innov[C];
    real yw[C], wac[C];                            // wb_c y_c and wa_c (zero for a point that contributes nothing)
#pragma unroll
    for (int c = 0; c < C; ++c) yw[c] = wac[c] = (real)0;
    if (half_point_setup<real, D, true>(G, x, p, n, lane == 0, err, bad, j0, w, dw)) {      // outside: dropped for every channel, counted once
#pragma unroll
      for (int c = 0; c < C; ++c) {
        yw[c] = wb[p * C + c] * y[p * C + c];
        wac[c] = wa[p * C + c];
      }
    }
    int amask = 0;                                 // channels that enter A: the same in every lane of the wave
#pragma unroll
    for (int c = 0; c < C; ++c) amask |= (wac[c] != (real)0) << c;
    amask = __builtin_amdgcn_readfirstlane(amask);
    half_tap_table<real, D, C>(G, j0, w, dw, lane, u, &s_val[loc][0][0], s_idx[loc], flat_t, val_t, wu);
    half_carry<real, C>(u, yw, wac, wu, mean_out, p, lane == 0 && valid, innov);
    half_tap_atomics<real, D, C>(valid, flat_t, val_t, yw, wac, innov, b, cnt, res);
    __syncthreads();
    if (valid && A && amask) half_pair_loop<real, D, C>(lane, H::NPAIR, s_pair, &s_val[loc][0][0], s_idx[loc], wac, amask, A, G.m);
    __syncthreads();
  }
  scatter_stats_pass<real, D, C>(G, x, y, wb, noise, n, stats, s_red);
  if (bad) atomicOr(err, 1);
}

template <typename real>
static int launch_grad(const GridDev<real>& G, const AbsorbArgs<real>& a, hipStream_t stream) {
  int64_t blocks = (a.n + 3) / 4;
  if (blocks > 256 * 8) blocks = 256 * 8;
#define CALL(DD)                                                                                                                                     \
  hipLaunchKernelGGL((k_scatter_stats_grad<real, DD>), dim3((unsigned)blocks), dim3(256), 0, stream, G, a.x, a.y, a.wa, a.wb, a.noise, a.n, a.b, a.A, \
                     a.stats, a.err, a.cnt, a.u, a.res, a.mean_out)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}
