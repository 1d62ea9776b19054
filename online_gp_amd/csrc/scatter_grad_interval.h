// Interval sites on the value and the partial derivatives of a point (AbsorbArgs::clo).  Included by
// scatter_stats.hip, after scatter_grad.h, scatter_site.h and scatter_interval.h, whose parts it combines.
//
// A point carries C = d + 1 channels as in scatter_grad.h (0: f(x_p), 1 + q: df/dx_q (x_p)), and every present channel
// (wa[p][c] != 0) says lo_c <= v_c . u_true + eps_c <= hi_c at noise sigma2 noise[p][c]: "increasing in dim q" is lo = 0 on channel
// 1 + q, a slope bound |df/dx_q| <= L is [-L, L].  Each channel is moment-matched against the posterior BEFORE the batch exactly
// as a value is in scatter_interval.h -- mu_c = v_c . u is what the C-channel tap table already reduces over the wave, pvar_c the
// posterior variance of that channel -- and enters as the pseudo-target ytilde_c at noise noise_c / omega_c.  The channels of a
// point are matched independently (their posterior cross-covariance is not used in the site); all sites of a launch are taken
// against the same u (parallel ADF).  A derivative channel in a one-hot boundary cell has a zero row and mu = 0; its site is
// evaluated like any other and enters b, A, cnt and res with zero rows, the two scalars with its own terms.
//
// Lanes are channels: lane l < C selects mu_l from the wave-uniform wu[] by a select chain (a run-time index would put the array
// in scratch), loads lo / hi / pvar / noise [p][l] -- contiguous over the lanes -- and evaluates interval_site once; omega wa and
// ytilde omega wb of each channel are then broadcast to the wave.  The kernel holds ONE inlined copy of the erfcx pair, not C, and
// no loop over channels around it.  The two scalars are kept per lane l < C in fp64 from the un-rounded sites and leave as one
// atomic pair per block, as in k_scatter_stats_site, whose launch geometry this form takes.
#pragma once

// lane `l` (wave-uniform) of v, in every lane: a v_readlane per 32-bit half, so the result sits in scalar registers
__device__ __forceinline__ float lane_bcast(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
__device__ __forceinline__ double lane_bcast(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// clo / chi / cpvar / wa / wb / noise / the three outputs / mean_out are [n][C].
template <typename real, int D>
__global__ __launch_bounds__(256) void k_scatter_stats_grad_site(GridDev<real> G, const real* __restrict__ x, const real* __restrict__ wa,
                                                                 const real* __restrict__ wb, const real* __restrict__ noise, int64_t n,
                                                                 real* __restrict__ b, real* __restrict__ A, double* __restrict__ stats,
                                                                 int32_t* __restrict__ err, real* __restrict__ cnt, const real* __restrict__ u,
                                                                 real* __restrict__ res, real* __restrict__ mean_out,
                                                                 const real* __restrict__ clo, const real* __restrict__ chi,
                                                                 const real* __restrict__ cpvar, double sigma2, real* __restrict__ ytilde_out,
                                                                 real* __restrict__ omega_out, double* __restrict__ logz_out) {
  constexpr int C = D + 1;
  using H = HalfTaps<D>;
  __shared__ __align__(16) real s_val[4][H::T][C];
  __shared__ int s_idx[4][H::T];
  __shared__ int s_pair[H::NPAIR];
  __shared__ double s_red[16];
  const int lane = threadIdx.x & 63, loc = threadIdx.x >> 6;
  half_pair_list<D>(s_pair, reinterpret_cast<int*>(s_red), 0, 1 << 30);         // the whole stencil: H::NPAIR pairs
  bool bad = false;
  double c_acc = 0, ld_acc = 0;                  // lanes < C: the share of their channel of this wave's points in the two scalars
  for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {
    const int64_t p = base + loc;
    const bool valid = p < n;
    int j0[D], flat_t[H::TPL];
    real w[D][4], dw[D][4], val_t[H::TPL][C], wu[C], innov[C], yw[C], wac[C];
    const bool inside = half_point_setup<real, D, true>(G, x, p, n, lane == 0, err, bad, j0, w, dw);   // outside: dropped for every channel, counted once
    // the lane's channel: the neutral datum for lanes >= C and for a wave past the batch
    const bool mine = valid && lane < C;
    const int64_t e = p * C + lane;
    double lo_l = 0, hi_l = 0, v_l = 0, n_l = 1;
    real wa_l = 0, wb_l = 0;
    if (mine) {
      lo_l = (double)clo[e];
      hi_l = (double)chi[e];
      v_l = (double)cpvar[e];
      n_l = (double)noise[e];
      wa_l = wa[e];
      wb_l = wb[e];
    }
    half_tap_table<real, D, C>(G, j0, w, dw, lane, u, &s_val[loc][0][0], s_idx[loc], flat_t, val_t, wu);   // wu[c]: the predictive mean of channel c before the batch
    real mu_l = wu[0];
#pragma unroll
    for (int c = 1; c < C; ++c) mu_l = lane == c ? wu[c] : mu_l;
    const bool present = mine && inside && wa_l != (real)0;
    IntervalSite st{0.0, 0.0, 0.0};              // an absent channel, a point outside the grid: (0, 0, 0)
    if (present) st = interval_site(lo_l, hi_l, (double)mu_l, v_l, sigma2 * n_l);
    const bool enters = st.omega > 0.0;          // (a skipped channel reports (mu, 0, log Z))
    const real omega = (real)st.omega, yt = (real)st.ytilde;
    wb_l *= omega;
    const real wac_l = wa_l * omega, yw_l = yt * wb_l;
    if (mine) {
      ytilde_out[e] = yt;
      omega_out[e] = omega;
      logz_out[e] = st.logz;
      if (enters) {
        c_acc += st.ytilde * st.ytilde * (double)wb_l;
        ld_acc += log(n_l / st.omega);
      }
    }
    const int amask = __builtin_amdgcn_readfirstlane((int)(__ballot(enters) & ((1ull << C) - 1ull)));   // channels that enter: the same in every lane
#pragma unroll
    for (int c = 0; c < C; ++c) {
      wac[c] = lane_bcast(wac_l, c);
      yw[c] = lane_bcast(yw_l, c);
    }
    half_carry<real, C>(u, yw, wac, wu, mean_out, p, lane == 0 && valid, innov);   // with the weights the channels enter with
    half_tap_atomics<real, D, C>(valid && amask != 0, flat_t, val_t, yw, wac, innov, b, cnt, res);
    __syncthreads();
    if (valid && amask) half_pair_loop<real, D, C>(lane, H::NPAIR, s_pair, &s_val[loc][0][0], s_idx[loc], wac, amask, A, G.m);
    __syncthreads();
  }
  stats_atomic_pair(c_acc, ld_acc, stats, s_red);
  if (bad) atomicOr(err, 1);
}

template <typename real>
static int launch_grad_site(const GridDev<real>& G, const AbsorbArgs<real>& a, hipStream_t stream) {
  int64_t blocks = (a.n + ROBUST_POINTS_PER_BLOCK - 1) / ROBUST_POINTS_PER_BLOCK;
  if (blocks > 256 * 8) blocks = 256 * 8;
#define CALL(DD)                                                                                                                                          \
  hipLaunchKernelGGL((k_scatter_stats_grad_site<real, DD>), dim3((unsigned)blocks), dim3(256), 0, stream, G, a.x, a.wa, a.wb, a.noise, a.n, a.b, a.A,    \
                     a.stats, a.err, a.cnt, a.u, a.res, a.mean_out, a.clo, a.chi, a.cpvar, a.sigma2, a.ytilde_out, a.omega_out, a.logz_out)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}
