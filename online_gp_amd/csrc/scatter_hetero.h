// Heteroscedastic absorb: a second field on the same grid, g(x) = log of the noise multiplier, learned from the stream's own
// residuals inside the launch that absorbs the batch.  Included by scatter_stats.hip, after scatter_count.h.
//
//   y_p = f(x_p) + eps_p,   eps_p ~ N(0, sigma2 noise_p exp g(x_p)),   g ~ GP(g0, k_g)
// f and g are two single-output models on ONE grid, each with its own statistics.  Against the two posteriors BEFORE the batch --
// mu_f = w_p . u_f, v_f = max(pvar_p, 0), mu_g = g0 + w_p . u_g, v_g = max(pvar2_p, 0) --
//   e_p   = exp(mu_g + v_g / 2)                      the mean of the log-normal multiplier
//   f     takes the point as its own target y_p at noise noise_p / omega_f, omega_f = 1 / e_p (NOT capped at 1), and
//         log Z_y = log N(y; mu_f, v_f + dn), dn = sigma2 noise_p e_p
//   rho_p = (y_p - mu_f)^2 / (sigma2 noise_p) * dn / (dn + v_f)
//         the squared residual in units of the known noise, deflated by the share of it that is f's own uncertainty
//   g     takes the site of the log-variance likelihood l(g) = (2 pi)^(-nu / 2) exp(-nu g / 2 - rho e^-g / 2), nu = 1, matched
//         against N(mu_g, v_g) by count_site (scatter_count.h) as the family WISKI_COUNT_LOGVAR: the target ytilde_g - g0 at noise
//         1 / tau_g, with the noise model's own sigma2 = noise = wa = wb = 1
// The likelihood is log-concave (g'' = -rho e^-g / 2 <= 0) for every rho >= 0, which is all count_site relies on.  rho = 0 has
// tau = 0 and is skipped by the omega < WISKI_COUNT_OMEGA_MIN rule; a skipped noise site does not keep the point out of f.
// The targets are two models, not C outputs of one, and the weight f receives is a function of g's posterior: the wave needs both
// means before it can weight anything, so this is a kernel of its own (as the label kernel is) and not a Site of k_scatter_stats_site.
#pragma once

template <>
struct CountFamily<WISKI_COUNT_LOGVAR> {           // y = rho, the sum of squares of t = nu residuals in units of the known noise
  static __device__ __forceinline__ bool valid(double y, double t) { return y >= 0.0 && t > 0.0 && isfinite(y) && isfinite(t); }
  static __device__ __forceinline__ double constant(double y, double t) { return -0.91893853320467274178 * t; }
  static __device__ __forceinline__ double g(double y, double t, double f) { return -0.5 * (t * f + y * exp(-f)); }
  static __device__ __forceinline__ double g1(double y, double t, double f) { return 0.5 * (y * exp(-f) - t); }
  static __device__ __forceinline__ double g2(double y, double t, double f) { return -0.5 * y * exp(-f); }
};

// One set of statistics: what a single-output half-stencil absorb with the carry writes and reads.
template <typename real>
struct HeteroSet {
  real* b;
  real* A;
  real* cnt;
  double* stats;
  const real* u;
  real* res;                                        // optional
};

// What the wave makes of a point inside the grid, in fp64 whatever the working precision; the same in every lane.
struct HeteroValue {
  double e, logzy;                                  // the multiplier f was weighted with, log N(y; mu_f, v_f + dn)
  bool enters;                                      // f takes the point: a finite y, a finite positive noise, and a multiplier whose value
                                                    // and reciprocal are both positive and finite in the working precision
  CountSite g;                                      // the noise site (omega = tau)
};

template <typename real>
__device__ __forceinline__ HeteroValue hetero_site(double y, double mu_f, double pvar_f, double wug, double pvar_g, double noise, double sigma2,
                                                   double g0, int lane) {
  constexpr double HALF_LOG_2PI = 0.91893853320467274178;
  HeteroValue r{0.0, NAN, false, {g0 + wug, 0.0, NAN}};
  const double v_f = pvar_f > 0.0 ? pvar_f : 0.0, v_g = pvar_g > 0.0 ? pvar_g : 0.0;      // (a NaN variance counts as 0, as a negative one)
  const double mu_g = g0 + wug;
  const double e = exp(mu_g + 0.5 * v_g), kn = sigma2 * noise, dn = kn * e;
  r.e = e;
  if (!isfinite(y) || !isfinite(mu_f) || !(dn > 0.0) || !isfinite(dn) || !(kn > 0.0)) return r;   // wave-uniform
  // e and omega_f = 1 / e reach the statistics and e_out in `real`: beyond its range (|mu_g + v_g / 2| > 87 in fp32) the point would
  // enter at weight inf or 0 while e_out says otherwise -- it is skipped for both models instead, like a y that is not finite
  const real er = (real)e, ofr = (real)(1.0 / e);
  if (!(er > (real)0) || !isfinite(er) || !(ofr > (real)0) || !isfinite(ofr)) return r;
  const double s = v_f + dn, d = y - mu_f;
  r.enters = true;
  r.logzy = -HALF_LOG_2PI - 0.5 * log(s) - 0.5 * d * d / s;
  const double rho = d * d / kn * (dn / s);
  r.g = count_site<WISKI_COUNT_LOGVAR>(rho, 1.0, mu_g, v_g, 1.0, lane);
  return r;
}

// The absorb.  One wave per point, four per block, the block loop of k_scatter_stats_site: the point is set up and its tap table
// built ONCE (both fields live on the same grid), both means are reduced over the wave -- w . u_f with the table, w . u_g from the
// lane's own taps, the way half_tap_grad reduces the slopes -- the wave evaluates the site, and the tap atomics and the pair loop run
// for the f set and, where the noise site entered, once more for the g set.  Each wave keeps the two scalars of each model in fp64.
// A NaN y skips the point for both models (log Z = NaN, no flag); a point outside the grid is dropped for both, flagged and counted
// once, and reports zeros.
template <typename real, int D>
__global__ __launch_bounds__(256) void k_scatter_stats_hetero(GridDev<real> G, const real* __restrict__ x, const real* __restrict__ y,
                                                              const real* __restrict__ wa, const real* __restrict__ wb,
                                                              const real* __restrict__ noise, const real* __restrict__ pvar,
                                                              const real* __restrict__ pvar2, double sigma2, double g0, int64_t n,
                                                              HeteroSet<real> F, HeteroSet<real> N, int32_t* __restrict__ err,
                                                              real* __restrict__ mean_out, real* __restrict__ e_out,
                                                              real* __restrict__ ytilde_out, real* __restrict__ omega_out,
                                                              double* __restrict__ logz_out, double* __restrict__ logzy_out) {
  using H = HalfTaps<D>;
  __shared__ real s_val[4][H::T];
  __shared__ int s_idx[4][H::T];
  __shared__ int s_pair[H::NPAIR];
  __shared__ double s_red[16];
  const int lane = threadIdx.x & 63, loc = threadIdx.x >> 6;
  half_pair_list<D>(s_pair, reinterpret_cast<int*>(s_red), 0, 1 << 30);         // the whole stencil: H::NPAIR pairs
  bool bad = false;
  double cf_acc = 0, ldf_acc = 0, cg_acc = 0, ldg_acc = 0;                      // lane 0: this wave's share of the two scalars of f and of g
  for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {
    const int64_t p = base + loc;
    const bool valid = p < n;
    int j0[D], flat_t[H::TPL];
    real w[D][4], val_t[H::TPL][1], yw[1], wac[1], wu[1], innov[1];
    const bool inside = half_point_setup<real, D>(G, x, p, n, lane == 0, err, bad, j0, w);
    double yp = NAN, pv = 0, pv2 = 0, n_p = 1;
    real wap = 0, wbp = 0;
    if (valid) {
      yp = (double)y[p];
      pv = (double)pvar[p];
      pv2 = (double)pvar2[p];
      n_p = (double)noise[p];
      wap = wa[p];
      wbp = wb[p];
    }
    half_tap_table<real, D, 1>(G, j0, w, nullptr, lane, F.u, s_val[loc], s_idx[loc], flat_t, val_t, wu);   // wu: mu_f
    real wug = 0;                                    // w . u_g, from the lane's own taps
#pragma unroll
    for (int t = 0; t < H::TPL; ++t)
      if (val_t[t][0] != (real)0) wug += val_t[t][0] * N.u[flat_t[t]];
    wug = wave_reduce_sum<real>(wug);
    HeteroValue st{0.0, 0.0, false, {0.0, 0.0, 0.0}};
    if (inside) st = hetero_site<real>(yp, (double)wu[0], pv, (double)wug, pv2, n_p, sigma2, g0, lane);
    const bool in_f = valid && st.enters, in_g = in_f && st.g.omega > 0.0;
    // f: its own target at noise noise_p e
    const real omega_f = in_f ? (real)(1.0 / st.e) : (real)0;
    wbp *= omega_f;
    wac[0] = wap * omega_f;
    yw[0] = in_f ? (real)yp * wbp : (real)0;
    half_carry<real, 1>(F.u, yw, wac, wu, mean_out, p, lane == 0 && valid, innov);
    // g: the site's target less the prior mean, at weight tau
    const real tau = (real)st.g.omega, tg = (real)(st.g.ytilde - g0);
    const real yw2[1] = {tg * tau}, wac2[1] = {tau}, innov2[1] = {tg * tau - tau * wug};
    if (lane == 0 && valid) {
      e_out[p] = (real)st.e;
      ytilde_out[p] = (real)st.g.ytilde;
      omega_out[p] = tau;
      logz_out[p] = st.g.logz;
      logzy_out[p] = st.logzy;
      if (in_f) {
        cf_acc += yp * yp * (double)wbp;
        ldf_acc += log(n_p * st.e);
      }
      if (in_g) {
        const double t = st.g.ytilde - g0;
        cg_acc += t * t * (double)tau;
        ldg_acc -= log(st.g.omega);
      }
    }
    half_tap_atomics<real, D, 1>(in_f, flat_t, val_t, yw, wac, innov, F.b, F.cnt, F.res);
    __syncthreads();
    if (in_f) half_pair_loop<real, D, 1>(lane, H::NPAIR, s_pair, s_val[loc], s_idx[loc], wac, 1, F.A, G.m);
    if (in_g) {                                      // (wave-uniform)
      half_tap_atomics<real, D, 1>(true, flat_t, val_t, yw2, wac2, innov2, N.b, N.cnt, N.res);
      half_pair_loop<real, D, 1>(lane, H::NPAIR, s_pair, s_val[loc], s_idx[loc], wac2, 1, N.A, G.m);
    }
    __syncthreads();
  }
  stats_atomic_pair(cf_acc, ldf_acc, F.stats, s_red);
  __syncthreads();
  stats_atomic_pair(cg_acc, ldg_acc, N.stats, s_red);
  if (bad) atomicOr(err, 1);
}

// Sites only (wiski_hetero_sites): count_sites_impl<real, WISKI_COUNT_LOGVAR> (scatter_count.h) from given mu_g, v_g, rho, nu.

template <typename real>
static int launch_hetero(const GridDev<real>& G, const AbsorbArgs<real>& a, hipStream_t stream) {
  int64_t blocks = (a.n + ROBUST_POINTS_PER_BLOCK - 1) / ROBUST_POINTS_PER_BLOCK;
  if (blocks > 256 * 8) blocks = 256 * 8;
  const HeteroSet<real> F{a.b, a.A, a.cnt, a.stats, a.u, a.res}, N{a.b2, a.A2, a.cnt2, a.stats2, a.u2, a.res2};
#define CALL(DD)                                                                                                                                     \
  hipLaunchKernelGGL((k_scatter_stats_hetero<real, DD>), dim3((unsigned)blocks), dim3(256), 0, stream, G, a.x, a.y, a.wa, a.wb, a.noise, a.pvar,     \
                     a.pvar2, a.sigma2, a.g0, a.n, F, N, a.err, a.mean_out, a.e_out, a.ytilde_out, a.omega_out, a.logz_out, a.logzy_out)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}
