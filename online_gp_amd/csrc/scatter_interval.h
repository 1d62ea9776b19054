// Interval-observation absorb (AbsorbArgs::lo).  Included by scatter_stats.hip.
//
// A point says y_p = f(x_p) + eps_p lies in [lo_p, hi_p] (either end may be infinite; lo_p == hi_p is an exact value).  It is
// moment-matched against the posterior BEFORE the batch, inside the launch that absorbs it (assumed-density filtering): with
//   mu = w_p . u,  v = pvar_p,  dn = sigma2 noise_p,  s^2 = v + dn,  a = (lo - mu) / s,  b = (hi - mu) / s,  Z = Phi(b) - Phi(a),
//   alpha = d log Z / d mu,   beta = -d^2 log Z / d mu^2,   omega = dn beta / (1 - v beta),   ytilde = mu + alpha / beta
// the point enters as the pseudo-target ytilde at noise noise_p / omega_p, exactly as k_scatter_stats_robust enters a point: A, cnt
// and the carried residual with omega wa, b and sum wb y^2 with omega wb and ytilde for y, log|D| with log(noise / omega).  w_p . u
// is what the sweep already reduces over the wave, so the site costs three loads (lo, hi, pvar), three stores and no second pass
// over the stencil.  All sites of a launch are taken against the same u and pvar (parallel ADF): they depend neither on the order
// of the points nor on the order of the atomics.
#pragma once

// A site whose omega falls below this enters nothing: an uninformative interval, or a bound satisfied by so many standard
// deviations that ytilde = mu + alpha / beta is 0 / 0.
#ifndef WISKI_INTERVAL_OMEGA_MIN
#define WISKI_INTERVAL_OMEGA_MIN 1e-12
#endif

struct IntervalSite {
  double ytilde, omega, logz;                     // omega = 0: the point is skipped (ytilde = mu)
};

// The site of one point, in fp64 whatever the working precision.  The interval is mirrored about mu so that its centre lies at or
// below the mean (|a| >= |b|, a < 0); a one-sided bound is then the open interval (-inf, b].  Both ends go through erfcx of a
// non-negative argument, Phi(-t) = erfcx(t / sqrt 2) exp(-t^2 / 2) / 2.  For b <= 0 both sit in the lower tail and Z, phi(a), phi(b)
// are carried in units of exp(-b^2 / 2) -- nothing underflows however far the bound is violated; for b > 0 > a, Z = 1 - Phi(-b) - Phi(a)
// and log Z is a log1p.  One straight line of two erfcx, two exp, a log and a log1p: the cases differ in selects, not in calls.
__device__ __forceinline__ IntervalSite interval_site(double lo, double hi, double mu, double v, double dn) {
  constexpr double RSQRT2 = 0.70710678118654752440, RSQRT2PI = 0.39894228040143267794, HALF_LOG_2PI = 0.91893853320467274178;
  IntervalSite r{mu, 0.0, lo > hi ? -INFINITY : NAN};
  if (!(lo <= hi)) return r;                                            // an empty interval, or a NaN bound
  v = v > 0.0 ? v : 0.0;
  const double s = sqrt(v + dn);
  if (lo == hi) {                                                       // an exact value (two equal infinities: the empty interval)
    const double z = (lo - mu) / s;
    if (isfinite(lo)) r = IntervalSite{lo, 1.0, -0.5 * z * z - log(s) - HALF_LOG_2PI};
    else r.logz = -INFINITY;
    return r;
  }
  double a = (lo - mu) / s, b = (hi - mu) / s;
  const bool flip = a + b > 0.0;
  if (flip) {
    const double t = a;
    a = -b;
    b = -t;
  }
  const bool open = isinf(a);                                           // a = -inf
  if (open && isinf(b)) {                                               // (-inf, inf): no information
    r.logz = 0.0;
    return r;
  }
  if (open) a = 0.0;                                                    // (its terms are switched off through ea)
  const bool tail = b <= 0.0;
  const double hb2 = 0.5 * b * b;
  const double eb = tail ? 1.0 : exp(-hb2);                             // phi(b), phi(a) / RSQRT2PI in the unit of the case
  const double ea = open ? 0.0 : exp(tail ? 0.5 * (b - a) * (b + a) : -0.5 * a * a);
  const double tb = erfcx(fabs(b) * RSQRT2), ta = erfcx(-a * RSQRT2);
  const double q = 0.5 * (eb * tb + ea * ta);                           // b > 0: Phi(-b) + Phi(a)
  const double Z = tail ? 0.5 * (tb - ea * ta) : 1.0 - q;
  const double logz = tail ? log(Z) - hb2 : log1p(-q);
  const double pa = RSQRT2PI * ea, pb = RSQRT2PI * eb;
  const double alpha = (pa - pb) / (s * Z);                             // of the mirrored interval
  const double beta = alpha * alpha + (b * pb - a * pa) / (s * s * Z);
  r.logz = logz;
  if (!(beta > 0.0) || !isfinite(beta)) return r;
  const double den = 1.0 - v * beta;                                    // >= dn / s^2 up to rounding
  const double omega = den > 0.0 ? fmin(dn * beta / den, 1.0) : 1.0;
  if (!(omega >= WISKI_INTERVAL_OMEGA_MIN)) return r;
  r.omega = omega;
  r.ytilde = mu + (flip ? -alpha : alpha) / beta;
  return r;
}

// The point sweep is that of k_scatter_stats_sym (scatter_half.h), the two scalars those of k_scatter_stats_robust and for its
// reason: the pseudo-targets and weights of a launch exist in the waves that computed them only.  A wave is one point, so the
// site and its case split are wave-uniform.  No guard, zero regions, shard or batch (absorb_validate).
template <typename real, int D>
__global__ __launch_bounds__(256) void k_scatter_stats_interval(GridDev<real> G, const real* __restrict__ x, const real* __restrict__ lo,
                                                                const real* __restrict__ hi, const real* __restrict__ pvar, double sigma2,
                                                                const real* __restrict__ wa, const real* __restrict__ wb,
                                                                const real* __restrict__ noise, int64_t n, real* __restrict__ b,
                                                                real* __restrict__ A, double* __restrict__ stats, int32_t* __restrict__ err,
                                                                real* __restrict__ cnt, const real* __restrict__ u, real* __restrict__ res,
                                                                real* __restrict__ mean_out, real* __restrict__ ytilde_out,
                                                                real* __restrict__ omega_out, double* __restrict__ logz_out) {
  using H = HalfTaps<D>;
  __shared__ real s_val[4][H::T];
  __shared__ int s_idx[4][H::T];
  __shared__ int s_pair[H::NPAIR];
  __shared__ double s_red[16];
  const int lane = threadIdx.x & 63, loc = threadIdx.x >> 6;
  half_pair_list<D>(s_pair, reinterpret_cast<int*>(s_red), 0, 1 << 30);         // the whole stencil: H::NPAIR pairs
  bool bad = false;
  double c_acc = 0, ld_acc = 0;                  // lane 0: this wave's share of the two scalars
  for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {
    const int64_t p = base + loc;
    const bool valid = p < n;
    int j0[D], flat_t[H::TPL];
    real w[D][4], val_t[H::TPL][1], yw[1], wac[1], wu[1], innov[1];
    const bool inside = half_point_setup<real, D>(G, x, p, n, lane == 0, err, bad, j0, w);
    double lo_p = 0, hi_p = 0, v_p = 0, n_p = 1;
    real wap = 0, wbp = 0;
    if (valid) {
      lo_p = (double)lo[p];
      hi_p = (double)hi[p];
      v_p = (double)pvar[p];
      n_p = (double)noise[p];
      wap = wa[p];
      wbp = wb[p];
    }
    half_tap_table<real, D, 1>(G, j0, w, nullptr, lane, u, s_val[loc], s_idx[loc], flat_t, val_t, wu);   // wu: the predictive mean of the point before the batch
    // the site, the same in every lane; a point outside the grid has zero rows and reports omega = 0, ytilde = 0, log Z = 0
    IntervalSite st{0.0, 0.0, 0.0};
    if (inside) st = interval_site(lo_p, hi_p, (double)wu[0], v_p, sigma2 * n_p);
    const bool enters = st.omega > 0.0;
    const real omega = (real)st.omega, yt = (real)st.ytilde;
    wbp *= omega;
    wac[0] = wap * omega;
    yw[0] = yt * wbp;
    half_carry<real, 1>(u, yw, wac, wu, mean_out, p, lane == 0 && valid, innov);   // with the weights the point enters with
    if (lane == 0 && valid) {
      ytilde_out[p] = yt;
      omega_out[p] = omega;
      logz_out[p] = st.logz;
      if (enters) {
        c_acc += st.ytilde * st.ytilde * (double)wbp;
        ld_acc += log(n_p / st.omega);
      }
    }
    half_tap_atomics<real, D, 1>(valid && enters, flat_t, val_t, yw, wac, innov, b, cnt, res);
    __syncthreads();
    if (valid && enters) half_pair_loop<real, D, 1>(lane, H::NPAIR, s_pair, s_val[loc], s_idx[loc], wac, 1, A, G.m);
    __syncthreads();
  }
  stats_atomic_pair(c_acc, ld_acc, stats, s_red);
  if (bad) atomicOr(err, 1);
}

template <typename real>
static int launch_interval(const GridDev<real>& G, const AbsorbArgs<real>& a, hipStream_t stream) {
  int64_t blocks = (a.n + ROBUST_POINTS_PER_BLOCK - 1) / ROBUST_POINTS_PER_BLOCK;     // one atomic pair per block, as launch_robust
  if (blocks > 256 * 8) blocks = 256 * 8;
#define CALL(DD)                                                                                                                                      \
  hipLaunchKernelGGL((k_scatter_stats_interval<real, DD>), dim3((unsigned)blocks), dim3(256), 0, stream, G, a.x, a.lo, a.hi, a.pvar, a.sigma2, a.wa, \
                     a.wb, a.noise, a.n, a.b, a.A, a.stats, a.err, a.cnt, a.u, a.res, a.mean_out, a.ytilde_out, a.omega_out, a.logz_out)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}
