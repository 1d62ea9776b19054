// Interval-observation absorb (AbsorbArgs::lo).  Included by scatter_stats.hip.
//
// A point says y_p = f(x_p) + eps_p lies in [lo_p, hi_p] (either end may be infinite; lo_p == hi_p is an exact value).  It is
// moment-matched against the posterior BEFORE the batch, inside the launch that absorbs it (assumed-density filtering): with
//   mu = w_p . u,  v = pvar_p,  dn = sigma2 noise_p,  s^2 = v + dn,  a = (lo - mu) / s,  b = (hi - mu) / s,  Z = Phi(b) - Phi(a),
//   alpha = d log Z / d mu,   beta = -d^2 log Z / d mu^2,   omega = dn beta / (1 - v beta),   ytilde = mu + alpha / beta
// the point enters as the pseudo-target ytilde at noise noise_p / omega_p, exactly as the robust form (scatter_robust.h) enters a point: A, cnt
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

// The site of the interval form (the sweep and the two scalars are k_scatter_stats_site's, scatter_site.h): the same closed form in
// every lane.  A wave past the batch holds the empty datum, and a site enters where its omega is positive.
template <typename real>
struct SiteInterval : SiteOutputs<real> {
  const real* lo;
  const real* hi;
  const real* pvar;
  const real* noise;
  double sigma2;
  static constexpr bool kGrad = false;
  struct Datum {
    double lo = 0, hi = 0, v = 0, noise = 1;
  };
  static SiteInterval of(const AbsorbArgs<real>& a) { return {{a.ytilde_out, a.omega_out, a.logz_out}, a.lo, a.hi, a.pvar, a.noise, a.sigma2}; }
  __device__ __forceinline__ Datum load(int64_t p) const { return {(double)lo[p], (double)hi[p], (double)pvar[p], (double)noise[p]}; }
  __device__ __forceinline__ SiteValue eval(const Datum& d, real mu, int) const {
    const IntervalSite st = interval_site(d.lo, d.hi, (double)mu, d.v, sigma2 * d.noise);
    return {st.ytilde, st.omega, st.logz, st.omega > 0.0};
  }
};

