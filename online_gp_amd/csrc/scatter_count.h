// Count-observation absorb (AbsorbArgs::count_y).  Included by scatter_stats.hip.
//
// A point carries a count y_p and a second number t_p: y ~ Poisson(t exp f) (family 0, t the exposure) or y successes of t trials at
// success probability sigmoid(f) (family 1).  It is moment-matched against the posterior BEFORE the batch, inside the launch that
// absorbs it, exactly as an interval observation is (scatter_interval.h): with mu = w_p . u, v = max(pvar_p, 0), l the likelihood,
//   Z = int l(f) N(f; mu, v) df,  alpha = d log Z / d mu,  beta = -d^2 log Z / d mu^2,  tau = beta / (1 - v beta),
//   ytilde = mu + alpha / beta,   omega = sigma2 noise_p tau
// and the point enters as the pseudo-target ytilde at noise noise_p / omega_p -- the effective noise variance 1 / tau; omega is NOT
// capped at 1, a count has no Gaussian noise of its own.  Z has no closed form, so the 64 lanes of the point's wave, which in the
// interval kernel all compute the same closed form, are the NODES of a quadrature here (count_site below): eleven fp64 exp per lane
// and six wave reductions per point instead of some 450 exp per lane for the same rule done redundantly.
#pragma once

// A site whose omega falls below this enters nothing (a count that says nothing: y = 0 at a vanishing rate).
#ifndef WISKI_COUNT_OMEGA_MIN
#define WISKI_COUNT_OMEGA_MIN 1e-12
#endif

struct CountSite {
  double ytilde, omega, logz;                     // omega = 0: the point is skipped (ytilde = mu)
};

// A family is its validity test, the constant of log l, and three functions of f: g = log l without the constant, g', g''.  Both
// are log-concave (g'' < 0), which is all count_site relies on; a third family is one more specialisation.
template <int FAM>
struct CountFamily;

template <>
struct CountFamily<WISKI_COUNT_POISSON> {          // l(f) = (t e^f)^y exp(-t e^f) / Gamma(y + 1)
  static __device__ __forceinline__ bool valid(double y, double t) { return y >= 0.0 && t > 0.0 && isfinite(y) && isfinite(t); }
  static __device__ __forceinline__ double constant(double y, double t) { return y * log(t) - lgamma(y + 1.0); }
  static __device__ __forceinline__ double g(double y, double t, double f) { return y * f - t * exp(f); }
  static __device__ __forceinline__ double g1(double y, double t, double f) { return y - t * exp(f); }
  static __device__ __forceinline__ double g2(double y, double t, double f) { return -t * exp(f); }
};

template <>
struct CountFamily<WISKI_COUNT_BINOMIAL> {         // l(f) = C(t, y) s^y (1 - s)^(t - y),  s = 1 / (1 + e^-f);  e = exp(-|f|) never overflows
  static __device__ __forceinline__ bool valid(double y, double t) { return y >= 0.0 && t > 0.0 && y <= t && isfinite(t); }
  static __device__ __forceinline__ double constant(double y, double t) { return lgamma(t + 1.0) - lgamma(y + 1.0) - lgamma(t - y + 1.0); }
  static __device__ __forceinline__ double g(double y, double t, double f) { return y * f - t * (fmax(f, 0.0) + log1p(exp(-fabs(f)))); }
  static __device__ __forceinline__ double g1(double y, double t, double f) {
    const double e = exp(-fabs(f));
    return y - t * (f >= 0.0 ? 1.0 : e) / (1.0 + e);
  }
  static __device__ __forceinline__ double g2(double y, double t, double f) {
    const double e = exp(-fabs(f));
    return -t * e / ((1.0 + e) * (1.0 + e));
  }
};

// The 64-point Gauss-Legendre rule on [-1, 1]: its 32 positive nodes and their weights (the rule is symmetric).
__device__ const double COUNT_GL_X[32] = {0.024350292663424429, 0.072993121787799042, 0.12146281929612056, 0.1696444204239928,
                                          0.21742364374000708,  0.26468716220876742,  0.31132287199021097, 0.35722015833766813,
                                          0.40227015796399163,  0.44636601725346409,  0.48940314570705296, 0.53127946401989457,
                                          0.571895646202634,    0.61115535517239328,  0.64896547125465731, 0.68523631305423327,
                                          0.71988185017161077,  0.75281990726053194,  0.78397235894334139, 0.81326531512279754,
                                          0.84062929625258032,  0.86599939815409277,  0.88931544599511414, 0.91052213707850282,
                                          0.92956917213193957,  0.94641137485840277,  0.96100879965205377, 0.97332682778991098,
                                          0.98333625388462598,  0.99101337147674429,  0.99634011677195522, 0.99930504173577217};
__device__ const double COUNT_GL_W[32] = {0.048690957009139751, 0.048575467441503456,  0.048344762234802954,  0.047999388596458317,
                                          0.047540165714830301, 0.04696818281621,      0.046284796581314375,  0.045491627927418114,
                                          0.044590558163756545, 0.043583724529323464,  0.042473515123653598,  0.041262563242623486,
                                          0.03995374113272035,  0.038550153178615591,  0.037055128540240151,  0.035472213256882323,
                                          0.033805161837141787, 0.032057928354851453,  0.030234657072402495,  0.028339672614259702,
                                          0.026377469715054627, 0.024352702568710853,  0.022270173808383007,  0.020134823153530094,
                                          0.017951715775697302, 0.015726030476025082,  0.013463047896718231,  0.011168139460131466,
                                          0.008846759826364391, 0.0065044579689796543, 0.0041470332605629233, 0.0017832807216942152};

constexpr int COUNT_SECTION_PASSES = 4, COUNT_NEWTON_STEPS = 2;
constexpr double COUNT_DROP = 40.0;                // the bracket ends where the log integrand has fallen by this much: e^-40 = 4e-18
constexpr double COUNT_LADDER = 1.3;               // ratio of the bracket ladder: 32 rungs span a factor 3 400

// D / COUNT_LADDER^k, 0 <= k < 64
__device__ __forceinline__ double count_rung(double D, int k) {
  double r = 1.0 / COUNT_LADDER;
#pragma unroll
  for (int bit = 0; bit < 6; ++bit) {
    if ((k >> bit) & 1) D *= r;
    r *= r;
  }
  return D;
}

// The site of one point, evaluated by its wave: every argument is wave-uniform, `lane` is the lane, and the result is the same in
// every lane.  In fp64 whatever the working precision.  h(f) = g(f) - (f - mu)^2 / 2v is the log integrand, concave.
//   1. The mode c of h lies between mu and mu + v g'(mu) (g' decreases).  Each sectioning pass puts the 64 lanes on the bracket, counts
//      with a ballot those with h' still on mu's side, and keeps that sixty-fourth; four passes shrink the bracket by 1.7e7, two
//      wave-uniform Newton steps finish.  The quadrature is split AT c, so c need not be the mode to rounding.
//   2. -h'' >= 1 / v, so h has fallen by COUNT_DROP within D = sqrt(2 COUNT_DROP v) of c on either side.  Lanes 0..31 look left and
//      32..63 right: rung k of a geometric ladder down from D, a ballot for the last rung that still reaches the drop, then 32 even
//      steps between that rung and the next, a second ballot: the bracket ends within 1 % of where h = h(c) - COUNT_DROP.
//   3. Two nodes per lane: the 64-point Gauss-Legendre rule on [c - e_left, c] and again on [c, c + e_right] -- a skewed integrand
//      (y = 0 under a wide prior: Gaussian to the left, doubly exponential to the right) is smooth on each side, and no trapezoid end
//      correction meets the other side's at c.  32 nodes a side leave 3e-9 on the binomial at v = 9 (the poles of the logistic at
//      +- i pi bound the rate), 64 leave rounding.  Six sums reduced over the wave, in units of exp(h(c)): nothing over- or underflows.
//   4. tau from the moments of g' and g'' (beta = -E g'' - Var g') where v beta < 1/2: a weak site, where 1 / Vhat - 1 / v would
//      cancel; from the moments of f (tau = 1 / Vhat - 1 / v) otherwise: a sharp one, where 1 - v beta would.
// v = 0 is the Laplace site at mu.  An invalid datum (log Z = NaN), a beta that is not positive and finite, an omega below
// WISKI_COUNT_OMEGA_MIN: the point is skipped.
template <int FAM>
__device__ __forceinline__ CountSite count_site(double y, double t, double mu, double v, double dn, int lane) {
  using F = CountFamily<FAM>;
  constexpr double HALF_LOG_2PI = 0.91893853320467274178;
  CountSite r{mu, 0.0, NAN};
  if (!F::valid(y, t) || !(mu == mu) || !(v == v)) return r;           // wave-uniform, as every branch below
  v = v > 0.0 ? v : 0.0;
  const double k0 = F::constant(y, t);
  double tau, alpha, beta;
  if (v == 0.0) {
    alpha = F::g1(y, t, mu);
    tau = beta = -F::g2(y, t, mu);
    r.logz = F::g(y, t, mu) + k0;
  } else {
    const double iv = 1.0 / v;
    // 1. the mode
    const double d0 = F::g1(y, t, mu);
    const bool up = d0 >= 0.0;
    double a = mu, W = v * d0;
#pragma unroll 1
    for (int pass = 0; pass < COUNT_SECTION_PASSES; ++pass) {
      const double x = a + W * (double)(lane + 1) * (1.0 / 64.0);
      const double dh = F::g1(y, t, x) - (x - mu) * iv;
      const int k = __popcll(__ballot(up ? dh > 0.0 : dh < 0.0));
      a += W * (double)k * (1.0 / 64.0);
      W *= 1.0 / 64.0;
    }
    double c = a + 0.5 * W;
#pragma unroll 1
    for (int it = 0; it < COUNT_NEWTON_STEPS; ++it) c -= (F::g1(y, t, c) - (c - mu) * iv) / (F::g2(y, t, c) - iv);
    const double g1c = F::g1(y, t, c);
    const double hc = F::g(y, t, c) - 0.5 * (c - mu) * (c - mu) * iv;
    // 2. the bracket
    const bool right = lane >= 32;
    const int k = lane & 31;
    const double side = right ? 1.0 : -1.0;
    const double D = sqrt(2.0 * COUNT_DROP * v);
    double e;
    {
      const double d = count_rung(D, k);
      const double f = c + side * d;
      const unsigned long long reach = __ballot(hc - (F::g(y, t, f) - 0.5 * (f - mu) * (f - mu) * iv) >= COUNT_DROP);
      const int n_ok = __popc(right ? (unsigned)(reach >> 32) : (unsigned)reach);   // the rungs 0 .. n_ok - 1 reach the drop
      const double outer = count_rung(D, n_ok > 0 ? n_ok - 1 : 0);
      const double inner = n_ok > 0 ? outer * (1.0 / COUNT_LADDER) : outer;
      const double width = outer - inner;
      const double f2 = c + side * (inner + width * (double)(k + 1) * (1.0 / 32.0));
      const unsigned long long miss = __ballot(hc - (F::g(y, t, f2) - 0.5 * (f2 - mu) * (f2 - mu) * iv) < COUNT_DROP);
      const int n_short = __popc(right ? (unsigned)(miss >> 32) : (unsigned)miss);
      e = inner + width * (double)((n_short < 31 ? n_short : 31) + 1) * (1.0 / 32.0);
    }
    // 3. the nodes: the pair -+ xi_k of the 64-point rule on the lane's side
    const double half = 0.5 * e, gw = half * COUNT_GL_W[k], gx = COUNT_GL_X[k];
    double s0 = 0, s1 = 0, s2 = 0, q1 = 0, q2 = 0, hh = 0;
#pragma unroll 1
    for (int j = 0; j < 2; ++j) {
      const double x = half * (j ? 1.0 + gx : 1.0 - gx);                  // distance from c
      const double f = c + side * x;
      const double w = gw * exp(F::g(y, t, f) - 0.5 * (f - mu) * (f - mu) * iv - hc);
      const double dg = F::g1(y, t, f) - g1c;
      s0 += w;
      s1 += w * side * x;
      s2 += w * x * x;
      q1 += w * dg;
      q2 += w * dg * dg;
      hh += w * F::g2(y, t, f);
    }
    const double S0 = wave_reduce_sum<double>(s0), iS = 1.0 / S0;
    const double S1 = wave_reduce_sum<double>(s1) * iS, S2 = wave_reduce_sum<double>(s2) * iS;
    const double G1 = wave_reduce_sum<double>(q1) * iS, G2 = wave_reduce_sum<double>(q2) * iS;
    const double H2 = wave_reduce_sum<double>(hh) * iS;
    r.logz = hc + k0 + log(S0) - 0.5 * log(v) - HALF_LOG_2PI;
    // 4. the site
    const double beta_w = -H2 - (G2 - G1 * G1);
    if (v * beta_w < 0.5) {
      beta = beta_w;
      alpha = g1c + G1;
      tau = beta / (1.0 - v * beta);
    } else {
      const double V = S2 - S1 * S1;
      tau = 1.0 / V - iv;
      beta = (v - V) * iv * iv;
      alpha = (c + S1 - mu) * iv;
    }
  }
  if (!(beta > 0.0) || !isfinite(beta)) return r;
  const double omega = dn * tau;
  if (!(omega >= WISKI_COUNT_OMEGA_MIN) || !isfinite(omega)) return r;
  r.omega = omega;
  r.ytilde = mu + alpha / beta;
  return r;
}

__device__ __forceinline__ CountSite count_site_of(int family, double y, double t, double mu, double v, double dn, int lane) {
  return family == WISKI_COUNT_POISSON ? count_site<WISKI_COUNT_POISSON>(y, t, mu, v, dn, lane)
                                       : count_site<WISKI_COUNT_BINOMIAL>(y, t, mu, v, dn, lane);
}

// The site of the count form (the sweep and the two scalars are k_scatter_stats_site's, scatter_site.h).  A wave past the batch holds
// an invalid datum (count_site's early return), and a site enters where its omega is positive.
template <typename real>
struct SiteCount : SiteOutputs<real> {
  const real* cy;
  const real* ct;
  const real* pvar;
  const real* noise;
  int family;
  double sigma2;
  static constexpr bool kGrad = false;
  struct Datum {
    double y = -1.0, t = 0, v = 0, noise = 1;
  };
  static SiteCount of(const AbsorbArgs<real>& a) { return {{a.ytilde_out, a.omega_out, a.logz_out}, a.count_y, a.count_t, a.pvar, a.noise, a.count_family, a.sigma2}; }
  __device__ __forceinline__ Datum load(int64_t p) const { return {(double)cy[p], (double)ct[p], (double)pvar[p], (double)noise[p]}; }
  __device__ __forceinline__ SiteValue eval(const Datum& d, real mu, int lane) const {
    const CountSite st = count_site_of(family, d.y, d.t, (double)mu, d.v, sigma2 * d.noise, lane);
    return {st.ytilde, st.omega, st.logz, st.omega > 0.0};
  }
};

// Sites only (wiski_count_sites): one wave per site, four per block, the same count_site; omega = tau (no noise scale).
// FAM < 0: the family is the run-time argument (Poisson or binomial); FAM >= 0: that family alone, `family` is not looked at
// (wiski_hetero_sites, scatter_hetero.h: its family is no count and the count entries do not take it).
template <typename real, int FAM = -1>
__global__ __launch_bounds__(256) void k_count_sites(const real* __restrict__ mu, const real* __restrict__ pvar, const real* __restrict__ cy,
                                                     const real* __restrict__ ct, int family, int64_t n, real* __restrict__ ytilde_out,
                                                     real* __restrict__ omega_out, double* __restrict__ logz_out) {
  const int lane = threadIdx.x & 63;
  for (int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); p < n; p += (int64_t)gridDim.x * 4) {   // (wave-uniform trip count)
    CountSite st;
    if constexpr (FAM < 0) st = count_site_of(family, (double)cy[p], (double)ct[p], (double)mu[p], (double)pvar[p], 1.0, lane);
    else st = count_site<FAM>((double)cy[p], (double)ct[p], (double)mu[p], (double)pvar[p], 1.0, lane);
    if (lane == 0) {
      ytilde_out[p] = (real)st.ytilde;
      omega_out[p] = (real)st.omega;
      logz_out[p] = st.logz;
    }
  }
}

template <typename real, int FAM = -1>
static int count_sites_impl(const real* mu, const real* pvar, const real* y, const real* t, int family, int64_t n, real* ytilde_out, real* omega_out,
                            double* logz_out, void* stream) {
  if (n == 0) return WISKI_OK;
  if (n < 0 || !mu || !pvar || !y || !t || !ytilde_out || !omega_out || !logz_out) return WISKI_E_BADARG;
  if (FAM < 0 && family != WISKI_COUNT_POISSON && family != WISKI_COUNT_BINOMIAL) return WISKI_E_BADARG;
  int64_t blocks = (n + 3) / 4;
  if (blocks > 256 * 8) blocks = 256 * 8;
  hipLaunchKernelGGL((k_count_sites<real, FAM>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mu, pvar, y, t, family, n, ytilde_out, omega_out,
                     logz_out);
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}
