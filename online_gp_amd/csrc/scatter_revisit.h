// Revisiting stored sites (AbsorbArgs::site_codes).  Included by scatter_stats.hip.
//
// The moment-matched forms (scatter_interval.h, scatter_count.h) match a point once, against the posterior before its batch, and
// never look at it again (assumed-density filtering).  A ring of `cap` slots on the device remembers such points -- x, the two data
// numbers (d0, d1) = (lo, hi) or (count, exposure / trials), a form code, noise, wa, wb and the site (ytilde, omega) the point is in
// the statistics with -- and ONE launch per form re-matches every stored site of that form against its CAVITY and scatters only
// the difference (an expectation-propagation sweep).  With dn = sigma2 noise, tau = omega / dn, nu = tau ytilde, and (mu, v) the
// marginal of f(x) under the CURRENT statistics (mu = w . u, v = pvar),
//   cavity:  p = 1 / v - tau,  v_ = 1 / p,  mu_ = v_ (mu / v - nu)
//   fresh:   (ytilde', omega', log Z') = the form's site function at (mu_, v_, dn)
//   damped:  tau_new = (1 - delta) tau + delta omega' / dn,  nu_new = (1 - delta) nu + delta (omega' / dn) ytilde',
//            omega_new = dn tau_new (below the form's OMEGA_MIN: exactly 0, the point leaves, ytilde_new = mu),  ytilde_new = nu_new / tau_new
// and the slot enters with the coefficients wa (omega_new - omega_old) and wb (omega_new ytilde_new - omega_old ytilde_old): one sweep
// of scatter_half.h.  The deltas are formed from the values as the ring stores them (rounded to the working precision), so the
// statistics stay the sums over the ring's sites exactly as a later sweep reads them.  All slots of a sweep are taken against the
// same u and pvar (parallel EP): the result depends neither on the order of the slots nor on the order of the atomics.
//
// Per slot s, the order of steps is that of k_scatter_stats_window: lane 0 reads the slot, the wave receives it (wave_first), runs one
// tap table and reduces w . u, computes cavity, site and damping in fp64 -- wave-uniform, so the count forms' quadrature over the
// lanes applies as it stands --, makes the one delta sweep, and lane 0 writes the slot's new (ytilde, omega).  The only reader and the
// only writer of a slot's site is lane 0 of one wave, in program order: nothing is assumed about the order of waves or blocks.
//
// A slot is left exactly as it is -- no atomic, no store to the ring, change 0 -- when it is empty or of another form (for those not
// even the outputs are written: the launches of a sweep share them), when its point lies outside the grid (no flag: the window's rule
// for a stored point), when it holds an exact value (d0 == d1 of the interval form: its site is exact whatever the cavity), when v is
// not positive and finite, when the cavity precision p is not above REVISIT_CAVITY_MIN / v (a difference of two precisions: below that
// relative size it is the rounding of pvar), or when delta = 0.
#pragma once

#ifndef WISKI_REVISIT_CAVITY_MIN
#define WISKI_REVISIT_CAVITY_MIN 1e-4
#endif

template <typename real>
struct SiteRingDev {
  const real* x;
  const real* d0;
  const real* d1;
  const real* noise;
  const real* wa;
  const real* wb;
  real* ytilde;
  real* omega;
  const int32_t* form;
  int64_t cap;
};

// the fresh site of one form at the cavity; every argument wave-uniform, the result the same in every lane
template <int FORM>
__device__ __forceinline__ SiteValue revisit_site(double d0, double d1, double mu, double v, double dn, int lane) {
  if constexpr (FORM == WISKI_SITE_INTERVAL) {
    const IntervalSite st = interval_site(d0, d1, mu, v, dn);
    return {st.ytilde, st.omega, st.logz, st.omega > 0.0};
  } else {
    constexpr int FAM = FORM == WISKI_SITE_POISSON ? WISKI_COUNT_POISSON : WISKI_COUNT_BINOMIAL;
    const CountSite st = count_site<FAM>(d0, d1, mu, v, dn, lane);
    return {st.ytilde, st.omega, st.logz, st.omega > 0.0};
  }
}

template <int FORM>
constexpr double revisit_omega_min() { return FORM == WISKI_SITE_INTERVAL ? WISKI_INTERVAL_OMEGA_MIN : WISKI_COUNT_OMEGA_MIN; }

// The point sweep is that of k_scatter_stats_sym (scatter_half.h), taken once per slot with the delta coefficients.  No guard, zero
// regions, shard or batch (absorb_validate).  The two scalars: each wave keeps, in fp64, the change of omega wb ytilde^2 and of
// log(noise / omega) of its slots (lane 0 holds them) and a block issues one atomic pair when it is done, as in the window form.
template <typename real, int D, int FORM>
__global__ __launch_bounds__(256) void k_scatter_stats_revisit(GridDev<real> G, SiteRingDev<real> R, const real* __restrict__ pvar, double sigma2,
                                                               double damping, real* __restrict__ b, real* __restrict__ A,
                                                               double* __restrict__ stats, real* __restrict__ cnt, const real* __restrict__ u,
                                                               real* __restrict__ res, double* __restrict__ logz_out, real* __restrict__ change_out) {
  using H = HalfTaps<D>;
  __shared__ real s_val[4][H::T];
  __shared__ int s_idx[4][H::T];
  __shared__ int s_pair[H::NPAIR];
  __shared__ double s_red[16];
  const int lane = threadIdx.x & 63, loc = threadIdx.x >> 6;
  half_pair_list<D>(s_pair, reinterpret_cast<int*>(s_red), 0, 1 << 30);         // the whole stencil: H::NPAIR pairs
  double c_acc = 0, ld_acc = 0;                  // lane 0: this wave's share of the two scalars
  for (int64_t base = (int64_t)blockIdx.x * 4; base < R.cap; base += (int64_t)gridDim.x * 4) {
    const int64_t s = base + loc;
    int j0[D], flat_t[H::TPL];
    real w[D][4], val_t[H::TPL][1], yw[1], wac[1], wu[1], innov[1];
    // 1. the slot, read by the one lane that also writes it
    int fs = WISKI_SITE_EMPTY;
    real sx[D], sd0 = 0, sd1 = 0, snz = 1, swa = 0, swb = 0, syt = 0, som = 0, sv = 0;
#pragma unroll
    for (int q = 0; q < D; ++q) sx[q] = 0;
    if (s < R.cap && lane == 0) {
      fs = R.form[s];
      if (fs == FORM) {
#pragma unroll
        for (int q = 0; q < D; ++q) sx[q] = R.x[s * D + q];
        sd0 = R.d0[s];
        sd1 = R.d1[s];
        snz = R.noise[s];
        swa = R.wa[s];
        swb = R.wb[s];
        syt = R.ytilde[s];
        som = R.omega[s];
        sv = pvar[s];
      }
    }
    const bool mine = __builtin_amdgcn_readfirstlane(fs) == FORM;          // (a wave past the ring: lane 0 read nothing)
#pragma unroll
    for (int q = 0; q < D; ++q) sx[q] = wave_first(sx[q]);
    sd0 = wave_first(sd0);
    sd1 = wave_first(sd1);
    snz = wave_first(snz);
    swa = wave_first(swa);
    swb = wave_first(swb);
    syt = wave_first(syt);
    som = wave_first(som);
    sv = wave_first(sv);
    // 2. the slot's stencil and mu = w . u (zero weights, and no read of u, for a slot that is not this launch's)
    bool gone = false;                           // a stored point the grid does not contain is left alone and raises no flag
    const bool inside = half_point_setup<real, D>(G, sx, 0, mine ? 1 : 0, false, nullptr, gone, j0, w);
    half_tap_table<real, D, 1>(G, j0, w, nullptr, lane, u, s_val[loc], s_idx[loc], flat_t, val_t, wu);
    // 3. cavity, fresh site, damping: fp64 and wave-uniform
    const double mu = (double)wu[0], v = (double)sv, dn = sigma2 * (double)snz;
    const double o_old = (double)som, y_old = (double)syt;
    const double tau = o_old / dn, nu = tau * y_old;
    const double p = 1.0 / v - tau;
    bool touch = inside && damping != 0.0 && v > 0.0 && isfinite(v) && p > WISKI_REVISIT_CAVITY_MIN / v;
    if (FORM == WISKI_SITE_INTERVAL && sd0 == sd1) touch = false;
    double o_new = o_old, y_new = y_old, logz = NAN;
    if (touch) {
      const double vc = 1.0 / p, muc = vc * (mu / v - nu);
      const SiteValue st = revisit_site<FORM>((double)sd0, (double)sd1, muc, vc, dn, lane);
      const double tf = st.omega / dn;
      const double tau_new = (1.0 - damping) * tau + damping * tf;
      const double nu_new = (1.0 - damping) * nu + damping * tf * st.ytilde;
      const double on = dn * tau_new;
      logz = st.logz;
      if (on >= revisit_omega_min<FORM>() && isfinite(on)) {
        o_new = (double)(real)on;                // as the ring stores them: the statistics hold what a later sweep takes out
        y_new = (double)(real)(nu_new / tau_new);
      } else {
        o_new = 0.0;
        y_new = (double)(real)mu;
      }
    }
    // 4. the one delta sweep
    const double dwo = o_new - o_old, dwy = o_new * y_new - o_old * y_old;
    const bool moved = touch && (dwo != 0.0 || dwy != 0.0);
    wac[0] = (real)((double)swa * dwo);
    yw[0] = (real)((double)swb * dwy);
    half_carry<real, 1>(u, yw, wac, wu, nullptr, 0, false, innov);
    if (mine && lane == 0) {
      if (touch) {
        R.ytilde[s] = (real)y_new;
        R.omega[s] = (real)o_new;
        c_acc += (double)swb * (o_new * y_new * y_new - o_old * y_old * y_old);
        ld_acc += (o_new > 0.0 ? log((double)snz / o_new) : 0.0) - (o_old > 0.0 ? log((double)snz / o_old) : 0.0);
      }
      const double big = o_new > o_old ? o_new : o_old;
      change_out[s] = (real)(touch && big > 0.0 ? fabs(dwo) / big : 0.0);
      logz_out[s] = logz;
    }
    half_tap_atomics<real, D, 1>(moved, flat_t, val_t, yw, wac, innov, b, cnt, res);
    __syncthreads();
    if (moved) half_pair_loop<real, D, 1>(lane, H::NPAIR, s_pair, s_val[loc], s_idx[loc], wac, 1, A, G.m);
    __syncthreads();
  }
  stats_atomic_pair(c_acc, ld_acc, stats, s_red);
}

// Slots a block takes: the window form's reasoning (WINDOW_POINTS_PER_BLOCK, WINDOW_MIN_BLOCKS) with one sweep per pass.
template <typename real, int FORM>
static int launch_revisit_form(const GridDev<real>& G, const AbsorbArgs<real>& a, const SiteRingDev<real>& R, int64_t blocks, hipStream_t stream) {
#define CALL(DD)                                                                                                                                  \
  hipLaunchKernelGGL((k_scatter_stats_revisit<real, DD, FORM>), dim3((unsigned)blocks), dim3(256), 0, stream, G, R, a.pvar, a.sigma2, a.site_damping, \
                     a.b, a.A, a.stats, a.cnt, a.u, a.res, a.logz_out, a.site_change_out)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

template <typename real>
static int launch_revisit(const GridDev<real>& G, const AbsorbArgs<real>& a, hipStream_t stream) {
  int64_t blocks = (a.n + WINDOW_POINTS_PER_BLOCK - 1) / WINDOW_POINTS_PER_BLOCK;
  const int64_t one_pass = (a.n + 3) / 4;
  if (blocks < WINDOW_MIN_BLOCKS) blocks = one_pass < WINDOW_MIN_BLOCKS ? one_pass : WINDOW_MIN_BLOCKS;
  if (blocks > 256 * 8) blocks = 256 * 8;
  const SiteRingDev<real> R{a.x, a.site_d0, a.site_d1, a.noise, a.wa, a.wb, a.site_ytilde, a.site_omega, a.site_codes, a.n};
  switch (a.site_form_code) {
    case WISKI_SITE_INTERVAL: return launch_revisit_form<real, WISKI_SITE_INTERVAL>(G, a, R, blocks, stream);
    case WISKI_SITE_POISSON: return launch_revisit_form<real, WISKI_SITE_POISSON>(G, a, R, blocks, stream);
    case WISKI_SITE_BINOMIAL: return launch_revisit_form<real, WISKI_SITE_BINOMIAL>(G, a, R, blocks, stream);
  }
  return WISKI_E_BADARG;
}
