// Categorical-observation absorb: multinomial probit sites over the C outputs of a point.  Included by
// scatter_stats.hip, after scatter_count.h (whose Gauss-Legendre table and bracket constants it reuses).
//
// A point carries a label y_p in {0 .. C - 1}: y = argmax_c (f_c(x) + eps_c), eps_c ~ N(0, s_c), s_c = sigma2_c noise_c,p.  Against the
// posterior BEFORE the batch -- mu_c = w_p . u_c, v_c = max(pvar_c,p, 0), a_c = v_c + s_c > 0, z_c(t) = (t - mu_c) / sqrt a_c,
// r = phi / Phi --
//   Z = int N(t; mu_y, a_y) prod_{c != y} Phi(z_c(t)) dt,               E[.] under the normalised integrand (log-concave in t)
//   c = y:   alpha = (E t - mu_y) / a_y = E g',    beta = 1 / a_y - Var t / a_y^2 = -E g'' - Var g',   g(t) = sum_{c != y} log Phi(z_c(t))
//   c != y:  alpha = -E r(z_c) / sqrt a_c,         beta = (E[r (r + z_c)] - Var r) / a_c
//   tau_c = beta_c / (1 - v_c beta_c),  ytilde_c = mu_c + alpha_c / beta_c,  omega_c = s_c tau_c
// and output c takes the point as ytilde_c at noise noise_c,p / omega_c.  This is the first form that couples outputs: the wave of a
// point needs all C means before it can weight any of them, so it is a kernel of its own and not a Site of k_scatter_stats_site.
// The integral is count_site's (scatter_count.h) with g above and N(mu_y, a_y) for N(mu, v): the 64 lanes are its nodes.  Class c of
// a point lives in lane c of its wave (mean, variances, site, the two scalars' share); what every lane reads of every class (mu_c,
// a_c, 1 / sqrt a_c) lies in LDS, written by lane c.  No lane holds a per-class array.
#pragma once

struct LabelSigma {
  double v[WISKI_LABEL_MAX_CLASSES];              // sigma2 of each output (HOST values, passed by value)
};

// log Phi(z) and r(z) = phi(z) / Phi(z), both to rounding for z -> -inf (erfcx: Phi(z) = erfcx(-z / sqrt 2) exp(-z^2 / 2) / 2)
__device__ __forceinline__ void label_phi(double z, double& lp, double& r) {
  constexpr double INV_SQRT2 = 0.70710678118654752440, SQRT_2_OVER_PI = 0.79788456080286535588, INV_SQRT_2PI = 0.39894228040143267794;
  if (z < 0.0) {
    const double e = erfcx(-z * INV_SQRT2);
    r = SQRT_2_OVER_PI / e;
    lp = log(0.5 * e) - 0.5 * z * z;
  } else {
    const double q = 0.5 * erfc(z * INV_SQRT2);
    lp = log1p(-q);
    r = INV_SQRT_2PI * exp(-0.5 * z * z) / (1.0 - q);
  }
}

// g(t) = sum_{c != y} log Phi(z_c(t)) with g' > 0 and g'' < 0
__device__ __forceinline__ void label_g(int C, int y, const double* s_mu, const double* s_isa, double t, double& g, double& g1, double& g2) {
  g = 0.0;
  g1 = 0.0;
  g2 = 0.0;
#pragma unroll 1
  for (int c = 0; c < C; ++c) {
    if (c == y) continue;
    const double ic = s_isa[c], z = (t - s_mu[c]) * ic;
    double lp, r;
    label_phi(z, lp, r);
    g += lp;
    g1 += r * ic;
    g2 -= r * (r + z) * ic * ic;
  }
}

// The evidence of label y and, with DERIV, its derivatives, evaluated by one wave: C, y and the LDS rows s_mu / s_a / s_isa [C]
// (mu_c, a_c, 1 / sqrt a_c) are wave-uniform and finite, a_c > 0.  Returns log Z in every lane; lane c < C receives alpha_c and
// beta_c.  The scheme is count_site's, step for step (mode by sectioning between mu_y and mu_y + a_y g'(mu_y), bracket by ballot,
// the 64-point Gauss-Legendre rule on each side of the mode), without its v = 0 branch: a_y > 0.  The label class takes count_site's
// two branches (moments of g' and g'' for a weak site, moments of t for a sharp one); another class reduces, in a second sweep over
// the classes, the sums of dr = r - r(mode) and of r (r + z) - dr^2, so that beta_c a_c = E[r (r + z) - dr^2] + (E dr)^2 is a sum of
// terms that do not cancel.  6 + 2 (C - 1) wave reductions.
template <bool DERIV>
__device__ __forceinline__ double label_site(int C, int y, const double* s_mu, const double* s_a, const double* s_isa, int lane, double& alpha_l,
                                             double& beta_l) {
  constexpr double HALF_LOG_2PI = 0.91893853320467274178;
  const double mu = s_mu[y], v = s_a[y], iv = 1.0 / v;
  double g0, d0, h0;
  label_g(C, y, s_mu, s_isa, mu, g0, d0, h0);
  // 1. the mode
  double a = mu, W = v * d0;
#pragma unroll 1
  for (int pass = 0; pass < COUNT_SECTION_PASSES; ++pass) {
    const double x = a + W * (double)(lane + 1) * (1.0 / 64.0);
    double gx, g1x, g2x;
    label_g(C, y, s_mu, s_isa, x, gx, g1x, g2x);
    const int k = __popcll(__ballot(g1x - (x - mu) * iv > 0.0));
    a += W * (double)k * (1.0 / 64.0);
    W *= 1.0 / 64.0;
  }
  double c = a + 0.5 * W, gc, g1c, g2c;
#pragma unroll 1
  for (int it = 0; it <= COUNT_NEWTON_STEPS; ++it) {
    label_g(C, y, s_mu, s_isa, c, gc, g1c, g2c);
    if (it < COUNT_NEWTON_STEPS) c -= (g1c - (c - mu) * iv) / (g2c - iv);
  }
  const double hc = gc - 0.5 * (c - mu) * (c - mu) * iv;
  // 2. the bracket
  const bool right = lane >= 32;
  const int k = lane & 31;
  const double side = right ? 1.0 : -1.0;
  const double Dd = sqrt(2.0 * COUNT_DROP * v);
  double e;
  {
    double outer = 0, inner = 0, width = 0;
#pragma unroll 1
    for (int stage = 0; stage < 2; ++stage) {
      const double dist = stage == 0 ? count_rung(Dd, k) : inner + width * (double)(k + 1) * (1.0 / 32.0);
      const double f = c + side * dist;
      double gf, g1f, g2f;
      label_g(C, y, s_mu, s_isa, f, gf, g1f, g2f);
      const double drop = hc - (gf - 0.5 * (f - mu) * (f - mu) * iv);
      if (stage == 0) {
        const unsigned long long reach = __ballot(drop >= COUNT_DROP);
        const int n_ok = __popc(right ? (unsigned)(reach >> 32) : (unsigned)reach);   // the rungs 0 .. n_ok - 1 reach the drop
        outer = count_rung(Dd, n_ok > 0 ? n_ok - 1 : 0);
        inner = n_ok > 0 ? outer * (1.0 / COUNT_LADDER) : outer;
        width = outer - inner;
      } else {
        const unsigned long long miss = __ballot(drop < COUNT_DROP);
        const int n_short = __popc(right ? (unsigned)(miss >> 32) : (unsigned)miss);
        e = inner + width * (double)((n_short < 31 ? n_short : 31) + 1) * (1.0 / 32.0);
      }
    }
  }
  // 3. the nodes: the pair -+ xi_k of the 64-point rule on the lane's side
  const double half = 0.5 * e, gw = half * COUNT_GL_W[k], gx = COUNT_GL_X[k];
  double tn[2], wn[2];
  double s0 = 0, s1 = 0, s2 = 0, q1 = 0, q2 = 0, hh = 0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const double x = half * (j ? 1.0 + gx : 1.0 - gx);                    // distance from c
    const double f = c + side * x;
    double gf, g1f, g2f;
    label_g(C, y, s_mu, s_isa, f, gf, g1f, g2f);
    const double w = gw * exp(gf - 0.5 * (f - mu) * (f - mu) * iv - hc);
    const double dg = g1f - g1c;
    tn[j] = f;
    wn[j] = w;
    s0 += w;
    s1 += w * side * x;
    s2 += w * x * x;
    q1 += w * dg;
    q2 += w * dg * dg;
    hh += w * g2f;
  }
  const double S0 = wave_reduce_sum<double>(s0), iS = 1.0 / S0;
  const double logz = hc + log(S0) - 0.5 * log(v) - HALF_LOG_2PI;
  if constexpr (DERIV) {
    const double S1 = wave_reduce_sum<double>(s1) * iS, S2 = wave_reduce_sum<double>(s2) * iS;
    const double G1 = wave_reduce_sum<double>(q1) * iS, G2 = wave_reduce_sum<double>(q2) * iS;
    const double H2 = wave_reduce_sum<double>(hh) * iS;
    // 4. the label's class
    double al, be;
    const double beta_w = -H2 - (G2 - G1 * G1);
    if (v * beta_w < 0.5) {
      be = beta_w;
      al = g1c + G1;
    } else {
      const double V = S2 - S1 * S1;
      be = (v - V) * iv * iv;
      al = (c + S1 - mu) * iv;
    }
    if (lane == y) {
      alpha_l = al;
      beta_l = be;
    }
    // 5. the other classes
#pragma unroll 1
    for (int cc = 0; cc < C; ++cc) {
      if (cc == y) continue;
      const double ic = s_isa[cc], mc = s_mu[cc];
      double lp, r0;
      label_phi((c - mc) * ic, lp, r0);
      double p1 = 0, p2 = 0;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const double z = (tn[j] - mc) * ic;
        double r;
        label_phi(z, lp, r);
        const double dr = r - r0;
        p1 += wn[j] * dr;
        p2 += wn[j] * (r * (r + z) - dr * dr);
      }
      const double P1 = wave_reduce_sum<double>(p1) * iS, P2 = wave_reduce_sum<double>(p2) * iS;
      if (lane == cc) {
        alpha_l = -(r0 + P1) * ic;
        beta_l = (P2 + P1 * P1) * ic * ic;
      }
    }
  }
  return logz;
}

// What lane c makes of its class's alpha, beta: the site (ytilde, omega) of output c at latent variance v and scale dn (omega = dn tau).
// omega = 0, ytilde = mu: the site is skipped for this output (beta not positive and finite, omega below WISKI_COUNT_OMEGA_MIN).
__device__ __forceinline__ void label_finish(double mu, double v, double dn, double alpha, double beta, double& ytilde, double& omega) {
  ytilde = mu;
  omega = 0.0;
  if (!(beta > 0.0) || !isfinite(beta)) return;
  const double om = dn * beta / (1.0 - v * beta);
  if (!(om >= WISKI_COUNT_OMEGA_MIN) || !isfinite(om)) return;
  omega = om;
  ytilde = mu + alpha / beta;
}

// The label of a point as a class, or -1: not an integer in [0, C), or NaN.
__device__ __forceinline__ int label_class(double lab, int C) { return lab >= 0.0 && lab < (double)C && lab == floor(lab) ? (int)lab : -1; }

// Lane c < C publishes its class to the wave's LDS rows; true (in every lane): the point can be evaluated -- a valid label, and every
// class finite with a_c > 0.
__device__ __forceinline__ bool label_publish(int C, int y, int lane, double mu_l, double a_l, double* s_mu, double* s_a, double* s_isa) {
  bool bad_l = false;
  if (lane < C) {
    s_mu[lane] = mu_l;
    s_a[lane] = a_l;
    s_isa[lane] = 1.0 / sqrt(a_l);
    bad_l = !(isfinite(mu_l) && isfinite(a_l) && a_l > 0.0);
  }
  return y >= 0 && __ballot(bad_l) == 0ull;
}

// The absorb.  One wave per point, four per block, the block loop of k_scatter_stats_site: the point is set up and its tap table
// built ONCE (it is the same for every output), the C means are reduced over the wave from u + c m, the wave evaluates the sites, and
// for each output whose site enters it runs the tap atomics and the pair loop into that output's statistics.  An invalid label skips
// the point for every output (log Z = NaN, no flag); a point outside the grid is dropped for every output and counted once.
// wa / wb / noise of output c are at + c w_stride (0: shared), pvar / ytilde_out / omega_out / mean_out are [C][n], logz_out [n].
template <typename real, int D>
__global__ __launch_bounds__(256) void k_scatter_stats_label(GridDev<real> G, const real* __restrict__ x, const real* __restrict__ labels,
                                                             const real* __restrict__ pvar, LabelSigma sig, int C, const real* __restrict__ wa,
                                                             const real* __restrict__ wb, const real* __restrict__ noise, int64_t w_stride,
                                                             int64_t n, real* __restrict__ b, real* __restrict__ A, int64_t A_stride,
                                                             double* __restrict__ stats, int32_t* __restrict__ err, real* __restrict__ cnt,
                                                             const real* __restrict__ u, real* __restrict__ res, real* __restrict__ mean_out,
                                                             real* __restrict__ ytilde_out, real* __restrict__ omega_out,
                                                             double* __restrict__ logz_out) {
  using H = HalfTaps<D>;
  __shared__ real s_val[4][H::T];
  __shared__ int s_idx[4][H::T];
  __shared__ int s_pair[H::NPAIR];
  __shared__ double s_red[16];
  __shared__ double s_mu[4][WISKI_LABEL_MAX_CLASSES], s_a[4][WISKI_LABEL_MAX_CLASSES], s_isa[4][WISKI_LABEL_MAX_CLASSES];
  __shared__ double s_stat[4][WISKI_LABEL_MAX_CLASSES][2];
  const int lane = threadIdx.x & 63, loc = threadIdx.x >> 6;
  half_pair_list<D>(s_pair, reinterpret_cast<int*>(s_red), 0, 1 << 30);         // the whole stencil: H::NPAIR pairs
  const int64_t m = G.m;
  double sig_l = 1.0;                              // lane c: sigma2 of output c (selects: no indexed read of the argument)
#pragma unroll
  for (int c = 0; c < WISKI_LABEL_MAX_CLASSES; ++c) sig_l = lane == c ? sig.v[c] : sig_l;
  bool bad = false;
  double c_acc = 0, ld_acc = 0;                    // lane c: this wave's share of the two scalars of output c
  for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {
    const int64_t p = base + loc;
    const bool valid = p < n;
    int j0[D], flat_t[H::TPL];
    real w[D][4], val_t[H::TPL][1], wu[1];
    const bool inside = half_point_setup<real, D>(G, x, p, n, lane == 0, err, bad, j0, w);
    half_tap_table<real, D, 1>(G, j0, w, nullptr, lane, nullptr, s_val[loc], s_idx[loc], flat_t, val_t, wu);
    real mu_r = 0;                                 // lane c: the predictive mean of output c before the batch
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
      real part = 0;
#pragma unroll
      for (int t = 0; t < H::TPL; ++t)
        if (val_t[t][0] != (real)0) part += val_t[t][0] * u[c * m + flat_t[t]];
      part = wave_reduce_sum<real>(part);
      if (lane == c) mu_r = part;
    }
    double v_l = 0, n_l = 1;
    real wa_l = 0, wb_l = 0;
    if (valid && lane < C) {
      const double pv = (double)pvar[lane * n + p];
      v_l = pv > 0.0 ? pv : (pv == pv ? 0.0 : pv);
      n_l = (double)noise[lane * w_stride + p];
      wa_l = wa[lane * w_stride + p];
      wb_l = wb[lane * w_stride + p];
    }
    const double dn_l = sig_l * n_l;
    const int y = valid ? label_class((double)labels[p], C) : -1;
    const bool ok = label_publish(C, y, lane, (double)mu_r, v_l + dn_l, s_mu[loc], s_a[loc], s_isa[loc]) && inside;
    __syncthreads();
    double alpha_l = 0, beta_l = 0, logz = inside ? NAN : 0.0, yt_l = inside ? (double)mu_r : 0.0, om_l = 0;
    if (ok) {
      logz = label_site<true>(C, y, s_mu[loc], s_a[loc], s_isa[loc], lane, alpha_l, beta_l);
      if (lane < C) label_finish((double)mu_r, v_l, dn_l, alpha_l, beta_l, yt_l, om_l);
    }
    const real omega = (real)om_l, yt = (real)yt_l;
    const real wbp = wb_l * omega, wac = wa_l * omega, yw = yt * wbp, innov = yw - wac * mu_r;
    const bool enters_l = lane < C && om_l > 0.0;
    if (valid && lane < C) {
      ytilde_out[lane * n + p] = yt;
      omega_out[lane * n + p] = omega;
      if (mean_out) mean_out[lane * n + p] = mu_r;
      if (enters_l) {
        c_acc += yt_l * yt_l * (double)wbp;
        ld_acc += log(n_l / om_l);
      }
    }
    if (valid && lane == 0) logz_out[p] = logz;
    const unsigned long long mask = __ballot(enters_l);
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
      if (!((mask >> c) & 1ull)) continue;
      const real yw_c[1] = {__shfl(yw, c)}, wac_c[1] = {__shfl(wac, c)}, innov_c[1] = {__shfl(innov, c)};
      half_tap_atomics<real, D, 1>(true, flat_t, val_t, yw_c, wac_c, innov_c, b + c * m, cnt + c * m, res ? res + c * m : nullptr);
      half_pair_loop<real, D, 1>(lane, H::NPAIR, s_pair, s_val[loc], s_idx[loc], wac_c, 1, A + c * A_stride, m);
    }
    __syncthreads();
  }
  // the two scalars of every output: one atomic pair per block and output that holds anything
  if (lane < WISKI_LABEL_MAX_CLASSES) {
    s_stat[loc][lane][0] = c_acc;
    s_stat[loc][lane][1] = ld_acc;
  }
  __syncthreads();
  if ((int)threadIdx.x < C) {
    const int c = threadIdx.x;
    const double c_tot = s_stat[0][c][0] + s_stat[1][c][0] + s_stat[2][c][0] + s_stat[3][c][0];
    const double ld_tot = s_stat[0][c][1] + s_stat[1][c][1] + s_stat[2][c][1] + s_stat[3][c][1];
    if (c_tot != 0 || ld_tot != 0) {
      unsafeAtomicAdd(stats + 2 * c + 0, c_tot);
      unsafeAtomicAdd(stats + 2 * c + 1, ld_tot);
    }
  }
  if (bad) atomicOr(err, 1);
}

// Sites alone (wiski_label_sites) and class probabilities (wiski_label_proba): one wave per point, four per block, the same
// label_site, from given means, latent variances and noise variances [C][n].  PROBA: P(y = k) for every k into out_p [n][C], the
// integral without its derivatives, once per class; otherwise the sites of the given labels with omega = tau.
template <typename real, bool PROBA>
__global__ __launch_bounds__(256) void k_label_sites(const real* __restrict__ mu, const real* __restrict__ pvar, const real* __restrict__ s,
                                                     const real* __restrict__ labels, int C, int64_t n, real* __restrict__ ytilde_out,
                                                     real* __restrict__ omega_out, double* __restrict__ logz_out, double* __restrict__ out_p) {
  __shared__ double s_mu[4][WISKI_LABEL_MAX_CLASSES], s_a[4][WISKI_LABEL_MAX_CLASSES], s_isa[4][WISKI_LABEL_MAX_CLASSES];
  const int lane = threadIdx.x & 63, loc = threadIdx.x >> 6;
  for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {      // (block-uniform trip count)
    const int64_t p = base + loc;
    const bool valid = p < n;
    double mu_l = 0, v_l = 0, s_l = 1;
    if (valid && lane < C) {
      mu_l = (double)mu[lane * n + p];
      const double pv = (double)pvar[lane * n + p];
      v_l = pv > 0.0 ? pv : (pv == pv ? 0.0 : pv);
      s_l = (double)s[lane * n + p];
    }
    int y = 0;
    if constexpr (!PROBA) y = valid ? label_class((double)labels[p], C) : -1;
    const bool ok = label_publish(C, y, lane, mu_l, v_l + s_l, s_mu[loc], s_a[loc], s_isa[loc]) && valid;
    __syncthreads();
    double alpha_l = 0, beta_l = 0;
    if constexpr (PROBA) {
#pragma unroll 1
      for (int k = 0; k < C; ++k) {
        const double pk = ok ? exp(label_site<false>(C, k, s_mu[loc], s_a[loc], s_isa[loc], lane, alpha_l, beta_l)) : NAN;
        if (valid && lane == 0) out_p[p * C + k] = pk;
      }
    } else {
      double logz = NAN, yt_l = mu_l, om_l = 0;
      if (ok) {
        logz = label_site<true>(C, y, s_mu[loc], s_a[loc], s_isa[loc], lane, alpha_l, beta_l);
        if (lane < C) label_finish(mu_l, v_l, 1.0, alpha_l, beta_l, yt_l, om_l);
      }
      if (valid && lane < C) {
        ytilde_out[lane * n + p] = (real)yt_l;
        omega_out[lane * n + p] = (real)om_l;
      }
      if (valid && lane == 0) logz_out[p] = logz;
    }
    __syncthreads();
  }
}

template <typename real>
static int label_sites_impl(const real* mu, const real* pvar, const real* s, const real* labels, int32_t C, int64_t n, real* ytilde_out, real* omega_out,
                            double* logz_out, void* stream) {
  if (n < 0 || C < 2 || C > WISKI_LABEL_MAX_CLASSES || !mu || !pvar || !s || !labels || !ytilde_out || !omega_out || !logz_out) return WISKI_E_BADARG;
  if (n == 0) return WISKI_OK;
  int64_t blocks = (n + 3) / 4;
  if (blocks > 256 * 8) blocks = 256 * 8;
  hipLaunchKernelGGL((k_label_sites<real, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mu, pvar, s, labels, (int)C, n, ytilde_out,
                     omega_out, logz_out, (double*)nullptr);
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

template <typename real>
static int label_proba_impl(const real* mu, const real* pvar, const real* s, int32_t C, int64_t n, double* proba_out, void* stream) {
  if (n < 0 || C < 2 || C > WISKI_LABEL_MAX_CLASSES || !mu || !pvar || !s || !proba_out) return WISKI_E_BADARG;
  if (n == 0) return WISKI_OK;
  int64_t blocks = (n + 3) / 4;
  if (blocks > 256 * 8) blocks = 256 * 8;
  hipLaunchKernelGGL((k_label_sites<real, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, mu, pvar, s, (const real*)nullptr, (int)C, n,
                     (real*)nullptr, (real*)nullptr, (double*)nullptr, proba_out);
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

// The label absorb behind its two entries.  `a` carries the points, the weights, the statistics and the carry as for
// wiski_scatter_stats_multi (a.nout = C, a.bt its strides; a.y is ignored); everything the form does not have is refused here, before
// a launch: fewer than 2 or more than WISKI_LABEL_MAX_CLASSES outputs, a full stencil, a missing u / A / cnt, a guard, zero regions,
// a shard, the owner workspace, channels, a sigma2 that is not positive and finite.
template <typename real>
static int label_absorb(const wiski_grid* grid, const AbsorbArgs<real>& a, const real* labels, const real* pvar, const double* sigma2, real* ytilde_out,
                        real* omega_out, double* logz_out, void* stream) {
  GridDev<real> G;
  const int rc = make_grid_dev<real>(grid, &G);
  if (rc != WISKI_OK) return rc;
  if (a.nout < 2 || a.nout > WISKI_LABEL_MAX_CLASSES || a.n < 0) return WISKI_E_BADARG;
  if (!a.x || !labels || !pvar || !sigma2 || !a.wa || !a.wb || !a.noise || !a.b || !a.A || !a.cnt || !a.u || !a.stats || !a.err) return WISKI_E_BADARG;
  if (!ytilde_out || !omega_out || !logz_out || !a.half || a.channels) return WISKI_E_BADARG;
  if (a.guard || a.n1_bytes || a.n2_bytes || a.z1 || a.z2 || a.sharded() || a.bin || a.bin_bytes) return WISKI_E_BADARG;
  if (a.bt.w_stride < 0 || a.bt.A_stride < 0) return WISKI_E_BADARG;
  LabelSigma sig;
  for (int c = 0; c < WISKI_LABEL_MAX_CLASSES; ++c) {
    sig.v[c] = c < a.nout ? sigma2[c] : 1.0;
    if (!(sig.v[c] > 0.0) || !std::isfinite(sig.v[c])) return WISKI_E_BADARG;
  }
  if (a.n == 0) return WISKI_OK;
  int64_t blocks = (a.n + ROBUST_POINTS_PER_BLOCK - 1) / ROBUST_POINTS_PER_BLOCK;
  if (blocks > 256 * 8) blocks = 256 * 8;
#define CALL(DD)                                                                                                                                       \
  hipLaunchKernelGGL((k_scatter_stats_label<real, DD>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, G, a.x, labels, pvar, sig, a.nout,  \
                     a.wa, a.wb, a.noise, a.bt.w_stride, a.n, a.b, a.A, a.bt.A_stride, a.stats, a.err, a.cnt, a.u, a.res, a.mean_out, ytilde_out,        \
                     omega_out, logz_out)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}
