// Noisy-input absorb (AbsorbArgs::xvar).  Included by scatter_stats.hip.
//
// A point says y_p = f(x_p + e_p) + eps_p with e_p ~ N(0, diag(xvar_p)): its location is known up to an error.  To first order
// (McHutchon & Rasmussen's noisy-input GP) the input error acts as extra output noise grad f(x)^T diag(xvar) grad f(x), and the
// model stays an exact GP of the same points at inflated noise.  The slope is taken under the posterior BEFORE the batch, inside
// the launch that absorbs it: with
//   mu = w_p . u,   g_k = (d w_p / d x_k) . u,   v = pvar_p,   gamma_k = gvar_p,k (the posterior variance of d f / d x_k),   dn = sigma2 noise_p
//   s_in = sum_k xvar_k (g_k^2 + max(gamma_k, 0))            -- xvar E[(d_k f)^2]; without gvar gamma = 0, the textbook rule
//   omega = dn / (dn + s_in)  in (0, 1],   ytilde = y,   log Z = log N(y; mu, max(v, 0) + dn + s_in)
// the point enters as y at noise noise_p / omega_p, exactly as the other sites enter a point (scatter_site.h).  The slope variance is
// what makes the rule usable in a stream: a cold start, whose mean is still flat, inflates by the prior's slope variance instead of
// not at all.  mu is what the sweep reduces over the wave already; the d slopes are reduced beside it from the lane's own taps
// (half_tap_grad, scatter_half.h), so the site costs its loads, d wave reductions and no second pass over the stencil.
#pragma once

// A site whose omega falls below this enters nothing: a location so uncertain on ground so steep that the point says nothing.
#ifndef WISKI_INPUT_NOISE_OMEGA_MIN
#define WISKI_INPUT_NOISE_OMEGA_MIN 1e-12
#endif

struct InputNoiseSite {
  double omega, logz;                             // omega = 0: the point is skipped
};

// The site of one point, in fp64 whatever the working precision.  xvar all zero: s_in = 0 and omega = dn / dn = 1 exactly.  A
// negative or NaN xvar_k (log Z = NaN), a non-finite s_in (log Z = NaN), an omega below WISKI_INPUT_NOISE_OMEGA_MIN: skipped.
template <int D>
__device__ __forceinline__ InputNoiseSite input_noise_site(double y, double mu, double v, double dn, const double xi[D], const double gam[D],
                                                           const double g[D]) {
  constexpr double HALF_LOG_2PI = 0.91893853320467274178;
  double s_in = 0.0;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < D; ++k) {
    ok &= xi[k] >= 0.0;                                                 // (false for a NaN)
    s_in += xi[k] * (g[k] * g[k] + (gam[k] > 0.0 ? gam[k] : 0.0));
  }
  if (!ok || !isfinite(s_in)) return {0.0, NAN};
  v = v > 0.0 ? v : 0.0;
  const double s2 = v + dn + s_in, z = y - mu;
  const double logz = -0.5 * z * z / s2 - 0.5 * log(s2) - HALF_LOG_2PI;
  const double omega = dn / (dn + s_in);
  return {omega >= WISKI_INPUT_NOISE_OMEGA_MIN ? omega : 0.0, logz};
}

// The site of the noisy-input form (the sweep and the two scalars are k_scatter_stats_site's, scatter_site.h), a kGrad site: the same
// closed form in every lane.  The datum keeps xvar and gvar in the working precision for WISKI_MAX_DIM dims, read with constant
// indices (a dim the grid does not have holds 0); a wave past the batch holds the neutral datum, whose omega is 1 and which is never
// evaluated.  The pseudo-target is y itself, so the form reports omega, log Z and, where asked, the slopes as the wave reduced them.
template <typename real>
struct SiteInputNoise {
  const real* y;
  const real* xvar;
  const real* gvar;                               // NULL: gamma = 0
  const real* pvar;
  const real* noise;
  int d;
  double sigma2;
  real* omega_out;
  double* logz_out;
  real* grad_out;                                 // NULL: not reported
  double g0[WISKI_MAX_DIM], h[WISKI_MAX_DIM];     // the grid as the caller gave it, in double (refine; 64 bytes of kernel argument the fp64 instantiations never read)
  static constexpr bool kGrad = true;
  struct Datum {
    double y = 0, v = 0, noise = 1;
    real xi[WISKI_MAX_DIM] = {}, gam[WISKI_MAX_DIM] = {};
  };
  static SiteInputNoise of(const AbsorbArgs<real>& a, const wiski_grid& grid) {
    SiteInputNoise S{a.y, a.xvar, a.gvar, a.pvar, a.noise, grid.d, a.sigma2, a.omega_out, a.logz_out, a.grad_out, {}, {}};
    for (int q = 0; q < WISKI_MAX_DIM; ++q) {
      S.g0[q] = q < grid.d ? grid.g0[q] : 0.0;
      S.h[q] = q < grid.d ? grid.h[q] : 1.0;
    }
    return S;
  }
  // The weights of a point inside the grid, once more, for the fp32 sweep: the cubic and its derivative evaluated in double from the
  // double grid and rounded once.  In fp32 the derivative weights lose several ulps of their TERMS to cancellation (a cubic with terms
  // of 2..5 against values below 1), and the offset t = (x - g0) / h another ulp of |x - g0| / h: at d = 1 that alone moved the slope by
  // twice the rounding error of its four-tap dot product.  The cell is the one half_point_setup chose (the same fp32 floor); where the
  // double offset falls a rounding outside [0, 1) the pieces of the C^1 cubic continue each other to second order.  A boundary cell of
  // a dim keeps its one-hot weights and zero derivative.  That the cell is the set-up's rests on (x - g0) / h rounding here as it does
  // in dim_stencil and point_stencil_grad -- one correctly rounded subtraction and division each, which holds while the build sets no
  // fast-math flag (it sets none).  fp64: nothing to do.
  template <int D>
  __device__ __forceinline__ void refine(const GridDev<real>& G, const real* __restrict__ x, int64_t p, bool inside, real (*w)[4], real (*dw)[4]) const {
    if constexpr (sizeof(real) == 4) {
      if (!inside) return;
#pragma unroll
      for (int q = 0; q < D; ++q) {
        const real xq = x[p * D + q];
        const real fl = floor((xq - G.g0[q]) / G.h[q]);
        const int jj = (int)fl - 1;
        if (!(jj < 0 || jj > G.g[q] - 4)) {
          const double ih = 1.0 / h[q], t = ((double)xq - g0[q]) * ih - (double)fl;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const double s = t + 1.0 - (double)c;
            w[q][c] = (real)keys_cubic<double>(s);
            dw[q][c] = (real)(keys_cubic_deriv<double>(s) * ih);
          }
        }
      }
    }
  }
  __device__ __forceinline__ Datum load(int64_t p) const {
    Datum r;
    r.y = (double)y[p];
    r.v = (double)pvar[p];
    r.noise = (double)noise[p];
#pragma unroll
    for (int k = 0; k < WISKI_MAX_DIM; ++k) {
      if (k < d) {
        r.xi[k] = xvar[p * d + k];
        if (gvar) r.gam[k] = gvar[p * d + k];
      }
    }
    return r;
  }
  template <int D>
  __device__ __forceinline__ SiteValue eval(const Datum& dt, real mu, const real (&g)[D], int) const {
    double xi[D], gam[D], gd[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
      xi[k] = (double)dt.xi[k];
      gam[k] = (double)dt.gam[k];
      gd[k] = (double)g[k];
    }
    const InputNoiseSite st = input_noise_site<D>(dt.y, (double)mu, dt.v, sigma2 * dt.noise, xi, gam, gd);
    return {dt.y, st.omega, st.logz, st.omega > 0.0};
  }
  template <int D>
  __device__ __forceinline__ void store(int64_t p, real, real omega, double logz, const real (&g)[D]) const {
    omega_out[p] = omega;
    logz_out[p] = logz;
    if (grad_out) {
#pragma unroll
      for (int k = 0; k < D; ++k) grad_out[p * D + k] = g[k];
    }
  }
};
