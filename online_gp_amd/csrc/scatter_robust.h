// Outlier-robust absorb (AbsorbArgs::inv_scale).  Included by scatter_stats.hip.
//
// Every point is Huber-weighted against the posterior BEFORE the batch, inside the launch that absorbs it:
//   z_p = (y_p - w_p . u) inv_scale_p,   omega_p = min(1, c / |z_p|)        (exactly 1 for |z_p| <= c; inv_scale_p = 0 exempts the point)
// and it enters A, cnt and the carried residual with omega_p wa_p, b and sum wb y^2 with omega_p wb_p, log|D| with
// log(noise_p / omega_p): the absorb of the same point at noise noise_p / omega_p.  w_p . u is what k_scatter_stats_sym already
// reduces over the wave for mean_out and the carry, so the weight costs one load (inv_scale_p) and one store (omega_out_p) per
// point and no second pass over the stencil.  The sweep and the two scalars are k_scatter_stats_site's (scatter_site.h).
#pragma once

// The site of the robust form: the target itself at the Huber weight.  Every point inside the grid enters, whatever its weight.
template <typename real>
struct SiteRobust {
  const real* y;
  const real* inv_scale;
  real huber_c;
  real* omega_out;
  static constexpr bool kGrad = false;
  struct Datum {
    real y = 0, is = 0;
  };
  static SiteRobust of(const AbsorbArgs<real>& a) { return {a.y, a.inv_scale, a.huber_c, a.omega_out}; }
  __device__ __forceinline__ Datum load(int64_t p) const { return {y[p], inv_scale[p]}; }
  __device__ __forceinline__ SiteValue eval(const Datum& d, real mu, int) const {
    const real az = fabs((d.y - mu) * d.is);
    const real omega = az > huber_c ? huber_c / az : (real)1;
    return {(double)d.y, (double)omega, 0.0, true};
  }
  __device__ __forceinline__ void store(int64_t p, real, real omega, double) const { omega_out[p] = omega; }
};
