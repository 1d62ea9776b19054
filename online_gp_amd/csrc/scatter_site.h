// The site-weighted absorb: what the outlier-robust, interval, count and noisy-input forms (scatter_robust.h, scatter_interval.h,
// scatter_count.h, scatter_input_noise.h) do alike, stated once.  Each of them turns a point's
// datum and its predictive mean mu = w_p . u (the last one also the mean's slope) under the posterior BEFORE the batch into a
// pseudo-target and a weight (ytilde, omega), and the point enters as
// ytilde at noise noise_p / omega: A, cnt and the carried residual with omega wa, b and sum wb y^2 with omega wb and ytilde for y,
// log|D| with log(noise / omega).  mu is what the sweep already reduces over the wave, so a site costs its loads and stores and no
// second pass over the stencil.  All sites of a launch are taken against the same u: they depend neither on the order of the
// points nor on the order of the atomics.  Included by scatter_stats.hip, before the headers of the forms.
//
// A form is a `Site`: a small struct, passed to the kernel by value, of the form's own pointers and scalars, with
//   Datum           what a point carries; value-initialised it is the neutral datum a wave past the batch holds
//   load(p)         the datum of point p < n: everything the site is evaluated from besides mu, noise_p included where it enters
//                   the site (the kernel's own read of it comes after the tap table, for the two scalars only: k_scatter_stats_site)
//   eval(datum, mu, lane)
//                   the SiteValue of a point INSIDE the grid.  Called by all 64 lanes of the point's wave with wave-uniform
//                   arguments (a site may ballot and reduce over the wave) and the same in every lane
//   store(p, ytilde, omega, logz)
//                   what the form reports per point, by lane 0: the rounded values the point entered with; all zero for a point
//                   outside the grid, which has zero rows
//   kGrad           compile-time: false for a site of mu alone.  true (scatter_input_noise.h): the site is also a function of the
//                   slope of the predictive mean, g_q = (d w_p / d x_q) . u.  The sweep then sets the point up with derivative
//                   weights (half_point_setup<real, D, true>), reduces the d slopes over the wave beside mu (half_tap_grad,
//                   scatter_half.h: from the lane's own taps -- the LDS tap table stays single-channel) and hands them on:
//                   eval(datum, mu, g, lane) and store(p, ytilde, omega, logz, g), g a real[D], zero for a point outside the grid.
//                   Between the set-up and the tap table the site may re-evaluate the weights of a point inside the grid in more
//                   than the working precision, refine<D>(G, x, p, inside, w, dw): the cell stays the one the set-up chose
// and a static of(AbsorbArgs) that fills it.  A new observation form supplies that struct and one entry in absorb_validate(),
// AbsorbArgs::site_form() and absorb().
#pragma once

struct SiteValue {
  double ytilde, omega, logz;                     // in fp64 whatever the working precision
  bool enters;                                    // false: the point is skipped -- nothing anywhere, no flag in err
};

// the three per-point outputs of the moment-matched forms
template <typename real>
struct SiteOutputs {
  real* ytilde_out;
  real* omega_out;
  double* logz_out;
  __device__ __forceinline__ void store(int64_t p, real ytilde, real omega, double logz) const {
    ytilde_out[p] = ytilde;
    omega_out[p] = omega;
    logz_out[p] = logz;
  }
};

// The point sweep is that of k_scatter_stats_sym (scatter_half.h).  No guard, zero regions, shard or batch (absorb_validate).
//
// The two scalars cannot come from scatter_stats_pass: its designated blocks would need the sites of points other blocks evaluate
// in the same launch, and nothing orders a read of omega_out behind those writes.  Each wave therefore keeps, in fp64 and from the
// un-rounded site, the omega wb ytilde^2 and log(noise / omega) of its own points (lane 0 holds them), and a block issues one
// atomic pair when it is done.  A wave is one point, so the site and its case split are wave-uniform.
// The kernel reads noise_p in every lane and only after the tap table: read before it, it costs the robust fp64 d = 2 instantiation two
// VGPRs and a wave (74 / 6 against 72 / 7); read by lane 0 at its use, the robust instantiations take 74-101 VGPRs.  The count kernel
// runs one wave per SIMD and cannot hide a load issued right before its site, so a site that needs the noise loads it with its datum.
template <typename real, int D, typename Site>
__global__ __launch_bounds__(256) void k_scatter_stats_site(GridDev<real> G, const real* __restrict__ x, const real* __restrict__ wa,
                                                            const real* __restrict__ wb, const real* __restrict__ noise, int64_t n,
                                                            real* __restrict__ b, real* __restrict__ A, double* __restrict__ stats,
                                                            int32_t* __restrict__ err, real* __restrict__ cnt, const real* __restrict__ u,
                                                            real* __restrict__ res, real* __restrict__ mean_out, Site S) {
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
    [[maybe_unused]] real dw[Site::kGrad ? D : 1][4], gu[D];
    bool inside;
    if constexpr (Site::kGrad) {
      inside = half_point_setup<real, D, true>(G, x, p, n, lane == 0, err, bad, j0, w, dw);
      S.template refine<D>(G, x, p, inside, w, dw);
    } else inside = half_point_setup<real, D>(G, x, p, n, lane == 0, err, bad, j0, w);
    typename Site::Datum dat{};
    real wap = 0, wbp = 0;
    if (valid) {
      dat = S.load(p);
      wap = wa[p];
      wbp = wb[p];
    }
    half_tap_table<real, D, 1>(G, j0, w, nullptr, lane, u, s_val[loc], s_idx[loc], flat_t, val_t, wu);   // wu: the predictive mean of the point before the batch
    if constexpr (Site::kGrad) half_tap_grad<real, D>(w, dw, lane, u, flat_t, gu);   // zero for a point outside the grid and past the batch
    const double n_p = valid ? (double)noise[p] : 1.0;
    SiteValue st{0.0, 0.0, 0.0, false};
    if (inside) {
      if constexpr (Site::kGrad) st = S.eval(dat, wu[0], gu, lane);
      else st = S.eval(dat, wu[0], lane);
    }
    const real omega = (real)st.omega, yt = (real)st.ytilde;
    wbp *= omega;
    wac[0] = wap * omega;
    yw[0] = yt * wbp;
    half_carry<real, 1>(u, yw, wac, wu, mean_out, p, lane == 0 && valid, innov);   // with the weights the point enters with
    if (lane == 0 && valid) {
      if constexpr (Site::kGrad) S.store(p, yt, omega, st.logz, gu);
      else S.store(p, yt, omega, st.logz);
      if (st.enters) {
        c_acc += st.ytilde * st.ytilde * (double)wbp;
        ld_acc += log(n_p / st.omega);
      }
    }
    half_tap_atomics<real, D, 1>(valid && st.enters, flat_t, val_t, yw, wac, innov, b, cnt, res);
    __syncthreads();
    if (valid && st.enters) half_pair_loop<real, D, 1>(lane, H::NPAIR, s_pair, s_val[loc], s_idx[loc], wac, 1, A, G.m);
    __syncthreads();
  }
  stats_atomic_pair(c_acc, ld_acc, stats, s_red);
  if (bad) atomicOr(err, 1);
}

// Points a block takes where the batch has them (a multiple of 4: four per pass of its loop).  Every block ends with one atomic
// pair on the two scalars, and atomics of many blocks on one address serialise at the memory side (scatter_stats_pass): at 50^3
// fp32 with 4 096 points, 4 points per block (1 024 pairs) measured 97.4 us, 16 (256 pairs) 94.4 us, the plain absorb 83-85 us
// (the robust form, which the macro is named after).
#ifndef WISKI_ROBUST_POINTS_PER_BLOCK
#define WISKI_ROBUST_POINTS_PER_BLOCK 16
#endif
constexpr int64_t ROBUST_POINTS_PER_BLOCK = WISKI_ROBUST_POINTS_PER_BLOCK;

template <typename real, typename Site>
static int launch_site(const GridDev<real>& G, const AbsorbArgs<real>& a, const Site& S, hipStream_t stream) {
  int64_t blocks = (a.n + ROBUST_POINTS_PER_BLOCK - 1) / ROBUST_POINTS_PER_BLOCK;
  if (blocks > 256 * 8) blocks = 256 * 8;
#define CALL(DD)                                                                                                                                    \
  hipLaunchKernelGGL((k_scatter_stats_site<real, DD, Site>), dim3((unsigned)blocks), dim3(256), 0, stream, G, a.x, a.wa, a.wb, a.noise, a.n, a.b, \
                     a.A, a.stats, a.err, a.cnt, a.u, a.res, a.mean_out, S)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}
