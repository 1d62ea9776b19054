// Outlier-robust absorb (AbsorbArgs::inv_scale).  Included by scatter_stats.hip.
//
// Every point is Huber-weighted against the posterior BEFORE the batch, inside the launch that absorbs it:
//   z_p = (y_p - w_p . u) inv_scale_p,   omega_p = min(1, c / |z_p|)        (exactly 1 for |z_p| <= c; inv_scale_p = 0 exempts the point)
// and it enters A, cnt and the carried residual with omega_p wa_p, b and sum wb y^2 with omega_p wb_p, log|D| with
// log(noise_p / omega_p): the absorb of the same point at noise noise_p / omega_p.  w_p . u is what k_scatter_stats_sym already
// reduces over the wave for mean_out and the carry, so the weight costs one load (inv_scale_p) and one store (omega_out_p) per
// point and no second pass over the stencil.  All omega of a launch are taken against the same u: they depend neither on the
// order of the points nor on the order of the atomics.
#pragma once

// The point sweep is that of k_scatter_stats_sym (scatter_half.h).  No guard, zero regions, shard or batch (absorb_validate).
//
// The two scalars cannot come from scatter_stats_pass: its designated blocks would need the omega of points other blocks weight
// in the same launch, and nothing orders a read of omega_out behind those writes.  Each wave therefore keeps, in fp64, the
// omega wb y^2 and log(noise / omega) of its own points (lane 0 holds them), and a block issues one atomic pair when it is done.
template <typename real, int D>
__global__ __launch_bounds__(256) void k_scatter_stats_robust(GridDev<real> G, const real* __restrict__ x, const real* __restrict__ y,
                                                              const real* __restrict__ wa, const real* __restrict__ wb,
                                                              const real* __restrict__ noise, int64_t n, real* __restrict__ b,
                                                              real* __restrict__ A, double* __restrict__ stats, int32_t* __restrict__ err,
                                                              real* __restrict__ cnt, const real* __restrict__ u, real* __restrict__ res,
                                                              real* __restrict__ mean_out, const real* __restrict__ inv_scale, real huber_c,
                                                              real* __restrict__ omega_out) {
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
    real yp = 0, wap = 0, wbp = 0, isp = 0;
    if (valid) {
      yp = y[p];
      wap = wa[p];
      wbp = wb[p];
      isp = inv_scale[p];
    }
    half_tap_table<real, D, 1>(G, j0, w, nullptr, lane, u, s_val[loc], s_idx[loc], flat_t, val_t, wu);   // wu: the predictive mean of the point before the batch
    // the Huber weight, the same in every lane; a point outside the grid has zero rows and reports omega = 0
    const real az = fabs((yp - wu[0]) * isp);
    const real omega = az > huber_c ? huber_c / az : (real)1;
    wbp *= omega;
    wac[0] = wap * omega;
    yw[0] = yp * wbp;
    half_carry<real, 1>(u, yw, wac, wu, mean_out, p, lane == 0 && valid, innov);   // with the weights the point enters with
    if (lane == 0 && valid) {
      omega_out[p] = inside ? omega : (real)0;
      if (inside) {
        c_acc += (double)yp * (double)yp * (double)wbp;
        ld_acc += log((double)noise[p] / (double)omega);
      }
    }
    half_tap_atomics<real, D, 1>(valid, flat_t, val_t, yw, wac, innov, b, cnt, res);
    __syncthreads();
    if (valid) half_pair_loop<real, D, 1>(lane, H::NPAIR, s_pair, s_val[loc], s_idx[loc], wac, 1, A, G.m);
    __syncthreads();
  }
  stats_atomic_pair(c_acc, ld_acc, stats, s_red);
  if (bad) atomicOr(err, 1);
}

// Points a block takes where the batch has them (a multiple of 4: four per pass of its loop).  Every block ends with one atomic
// pair on the two scalars, and atomics of many blocks on one address serialise at the memory side (scatter_stats_pass): at 50^3
// fp32 with 4 096 points, 4 points per block (1 024 pairs) measured 97.4 us, 16 (256 pairs) 94.4 us, the plain absorb 83-85 us.
#ifndef WISKI_ROBUST_POINTS_PER_BLOCK
#define WISKI_ROBUST_POINTS_PER_BLOCK 16
#endif
constexpr int64_t ROBUST_POINTS_PER_BLOCK = WISKI_ROBUST_POINTS_PER_BLOCK;

template <typename real>
static int launch_robust(const GridDev<real>& G, const AbsorbArgs<real>& a, hipStream_t stream) {
  int64_t blocks = (a.n + ROBUST_POINTS_PER_BLOCK - 1) / ROBUST_POINTS_PER_BLOCK;
  if (blocks > 256 * 8) blocks = 256 * 8;
#define CALL(DD)                                                                                                                                        \
  hipLaunchKernelGGL((k_scatter_stats_robust<real, DD>), dim3((unsigned)blocks), dim3(256), 0, stream, G, a.x, a.y, a.wa, a.wb, a.noise, a.n, a.b, a.A, \
                     a.stats, a.err, a.cnt, a.u, a.res, a.mean_out, a.inv_scale, a.huber_c, a.omega_out)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}
