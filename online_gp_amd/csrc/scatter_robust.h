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

// The lane mapping, the LDS tables, the pair list and the row-interleaved half-stencil layout are those of k_scatter_stats_sym:
// one wave per point, four points per block, lane = (a2, b2, pair slot).  No guard, zero regions, shard or batch (absorb_validate).
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
  constexpr int T = 1 << (2 * D);
  constexpr int TP = T / 4;                      // tap prefixes (leading d-1 digits)
  constexpr int NPAIR = TP * (TP + 1) / 2;       // prefix pairs with pb >= pa
  constexpr int TPL = T > 64 ? T / 64 : 1;       // taps per lane when filling the per-point tables
  __shared__ real s_val[4][T];
  __shared__ int s_idx[4][T];
  __shared__ int s_pair[NPAIR];                  // pa | pb << 8 | g << 16
  __shared__ double s_red[16];
  const int lane = threadIdx.x & 63, loc = threadIdx.x >> 6;
  // the prefix pairs in the order k_scatter_stats_sym lists them (closed form: scatter_grad.h)
  for (int idx = threadIdx.x; idx < TP * TP; idx += 256) {
    const int pa = idx / TP, pb = idx % TP;
    int ca = 0, cb = 0;
#pragma unroll
    for (int q = 0; q < D - 1; ++q) {
      ca = ca * 7 + ((pa >> (2 * (D - 2 - q))) & 3);
      cb = cb * 7 + ((pb >> (2 * (D - 2 - q))) & 3);
    }
    if (pb >= pa) s_pair[pa * TP - pa * (pa - 1) / 2 + (pb - pa)] = pa | (pb << 8) | ((cb - ca) << 16);
  }
  bool bad = false;
  double c_acc = 0, ld_acc = 0;                  // lane 0: this wave's share of the two scalars
  const int64_t m = G.m;
  for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {
    const int64_t p = base + loc;
    const bool valid = p < n;
    bool inside = false;
    int j0[D];
    real w[D][4];
    real yp = 0, wap = 0, wbp = 0, isp = 0;
    if (valid) {
      real xp[D];
#pragma unroll
      for (int q = 0; q < D; ++q) xp[q] = x[p * D + q];
      inside = point_stencil<real, D>(G, xp, j0, w);
      if (!inside) flag_outside(err, lane == 0, bad);
      yp = y[p];
      wap = wa[p];
      wbp = wb[p];
      isp = inv_scale[p];
    } else {
#pragma unroll
      for (int q = 0; q < D; ++q) {
        j0[q] = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) w[q][c] = 0;
      }
    }
    int flat_t[TPL];
    real val_t[TPL];
    real wu = (real)0;                            // this lane's share of w_p . u
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
      const int a = lane + t * 64;
      flat_t[t] = 0;
      val_t[t] = (real)0;
      if (a < T) {
        int flat = 0;
        real v = (real)1;
#pragma unroll
        for (int q = 0; q < D; ++q) {
          const int c = (a >> (2 * (D - 1 - q))) & 3;
          flat += (j0[q] + c) * G.stride[q];
          v *= w[q][c];
        }
        s_val[loc][a] = v;
        s_idx[loc][a] = flat;
        flat_t[t] = flat;
        val_t[t] = v;
        if (v != (real)0) wu += v * u[flat];
      }
    }
    wu = wave_reduce_sum<real>(wu);               // the predictive mean of the point before the batch, in every lane
    // the Huber weight, the same in every lane; a point outside the grid has zero rows and reports omega = 0
    const real az = fabs((yp - wu) * isp);
    const real omega = az > huber_c ? huber_c / az : (real)1;
    wap *= omega;
    wbp *= omega;
    const real innov = yp * wbp - wap * wu;       // res += W^T (wb y - wa (W u)), with the weights the point enters with
    if (lane == 0 && valid) {
      if (mean_out) mean_out[p] = wu;
      omega_out[p] = inside ? omega : (real)0;
      if (inside) {
        c_acc += (double)yp * (double)yp * (double)wbp;
        ld_acc += log((double)noise[p] / (double)omega);
      }
    }
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
      if (valid && val_t[t] != (real)0) {
        atomic_add_real(b + flat_t[t], val_t[t] * yp * wbp);
        atomic_add_real(cnt + flat_t[t], val_t[t] * wap);
        if (res) atomic_add_real(res + flat_t[t], val_t[t] * innov);
      }
    }
    __syncthreads();
    if (valid) {
      const int a2 = lane & 3, b2 = (lane >> 2) & 3, ps = lane >> 4;
#pragma unroll 2
      for (int t0 = 0; t0 < NPAIR; t0 += 4) {
        const int t = t0 + ps;
        if (t < NPAIR) {
          const int pk = s_pair[t];
          const int g = pk >> 16;
          const int a = (pk & 0xff) * 4 + a2;
          const real v = wap * s_val[loc][a] * s_val[loc][((pk >> 8) & 0xff) * 4 + b2];
          const int64_t row = s_idx[loc][a];
          if (g == 0) {
            if (b2 >= a2 && v != (real)0) stencil_atomic(A + row * 4 + (b2 - a2), v);
          } else if (v != (real)0) {
            stencil_atomic(A + (int64_t)(7 * g - 3) * m + row * 7 + (b2 - a2 + 3), v);
          }
        }
      }
    }
    __syncthreads();
  }
  const double c_tot = block_reduce_sum(c_acc, s_red);
  const double ld_tot = block_reduce_sum(ld_acc, s_red);
  if (threadIdx.x == 0 && (c_tot != 0 || ld_tot != 0)) {
    unsafeAtomicAdd(stats + 0, c_tot);
    unsafeAtomicAdd(stats + 1, ld_tot);
  }
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
