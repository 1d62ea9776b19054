// Absorb of derivative observations (AbsorbArgs::channels = d + 1).  Included by scatter_stats.hip.
//
// A point carries C = d + 1 scalar observations: channel 0 is f(x_p), channel 1 + q is df/dx_q (x_p).  Under the SKI model each is
// one linear observation of the grid values; its row v_c of W is the value row with dim q's four weights replaced by
// keys_cubic_deriv / h_q (zero in a dim whose cell is a one-hot boundary cell: the convention of wiski_gather_grad).  All C rows
// sit on the same 4^d taps, so per point
//   A[a, b] += sum_c wa_c v_c[a] v_c[b]
// is formed in registers from the C-channel tap tables in LDS and leaves as ONE atomic per tap pair: a point with a full gradient
// costs the memory side what a point with a value costs (T (T + 1) / 2 tap-pair atomics), not C times that.
// An absent channel is wa = wb = 0, noise = 1 and contributes nothing anywhere; channels with wa_c = 0 are skipped wave-uniformly.
#pragma once

// point_stencil plus the derivative weights dw[q][c] = k'(t + 1 - c) / h_q (zero in a boundary cell of dim q, and everywhere for a
// point outside the grid)
template <typename real, int D>
__device__ __forceinline__ bool point_stencil_grad(const GridDev<real>& G, const real* __restrict__ xp, int j0[D], real w[D][4], real dw[D][4]) {
  bool ok = true;
#pragma unroll
  for (int q = 0; q < D; ++q) {
    int j = dim_stencil<real>(xp[q], G.g0[q], G.h[q], G.hi[q], G.g[q], w[q]);
    const real uu = (xp[q] - G.g0[q]) / G.h[q];
    const real fl = floor(uu);
    const int jj = (int)fl - 1;
    const bool interior = !(jj < 0 || jj > G.g[q] - 4);
#pragma unroll
    for (int c = 0; c < 4; ++c) dw[q][c] = interior ? keys_cubic_deriv<real>(uu - fl + (real)1 - (real)c) / G.h[q] : (real)0;
    if (j < 0) {
      ok = false;
      j = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) w[q][c] = dw[q][c] = (real)0;
    }
    j0[q] = j;
  }
  return ok;
}

// scatter_stats_pass over C channels per point: stats += (sum_c wb_c y_c^2, sum_c log noise_c) over the points inside the grid
template <typename real, int D>
__device__ __forceinline__ void scatter_stats_pass_grad(const GridDev<real>& G, const real* __restrict__ x, const real* __restrict__ y,
                                                        const real* __restrict__ wb, const real* __restrict__ noise, int64_t n,
                                                        double* __restrict__ stats, double* s_red) {
  constexpr int C = D + 1;
  int64_t want = n / 512;
  want = want < 1 ? 1 : (want > 64 ? 64 : want);
  const int ns = (int64_t)gridDim.x < want ? (int)gridDim.x : (int)want;
  if ((int)blockIdx.x >= ns) return;                       // block-uniform
  double c_acc = 0, ld_acc = 0;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (int64_t)ns * blockDim.x) {
    real xp[D], w[D][4];
    int j0[D];
#pragma unroll
    for (int q = 0; q < D; ++q) xp[q] = x[p * D + q];
    if (point_stencil<real, D>(G, xp, j0, w)) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const double yp = (double)y[p * C + c];
        c_acc += yp * yp * (double)wb[p * C + c];
        ld_acc += log((double)noise[p * C + c]);
      }
    }
  }
  const double c_tot = block_reduce_sum(c_acc, s_red);
  const double ld_tot = block_reduce_sum(ld_acc, s_red);
  if (threadIdx.x == 0 && (c_tot != 0 || ld_tot != 0)) {
    unsafeAtomicAdd(stats + 0, c_tot);
    unsafeAtomicAdd(stats + 1, ld_tot);
  }
}

// The lane mapping and the row-interleaved half-stencil layout are those of k_scatter_stats_sym: one wave per point, four points per
// block, lane = (a2, b2, pair slot).  The per-point tap table is channel-minor, s_val[point][tap][C], so that the C values of a tap
// are one contiguous LDS read (a ds_read_b128 at d = 3 in fp32): per tap-pair atomic the inner loop reads two such vectors and
// spends C multiply-adds.  LDS at d = 4 in fp64: 4 x 256 x 5 x 8 B = 40 KB of tables + 4 KB of row indices + 8 KB of pairs.
// y / wa / wb / noise / mean_out are [n][C].  cnt (preconditioner density model only) receives the value channel's row sums as
// today plus the diagonal the derivative channels add: cnt[a] += wa_0 v_0[a] + sum_{c >= 1} wa_c v_c[a]^2.
template <typename real, int D>
__global__ __launch_bounds__(256) void k_scatter_stats_grad(GridDev<real> G, const real* __restrict__ x, const real* __restrict__ y,
                                                            const real* __restrict__ wa, const real* __restrict__ wb,
                                                            const real* __restrict__ noise, int64_t n, real* __restrict__ b,
                                                            real* __restrict__ A, double* __restrict__ stats, int32_t* __restrict__ err,
                                                            real* __restrict__ cnt, const real* __restrict__ u, real* __restrict__ res,
                                                            real* __restrict__ mean_out) {
  constexpr int C = D + 1;
  constexpr int T = 1 << (2 * D);
  constexpr int TP = T / 4;                      // tap prefixes (leading d-1 digits)
  constexpr int NPAIR = TP * (TP + 1) / 2;       // prefix pairs with pb >= pa
  constexpr int TPL = T > 64 ? T / 64 : 1;       // taps per lane when filling the per-point tables
  __shared__ __align__(16) real s_val[4][T][C];
  __shared__ int s_idx[4][T];
  __shared__ int s_pair[NPAIR];                  // pa | pb << 8 | g << 16
  __shared__ double s_red[16];
  const int lane = threadIdx.x & 63, loc = threadIdx.x >> 6;
  // the prefix pairs in the order k_scatter_stats_sym lists them: base-4 digits map to base-7 codes monotonically, so the pairs
  // with code(pb) >= code(pa) are those with pb >= pa and row-major order gives each its slot in closed form
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
  const int64_t m = G.m;
  for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {
    const int64_t p = base + loc;
    const bool valid = p < n;
    int j0[D];
    real w[D][4], dw[D][4];
    real yw[C], wac[C];                            // wb_c y_c and wa_c (zero for a point that contributes nothing)
#pragma unroll
    for (int c = 0; c < C; ++c) yw[c] = wac[c] = (real)0;
    if (valid) {
      real xp[D];
#pragma unroll
      for (int q = 0; q < D; ++q) xp[q] = x[p * D + q];
      if (!point_stencil_grad<real, D>(G, xp, j0, w, dw)) {
        flag_outside(err, lane == 0, bad);        // dropped for every channel, counted once
      } else {
#pragma unroll
        for (int c = 0; c < C; ++c) {
          yw[c] = wb[p * C + c] * y[p * C + c];
          wac[c] = wa[p * C + c];
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < D; ++q) {
        j0[q] = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) w[q][c] = dw[q][c] = (real)0;
      }
    }
    int amask = 0;                                 // channels that enter A: the same in every lane of the wave
#pragma unroll
    for (int c = 0; c < C; ++c) amask |= (wac[c] != (real)0) << c;
    amask = __builtin_amdgcn_readfirstlane(amask);
    int flat_t[TPL];
    real val_t[TPL][C];
    real wu[C];                                    // this lane's share of v_c . u
#pragma unroll
    for (int c = 0; c < C; ++c) wu[c] = (real)0;
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
      const int a = lane + t * 64;
      flat_t[t] = 0;
#pragma unroll
      for (int c = 0; c < C; ++c) val_t[t][c] = (real)0;
      if (a < T) {
        int flat = 0;
        real v[C];
        v[0] = (real)1;
#pragma unroll
        for (int q = 0; q < D; ++q) {
          const int cq = (a >> (2 * (D - 1 - q))) & 3;
          flat += (j0[q] + cq) * G.stride[q];
          v[0] *= w[q][cq];
        }
#pragma unroll
        for (int q = 0; q < D; ++q) {
          real vq = (real)1;
#pragma unroll
          for (int o = 0; o < D; ++o) {
            const int co = (a >> (2 * (D - 1 - o))) & 3;
            vq *= o == q ? dw[o][co] : w[o][co];
          }
          v[1 + q] = vq;
        }
        bool touched = false;
#pragma unroll
        for (int c = 0; c < C; ++c) {
          s_val[loc][a][c] = v[c];
          val_t[t][c] = v[c];
          touched |= v[c] != (real)0;
        }
        s_idx[loc][a] = flat;
        flat_t[t] = flat;
        if (u && touched) {
          const real ug = u[flat];
#pragma unroll
          for (int c = 0; c < C; ++c) wu[c] += v[c] * ug;
        }
      }
    }
    // the carry (optional), per channel: v_c . u is the predictive mean (c = 0) / gradient (c = 1 + q) of the point BEFORE this
    // update, and res += sum_c v_c (wb_c y_c - wa_c (v_c . u)) keeps res = b - z - A u exact under the increment
    real innov[C];
#pragma unroll
    for (int c = 0; c < C; ++c) innov[c] = yw[c];
    if (u) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        wu[c] = wave_reduce_sum<real>(wu[c]);
        innov[c] -= wac[c] * wu[c];
      }
      if (mean_out && lane == 0 && valid) {
#pragma unroll
        for (int c = 0; c < C; ++c) mean_out[p * C + c] = wu[c];
      }
    }
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
      real sb = (real)0, sc = (real)0, sr = (real)0;
      bool touched = false;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const real v = val_t[t][c];
        touched |= v != (real)0;
        sb += v * yw[c];
        sr += v * innov[c];
        sc += c == 0 ? wac[c] * v : wac[c] * v * v;
      }
      if (valid && touched) {
        atomic_add_real(b + flat_t[t], sb);
        if (cnt) atomic_add_real(cnt + flat_t[t], sc);
        if (res) atomic_add_real(res + flat_t[t], sr);
      }
    }
    __syncthreads();
    if (valid && A && amask) {
      const int a2 = lane & 3, b2 = (lane >> 2) & 3, ps = lane >> 4;
#pragma unroll 2
      for (int t0 = 0; t0 < NPAIR; t0 += 4) {
        const int t = t0 + ps;
        if (t < NPAIR) {
          const int pk = s_pair[t];
          const int g = pk >> 16;
          const int a = (pk & 0xff) * 4 + a2;
          const real* __restrict__ va = s_val[loc][a];
          const real* __restrict__ vb = s_val[loc][((pk >> 8) & 0xff) * 4 + b2];
          real v = (real)0;
#pragma unroll
          for (int c = 0; c < C; ++c)
            if ((amask >> c) & 1) v += wac[c] * va[c] * vb[c];
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
  scatter_stats_pass_grad<real, D>(G, x, y, wb, noise, n, stats, s_red);
  if (bad) atomicOr(err, 1);
}

template <typename real>
static int launch_grad(const GridDev<real>& G, const AbsorbArgs<real>& a, hipStream_t stream) {
  int64_t blocks = (a.n + 3) / 4;
  if (blocks > 256 * 8) blocks = 256 * 8;
#define CALL(DD)                                                                                                                                     \
  hipLaunchKernelGGL((k_scatter_stats_grad<real, DD>), dim3((unsigned)blocks), dim3(256), 0, stream, G, a.x, a.y, a.wa, a.wb, a.noise, a.n, a.b, a.A, \
                     a.stats, a.err, a.cnt, a.u, a.res, a.mean_out)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}
