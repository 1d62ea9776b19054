// The half-stencil point sweep: what the three atomic forms of the absorb that keep the symmetric half of W^T D^-1 W
// (k_scatter_stats_sym in scatter_stats.hip, k_scatter_stats_grad in scatter_grad.h, k_scatter_stats_site in scatter_site.h)
// do per point, stated once.  One wave per point, four points per block: each lane fills its taps of the point's LDS tables,
// the wave reduces v . u, every lane issues the atomics of its own taps on b / cnt / res, and then the wave walks the prefix-pair
// list with lane = (a2, b2, pair slot).  C is the number of observation channels a point carries: 1 for a value, d + 1 for a
// value and its gradient (scatter_grad.h), whose tap tables are channel-minor.  Included by scatter_stats.hip.
#pragma once

template <int D>
struct HalfTaps {
  static constexpr int T = 1 << (2 * D);
  static constexpr int TP = T / 4;                      // tap prefixes (leading d-1 digits)
  static constexpr int NPAIR = TP * (TP + 1) / 2;       // prefix pairs with code(pb) >= code(pa)
  static constexpr int TPL = T > 64 ? T / 64 : 1;       // taps per lane when filling the per-point tables
};

// digit q (0 = outermost dim) of a tap, or of a tap prefix, of ND base-4 digits
template <int ND>
__device__ __forceinline__ int tap_digit(int a, int q) { return (a >> (2 * (ND - 1 - q))) & 3; }

// The half-stencil atomics.  Cache-policy bits on the fp32 atomic (sc1, nt, sc1 nt) leave A_h no better
// placed for the SpMV that follows -- SpMV dispatches right after the absorb / absorb kernel: default 18.0-18.2 us / 66.6-67.4 us,
// sc1 18.1-18.4 / 67.7, nt 18.3-18.4 / 69.3, sc1 nt 18.2-18.3 / 68.7 -- so it is the plain fire-and-forget add.
__device__ __forceinline__ void stencil_atomic(float* p, float v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void stencil_atomic(double* p, double v) { unsafeAtomicAdd(p, v); }

// A point outside the grid raises the flag and contributes nothing at all (zero weights; no y^2 / log-noise term either, so a
// caller that catches the error keeps statistics that agree with A and b).  `count`: the one lane that counts the point --
// bits 1..: number of training points dropped; bit 0 (any point outside) is set from `bad` when the kernel ends.
__device__ __forceinline__ void flag_outside(int32_t* __restrict__ err, bool count, bool& bad) {
  bad = true;
  if (count) atomicAdd(err, 2);
}

// stats += (c_acc, ld_acc) summed over the block, as one atomic pair (none from a block that holds nothing).  `s_red`: 16 doubles.
__device__ __forceinline__ void stats_atomic_pair(double c_acc, double ld_acc, double* __restrict__ stats, double* s_red) {
  const double c_tot = block_reduce_sum(c_acc, s_red);
  const double ld_tot = block_reduce_sum(ld_acc, s_red);
  if (threadIdx.x == 0 && (c_tot != 0 || ld_tot != 0)) {
    unsafeAtomicAdd(stats + 0, c_tot);
    unsafeAtomicAdd(stats + 1, ld_tot);
  }
}

// One point's terms of the two scalars, channels e .. e + C - 1 of [n][C] arrays.  Recursion, not a loop: with an inner loop in it,
// the sweep of scatter_stats_pass costs k_scatter_stats_sym<float, 3> four more VGPRs although C = 1 has one trip.
template <typename real, int C>
__device__ __forceinline__ void stats_terms(const real* __restrict__ y, const real* __restrict__ wb, const real* __restrict__ noise, int64_t e,
                                            double& c_acc, double& ld_acc) {
  const double yp = (double)y[e];
  c_acc += yp * yp * (double)wb[e];
  ld_acc += log((double)noise[e]);
  if constexpr (C > 1) stats_terms<real, C - 1>(y, wb, noise, e + 1, c_acc, ld_acc);
}

// stats[0] += sum wb y^2, stats[1] += sum log(noise) over the points inside the grid and their C channels (y / wb / noise are
// [n][C]).  Atomics of many blocks on one address serialise at the memory side (~12 ns each): with one pair per block the 1 024
// blocks of a q = 4 096 absorb spent 25 us of their 87 us queueing on these two doubles.  So a few designated blocks sweep the
// points once more (x, y, wb, noise: 24 B per point) and issue one pair each.
template <typename real, int D, int C = 1>
__device__ __forceinline__ void scatter_stats_pass(const GridDev<real>& G, const real* __restrict__ x, const real* __restrict__ y,
                                                   const real* __restrict__ wb, const real* __restrict__ noise, int64_t n,
                                                   double* __restrict__ stats, double* s_red) {
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
    if (point_stencil<real, D>(G, xp, j0, w)) stats_terms<real, C>(y, wb, noise, p * C, c_acc, ld_acc);
  }
  stats_atomic_pair(c_acc, ld_acc, stats, s_red);
}

// Fills s_pair with the prefix pairs (pa, pb), code(pb) >= code(pa), of the stencil groups g = code(pb) - code(pa) in
// [g_lo, g_hi), packed pa | pb << 8 | g << 16 in row-major (pa, pb) order, and returns their number: NPAIR for the whole
// stencil, fewer for a shard (block-uniform).  Block-cooperative stream compaction, 256 candidates at a time; `s_scan`: four
// ints of LDS nothing else uses meanwhile (the kernels lend the head of their reduction buffer).
template <int D>
__device__ __forceinline__ int half_pair_list(int* s_pair, int* s_scan, int g_lo, int g_hi) {
  constexpr int TP = HalfTaps<D>::TP;
  const int lane = threadIdx.x & 63, loc = threadIdx.x >> 6;
  int running = 0;
  for (int base = 0; base < TP * TP; base += 256) {
    const int idx = base + threadIdx.x;
    const int pa = idx / TP, pb = idx % TP;
    int ca = 0, cb = 0;
#pragma unroll
    for (int q = 0; q < D - 1; ++q) {
      ca = ca * 7 + tap_digit<D - 1>(pa, q);
      cb = cb * 7 + tap_digit<D - 1>(pb, q);
    }
    const bool ok = idx < TP * TP && cb >= ca && cb - ca >= g_lo && cb - ca < g_hi;
    const unsigned long long mask = __ballot(ok);
    if (lane == 0) s_scan[loc] = __popcll(mask);
    __syncthreads();
    int off = running;
    for (int w = 0; w < loc; ++w) off += s_scan[w];
    if (ok) s_pair[off + __popcll(mask & ((1ull << lane) - 1ull))] = pa | (pb << 8) | ((cb - ca) << 16);
    running += s_scan[0] + s_scan[1] + s_scan[2] + s_scan[3];
    __syncthreads();
  }
  return running;
}

template <typename real, int D>
__device__ __forceinline__ bool point_stencil_grad(const GridDev<real>& G, const real* __restrict__ xp, int j0[D], real w[D][4], real dw[D][4]);   // scatter_grad.h

// The stencil of point p for the lanes of its wave: j0 and w (with DW also the derivative weights dw, scatter_grad.h), all zero
// for a wave past the batch (p >= n) and for a point outside the grid, which is flagged and counted by the lane with `count`.
// True: the point exists and lies inside the grid.
template <typename real, int D, bool DW = false>
__device__ __forceinline__ bool half_point_setup(const GridDev<real>& G, const real* __restrict__ x, int64_t p, int64_t n, bool count,
                                                 int32_t* __restrict__ err, bool& bad, int j0[D], real w[D][4], real (*dw)[4] = nullptr) {
  if (p < n) {
    real xp[D];
#pragma unroll
    for (int q = 0; q < D; ++q) xp[q] = x[p * D + q];
    bool inside;
    if constexpr (DW) inside = point_stencil_grad<real, D>(G, xp, j0, w, dw);
    else inside = point_stencil<real, D>(G, xp, j0, w);
    if (!inside) flag_outside(err, count, bad);
    return inside;
  }
#pragma unroll
  for (int q = 0; q < D; ++q) {
    j0[q] = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      w[q][c] = (real)0;
      if constexpr (DW) dw[q][c] = (real)0;
    }
  }
  return false;
}

// The point's tap tables, filled by its wave (lane <-> taps lane, lane + 64, ...): sv[a][c] = v_c[a], the value of tap a in
// channel c -- c = 0: the product of the w digits, c = 1 + q: the same with dim q's weight replaced by dw -- and si[a] its grid
// row.  The lane keeps its own taps in flat_t / val_t.  With u, wu[c] = v_c . u comes back reduced over the wave, in every lane.
template <typename real, int D, int C>
__device__ __forceinline__ void half_tap_table(const GridDev<real>& G, const int j0[D], const real w[D][4], const real (*dw)[4], int lane,
                                               const real* __restrict__ u, real* sv, int* si, int flat_t[HalfTaps<D>::TPL],
                                               real val_t[HalfTaps<D>::TPL][C], real wu[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) wu[c] = (real)0;
#pragma unroll
  for (int t = 0; t < HalfTaps<D>::TPL; ++t) {
    const int a = lane + t * 64;
    flat_t[t] = 0;
#pragma unroll
    for (int c = 0; c < C; ++c) val_t[t][c] = (real)0;
    if (a < HalfTaps<D>::T) {
      int flat = 0, cq[D];
      real v[C];
      v[0] = (real)1;
#pragma unroll
      for (int q = 0; q < D; ++q) {
        cq[q] = tap_digit<D>(a, q);
        flat += (j0[q] + cq[q]) * G.stride[q];
        v[0] *= w[q][cq[q]];
      }
      if constexpr (C > 1) {
#pragma unroll
        for (int q = 0; q < D; ++q) {
          real vq = (real)1;
#pragma unroll
          for (int o = 0; o < D; ++o) vq *= o == q ? dw[o][cq[o]] : w[o][cq[o]];
          v[1 + q] = vq;
        }
      }
      bool touched = false;
#pragma unroll
      for (int c = 0; c < C; ++c) {
        sv[a * C + c] = v[c];
        val_t[t][c] = v[c];
        touched |= v[c] != (real)0;
      }
      si[a] = flat;
      flat_t[t] = flat;
      if (u && touched) {
        const real ug = u[flat];
#pragma unroll
        for (int c = 0; c < C; ++c) wu[c] += v[c] * ug;
      }
    }
  }
  if (u) {
#pragma unroll
    for (int c = 0; c < C; ++c) wu[c] = wave_reduce_sum<real>(wu[c]);
  }
}

// The gradient of the point's predictive mean beside a single-channel tap table: gu[q] = (d w_p / d x_q) . u, from the lane's own
// taps (flat_t, as half_tap_table left them) and reduced over the wave, in every lane.  The derivative row of dim q is the product of
// the w digits with dim q's replaced by dw (point_stencil_grad: zero in a one-hot boundary cell of the dim), so a site that needs
// the slope (scatter_input_noise.h) costs d products and one more read of u per tap and d wave reductions per point, and the LDS
// table, the atomics and the pair loop stay those of C = 1.  u is read where ANY derivative weight is non-zero: at a node the value
// weight of a neighbour vanishes and its derivative weight does not.
template <typename real>
__device__ __forceinline__ real half_pick4(const real v[4], int c) { return c == 0 ? v[0] : (c == 1 ? v[1] : (c == 2 ? v[2] : v[3])); }

template <typename real, int D>
__device__ __forceinline__ void half_tap_grad(const real w[D][4], const real (*dw)[4], int lane, const real* __restrict__ u,
                                              const int flat_t[HalfTaps<D>::TPL], real gu[D]) {
#pragma unroll
  for (int q = 0; q < D; ++q) gu[q] = (real)0;
#pragma unroll
  for (int t = 0; t < HalfTaps<D>::TPL; ++t) {
    const int a = lane + t * 64;
    if (a < HalfTaps<D>::T) {
      // the tap's digits: w by index, as half_tap_table reads it, dw by selects.  Both by index cost the d = 1 instantiations 36 B
      // of scratch per lane, both by selects the d >= 2 ones 48-144 B (the compiler's resource remarks); this way none has any
      real wd[D], dwd[D], v[D];
      bool touched = false;
#pragma unroll
      for (int q = 0; q < D; ++q) {
        const int c = tap_digit<D>(a, q);
        wd[q] = w[q][c];
        dwd[q] = half_pick4<real>(dw[q], c);
      }
#pragma unroll
      for (int q = 0; q < D; ++q) {
        real vq = (real)1;
#pragma unroll
        for (int o = 0; o < D; ++o) vq *= o == q ? dwd[o] : wd[o];
        v[q] = vq;
        touched |= vq != (real)0;
      }
      if (touched) {
        const real ug = u[flat_t[t]];
#pragma unroll
        for (int q = 0; q < D; ++q) gu[q] += v[q] * ug;
      }
    }
  }
#pragma unroll
  for (int q = 0; q < D; ++q) gu[q] = wave_reduce_sum<real>(gu[q]);
}

// The carry (optional), per channel: v_c . u is the predictive mean (c = 0) / gradient (c = 1 + q) of the point under the
// posterior BEFORE this update (u = the current posterior mean on the grid) -- mean_out, [n][C], makes the separate gather launch
// of a streaming step unnecessary -- and innov_c = wb_c y_c - wa_c (v_c . u): res += sum_c v_c innov_c keeps res = b - z - A u
// exact under the increment (b, A) += (W^T wb y, W^T wa W), so the next warm-started solve needs no A u product.
template <typename real, int C>
__device__ __forceinline__ void half_carry(const real* __restrict__ u, const real yw[C], const real wac[C], const real wu[C],
                                           real* __restrict__ mean_out, int64_t p, bool writer, real innov[C]) {
#pragma unroll
  for (int c = 0; c < C; ++c) innov[c] = yw[c];
  if (u) {
#pragma unroll
    for (int c = 0; c < C; ++c) innov[c] -= wac[c] * wu[c];
    if (mean_out && writer) {
#pragma unroll
      for (int c = 0; c < C; ++c) mean_out[p * C + c] = wu[c];
    }
  }
}

// The atomics of the lane's own taps: b += sum_c v_c wb_c y_c, res += sum_c v_c innov_c, and cnt -- the row sums of the increment
// (preconditioner density model) -- receives the value channel's row sums plus the diagonal the derivative channels add:
// cnt[a] += wa_0 v_0[a] + sum_{c >= 1} wa_c v_c[a]^2.
template <typename real, int D, int C>
__device__ __forceinline__ void half_tap_atomics(bool valid, const int flat_t[HalfTaps<D>::TPL], const real val_t[HalfTaps<D>::TPL][C],
                                                 const real yw[C], const real wac[C], const real innov[C], real* __restrict__ b,
                                                 real* __restrict__ cnt, real* __restrict__ res) {
#pragma unroll
  for (int t = 0; t < HalfTaps<D>::TPL; ++t) {
    real sb = val_t[t][0] * yw[0], sc = wac[0] * val_t[t][0], sr = val_t[t][0] * innov[0];
    bool touched = val_t[t][0] != (real)0;
#pragma unroll
    for (int c = 1; c < C; ++c) {
      const real v = val_t[t][c];
      touched |= v != (real)0;
      sb += v * yw[c];
      sr += v * innov[c];
      sc += wac[c] * v * v;
    }
    if (valid && touched) {
      atomic_add_real(b + flat_t[t], sb);
      if (cnt) atomic_add_real(cnt + flat_t[t], sc);
      if (res) atomic_add_real(res + flat_t[t], sr);
    }
  }
}

// The same adds of a single-channel fp32 point at d = 3 through the tap stage (AbsorbArgs::tap_stage): b, cnt and res of a node are
// floats 0..2 of its 16-byte record, so the 4 taps of a row run (consecutive rows) are 64 contiguous bytes -- 1.75 memory-side requests
// of 64 bytes per run on average with 12 lanes each, against 2 x 3 with 4 lanes each on the three arrays (the atomics are
// request-bound, scatter_owner.h).  Four wave instructions per point: instruction k covers the taps 16 k .. 16 k + 15, lane l the
// component l & 3 of tap 16 k + (l >> 2), read from the wave's tables -- call it behind the barrier that follows half_tap_table.
__device__ __forceinline__ void half_tap_stage(bool valid, int lane, const float* sv, const int* si, float yw, float wac, float innov,
                                               float* __restrict__ stage) {
  const int c = lane & 3;
  const float coef = c == 0 ? yw : (c == 1 ? wac : innov);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int a = 16 * k + (lane >> 2);
    const float v = sv[a];
    if (valid && c != 3 && v != 0.f) unsafeAtomicAdd(stage + (int64_t)si[a] * 4 + c, v * coef);
  }
}

// A[a, b] += sum_c wa_c v_c[a] v_c[b] over the tap pairs of the first `npair` prefix pairs of s_pair, one atomic per tap pair.
// The symmetric half stencil (the model's native W^T D^-1 W storage) is "row-interleaved":
// with P = the leading d-1 stencil digits of an offset and s its innermost digit, only offsets >= centre
// are kept, grouped by g = P - P_centre:
//   group 0      :  A_h[4 i + (s - 3)]                 s = 3..6   (4 reals per row; s = 3 is the diagonal)
//   group g >= 1 :  A_h[(7 g - 3) m + 7 i + s]         s = 0..6   (7 reals per row)
// -- (7^d + 1)/2 * m reals in total, the same as a row-major [(7^d+1)/2][m] half stencil.  The layout is
// chosen for this loop: one wave per point, lane = (a2, b2, pair slot) with a2/b2 the innermost tap
// digits of taps a/b, looping over the (prefix_a <= prefix_b) pairs four at a time.  The 16 (a2, b2)
// combinations of a pair land in one 88-byte span (rows i..i+3 x 7 slots), so a wave instruction touches
// ~9 cache lines with ~7 lanes each instead of 16 lines with 4 lanes (offset-major layout) -- measured
// 72 us vs 208 us per 4096 uniform points at 50^3 (the memory-side atomic units are transaction-bound).
// The stencil SpMV re-tiles the 7-wide rows through LDS (solve.hip).
// With C > 1 the channels of `amask` (those with wa_c != 0, the same in every lane) are summed in registers first; a kernel that
// always holds the whole stencil passes HalfTaps<D>::NPAIR and gets a compile-time trip count.
template <typename real, int D, int C>
__device__ __forceinline__ void half_pair_loop(int lane, int npair, const int* s_pair, const real* sv, const int* si, const real wac[C],
                                               int amask, real* __restrict__ A, int64_t m) {
  const int a2 = lane & 3, b2 = (lane >> 2) & 3, ps = lane >> 4;
#pragma unroll 2
  for (int t0 = 0; t0 < npair; t0 += 4) {
    const int t = t0 + ps;
    if (t < npair) {
      const int pk = s_pair[t];
      const int g = pk >> 16;
      const int a = (pk & 0xff) * 4 + a2;
      const real* __restrict__ va = sv + a * C;
      const real* __restrict__ vb = sv + (((pk >> 8) & 0xff) * 4 + b2) * C;
      real v;
      if constexpr (C == 1) {
        v = wac[0] * va[0] * vb[0];
      } else {
        v = (real)0;
#pragma unroll
        for (int c = 0; c < C; ++c)
          if ((amask >> c) & 1) v += wac[c] * va[c] * vb[c];
      }
      const int64_t row = si[a];
      if (g == 0) {
        if (b2 >= a2 && v != (real)0) stencil_atomic(A + row * 4 + (b2 - a2), v);
      } else if (v != (real)0) {
        stencil_atomic(A + (int64_t)(7 * g - 3) * m + row * 7 + (b2 - a2 + 3), v);
      }
    }
  }
}
