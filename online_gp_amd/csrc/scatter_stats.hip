// a2+a3+a4+a5: streaming accumulation of the additive sufficient statistics
//   b  = W^T D^-1 y   (interpolation_cache, BFN:46,160)
//   A  = W^T D^-1 W   (WtW, BFN:50-53; URLT:58 `tensor + V V^T`), block stencil
//   c  = y^T D^-1 y   (response_cache, BFN:45), ld = logdet D (BFN:55)
// The reference densifies W^T (m x q) and adds a dense m x m outer product per
// update; here each streamed point touches exactly its 4^d x 4^d stencil block.
#include "absorb.h"
#include "scatter_half.h"
#include <atomic>
#include <cmath>
#include <cstdlib>

// What the point-sweeping kernels of an absorb (k_scatter_stats_sym, k_bin_points) do before their first point.  False: a guarded
// launch (AbsorbArgs::guard) that is not to happen.  Otherwise the two zero regions are cleared on the way, grid-strided.
// nt / nb = blockDim.x / gridDim.x: read in here they would lose what the kernel's launch bounds tell the compiler about them.
__device__ __forceinline__ bool absorb_prologue(const long long* __restrict__ guard, long long guard_expect, uint32_t* __restrict__ z1, int64_t n1,
                                                uint32_t* __restrict__ z2, int64_t n2, unsigned nt, unsigned nb) {
  if (guard && *guard != guard_expect) return false;
  for (int64_t e = (int64_t)blockIdx.x * nt + threadIdx.x; e < n1; e += (int64_t)nb * nt) z1[e] = 0u;
  for (int64_t e = (int64_t)blockIdx.x * nt + threadIdx.x; e < n2; e += (int64_t)nb * nt) z2[e] = 0u;
  return true;
}

// GRP = min(T, 64) lanes cooperate on one point (lane <-> tap a); each lane
// walks all taps b and issues fire-and-forget L2 atomics on A_st[o(a,b)][idx_a].
// Tap values are exchanged through LDS (broadcast reads, conflict-free).
// This is the full offset-major form A_st[o][i] (all 7^d offsets, T^2 atomics per point); the model itself
// keeps the symmetric half (k_scatter_stats_sym below: T(T+1)/2 atomics, ~5x faster).
template <typename real, int D>
__global__ __launch_bounds__(256) void k_scatter_stats(GridDev<real> G, const real* __restrict__ x, const real* __restrict__ y,
                                                       const real* __restrict__ wa, const real* __restrict__ wb,
                                                       const real* __restrict__ noise, int64_t n, real* __restrict__ b,
                                                       real* __restrict__ A_st, double* __restrict__ stats, int32_t* __restrict__ err,
                                                       real* __restrict__ cnt) {
  constexpr int T = 1 << (2 * D);
  constexpr int GRP = T < 64 ? T : 64;      // lanes per point
  constexpr int PPB = 256 / GRP;            // points per block pass
  constexpr int TPL = T / GRP;              // taps per lane
  __shared__ real s_val[PPB][T];
  __shared__ double s_red[16];
  const int sub = threadIdx.x % GRP;
  const int loc = threadIdx.x / GRP;
  int R = 1;
#pragma unroll
  for (int q = 0; q < D; ++q) R *= 7;
  const int center = (R - 1) / 2;
  bool bad = false;

  for (int64_t base = (int64_t)blockIdx.x * PPB; base < n; base += (int64_t)gridDim.x * PPB) {
    const int64_t p = base + loc;
    const bool valid = p < n;
    int j0[D];
    real w[D][4];
    real yp = 0, wap = 0, wbp = 0;
    if (valid) {
      real xp[D];
#pragma unroll
      for (int q = 0; q < D; ++q) xp[q] = x[p * D + q];
      if (!point_stencil<real, D>(G, xp, j0, w)) flag_outside(err, sub == 0, bad);
      yp = y[p];
      wap = wa[p];
      wbp = wb[p];
    } else {
#pragma unroll
      for (int q = 0; q < D; ++q) {
        j0[q] = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) w[q][c] = 0;
      }
    }
    int idx_a[TPL], code_a[TPL];
    real val_a[TPL];
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
      const int a = sub + t * GRP;
      int flat = 0, code = 0;
      real v = (real)1;
#pragma unroll
      for (int q = 0; q < D; ++q) {
        const int c = tap_digit<D>(a, q);
        flat += (j0[q] + c) * G.stride[q];
        code = code * 7 + c;
        v *= w[q][c];
      }
      idx_a[t] = flat;
      code_a[t] = code;
      val_a[t] = v;
      s_val[loc][a] = v;
    }
    __syncthreads();
    if (valid) {
#pragma unroll
      for (int t = 0; t < TPL; ++t) {
        if (val_a[t] != (real)0) {
          atomic_add_real(b + idx_a[t], val_a[t] * yp * wbp);
          if (cnt) atomic_add_real(cnt + idx_a[t], val_a[t] * wap);     // row sums of the increment (preconditioner density model)
          if (A_st) {
            const real va = val_a[t] * wap;
            real* __restrict__ Arow = A_st + idx_a[t];
            const int obase = center - code_a[t];
#pragma unroll 4
            for (int bb0 = 0; bb0 < T; ++bb0) {
              // skew the last-dim digit of b by this lane's own last-dim digit: the 4 lanes that share
              // (c0, c1) of tap a then target the same stencil offset at 4 consecutive rows, i.e. one
              // 16-byte run of A -- up to 4 lane-atomics per L2 transaction instead of 1.
              const int bb = (bb0 & ~3) | ((bb0 + (sub + t * GRP)) & 3);
              int codeb = 0;
#pragma unroll
              for (int q = 0; q < D; ++q) codeb = codeb * 7 + tap_digit<D>(bb, q);
              const real vb = s_val[loc][bb];
              if (vb != (real)0) atomic_add_real(Arow + (int64_t)(obase + codeb) * G.m, va * vb);
            }
          }
        }
      }
    }
    __syncthreads();
  }
  scatter_stats_pass<real, D>(G, x, y, wb, noise, n, stats, s_red);
  if (bad) atomicOr(err, 1);
}

// Symmetric half-stencil accumulation (the model's native W^T D^-1 W storage; the row-interleaved layout and the point sweep are
// scatter_half.h), with everything the plain form carries besides: the guard, the zero regions, stencil shards, batched outputs.
// STAGE (float, D = 3, one output, whole stencil, cnt / u / res given -- absorb_validate): the per-tap adds go into the records of
// tap_stage instead of b / cnt / res (half_tap_stage); a kernel of its own, so that the direct form keeps its registers.
template <typename real, int D, bool STAGE = false>
__global__ __launch_bounds__(256) void k_scatter_stats_sym(GridDev<real> G, const real* __restrict__ x, const real* __restrict__ y,
                                                           const real* __restrict__ wa, const real* __restrict__ wb,
                                                           const real* __restrict__ noise, int64_t n, real* __restrict__ b,
                                                           real* __restrict__ A, double* __restrict__ stats, int32_t* __restrict__ err,
                                                           real* __restrict__ cnt, const real* __restrict__ u, real* __restrict__ res,
                                                           real* __restrict__ mean_out, uint32_t* __restrict__ z1, int64_t n1,
                                                           uint32_t* __restrict__ z2, int64_t n2, const long long* __restrict__ guard,
                                                           long long guard_expect, int g_lo, int g_hi, ScatterBatch bt,
                                                           real* __restrict__ tap_stage) {
  // the parameters are the members of AbsorbArgs (absorb.h), which documents them
  // several independent outputs in ONE launch (BFN:37-55 carries num_outputs as a batch dimension): blockIdx.y = output
  {
    const int64_t o = blockIdx.y;
    y += o * bt.y_stride; wa += o * bt.w_stride; wb += o * bt.w_stride; noise += o * bt.w_stride;
    b += o * bt.vec_stride; stats += 2 * o;
    if (A) A += o * bt.A_stride;
    if (cnt) cnt += o * bt.vec_stride;
    if (u) u += o * bt.vec_stride;
    if (res) res += o * bt.vec_stride;
  }
  if (!absorb_prologue(guard, guard_expect, z1, n1, z2, n2, blockDim.x, gridDim.x)) return;
  using H = HalfTaps<D>;
  __shared__ real s_val[4][H::T];
  __shared__ int s_idx[4][H::T];
  __shared__ int s_pair[H::NPAIR];
  __shared__ double s_red[16];
  const int lane = threadIdx.x & 63, loc = threadIdx.x >> 6;
  const int npair = half_pair_list<D>(s_pair, reinterpret_cast<int*>(s_red), g_lo, g_hi);
  bool bad = false;
  for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {
    const int64_t p = base + loc;
    const bool valid = p < n;
    int j0[D], flat_t[H::TPL];
    real w[D][4], val_t[H::TPL][1], yw[1] = {0}, wac[1] = {0}, wu[1], innov[1];
    half_point_setup<real, D>(G, x, p, n, lane == 0 && blockIdx.y == 0, err, bad, j0, w);      // (a dropped point counts once, not once per output)
    if (valid) {
      yw[0] = y[p] * wb[p];
      wac[0] = wa[p];
    }
    half_tap_table<real, D, 1>(G, j0, w, nullptr, lane, u, s_val[loc], s_idx[loc], flat_t, val_t, wu);
    half_carry<real, 1>(u, yw, wac, wu, mean_out, p, lane == 0 && valid, innov);
    if constexpr (!STAGE) half_tap_atomics<real, D, 1>(valid, flat_t, val_t, yw, wac, innov, b, cnt, res);
    __syncthreads();
    if constexpr (STAGE) half_tap_stage(valid, lane, s_val[loc], s_idx[loc], yw[0], wac[0], innov[0], tap_stage);
    if (valid && A) half_pair_loop<real, D, 1>(lane, npair, s_pair, s_val[loc], s_idx[loc], wac, 1, A, G.m);
    __syncthreads();
  }
  scatter_stats_pass<real, D>(G, x, y, wb, noise, n, stats, s_red);
  if (bad) atomicOr(err, 1);
}

#include "scatter_owner.h"
#include "scatter_grad.h"
#include "scatter_site.h"
#include "scatter_robust.h"
#include "scatter_window.h"
#include "scatter_interval.h"
#include "scatter_count.h"
#include "scatter_hetero.h"
#include "scatter_label.h"
#include "scatter_input_noise.h"
#include "scatter_grad_interval.h"
#include "scatter_revisit.h"

// Unpacks the row-interleaved half stencil into a full offset-major stencil full[o][i] = A[i, i + off(o)]
// (diagnostics, tests, and models handed a full-stencil cache):
//   full[c + oh][i] += h(oh, i);  full[c - oh][i + off(oh)] += h(oh, i) (oh > 0);  h(oh, i) = 0.
// Every full entry is touched by exactly one (oh, i), so no atomics.
template <typename real>
__global__ __launch_bounds__(256) void k_stencil_expand_add(GridDev<real> G, real* __restrict__ half, real* __restrict__ full) {
  const int m = G.m, d = G.d;
  const int c = (G.R - 1) / 2;
  const int oh = blockIdx.y;
  // flat offset of stencil index o = c + oh
  int rem = c + oh, off = 0;
  for (int q = d - 1; q >= 0; --q) {
    off += (rem % 7 - 3) * G.stride[q];
    rem /= 7;
  }
  const int g = oh < 4 ? 0 : (oh - 4) / 7 + 1;
  real* __restrict__ h = oh < 4 ? half + oh : half + (int64_t)(7 * g - 3) * m + (oh - 4) % 7;
  const int hs = oh < 4 ? 4 : 7;
  real* __restrict__ fd = full + (int64_t)(c + oh) * m;
  real* __restrict__ fm = full + (int64_t)(c - oh) * m;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m; i += gridDim.x * blockDim.x) {
    const real v = h[(int64_t)i * hs];
    if (v != (real)0) {
      fd[i] += v;
      if (oh > 0) {
        const int j = i + off;
        if (j >= 0 && j < m) fm[j] += v;
      }
      h[(int64_t)i * hs] = (real)0;
    }
  }
}

template <typename real>
static int expand_impl(const wiski_grid* grid, real* d_half, real* d_full, void* stream) {
  GridDev<real> G;
  int rc = make_grid_dev<real>(grid, &G);
  if (rc) return rc;
  if (!d_half || !d_full) return WISKI_E_BADARG;
  int bx = (G.m + 255) / 256;
  if (bx > 64) bx = 64;
  dim3 grd((unsigned)bx, (unsigned)((G.R + 1) / 2));
  hipLaunchKernelGGL((k_stencil_expand_add<real>), grd, dim3(256), 0, (hipStream_t)stream, G, d_half, d_full);
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

// batches at least this large take the owner-computes absorb when the caller provides its workspace (WISKI_OWNER_MIN_POINTS;
// 0 disables): its cost is a sweep over the touched part of A_h, that of the atomic form 19 ns per point
static int64_t owner_min_points() {
  static int64_t v = -1;
  if (v < 0) {
    const char* e = getenv("WISKI_OWNER_MIN_POINTS");
    // 50^3: 69 vs 79 us at 4096 uniform points (clustered: 80 vs 80), 255 vs 585 us at 32768.  At 4096 the streaming step gains
    // only 2 % (0.209 -> 0.205 ms): the rows written through the XCDs' L2s leave A_h less Infinity-Cache resident than memory-side
    // atomics do, and the SpMVs of the following solve slow down from 20.0 to 21.0 us -- so the default starts above that size
    v = e ? atoll(e) : 8192;
    if (v <= 0) v = (int64_t)1 << 62;
  }
  return v;
}

// Every combination of AbsorbArgs an absorb refuses, each with its reason.  Nothing has been launched when this returns.
template <typename real>
static int absorb_validate(const AbsorbArgs<real>& a, int d) {
  if (a.n == 0) return WISKI_OK;                       // nothing to absorb: not even the pointers are looked at
  // the tap stage: the plain single-output fp32 half-stencil atomic form at d = 3 with cnt and the carry pair, the whole stencil, only
  if (a.tap_stage && (sizeof(real) != 4 || d != 3 || !a.half || !a.cnt || !a.u || !a.res || a.nout != 1 || a.channels || a.sharded() ||
                      a.revisit() || a.hetero() || a.grad_interval() || a.site_form() || a.windowed()))
    return WISKI_E_BADARG;
  if (a.revisit()) {
    // revisit (scatter_revisit.h): the points are the slots of a ring of stored sites -- its x, wa, wb and noise, no y -- and the
    // launch is the single-output half-stencil atomic sweep with u, A and cnt: the whole group with a known form code, the
    // posterior variance at the slots, a noise scale, a damping in [0, 1], log Z -- and nothing of any other group: no full stencil,
    // no channels, no second output, no mean_out, no guard, zero regions, shard or owner workspace
    if (!a.x || !a.wa || !a.wb || !a.noise || !a.b || !a.stats || !a.err) return WISKI_E_BADARG;
    if (!a.half || !a.u || !a.A || !a.cnt || a.nout != 1 || a.channels || a.mean_out) return WISKI_E_BADARG;
    if (!a.site_d0 || !a.site_d1 || !a.site_ytilde || !a.site_omega || !a.site_codes || !a.site_change_out || !a.pvar || !a.logz_out) return WISKI_E_BADARG;
    if (a.site_form_code != WISKI_SITE_INTERVAL && a.site_form_code != WISKI_SITE_POISSON && a.site_form_code != WISKI_SITE_BINOMIAL) return WISKI_E_BADARG;
    if (!(a.sigma2 > 0) || !std::isfinite(a.sigma2) || !(a.site_damping >= 0 && a.site_damping <= 1)) return WISKI_E_BADARG;
    if (a.lo || a.hi || a.ytilde_out || a.omega_out || a.counted() || a.input_noise() || a.grad_interval() || a.hetero() || a.inv_scale || a.huber_c != (real)0 || a.windowed()) return WISKI_E_BADARG;
    if (a.guard || a.n1_bytes || a.n2_bytes || a.z1 || a.z2 || a.sharded() || a.bin || a.bin_bytes) return WISKI_E_BADARG;
    return WISKI_OK;
  }
  if (!a.x || (!a.y && !a.lo && !a.count_y && !a.clo) || !a.wa || !a.wb || !a.noise || !a.b || !a.stats || !a.err) return WISKI_E_BADARG;   // what every form reads and writes (the interval, count and channel-interval forms have no y)
  if (a.hetero()) {
    // heteroscedastic (scatter_hetero.h): the plain single-output half-stencil atomic absorb of y with u, A and cnt, twice -- the whole
    // second target set (res2 optional, as res), both variances, a noise scale, a finite prior mean, the five outputs -- and nothing
    // of any other group: no full stencil, no channels, no second output, no guard, zero regions, shard or owner workspace
    if (!a.y || !a.half || !a.u || !a.A || !a.cnt || a.nout != 1 || a.channels) return WISKI_E_BADARG;
    if (!a.b2 || !a.A2 || !a.cnt2 || !a.stats2 || !a.u2 || !a.pvar || !a.pvar2 || !a.e_out || !a.logzy_out) return WISKI_E_BADARG;
    if (!a.ytilde_out || !a.omega_out || !a.logz_out || !(a.sigma2 > 0) || !std::isfinite(a.sigma2) || !std::isfinite(a.g0)) return WISKI_E_BADARG;
    if (a.lo || a.hi || a.counted() || a.input_noise() || a.grad_interval() || a.inv_scale || a.huber_c != (real)0 || a.windowed()) return WISKI_E_BADARG;
    if (a.guard || a.n1_bytes || a.n2_bytes || a.z1 || a.z2 || a.sharded() || a.bin || a.bin_bytes) return WISKI_E_BADARG;
    return WISKI_OK;
  }
  if (a.grad_interval()) {
    // channel intervals (scatter_grad_interval.h): the derivative form's single-output half-stencil atomic absorb with u, A and cnt, the
    // whole group, a noise scale and the three outputs -- and nothing of any other group
    if (a.channels != d + 1 || !a.half || !a.u || !a.A || !a.cnt || !a.clo || !a.chi || !a.cpvar) return WISKI_E_BADARG;
    if (!a.ytilde_out || !a.omega_out || !a.logz_out || !(a.sigma2 > 0) || !std::isfinite(a.sigma2) || a.nout != 1) return WISKI_E_BADARG;
    if (a.lo || a.hi || a.pvar || a.counted() || a.input_noise() || a.inv_scale || a.huber_c != (real)0 || a.windowed()) return WISKI_E_BADARG;
    if (a.guard || a.n1_bytes || a.n2_bytes || a.z1 || a.z2 || a.sharded() || a.bin || a.bin_bytes) return WISKI_E_BADARG;
    return WISKI_OK;
  }
  if (a.site_form() || a.windowed()) {
    // The site-weighted forms (scatter_site.h) and the window form (scatter_window.h) are the plain single-output half-stencil
    // atomic absorb with cnt: their sites and sweeps need u; A and cnt are written unconditionally; no channels.  None of them
    // has a guard, zero regions, a shard or the owner workspace.  res and mean_out are optional: u alone is a complete request
    if (!a.u || !a.half || !a.A || !a.cnt || a.nout != 1 || a.channels) return WISKI_E_BADARG;
    if (a.guard || a.n1_bytes || a.n2_bytes || a.z1 || a.z2 || a.sharded() || a.bin || a.bin_bytes) return WISKI_E_BADARG;
    if (a.counted() || a.interval() || a.input_noise()) {
      // the matched forms: the posterior variance, a noise scale, their outputs (the noisy-input form's pseudo-target is y itself: it
      // has no ytilde_out); neither robust nor windowed
      if (!a.pvar || !a.omega_out || !a.logz_out || (a.ytilde_out == nullptr) != a.input_noise()) return WISKI_E_BADARG;
      if (!(a.sigma2 > 0) || !std::isfinite(a.sigma2)) return WISKI_E_BADARG;
      if (a.inv_scale || a.huber_c != (real)0 || a.windowed()) return WISKI_E_BADARG;
      // input noise (scatter_input_noise.h): its variances and the targets, and neither of the other two groups; count
      // (scatter_count.h): the whole group, and not the interval form's bounds; interval (scatter_interval.h): both bounds
      if (a.input_noise()) {
        if (!a.xvar || !a.y || a.counted() || a.lo || a.hi) return WISKI_E_BADARG;
      } else if (a.counted()) {
        if (a.lo || a.hi) return WISKI_E_BADARG;
        if (!a.count_y || !a.count_t || (a.count_family != WISKI_COUNT_POISSON && a.count_family != WISKI_COUNT_BINOMIAL)) return WISKI_E_BADARG;
      } else if (!a.lo || !a.hi) return WISKI_E_BADARG;
    } else if (a.windowed()) {
      // window: a whole ring with head inside it and no more entering points than slots, so that the slots of the launch are
      // distinct; void_left is used unconditionally; not the robust form either
      if (!a.ring_x || !a.ring_y || !a.ring_wa || !a.ring_wb || !a.ring_noise || !a.void_left) return WISKI_E_BADARG;
      if (a.ring_cap < 1 || a.ring_head < 0 || a.ring_head >= a.ring_cap || a.n > a.ring_cap) return WISKI_E_BADARG;
      if (a.inv_scale || a.omega_out || a.huber_c != (real)0) return WISKI_E_BADARG;
    } else if (!a.omega_out || !(a.huber_c > (real)0) || !std::isfinite(a.huber_c)) {
      return WISKI_E_BADARG;                             // robust (scatter_robust.h): omega_out is written unconditionally, a finite threshold
    }
    return WISKI_OK;
  }
  if (a.omega_out || a.huber_c != (real)0) return WISKI_E_BADARG;                                        // the robust group without inv_scale
  if (a.mean_out == nullptr && (a.u != nullptr) != (a.res != nullptr)) return WISKI_E_BADARG;            // a carry without the mean is the pair (u, res)
  if ((a.res && !a.u) || (a.mean_out && !a.u) || (a.u && !a.half)) return WISKI_E_BADARG;                // residual carry-over / mean: need u, half-stencil form only
  if (a.guard && !a.half) return WISKI_E_BADARG;                                                         // so is the guard
  // zero regions: whole words, with somewhere to write them, half-stencil form only
  if ((a.n1_bytes | a.n2_bytes) & 3 || (a.n1_bytes && !a.z1) || (a.n2_bytes && !a.z2) || ((a.n1_bytes || a.n2_bytes) && !a.half)) return WISKI_E_BADARG;
  if (a.sharded() && !a.half) return WISKI_E_BADARG;                                                     // stencil groups are groups of the half stencil
  // batched outputs: the plain half-stencil absorb (with cnt and the carry pair) only
  if (a.nout < 1 || (a.nout > 1 && (!a.half || a.mean_out || a.n1_bytes || a.n2_bytes || a.guard))) return WISKI_E_BADARG;
  // channels (value + d partials per point, scatter_grad.h): d + 1 of them, on the plain single-output half-stencil absorb only
  if (a.channels && (a.channels != d + 1 || !a.half || a.guard || a.n1_bytes || a.n2_bytes || a.sharded() || a.nout > 1)) return WISKI_E_BADARG;
  return WISKI_OK;
}

// Large single-output batches on a d = 3 half stencil with a binning workspace take the owner-computes form (scatter_owner.h);
// a stencil shard never does (the owner form walks whole lines).  Its LDS accumulators ((g2 * 175 + 512) reals per block:
// 172 slots + b, cnt, res per row, one scratch word per thread) must fit the device limit and the opt-in must succeed HERE,
// before the first kernel of the pair is queued -- k_bin_points already updates statistics; otherwise the atomic form runs.
template <typename real>
static size_t owner_lds_bytes(const GridDev<real>& G) { return ((size_t)G.g[2] * (172 + 3) + 512) * sizeof(real); }

template <typename real>
static bool owner_applies(const GridDev<real>& G, const AbsorbArgs<real>& a) {
  if (a.sharded() || a.nout != 1 || a.channels || !a.half || G.d != 3 || !a.bin || !a.cnt || !a.A) return false;
  if (G.g[2] > 64 || G.g[0] <= 3 || G.g[1] <= 3 || G.g[2] <= 3 || a.n >= (int64_t)1 << 31) return false;
  if (a.n < owner_min_points() || a.bin_bytes < owner_work_bytes<real>(G, a.n)) return false;
  static int lds_max = -1;
  static size_t lds_set = 0;
  if (lds_max < 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) v = 64 * 1024;
    lds_max = v;
  }
  const size_t lds = owner_lds_bytes(G);
  if (lds > (size_t)lds_max) return false;
  if (lds > 48 * 1024 && lds > lds_set) {
    if (hipFuncSetAttribute((const void*)k_owner_lines<real, OWNER_NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
      (void)hipGetLastError();
      return false;                                    // the atomic form needs no opt-in
    }
    lds_set = lds;
  }
  return true;
}

template <typename real>
static int launch_owner(const GridDev<real>& G, const AbsorbArgs<real>& a, hipStream_t stream) {
  static std::atomic<unsigned> epoch_src{0};
  unsigned epoch = ++epoch_src;                        // never 0 (a zero-initialised head is "empty")
  if (!epoch) epoch = ++epoch_src;
  const int64_t n = a.n, ncell = (int64_t)(G.g[0] - 3) * (G.g[1] - 3) * (G.g[2] - 3);
  char* w = static_cast<char*>(a.bin);                 // heads | next | records (owner_work_bytes)
  unsigned long long* head = reinterpret_cast<unsigned long long*>(w);
  int32_t* next = reinterpret_cast<int32_t*>(w + (ncell * 8 + 255) / 256 * 256);
  real* rec = reinterpret_cast<real*>(w + (ncell * 8 + 255) / 256 * 256 + (n * 4 + 255) / 256 * 256);
  int64_t nb = (n + 3) / 4;
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL((k_bin_points<real>), dim3((unsigned)nb), dim3(256), 0, stream, G, a.x, a.y, a.wa, a.wb, a.noise, n, a.stats, a.err, a.u,
                     a.res != nullptr ? 1 : 0, a.mean_out, head, next, rec, epoch, (uint32_t*)a.z1, a.n1_bytes / 4, (uint32_t*)a.z2, a.n2_bytes / 4,
                     (const long long*)a.guard, (long long)a.guard_expect);
  hipLaunchKernelGGL((k_owner_lines<real, OWNER_NT>), dim3((unsigned)(G.g[0] * G.g[1])), dim3(OWNER_NT), owner_lds_bytes(G), stream, G, a.A, a.b, a.cnt, a.res,
                     (const unsigned long long*)head, (const int32_t*)next, (const real*)rec, epoch, (const long long*)a.guard, (long long)a.guard_expect);
  return hipGetLastError() == hipSuccess ? WISKI_OK : WISKI_E_LAUNCH;
}

template <typename real>
static int launch_atomic(const GridDev<real>& G, const AbsorbArgs<real>& a, hipStream_t stream) {
  const int grp = a.half ? 64 : (G.T < 64 ? G.T : 64);
  const int64_t ppb = 256 / grp;
  int64_t blocks = (a.n + ppb - 1) / ppb;
  if (blocks > 256 * 8) blocks = 256 * 8;
  dim3 grd((unsigned)blocks, (unsigned)a.nout);
  ScatterBatch bt = a.bt;
  bt.vec_stride = G.m;                                 // b / cnt / u / res of consecutive outputs are one grid vector apart
  if constexpr (sizeof(real) == 4) {
    if (a.tap_stage) {                                 // (absorb_validate: d = 3, half, one output, cnt / u / res, the whole stencil)
      hipLaunchKernelGGL((k_scatter_stats_sym<float, 3, true>), grd, dim3(256), 0, stream, G, a.x, a.y, a.wa, a.wb, a.noise, a.n, a.b, a.A, a.stats, a.err,
                         a.cnt, a.u, a.res, a.mean_out, (uint32_t*)a.z1, a.n1_bytes / 4, (uint32_t*)a.z2, a.n2_bytes / 4, (const long long*)a.guard,
                         (long long)a.guard_expect, a.g_lo, a.g_hi, bt, a.tap_stage);
      WISKI_LAUNCH_CHECK();
      return WISKI_OK;
    }
  }
#define CALL(DD)                                                                                                                                             \
  do {                                                                                                                                                       \
    if (a.half) hipLaunchKernelGGL((k_scatter_stats_sym<real, DD>), grd, dim3(256), 0, stream, G, a.x, a.y, a.wa, a.wb, a.noise, a.n, a.b, a.A, a.stats, a.err, \
                                   a.cnt, a.u, a.res, a.mean_out, (uint32_t*)a.z1, a.n1_bytes / 4, (uint32_t*)a.z2, a.n2_bytes / 4, (const long long*)a.guard,  \
                                   (long long)a.guard_expect, a.g_lo, a.g_hi, bt, (real*)nullptr);                                                              \
    else hipLaunchKernelGGL((k_scatter_stats<real, DD>), grd, dim3(256), 0, stream, G, a.x, a.y, a.wa, a.wb, a.noise, a.n, a.b, a.A, a.stats, a.err, a.cnt);     \
  } while (0)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

template <typename real>
int absorb(const wiski_grid* grid, const AbsorbArgs<real>& a, void* stream) {
  // validation comes first: no branch below may start mutating statistics on arguments another branch would have refused
  GridDev<real> G;
  int rc = make_grid_dev<real>(grid, &G);
  if (rc == WISKI_OK) rc = absorb_validate(a, G.d);
  if (rc != WISKI_OK || a.n == 0) return rc;
  if (a.revisit()) return launch_revisit(G, a, (hipStream_t)stream);
  if (a.hetero()) return launch_hetero(G, a, (hipStream_t)stream);
  if (a.grad_interval()) return launch_grad_site(G, a, (hipStream_t)stream);
  if (a.input_noise()) return launch_site(G, a, SiteInputNoise<real>::of(a, *grid), (hipStream_t)stream);
  if (a.counted()) return launch_site(G, a, SiteCount<real>::of(a), (hipStream_t)stream);
  if (a.interval()) return launch_site(G, a, SiteInterval<real>::of(a), (hipStream_t)stream);
  if (a.windowed()) return launch_window(G, a, (hipStream_t)stream);
  if (a.inv_scale) return launch_site(G, a, SiteRobust<real>::of(a), (hipStream_t)stream);
  if (a.channels) return launch_grad(G, a, (hipStream_t)stream);
  return owner_applies(G, a) ? launch_owner(G, a, (hipStream_t)stream) : launch_atomic(G, a, (hipStream_t)stream);
}
template int absorb<float>(const wiski_grid*, const AbsorbArgs<float>&, void*);
template int absorb<double>(const wiski_grid*, const AbsorbArgs<double>&, void*);

// the points and targets every entry point passes on, in the order of its own parameter list
template <typename real>
static AbsorbArgs<real> absorb_args(const real* x, const real* y, const real* wa, const real* wb, const real* noise, int64_t n, real* b, real* A, bool half,
                                    double* stats, int32_t* err) {
  AbsorbArgs<real> a;
  a.x = x; a.y = y; a.wa = wa; a.wb = wb; a.noise = noise; a.n = n;
  a.b = b; a.A = A; a.half = half; a.stats = stats; a.err = err;
  return a;
}
// cnt and the carry, as the entry points that take them list them
template <typename real>
static void absorb_carry(AbsorbArgs<real>& a, real* cnt, const real* u, real* res, real* mean_out = nullptr) {
  a.cnt = cnt; a.u = u; a.res = res; a.mean_out = mean_out;
}
// the zero regions and the guard of a streaming step
template <typename real>
static void absorb_step(AbsorbArgs<real>& a, void* z1, int64_t n1, void* z2, int64_t n2, const void* guard, int64_t guard_expect) {
  a.z1 = z1; a.n1_bytes = n1; a.z2 = z2; a.n2_bytes = n2; a.guard = guard; a.guard_expect = guard_expect;
}
// the public record (wiski_absorb_args, include/wiski.h) as the typed one
template <typename real>
static AbsorbArgs<real> absorb_args(const wiski_absorb_args& p) {
  AbsorbArgs<real> a = absorb_args((const real*)p.d_x, (const real*)p.d_y, (const real*)p.d_wa, (const real*)p.d_wb, (const real*)p.d_noise, p.n, (real*)p.d_b,
                                   (real*)p.d_A, p.half != 0, p.d_stats, p.d_err);
  absorb_carry(a, (real*)p.d_cnt, (const real*)p.d_u, (real*)p.d_res, (real*)p.d_mean_out);
  absorb_step(a, p.z1, p.n1_bytes, p.z2, p.n2_bytes, p.d_guard, p.guard_expect);
  a.bin = p.d_bin; a.bin_bytes = p.bin_bytes;
  if (p.g_hi > 0) { a.g_lo = p.g_lo; a.g_hi = p.g_hi; }
  a.nout = p.nout; a.bt.y_stride = p.y_stride; a.bt.w_stride = p.w_stride; a.bt.A_stride = p.A_stride;
  a.channels = p.channels;
  return a;
}

// The bodies of the extern "C" entry points below (include/wiski.h documents each), once for both scalar types.
template <typename real>
static int entry_absorb(const wiski_grid* g, const wiski_absorb_args* p, void* s) { return p ? absorb(g, absorb_args<real>(*p), s) : WISKI_E_BADARG; }
// One per observation form: the record plus the form's own arguments.  The argument that makes the record this form's (without it
// absorb_validate would read another form's request) is required here; everything else is absorb_validate's to refuse.
template <typename real>
static int entry_robust(const wiski_grid* g, const wiski_absorb_args* p, const real* inv_scale, real huber_c, real* omega_out, void* s) {
  if (!p || !inv_scale) return WISKI_E_BADARG;
  AbsorbArgs<real> a = absorb_args<real>(*p);
  a.inv_scale = inv_scale; a.huber_c = huber_c; a.omega_out = omega_out;
  return absorb(g, a, s);
}
template <typename real>
static int entry_window(const wiski_grid* g, const wiski_absorb_args* p, const wiski_window_ring* r, int32_t* void_left, void* s) {
  if (!p || !r || !r->d_x) return WISKI_E_BADARG;
  AbsorbArgs<real> a = absorb_args<real>(*p);
  a.ring_x = (real*)r->d_x; a.ring_y = (real*)r->d_y; a.ring_wa = (real*)r->d_wa; a.ring_wb = (real*)r->d_wb; a.ring_noise = (real*)r->d_noise;
  a.ring_cap = r->cap; a.ring_head = r->head; a.void_left = void_left;
  return absorb(g, a, s);
}
template <typename real>
static int entry_interval(const wiski_grid* g, const wiski_absorb_args* p, const real* lo, const real* hi, const real* pvar, double sigma2, real* ytilde_out, real* omega_out, double* logz_out, void* s) {
  if (!p || !lo) return WISKI_E_BADARG;
  AbsorbArgs<real> a = absorb_args<real>(*p);
  a.y = nullptr;                                       // ignored by the form
  a.lo = lo; a.hi = hi; a.pvar = pvar; a.sigma2 = sigma2; a.ytilde_out = ytilde_out; a.omega_out = omega_out; a.logz_out = logz_out;
  return absorb(g, a, s);
}
template <typename real>
static int entry_grad_interval(const wiski_grid* g, const wiski_absorb_args* p, const real* lo, const real* hi, const real* pvar, double sigma2, real* ytilde_out, real* omega_out, double* logz_out, void* s) {
  if (!p || !lo) return WISKI_E_BADARG;
  AbsorbArgs<real> a = absorb_args<real>(*p);
  a.y = nullptr;                                       // ignored by the form
  a.clo = lo; a.chi = hi; a.cpvar = pvar; a.sigma2 = sigma2; a.ytilde_out = ytilde_out; a.omega_out = omega_out; a.logz_out = logz_out;
  return absorb(g, a, s);
}
template <typename real>
static int entry_count(const wiski_grid* g, const wiski_absorb_args* p, const real* cy, const real* ct, int family, const real* pvar, double sigma2, real* ytilde_out, real* omega_out, double* logz_out, void* s) {
  if (!p || !cy) return WISKI_E_BADARG;
  AbsorbArgs<real> a = absorb_args<real>(*p);
  a.y = nullptr;                                       // ignored by the form
  a.count_y = cy; a.count_t = ct; a.count_family = family; a.pvar = pvar; a.sigma2 = sigma2; a.ytilde_out = ytilde_out; a.omega_out = omega_out; a.logz_out = logz_out;
  return absorb(g, a, s);
}
template <typename real>
static int entry_label(const wiski_grid* g, const wiski_absorb_args* p, const real* labels, const real* pvar, const double* sigma2, real* ytilde_out, real* omega_out, double* logz_out, void* s) {
  return p ? label_absorb(g, absorb_args<real>(*p), labels, pvar, sigma2, ytilde_out, omega_out, logz_out, s) : WISKI_E_BADARG;
}
template <typename real>
static int entry_hetero(const wiski_grid* g, const wiski_absorb_args* p, const real* pvar, const real* pvar2, double sigma2, double g0, real* b2, real* A2_half, real* cnt2, const real* u2, real* res2, double* stats2, real* e_out, real* ytilde_out, real* omega_out, double* logz_out, double* logzy_out, void* s) {
  if (!p || (!b2 && p->n != 0)) return WISKI_E_BADARG;  // (n = 0 does nothing)
  AbsorbArgs<real> a = absorb_args<real>(*p);
  a.pvar = pvar; a.pvar2 = pvar2; a.sigma2 = sigma2; a.g0 = g0; a.b2 = b2; a.A2 = A2_half; a.cnt2 = cnt2; a.u2 = u2; a.res2 = res2; a.stats2 = stats2;
  a.e_out = e_out; a.ytilde_out = ytilde_out; a.omega_out = omega_out; a.logz_out = logz_out; a.logzy_out = logzy_out;
  return absorb(g, a, s);
}
template <typename real>
static int entry_input_noise(const wiski_grid* g, const wiski_absorb_args* p, const real* xvar, const real* gvar, const real* pvar, double sigma2, real* omega_out, double* logz_out, real* grad_out, void* s) {
  if (!p || !xvar) return WISKI_E_BADARG;
  AbsorbArgs<real> a = absorb_args<real>(*p);
  a.xvar = xvar; a.gvar = gvar; a.grad_out = grad_out; a.pvar = pvar; a.sigma2 = sigma2; a.omega_out = omega_out; a.logz_out = logz_out;
  return absorb(g, a, s);
}
// the revisit: the record's points are replaced by the ring's slots (its d_x / d_y / d_wa / d_wb / d_noise / n are not looked at)
template <typename real>
static int entry_revisit(const wiski_grid* g, const wiski_absorb_args* p, const wiski_site_ring* r, int form, const real* pvar, double sigma2, double damping, double* logz_out, real* change_out, void* s) {
  if (!p || !r || r->cap < 0 || (r->cap != 0 && !r->d_form)) return WISKI_E_BADARG;
  AbsorbArgs<real> a = absorb_args<real>(*p);
  a.x = (const real*)r->d_x; a.y = nullptr; a.wa = (const real*)r->d_wa; a.wb = (const real*)r->d_wb; a.noise = (const real*)r->d_noise; a.n = r->cap;
  a.site_d0 = (const real*)r->d_d0; a.site_d1 = (const real*)r->d_d1; a.site_ytilde = (real*)r->d_ytilde; a.site_omega = (real*)r->d_omega;
  a.site_codes = r->d_form; a.site_form_code = form; a.site_damping = damping; a.site_change_out = change_out;
  a.pvar = pvar; a.sigma2 = sigma2; a.logz_out = logz_out;
  return absorb(g, a, s);
}
template <typename real>
static int entry_plain(const wiski_grid* g, const real* x, const real* y, const real* wa, const real* wb, const real* noise, int64_t n, real* b, real* A, bool half, double* stats, int32_t* err, void* s) {
  return absorb(g, absorb_args(x, y, wa, wb, noise, n, b, A, half, stats, err), s);
}
template <typename real>
static int entry_cnt(const wiski_grid* g, const real* x, const real* y, const real* wa, const real* wb, const real* noise, int64_t n, real* b, real* A, int32_t half, real* cnt, const real* u, real* res, double* stats, int32_t* err, void* s) {
  AbsorbArgs<real> a = absorb_args(x, y, wa, wb, noise, n, b, A, half != 0, stats, err);
  absorb_carry(a, cnt, u, res);
  return absorb(g, a, s);
}
// the streaming step; `bin`: its owner workspace (plain step), [g_lo, g_hi): its stencil shard (sharded step)
template <typename real>
static int entry_step(const wiski_grid* g, const real* x, const real* y, const real* wa, const real* wb, const real* noise, int64_t n, real* b, real* A_half, real* cnt, const real* u, real* res, real* mean_out, double* stats, int32_t* err, void* z1, int64_t n1, void* z2, int64_t n2, const void* guard, int64_t guard_expect, void* bin, int64_t bin_bytes, int32_t g_lo, int32_t g_hi, void* s) {
  AbsorbArgs<real> a = absorb_args(x, y, wa, wb, noise, n, b, A_half, true, stats, err);
  absorb_carry(a, cnt, u, res, mean_out);
  absorb_step(a, z1, n1, z2, n2, guard, guard_expect);
  a.bin = bin; a.bin_bytes = bin_bytes;
  a.g_lo = g_lo; a.g_hi = g_hi;
  return absorb(g, a, s);
}
template <typename real>
static int entry_multi(const wiski_grid* g, const real* x, const real* y, const real* wa, const real* wb, const real* noise, int64_t n, int32_t nout, int64_t y_stride, int64_t w_stride, real* b, real* A_half, int64_t A_stride, real* cnt, const real* u, real* res, double* stats, int32_t* err, void* s) {
  AbsorbArgs<real> a = absorb_args(x, y, wa, wb, noise, n, b, A_half, true, stats, err);
  absorb_carry(a, cnt, u, res);
  a.nout = nout; a.bt.y_stride = y_stride; a.bt.w_stride = w_stride; a.bt.A_stride = A_stride;
  return absorb(g, a, s);
}
constexpr int32_t G_ALL = 1 << 30;                     // AbsorbArgs::g_hi of an unsharded absorb

extern "C" {
int wiski_absorb_f32(const wiski_grid* g, const wiski_absorb_args* p, void* s) { return entry_absorb<float>(g, p, s); }
int wiski_absorb_f64(const wiski_grid* g, const wiski_absorb_args* p, void* s) { return entry_absorb<double>(g, p, s); }
int wiski_absorb_staged_f32(const wiski_grid* g, const wiski_absorb_args* p, float* d_tap_stage, void* s) {
  if (!p || !d_tap_stage) return WISKI_E_BADARG;
  AbsorbArgs<float> a = absorb_args<float>(*p);
  a.tap_stage = d_tap_stage;
  return absorb(g, a, s);
}
int wiski_absorb_robust_f32(const wiski_grid* g, const wiski_absorb_args* p, const float* inv_scale, float huber_c, float* omega_out, void* s) { return entry_robust(g, p, inv_scale, huber_c, omega_out, s); }
int wiski_absorb_robust_f64(const wiski_grid* g, const wiski_absorb_args* p, const double* inv_scale, double huber_c, double* omega_out, void* s) { return entry_robust(g, p, inv_scale, huber_c, omega_out, s); }
int wiski_absorb_window_f32(const wiski_grid* g, const wiski_absorb_args* p, const wiski_window_ring* ring, int32_t* void_left, void* s) { return entry_window<float>(g, p, ring, void_left, s); }
int wiski_absorb_window_f64(const wiski_grid* g, const wiski_absorb_args* p, const wiski_window_ring* ring, int32_t* void_left, void* s) { return entry_window<double>(g, p, ring, void_left, s); }
int wiski_absorb_interval_f32(const wiski_grid* g, const wiski_absorb_args* p, const float* lo, const float* hi, const float* pvar, double sigma2, float* ytilde_out, float* omega_out, double* logz_out, void* s) { return entry_interval(g, p, lo, hi, pvar, sigma2, ytilde_out, omega_out, logz_out, s); }
int wiski_absorb_interval_f64(const wiski_grid* g, const wiski_absorb_args* p, const double* lo, const double* hi, const double* pvar, double sigma2, double* ytilde_out, double* omega_out, double* logz_out, void* s) { return entry_interval(g, p, lo, hi, pvar, sigma2, ytilde_out, omega_out, logz_out, s); }
int wiski_absorb_count_f32(const wiski_grid* g, const wiski_absorb_args* p, const float* y, const float* t, int family, const float* pvar, double sigma2, float* ytilde_out, float* omega_out, double* logz_out, void* s) { return entry_count(g, p, y, t, family, pvar, sigma2, ytilde_out, omega_out, logz_out, s); }
int wiski_absorb_count_f64(const wiski_grid* g, const wiski_absorb_args* p, const double* y, const double* t, int family, const double* pvar, double sigma2, double* ytilde_out, double* omega_out, double* logz_out, void* s) { return entry_count(g, p, y, t, family, pvar, sigma2, ytilde_out, omega_out, logz_out, s); }
int wiski_count_sites_f32(const float* mu, const float* pvar, const float* y, const float* t, int family, int64_t n, float* ytilde_out, float* omega_out, double* logz_out, void* s) { return count_sites_impl(mu, pvar, y, t, family, n, ytilde_out, omega_out, logz_out, s); }
int wiski_count_sites_f64(const double* mu, const double* pvar, const double* y, const double* t, int family, int64_t n, double* ytilde_out, double* omega_out, double* logz_out, void* s) { return count_sites_impl(mu, pvar, y, t, family, n, ytilde_out, omega_out, logz_out, s); }
int wiski_absorb_hetero_f32(const wiski_grid* g, const wiski_absorb_args* p, const float* pvar, const float* pvar2, double sigma2, double g0, float* b2, float* A2_half, float* cnt2, const float* u2, float* res2, double* stats2, float* e_out, float* ytilde_out, float* omega_out, double* logz_out, double* logzy_out, void* s) { return entry_hetero(g, p, pvar, pvar2, sigma2, g0, b2, A2_half, cnt2, u2, res2, stats2, e_out, ytilde_out, omega_out, logz_out, logzy_out, s); }
int wiski_absorb_hetero_f64(const wiski_grid* g, const wiski_absorb_args* p, const double* pvar, const double* pvar2, double sigma2, double g0, double* b2, double* A2_half, double* cnt2, const double* u2, double* res2, double* stats2, double* e_out, double* ytilde_out, double* omega_out, double* logz_out, double* logzy_out, void* s) { return entry_hetero(g, p, pvar, pvar2, sigma2, g0, b2, A2_half, cnt2, u2, res2, stats2, e_out, ytilde_out, omega_out, logz_out, logzy_out, s); }
int wiski_hetero_sites_f32(const float* mu, const float* pvar, const float* rho, const float* nu, int64_t n, float* ytilde_out, float* omega_out, double* logz_out, void* s) { return count_sites_impl<float, WISKI_COUNT_LOGVAR>(mu, pvar, rho, nu, WISKI_COUNT_LOGVAR, n, ytilde_out, omega_out, logz_out, s); }
int wiski_hetero_sites_f64(const double* mu, const double* pvar, const double* rho, const double* nu, int64_t n, double* ytilde_out, double* omega_out, double* logz_out, void* s) { return count_sites_impl<double, WISKI_COUNT_LOGVAR>(mu, pvar, rho, nu, WISKI_COUNT_LOGVAR, n, ytilde_out, omega_out, logz_out, s); }
int wiski_absorb_label_f32(const wiski_grid* g, const wiski_absorb_args* p, const float* labels, const float* pvar, const double* sigma2, float* ytilde_out, float* omega_out, double* logz_out, void* s) { return entry_label(g, p, labels, pvar, sigma2, ytilde_out, omega_out, logz_out, s); }
int wiski_absorb_label_f64(const wiski_grid* g, const wiski_absorb_args* p, const double* labels, const double* pvar, const double* sigma2, double* ytilde_out, double* omega_out, double* logz_out, void* s) { return entry_label(g, p, labels, pvar, sigma2, ytilde_out, omega_out, logz_out, s); }
int wiski_label_sites_f32(const float* mu, const float* pvar, const float* s_var, const float* labels, int32_t nout, int64_t n, float* ytilde_out, float* omega_out, double* logz_out, void* s) { return label_sites_impl(mu, pvar, s_var, labels, nout, n, ytilde_out, omega_out, logz_out, s); }
int wiski_label_sites_f64(const double* mu, const double* pvar, const double* s_var, const double* labels, int32_t nout, int64_t n, double* ytilde_out, double* omega_out, double* logz_out, void* s) { return label_sites_impl(mu, pvar, s_var, labels, nout, n, ytilde_out, omega_out, logz_out, s); }
int wiski_label_proba_f32(const float* mu, const float* pvar, const float* s_var, int32_t nout, int64_t n, double* proba_out, void* s) { return label_proba_impl(mu, pvar, s_var, nout, n, proba_out, s); }
int wiski_label_proba_f64(const double* mu, const double* pvar, const double* s_var, int32_t nout, int64_t n, double* proba_out, void* s) { return label_proba_impl(mu, pvar, s_var, nout, n, proba_out, s); }
int wiski_absorb_input_noise_f32(const wiski_grid* g, const wiski_absorb_args* p, const float* xvar, const float* gvar, const float* pvar, double sigma2, float* omega_out, double* logz_out, float* grad_out, void* s) { return entry_input_noise(g, p, xvar, gvar, pvar, sigma2, omega_out, logz_out, grad_out, s); }
int wiski_absorb_input_noise_f64(const wiski_grid* g, const wiski_absorb_args* p, const double* xvar, const double* gvar, const double* pvar, double sigma2, double* omega_out, double* logz_out, double* grad_out, void* s) { return entry_input_noise(g, p, xvar, gvar, pvar, sigma2, omega_out, logz_out, grad_out, s); }
int wiski_absorb_grad_interval_f32(const wiski_grid* g, const wiski_absorb_args* p, const float* lo, const float* hi, const float* pvar, double sigma2, float* ytilde_out, float* omega_out, double* logz_out, void* s) { return entry_grad_interval(g, p, lo, hi, pvar, sigma2, ytilde_out, omega_out, logz_out, s); }
int wiski_absorb_grad_interval_f64(const wiski_grid* g, const wiski_absorb_args* p, const double* lo, const double* hi, const double* pvar, double sigma2, double* ytilde_out, double* omega_out, double* logz_out, void* s) { return entry_grad_interval(g, p, lo, hi, pvar, sigma2, ytilde_out, omega_out, logz_out, s); }
int wiski_absorb_revisit_f32(const wiski_grid* g, const wiski_absorb_args* p, const wiski_site_ring* ring, int form, const float* pvar, double sigma2, double damping, double* logz_out, float* change_out, void* s) { return entry_revisit(g, p, ring, form, pvar, sigma2, damping, logz_out, change_out, s); }
int wiski_absorb_revisit_f64(const wiski_grid* g, const wiski_absorb_args* p, const wiski_site_ring* ring, int form, const double* pvar, double sigma2, double damping, double* logz_out, double* change_out, void* s) { return entry_revisit(g, p, ring, form, pvar, sigma2, damping, logz_out, change_out, s); }
int wiski_scatter_stats_f32(const wiski_grid* g, const float* x, const float* y, const float* wa, const float* wb, const float* noise, int64_t n, float* b, float* A, double* stats, int32_t* err, void* s) { return entry_plain(g, x, y, wa, wb, noise, n, b, A, false, stats, err, s); }
int wiski_scatter_stats_f64(const wiski_grid* g, const double* x, const double* y, const double* wa, const double* wb, const double* noise, int64_t n, double* b, double* A, double* stats, int32_t* err, void* s) { return entry_plain(g, x, y, wa, wb, noise, n, b, A, false, stats, err, s); }
int wiski_scatter_stats_sym_f32(const wiski_grid* g, const float* x, const float* y, const float* wa, const float* wb, const float* noise, int64_t n, float* b, float* A_half, double* stats, int32_t* err, void* s) { return entry_plain(g, x, y, wa, wb, noise, n, b, A_half, true, stats, err, s); }
int wiski_scatter_stats_sym_f64(const wiski_grid* g, const double* x, const double* y, const double* wa, const double* wb, const double* noise, int64_t n, double* b, double* A_half, double* stats, int32_t* err, void* s) { return entry_plain(g, x, y, wa, wb, noise, n, b, A_half, true, stats, err, s); }
int wiski_scatter_stats_cnt_f32(const wiski_grid* g, const float* x, const float* y, const float* wa, const float* wb, const float* noise, int64_t n, float* b, float* A, int32_t half, float* cnt, const float* u, float* res, double* stats, int32_t* err, void* s) { return entry_cnt(g, x, y, wa, wb, noise, n, b, A, half, cnt, u, res, stats, err, s); }
int wiski_scatter_stats_cnt_f64(const wiski_grid* g, const double* x, const double* y, const double* wa, const double* wb, const double* noise, int64_t n, double* b, double* A, int32_t half, double* cnt, const double* u, double* res, double* stats, int32_t* err, void* s) { return entry_cnt(g, x, y, wa, wb, noise, n, b, A, half, cnt, u, res, stats, err, s); }
int wiski_scatter_stats_step_f32(const wiski_grid* g, const float* x, const float* y, const float* wa, const float* wb, const float* noise, int64_t n, float* b, float* A_half, float* cnt, const float* u, float* res, float* mean_out, double* stats, int32_t* err, void* z1, int64_t n1, void* z2, int64_t n2, const void* guard, int64_t guard_expect, void* bin, int64_t bin_bytes, void* s) { return entry_step(g, x, y, wa, wb, noise, n, b, A_half, cnt, u, res, mean_out, stats, err, z1, n1, z2, n2, guard, guard_expect, bin, bin_bytes, 0, G_ALL, s); }
int wiski_scatter_stats_step_f64(const wiski_grid* g, const double* x, const double* y, const double* wa, const double* wb, const double* noise, int64_t n, double* b, double* A_half, double* cnt, const double* u, double* res, double* mean_out, double* stats, int32_t* err, void* z1, int64_t n1, void* z2, int64_t n2, const void* guard, int64_t guard_expect, void* bin, int64_t bin_bytes, void* s) { return entry_step(g, x, y, wa, wb, noise, n, b, A_half, cnt, u, res, mean_out, stats, err, z1, n1, z2, n2, guard, guard_expect, bin, bin_bytes, 0, G_ALL, s); }
int wiski_scatter_stats_step_sharded_f32(const wiski_grid* g, const float* x, const float* y, const float* wa, const float* wb, const float* noise, int64_t n, float* b, float* A_half, float* cnt, const float* u, float* res, float* mean_out, double* stats, int32_t* err, void* z1, int64_t n1, void* z2, int64_t n2, const void* guard, int64_t guard_expect, int32_t g_lo, int32_t g_hi, void* s) { return entry_step(g, x, y, wa, wb, noise, n, b, A_half, cnt, u, res, mean_out, stats, err, z1, n1, z2, n2, guard, guard_expect, (void*)nullptr, 0, g_lo, g_hi, s); }
int wiski_scatter_stats_step_sharded_f64(const wiski_grid* g, const double* x, const double* y, const double* wa, const double* wb, const double* noise, int64_t n, double* b, double* A_half, double* cnt, const double* u, double* res, double* mean_out, double* stats, int32_t* err, void* z1, int64_t n1, void* z2, int64_t n2, const void* guard, int64_t guard_expect, int32_t g_lo, int32_t g_hi, void* s) { return entry_step(g, x, y, wa, wb, noise, n, b, A_half, cnt, u, res, mean_out, stats, err, z1, n1, z2, n2, guard, guard_expect, (void*)nullptr, 0, g_lo, g_hi, s); }
int wiski_scatter_stats_multi_f32(const wiski_grid* g, const float* x, const float* y, const float* wa, const float* wb, const float* noise, int64_t n, int32_t nout, int64_t y_stride, int64_t w_stride, float* b, float* A_half, int64_t A_stride, float* cnt, const float* u, float* res, double* stats, int32_t* err, void* s) { return entry_multi(g, x, y, wa, wb, noise, n, nout, y_stride, w_stride, b, A_half, A_stride, cnt, u, res, stats, err, s); }
int wiski_scatter_stats_multi_f64(const wiski_grid* g, const double* x, const double* y, const double* wa, const double* wb, const double* noise, int64_t n, int32_t nout, int64_t y_stride, int64_t w_stride, double* b, double* A_half, int64_t A_stride, double* cnt, const double* u, double* res, double* stats, int32_t* err, void* s) { return entry_multi(g, x, y, wa, wb, noise, n, nout, y_stride, w_stride, b, A_half, A_stride, cnt, u, res, stats, err, s); }
int64_t wiski_scatter_bin_bytes(const wiski_grid* g, int64_t n, int32_t elem_size) {
  if (!g || g->d != 3 || n < 0 || (elem_size != 4 && elem_size != 8)) return -1;
  return elem_size == 4 ? owner_work_bytes<float>(*g, n) : owner_work_bytes<double>(*g, n);
}
int wiski_stencil_expand_add_f32(const wiski_grid* g, float* half, float* full, void* s) { return expand_impl<float>(g, half, full, s); }
int wiski_stencil_expand_add_f64(const wiski_grid* g, double* half, double* full, void* s) { return expand_impl<double>(g, half, full, s); }
}
