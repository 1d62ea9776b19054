// a2+a3+a4+a5: streaming accumulation of the additive sufficient statistics
//   b  = W^T D^-1 y   (interpolation_cache, BFN:46,160)
//   A  = W^T D^-1 W   (WtW, BFN:50-53; URLT:58 `tensor + V V^T`), block stencil
//   c  = y^T D^-1 y   (response_cache, BFN:45), ld = logdet D (BFN:55)
// The reference densifies W^T (m x q) and adds a dense m x m outer product per
// update; here each streamed point touches exactly its 4^d x 4^d stencil block.
#include "absorb.h"
#include <atomic>
#include <cmath>
#include <cstdlib>

// The half-stencil atomics of k_scatter_stats_sym.  Cache-policy bits on the fp32 atomic (sc1, nt, sc1 nt) leave A_h no better
// placed for the SpMV that follows -- SpMV dispatches right after the absorb / absorb kernel: default 18.0-18.2 us / 66.6-67.4 us,
// sc1 18.1-18.4 / 67.7, nt 18.3-18.4 / 69.3, sc1 nt 18.2-18.3 / 68.7 -- so it is the plain fire-and-forget add.
__device__ __forceinline__ void stencil_atomic(float* p, float v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void stencil_atomic(double* p, double v) { unsafeAtomicAdd(p, v); }

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

// A point outside the grid raises the flag and contributes nothing at all (zero weights; no y^2 / log-noise term either, so a
// caller that catches the error keeps statistics that agree with A and b).  `count`: the one lane that counts the point --
// bits 1..: number of training points dropped; bit 0 (any point outside) is set from `bad` when the kernel ends.
__device__ __forceinline__ void flag_outside(int32_t* __restrict__ err, bool count, bool& bad) {
  bad = true;
  if (count) atomicAdd(err, 2);
}

// stats[0] += sum wb y^2, stats[1] += sum log(noise) over the points inside the grid.  Atomics of many blocks on one address
// serialise at the memory side (~12 ns each): with one pair per block the 1 024 blocks of a q = 4 096 absorb spent 25 us of
// their 87 us queueing on these two doubles.  So a few designated blocks sweep the points once more (x, y, wb, noise: 24 B per
// point) and issue one pair each.
template <typename real, int D>
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
    if (point_stencil<real, D>(G, xp, j0, w)) {
      const double yp = (double)y[p];
      c_acc += yp * yp * (double)wb[p];
      ld_acc += log((double)noise[p]);
    }
  }
  const double c_tot = block_reduce_sum(c_acc, s_red);
  const double ld_tot = block_reduce_sum(ld_acc, s_red);
  if (threadIdx.x == 0 && (c_tot != 0 || ld_tot != 0)) {
    unsafeAtomicAdd(stats + 0, c_tot);
    unsafeAtomicAdd(stats + 1, ld_tot);
  }
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
        const int c = (a >> (2 * (D - 1 - q))) & 3;
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
              for (int q = 0; q < D; ++q) codeb = codeb * 7 + ((bb >> (2 * (D - 1 - q))) & 3);
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

// Symmetric half-stencil accumulation (the model's native W^T D^-1 W storage), "row-interleaved" layout:
// with P = the leading d-1 stencil digits of an offset and s its innermost digit, only offsets >= centre
// are kept, grouped by g = P - P_centre:
//   group 0      :  A_h[4 i + (s - 3)]                 s = 3..6   (4 reals per row; s = 3 is the diagonal)
//   group g >= 1 :  A_h[(7 g - 3) m + 7 i + s]         s = 0..6   (7 reals per row)
// -- (7^d + 1)/2 * m reals in total, the same as a row-major [(7^d+1)/2][m] half stencil.  The layout is
// chosen for this kernel: one wave per point, lane = (a2, b2, pair slot) with a2/b2 the innermost tap
// digits of taps a/b, looping over the (prefix_a <= prefix_b) pairs four at a time.  The 16 (a2, b2)
// combinations of a pair land in one 88-byte span (rows i..i+3 x 7 slots), so a wave instruction touches
// ~9 cache lines with ~7 lanes each instead of 16 lines with 4 lanes (offset-major layout) -- measured
// 72 us vs 208 us per 4096 uniform points at 50^3 (the memory-side atomic units are transaction-bound).
// The stencil SpMV re-tiles the 7-wide rows through LDS (solve.hip).
template <typename real, int D>
__global__ __launch_bounds__(256) void k_scatter_stats_sym(GridDev<real> G, const real* __restrict__ x, const real* __restrict__ y,
                                                           const real* __restrict__ wa, const real* __restrict__ wb,
                                                           const real* __restrict__ noise, int64_t n, real* __restrict__ b,
                                                           real* __restrict__ A, double* __restrict__ stats, int32_t* __restrict__ err,
                                                           real* __restrict__ cnt, const real* __restrict__ u, real* __restrict__ res,
                                                           real* __restrict__ mean_out, uint32_t* __restrict__ z1, int64_t n1,
                                                           uint32_t* __restrict__ z2, int64_t n2, const long long* __restrict__ guard,
                                                           long long guard_expect, int g_lo, int g_hi, ScatterBatch bt) {
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
  constexpr int T = 1 << (2 * D);
  constexpr int TP = T / 4;                      // tap prefixes (leading d-1 digits)
  constexpr int NPAIR = TP * (TP + 1) / 2;       // prefix pairs with code(pb) >= code(pa)
  constexpr int TPL = T > 64 ? T / 64 : 1;       // taps per lane when filling the per-point tables
  __shared__ real s_val[4][T];
  __shared__ int s_idx[4][T];
  __shared__ int s_pair[NPAIR];                  // pa | pb << 8 | g << 16
  __shared__ int s_scan[4];
  __shared__ double s_red[16];
  const int lane = threadIdx.x & 63, loc = threadIdx.x >> 6;
  int npair = 0;
  {  // compact list of the valid prefix pairs (block-cooperative stream compaction)
    int running = 0;
    for (int base = 0; base < TP * TP; base += 256) {
      const int idx = base + threadIdx.x;
      const int pa = idx / TP, pb = idx % TP;
      int ca = 0, cb = 0;
#pragma unroll
      for (int q = 0; q < D - 1; ++q) {
        ca = ca * 7 + ((pa >> (2 * (D - 2 - q))) & 3);
        cb = cb * 7 + ((pb >> (2 * (D - 2 - q))) & 3);
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
    npair = running;                              // block-uniform: NPAIR for the whole stencil, fewer for a shard
  }
  bool bad = false;
  const int64_t m = G.m;
  for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {
    const int64_t p = base + loc;
    const bool valid = p < n;
    int j0[D];
    real w[D][4];
    real yp = 0, wap = 0, wbp = 0;
    if (valid) {
      real xp[D];
#pragma unroll
      for (int q = 0; q < D; ++q) xp[q] = x[p * D + q];
      if (!point_stencil<real, D>(G, xp, j0, w)) flag_outside(err, lane == 0 && blockIdx.y == 0, bad);      // (a dropped point counts once, not once per output)
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
        if (u && v != (real)0) wu += v * u[flat];
      }
    }
    // residual carry-over (optional): res += W^T (wb y - wa (W u)) keeps res = b - z - A u exact under the
    // increment (b, A) += (W^T wb y, W^T wa W), so the next warm-started solve needs no A u product
    // w_p . u is also the predictive mean of the point under the posterior BEFORE this update (u = the current posterior mean
    // on the grid): mean_out makes the separate gather launch of a streaming step unnecessary
    real innov = yp * wbp;
    if (u) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) wu += __shfl_xor(wu, off, 64);
      innov -= wap * wu;
      if (mean_out && lane == 0 && valid) mean_out[p] = wu;
    }
#pragma unroll
    for (int t = 0; t < TPL; ++t) {
      if (valid && val_t[t] != (real)0) {
        atomic_add_real(b + flat_t[t], val_t[t] * yp * wbp);
        if (cnt) atomic_add_real(cnt + flat_t[t], val_t[t] * wap);     // row sums of the increment (preconditioner density model)
        if (res) atomic_add_real(res + flat_t[t], val_t[t] * innov);
      }
    }
    __syncthreads();
    if (valid && A) {
      const int a2 = lane & 3, b2 = (lane >> 2) & 3, ps = lane >> 4;
#pragma unroll 2
      for (int t0 = 0; t0 < npair; t0 += 4) {
        const int t = t0 + ps;
        if (t < npair) {
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
  scatter_stats_pass<real, D>(G, x, y, wb, noise, n, stats, s_red);
  if (bad) atomicOr(err, 1);
}

#include "scatter_owner.h"
#include "scatter_grad.h"
#include "scatter_robust.h"

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
  if (!a.x || !a.y || !a.wa || !a.wb || !a.noise || !a.b || !a.stats || !a.err) return WISKI_E_BADARG;   // what every form reads and writes
  if (a.inv_scale) {
    // robust (scatter_robust.h): the weights need u; A, cnt and omega_out are written unconditionally; the plain single-output
    // half-stencil atomic form only.  res and mean_out are optional here: u alone is a complete request
    if (!a.u || !a.half || !a.A || !a.cnt || !a.omega_out || a.nout != 1 || a.channels) return WISKI_E_BADARG;
    if (a.guard || a.n1_bytes || a.n2_bytes || a.z1 || a.z2 || a.sharded() || a.bin || a.bin_bytes) return WISKI_E_BADARG;
    if (!(a.huber_c > (real)0) || !std::isfinite(a.huber_c)) return WISKI_E_BADARG;
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
#define CALL(DD)                                                                                                                                             \
  do {                                                                                                                                                       \
    if (a.half) hipLaunchKernelGGL((k_scatter_stats_sym<real, DD>), grd, dim3(256), 0, stream, G, a.x, a.y, a.wa, a.wb, a.noise, a.n, a.b, a.A, a.stats, a.err, \
                                   a.cnt, a.u, a.res, a.mean_out, (uint32_t*)a.z1, a.n1_bytes / 4, (uint32_t*)a.z2, a.n2_bytes / 4, (const long long*)a.guard,  \
                                   (long long)a.guard_expect, a.g_lo, a.g_hi, bt);                                                                              \
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
  if (a.inv_scale) return launch_robust(G, a, (hipStream_t)stream);
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
// the public record (wiski_absorb_args, include/wiski.h) as the typed one
template <typename real>
static AbsorbArgs<real> absorb_args(const wiski_absorb_args& p) {
  AbsorbArgs<real> a = absorb_args((const real*)p.d_x, (const real*)p.d_y, (const real*)p.d_wa, (const real*)p.d_wb, (const real*)p.d_noise, p.n, (real*)p.d_b,
                                   (real*)p.d_A, p.half != 0, p.d_stats, p.d_err);
  a.cnt = (real*)p.d_cnt; a.u = (const real*)p.d_u; a.res = (real*)p.d_res; a.mean_out = (real*)p.d_mean_out;
  a.z1 = p.z1; a.n1_bytes = p.n1_bytes; a.z2 = p.z2; a.n2_bytes = p.n2_bytes; a.guard = p.d_guard; a.guard_expect = p.guard_expect;
  a.bin = p.d_bin; a.bin_bytes = p.bin_bytes;
  if (p.g_hi > 0) { a.g_lo = p.g_lo; a.g_hi = p.g_hi; }
  a.nout = p.nout; a.bt.y_stride = p.y_stride; a.bt.w_stride = p.w_stride; a.bt.A_stride = p.A_stride;
  a.channels = p.channels;
  return a;
}
extern "C" {
int wiski_absorb_f32(const wiski_grid* g, const wiski_absorb_args* p, void* s) { return p ? absorb(g, absorb_args<float>(*p), s) : WISKI_E_BADARG; }
int wiski_absorb_f64(const wiski_grid* g, const wiski_absorb_args* p, void* s) { return p ? absorb(g, absorb_args<double>(*p), s) : WISKI_E_BADARG; }
int wiski_scatter_stats_grad_f32(const wiski_grid* g, const float* x, const float* y, const float* wa, const float* wb, const float* noise, int64_t n, float* b, float* A_half, float* cnt, const float* u, float* res, float* mean_out, double* stats, int32_t* err, void* s) {
  AbsorbArgs<float> a = absorb_args(x, y, wa, wb, noise, n, b, A_half, true, stats, err);
  a.cnt = cnt; a.u = u; a.res = res; a.mean_out = mean_out;
  a.channels = g ? g->d + 1 : 0;
  return absorb(g, a, s);
}
int wiski_scatter_stats_grad_f64(const wiski_grid* g, const double* x, const double* y, const double* wa, const double* wb, const double* noise, int64_t n, double* b, double* A_half, double* cnt, const double* u, double* res, double* mean_out, double* stats, int32_t* err, void* s) {
  AbsorbArgs<double> a = absorb_args(x, y, wa, wb, noise, n, b, A_half, true, stats, err);
  a.cnt = cnt; a.u = u; a.res = res; a.mean_out = mean_out;
  a.channels = g ? g->d + 1 : 0;
  return absorb(g, a, s);
}
int wiski_scatter_stats_robust_f32(const wiski_grid* g, const float* x, const float* y, const float* wa, const float* wb, const float* noise, int64_t n, float* b, float* A_half, float* cnt, const float* u, float* res, float* mean_out, double* stats, int32_t* err, const float* inv_scale, float huber_c, float* omega_out, void* s) {
  AbsorbArgs<float> a = absorb_args(x, y, wa, wb, noise, n, b, A_half, true, stats, err);
  a.cnt = cnt; a.u = u; a.res = res; a.mean_out = mean_out;
  a.inv_scale = inv_scale; a.huber_c = huber_c; a.omega_out = omega_out;
  return inv_scale ? absorb(g, a, s) : WISKI_E_BADARG;
}
int wiski_scatter_stats_robust_f64(const wiski_grid* g, const double* x, const double* y, const double* wa, const double* wb, const double* noise, int64_t n, double* b, double* A_half, double* cnt, const double* u, double* res, double* mean_out, double* stats, int32_t* err, const double* inv_scale, double huber_c, double* omega_out, void* s) {
  AbsorbArgs<double> a = absorb_args(x, y, wa, wb, noise, n, b, A_half, true, stats, err);
  a.cnt = cnt; a.u = u; a.res = res; a.mean_out = mean_out;
  a.inv_scale = inv_scale; a.huber_c = huber_c; a.omega_out = omega_out;
  return inv_scale ? absorb(g, a, s) : WISKI_E_BADARG;
}
int wiski_absorb_robust_f32(const wiski_grid* g, const wiski_absorb_args* p, const float* inv_scale, float huber_c, float* omega_out, void* s) {
  if (!p || !inv_scale) return WISKI_E_BADARG;
  AbsorbArgs<float> a = absorb_args<float>(*p);
  a.inv_scale = inv_scale; a.huber_c = huber_c; a.omega_out = omega_out;
  return absorb(g, a, s);
}
int wiski_absorb_robust_f64(const wiski_grid* g, const wiski_absorb_args* p, const double* inv_scale, double huber_c, double* omega_out, void* s) {
  if (!p || !inv_scale) return WISKI_E_BADARG;
  AbsorbArgs<double> a = absorb_args<double>(*p);
  a.inv_scale = inv_scale; a.huber_c = huber_c; a.omega_out = omega_out;
  return absorb(g, a, s);
}
int wiski_scatter_stats_f32(const wiski_grid* g, const float* x, const float* y, const float* wa, const float* wb, const float* noise, int64_t n, float* b, float* A, double* stats, int32_t* err, void* s) {
  return absorb(g, absorb_args(x, y, wa, wb, noise, n, b, A, false, stats, err), s);
}
int wiski_scatter_stats_f64(const wiski_grid* g, const double* x, const double* y, const double* wa, const double* wb, const double* noise, int64_t n, double* b, double* A, double* stats, int32_t* err, void* s) {
  return absorb(g, absorb_args(x, y, wa, wb, noise, n, b, A, false, stats, err), s);
}
int wiski_scatter_stats_sym_f32(const wiski_grid* g, const float* x, const float* y, const float* wa, const float* wb, const float* noise, int64_t n, float* b, float* A_half, double* stats, int32_t* err, void* s) {
  return absorb(g, absorb_args(x, y, wa, wb, noise, n, b, A_half, true, stats, err), s);
}
int wiski_scatter_stats_sym_f64(const wiski_grid* g, const double* x, const double* y, const double* wa, const double* wb, const double* noise, int64_t n, double* b, double* A_half, double* stats, int32_t* err, void* s) {
  return absorb(g, absorb_args(x, y, wa, wb, noise, n, b, A_half, true, stats, err), s);
}
int wiski_scatter_stats_cnt_f32(const wiski_grid* g, const float* x, const float* y, const float* wa, const float* wb, const float* noise, int64_t n, float* b, float* A, int32_t half, float* cnt, const float* u, float* res, double* stats, int32_t* err, void* s) {
  AbsorbArgs<float> a = absorb_args(x, y, wa, wb, noise, n, b, A, half != 0, stats, err);
  a.cnt = cnt; a.u = u; a.res = res;
  return absorb(g, a, s);
}
int wiski_scatter_stats_cnt_f64(const wiski_grid* g, const double* x, const double* y, const double* wa, const double* wb, const double* noise, int64_t n, double* b, double* A, int32_t half, double* cnt, const double* u, double* res, double* stats, int32_t* err, void* s) {
  AbsorbArgs<double> a = absorb_args(x, y, wa, wb, noise, n, b, A, half != 0, stats, err);
  a.cnt = cnt; a.u = u; a.res = res;
  return absorb(g, a, s);
}
int wiski_scatter_stats_step_f32(const wiski_grid* g, const float* x, const float* y, const float* wa, const float* wb, const float* noise, int64_t n, float* b, float* A_half, float* cnt, const float* u, float* res, float* mean_out, double* stats, int32_t* err, void* z1, int64_t n1, void* z2, int64_t n2, const void* guard, int64_t guard_expect, void* bin, int64_t bin_bytes, void* s) {
  AbsorbArgs<float> a = absorb_args(x, y, wa, wb, noise, n, b, A_half, true, stats, err);
  a.cnt = cnt; a.u = u; a.res = res; a.mean_out = mean_out;
  a.z1 = z1; a.n1_bytes = n1; a.z2 = z2; a.n2_bytes = n2; a.guard = guard; a.guard_expect = guard_expect;
  a.bin = bin; a.bin_bytes = bin_bytes;
  return absorb(g, a, s);
}
int wiski_scatter_stats_step_f64(const wiski_grid* g, const double* x, const double* y, const double* wa, const double* wb, const double* noise, int64_t n, double* b, double* A_half, double* cnt, const double* u, double* res, double* mean_out, double* stats, int32_t* err, void* z1, int64_t n1, void* z2, int64_t n2, const void* guard, int64_t guard_expect, void* bin, int64_t bin_bytes, void* s) {
  AbsorbArgs<double> a = absorb_args(x, y, wa, wb, noise, n, b, A_half, true, stats, err);
  a.cnt = cnt; a.u = u; a.res = res; a.mean_out = mean_out;
  a.z1 = z1; a.n1_bytes = n1; a.z2 = z2; a.n2_bytes = n2; a.guard = guard; a.guard_expect = guard_expect;
  a.bin = bin; a.bin_bytes = bin_bytes;
  return absorb(g, a, s);
}
int wiski_scatter_stats_step_sharded_f32(const wiski_grid* g, const float* x, const float* y, const float* wa, const float* wb, const float* noise, int64_t n, float* b, float* A_half, float* cnt, const float* u, float* res, float* mean_out, double* stats, int32_t* err, void* z1, int64_t n1, void* z2, int64_t n2, const void* guard, int64_t guard_expect, int32_t g_lo, int32_t g_hi, void* s) {
  AbsorbArgs<float> a = absorb_args(x, y, wa, wb, noise, n, b, A_half, true, stats, err);
  a.cnt = cnt; a.u = u; a.res = res; a.mean_out = mean_out;
  a.z1 = z1; a.n1_bytes = n1; a.z2 = z2; a.n2_bytes = n2; a.guard = guard; a.guard_expect = guard_expect;
  a.g_lo = g_lo; a.g_hi = g_hi;
  return absorb(g, a, s);
}
int wiski_scatter_stats_step_sharded_f64(const wiski_grid* g, const double* x, const double* y, const double* wa, const double* wb, const double* noise, int64_t n, double* b, double* A_half, double* cnt, const double* u, double* res, double* mean_out, double* stats, int32_t* err, void* z1, int64_t n1, void* z2, int64_t n2, const void* guard, int64_t guard_expect, int32_t g_lo, int32_t g_hi, void* s) {
  AbsorbArgs<double> a = absorb_args(x, y, wa, wb, noise, n, b, A_half, true, stats, err);
  a.cnt = cnt; a.u = u; a.res = res; a.mean_out = mean_out;
  a.z1 = z1; a.n1_bytes = n1; a.z2 = z2; a.n2_bytes = n2; a.guard = guard; a.guard_expect = guard_expect;
  a.g_lo = g_lo; a.g_hi = g_hi;
  return absorb(g, a, s);
}
int wiski_scatter_stats_multi_f32(const wiski_grid* g, const float* x, const float* y, const float* wa, const float* wb, const float* noise, int64_t n, int32_t nout, int64_t y_stride, int64_t w_stride, float* b, float* A_half, int64_t A_stride, float* cnt, const float* u, float* res, double* stats, int32_t* err, void* s) {
  AbsorbArgs<float> a = absorb_args(x, y, wa, wb, noise, n, b, A_half, true, stats, err);
  a.cnt = cnt; a.u = u; a.res = res;
  a.nout = nout; a.bt.y_stride = y_stride; a.bt.w_stride = w_stride; a.bt.A_stride = A_stride;
  return absorb(g, a, s);
}
int wiski_scatter_stats_multi_f64(const wiski_grid* g, const double* x, const double* y, const double* wa, const double* wb, const double* noise, int64_t n, int32_t nout, int64_t y_stride, int64_t w_stride, double* b, double* A_half, int64_t A_stride, double* cnt, const double* u, double* res, double* stats, int32_t* err, void* s) {
  AbsorbArgs<double> a = absorb_args(x, y, wa, wb, noise, n, b, A_half, true, stats, err);
  a.cnt = cnt; a.u = u; a.res = res;
  a.nout = nout; a.bt.y_stride = y_stride; a.bt.w_stride = w_stride; a.bt.A_stride = A_stride;
  return absorb(g, a, s);
}
int64_t wiski_scatter_bin_bytes(const wiski_grid* g, int64_t n, int32_t elem_size) {
  if (!g || g->d != 3 || n < 0 || (elem_size != 4 && elem_size != 8)) return -1;
  return elem_size == 4 ? owner_work_bytes<float>(*g, n) : owner_work_bytes<double>(*g, n);
}
int wiski_stencil_expand_add_f32(const wiski_grid* g, float* half, float* full, void* s) { return expand_impl<float>(g, half, full, s); }
int wiski_stencil_expand_add_f64(const wiski_grid* g, double* half, double* full, void* s) { return expand_impl<double>(g, half, full, s); }
}
