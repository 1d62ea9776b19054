// Sliding-window absorb (AbsorbArgs::ring).  Included by scatter_stats.hip.
//
// The statistics are sums over the points, so a point that was absorbed leaves them again by being absorbed once more with its
// weights negated.  A ring of `cap` slots on the device remembers what entered -- x, y, wa, wb, noise per slot -- and ONE launch
// absorbs the n <= cap entering points, stores them in the slots head, head + 1, ... (mod cap) and takes out what those slots
// held: the model is then the GP of exactly the points in the ring.  Per entering point j, the wave of slot s = (head + j) mod cap
//   1. reads the old occupant of s into registers (lane 0 reads, the wave receives a broadcast),
//   2. writes the entering point into s (lane 0),
//   3. sweeps the entering point with (+wa, +wb): mean_out[j] = w_j . u as in the other forms,
//   4. sweeps the old occupant, if it holds weight, with (-wa, -wb), in the same LDS tap tables.
// n <= cap makes the slots of a launch distinct, so the only reader and the only writer of a slot is lane 0 of one wave, in
// program order: nothing is assumed about the order of waves or blocks.  Both sweeps are taken against the same u, so the
// result depends neither on the order of the points nor on the order of the atomics.
//
// Slot states.  Empty (never written): wa = wb = 0, noise = 1, x finite -- the ring is created that way.  Void: the entering
// point lay outside the grid; it is flagged and counted in err as everywhere, contributes nothing, and is stored with
// wa = wb = 0, noise = 1, y = 0 and x = NaN, the coordinates of a point no grid ever contains (a grown grid included).  When its slot
// comes round nothing is taken out that never went in, and void_left counts it so that the host can keep its point count.
#pragma once

template <typename real>
struct WindowRingDev {
  real* x;
  real* y;
  real* wa;
  real* wb;
  real* noise;
  int64_t cap, head;
};

// lane 0's value in every lane, as a wave-uniform (scalar) value
__device__ __forceinline__ float wave_first(float v) { return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v))); }
__device__ __forceinline__ double wave_first(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_readfirstlane((int)(b & 0xffffffffll)), hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __builtin_bit_cast(double, ((long long)hi << 32) | (long long)(unsigned)lo);
}

// The point sweep is that of k_scatter_stats_sym (scatter_half.h), taken twice.  No guard, zero regions, shard or batch
// (absorb_validate).  The two scalars cannot come from scatter_stats_pass, which sees the entering arrays only: as in the
// robust form each wave keeps, in fp64, the +- wb y^2 and +- log noise of its slot (lane 0 holds them) and a block issues one
// atomic pair when it is done.  The second sweep reuses the wave's tap tables: the LDS footprint is that of the robust kernel.
template <typename real, int D>
__global__ __launch_bounds__(256) void k_scatter_stats_window(GridDev<real> G, const real* __restrict__ x, const real* __restrict__ y,
                                                              const real* __restrict__ wa, const real* __restrict__ wb,
                                                              const real* __restrict__ noise, int64_t n, real* __restrict__ b,
                                                              real* __restrict__ A, double* __restrict__ stats, int32_t* __restrict__ err,
                                                              real* __restrict__ cnt, const real* __restrict__ u, real* __restrict__ res,
                                                              real* __restrict__ mean_out, WindowRingDev<real> R, int32_t* __restrict__ void_left) {
  using H = HalfTaps<D>;
  __shared__ real s_val[4][H::T];
  __shared__ int s_idx[4][H::T];
  __shared__ int s_pair[H::NPAIR];
  __shared__ double s_red[16];
  const int lane = threadIdx.x & 63, loc = threadIdx.x >> 6;
  half_pair_list<D>(s_pair, reinterpret_cast<int*>(s_red), 0, 1 << 30);         // the whole stencil: H::NPAIR pairs
  // the block's vote on whether any of its four slots holds weight: eight ints at the tail of the reduction buffer (its head is
  // what block_reduce_sum writes), one set per parity of the pass so that a wave ahead by one pass overwrites nothing still read
  int* s_live = reinterpret_cast<int*>(s_red + 12);
  int par = 0;
  bool bad = false;
  double c_acc = 0, ld_acc = 0, void_acc = 0;    // lane 0: this wave's share of the two scalars and of the void count
  for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {
    const int64_t p = base + loc;
    const bool valid = p < n;
    const int64_t s = valid ? (R.head + p) % R.cap : 0;
    int j0[D], flat_t[H::TPL];
    real w[D][4], val_t[H::TPL][1], yw[1], wac[1], wu[1], innov[1];
    // 1. the old occupant, read by the one lane that also writes the slot
    real ox[D], oy = 0, owa = 0, owb = 0, onz = 1;
#pragma unroll
    for (int q = 0; q < D; ++q) ox[q] = 0;
    if (valid && lane == 0) {
#pragma unroll
      for (int q = 0; q < D; ++q) ox[q] = R.x[s * D + q];
      oy = R.y[s];
      owa = R.wa[s];
      owb = R.wb[s];
      onz = R.noise[s];
    }
    const bool inside = half_point_setup<real, D>(G, x, p, n, lane == 0, err, bad, j0, w);
    real yp = 0, wap = 0, wbp = 0;
    if (inside) {                                // a point outside the grid enters, and is stored, with no weight at all
      yp = y[p];
      wap = wa[p];
      wbp = wb[p];
    }
    // 2. the entering point takes the slot
    if (valid && lane == 0) {
      const real nz = inside ? noise[p] : (real)1;
#pragma unroll
      for (int q = 0; q < D; ++q) R.x[s * D + q] = inside ? x[p * D + q] : (real)NAN;
      R.y[s] = yp;
      R.wa[s] = wap;
      R.wb[s] = wbp;
      R.noise[s] = nz;
      const bool was_void = owa == (real)0 && owb == (real)0 && ox[0] != ox[0];
      if (was_void) void_acc += 1;
      c_acc += (double)yp * (double)yp * (double)wbp - (double)oy * (double)oy * (double)owb;
      ld_acc += log((double)nz) - log((double)onz);
    }
#pragma unroll
    for (int q = 0; q < D; ++q) ox[q] = wave_first(ox[q]);
    oy = wave_first(oy);
    owa = wave_first(owa);
    owb = wave_first(owb);
    const bool live = owa != (real)0 || owb != (real)0;
    if (lane == 0) s_live[par * 4 + loc] = live ? 1 : 0;
    // 3. the entering point, with (+wa, +wb)
    half_tap_table<real, D, 1>(G, j0, w, nullptr, lane, u, s_val[loc], s_idx[loc], flat_t, val_t, wu);   // wu: the predictive mean of the point before the batch
    wac[0] = wap;
    yw[0] = yp * wbp;
    half_carry<real, 1>(u, yw, wac, wu, mean_out, p, lane == 0 && valid, innov);
    half_tap_atomics<real, D, 1>(valid, flat_t, val_t, yw, wac, innov, b, cnt, res);
    __syncthreads();
    if (valid) half_pair_loop<real, D, 1>(lane, H::NPAIR, s_pair, s_val[loc], s_idx[loc], wac, 1, A, G.m);
    __syncthreads();
    // 4. the old occupant, with (-wa, -wb): wave-uniform per slot, and the block skips the sweep as one -- every thread reads the
    // same four votes, so every thread reaches the same barriers -- when none of its four slots held weight (while the ring fills)
    const bool any_live = (s_live[par * 4] | s_live[par * 4 + 1] | s_live[par * 4 + 2] | s_live[par * 4 + 3]) != 0;
    par ^= 1;
    if (any_live) {
      bool gone = false;                         // a stored point the grid no longer contains takes nothing out and raises no flag
      half_point_setup<real, D>(G, ox, 0, live ? 1 : 0, false, err, gone, j0, w);
      half_tap_table<real, D, 1>(G, j0, w, nullptr, lane, u, s_val[loc], s_idx[loc], flat_t, val_t, wu);
      wac[0] = -owa;
      yw[0] = -(oy * owb);
      half_carry<real, 1>(u, yw, wac, wu, nullptr, 0, false, innov);
      half_tap_atomics<real, D, 1>(live, flat_t, val_t, yw, wac, innov, b, cnt, res);
      __syncthreads();
      if (live) half_pair_loop<real, D, 1>(lane, H::NPAIR, s_pair, s_val[loc], s_idx[loc], wac, 1, A, G.m);
      __syncthreads();
    }
  }
  stats_atomic_pair(c_acc, ld_acc, stats, s_red);
  const double void_tot = block_reduce_sum(void_acc, s_red);
  if (threadIdx.x == 0 && void_tot != 0) atomicAdd(void_left, (int32_t)void_tot);
  if (bad) atomicOr(err, 1);
}

// Points a block takes where the batch is large (a multiple of 4: four per pass of its loop).  Every block ends with one atomic
// pair on the two scalars, as in the robust form, and atomics of many blocks on one address serialise at the memory side: the
// reasoning of ROBUST_POINTS_PER_BLOCK -- 16 points, 256 pairs at 4 096 points.  A block's passes run one after another, though,
// and here every pass is two dependent sweeps: a small batch spread over few blocks pays their latency eight times over (measured at
// 50^3 fp32 with 16 points per block throughout: 89 us at 64 and at 1 024 points, where the plain absorb of twice the points takes
// 26 and 55 us).  So up to WINDOW_MIN_BLOCKS blocks take four points each -- no more atomic pairs than a large batch issues anyway.
#ifndef WISKI_WINDOW_POINTS_PER_BLOCK
#define WISKI_WINDOW_POINTS_PER_BLOCK 16
#endif
constexpr int64_t WINDOW_POINTS_PER_BLOCK = WISKI_WINDOW_POINTS_PER_BLOCK;
constexpr int64_t WINDOW_MIN_BLOCKS = 256;

template <typename real>
static int launch_window(const GridDev<real>& G, const AbsorbArgs<real>& a, hipStream_t stream) {
  int64_t blocks = (a.n + WINDOW_POINTS_PER_BLOCK - 1) / WINDOW_POINTS_PER_BLOCK;
  const int64_t one_pass = (a.n + 3) / 4;
  if (blocks < WINDOW_MIN_BLOCKS) blocks = one_pass < WINDOW_MIN_BLOCKS ? one_pass : WINDOW_MIN_BLOCKS;
  if (blocks > 256 * 8) blocks = 256 * 8;
  const WindowRingDev<real> R{a.ring_x, a.ring_y, a.ring_wa, a.ring_wb, a.ring_noise, a.ring_cap, a.ring_head};
#define CALL(DD)                                                                                                                                        \
  hipLaunchKernelGGL((k_scatter_stats_window<real, DD>), dim3((unsigned)blocks), dim3(256), 0, stream, G, a.x, a.y, a.wa, a.wb, a.noise, a.n, a.b, a.A, \
                     a.stats, a.err, a.cnt, a.u, a.res, a.mean_out, R, a.void_left)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}
