// One streaming step behind ONE C-ABI call: the launches of
//   predictive mean of the incoming batch + absorb   wiski_scatter_stats_step (BFN:206-210, BFN:155-171 + URLT:58; carries the residual)
//   warm-started refresh of the mean                 pcg()                    (CG branch of BFN:368-383)
// are queued back to back on the caller's stream without returning to the host language in between (the Python
// front-end left the GPU idle for ~30 us between the gather and the scatter and ~40 us after the solver's last poll).
// With a deferred solve pending, the absorb of the NEXT batch is queued before the host has read that solve's convergence
// poll, guarded on the device by the poll's own verdict (wiski_pcg_async_guard): the GPU goes from the last iteration
// straight into the absorb instead of idling through the host's poll round trip (~20 us of a 220 us step).
// With a tap stage (wiski_stream_args_f32.d_tap_stage) the absorb leaves its per-tap adds on b / cnt / R in the stage's records and
// the solve queued behind it in the same call folds them in (PcgArgs::tap_stage): the stage is zero again whenever a call returns.
// Pure host code: it fills the two argument records (absorb.h, pcg.h) and sequences absorb() and pcg().
#include "absorb.h"
#include "pcg.h"

template <typename real>
struct StreamArgs;
template <>
struct StreamArgs<float> { using type = wiski_stream_args_f32; };
template <>
struct StreamArgs<double> { using type = wiski_stream_args_f64; };

// The absorb of one batch into the statistics `a` points at.  mean_out given: absorb + predictive mean of the batch in ONE
// kernel -- it reads U whether or not it carries the residual, takes the owner-computes form or this rank's stencil groups
// where they apply and, with `zero`, does the zeroing the following solve would do in a launch of its own; `guard`: see
// wiski_pcg_async_guard.  Without mean_out: the plain absorb, U read for the residual carry only.
// The stage this call's absorb and solve share, or NULL: fp32 at d = 3 with the carry and cnt, the whole stencil on this replica
// (AbsorbArgs::tap_stage).  One rule for both sides: the absorb is handed the stage only where the solve is handed it too.
static float* step_tap_stage(const wiski_grid* g, const wiski_stream_args_f32* a, int carry) {
  return g->d == 3 && carry && a->d_cnt && !wiski_shard_active(a->shard) ? a->d_tap_stage : nullptr;
}
static double* step_tap_stage(const wiski_grid*, const wiski_stream_args_f64*, int) { return nullptr; }
static int64_t grid_nodes(const wiski_grid* g) {
  int64_t m = 1;
  for (int q = 0; q < g->d; ++q) m *= g->g[q];
  return m;
}

template <typename real>
static int absorb_batch(const wiski_grid* g, const typename StreamArgs<real>::type* a, AbsorbArgs<real> r, int carry, int zero, void* s) {
  r.b = a->d_b; r.A = a->d_A_half; r.half = true; r.cnt = a->d_cnt; r.stats = a->d_stats; r.err = a->d_err;
  r.u = carry || r.mean_out ? a->d_U : nullptr;
  r.res = carry ? a->d_R : nullptr;
  r.tap_stage = step_tap_stage(g, a, carry);
  if (!r.mean_out) return absorb(g, r, s);
  if (zero) {
    if (int rc = pcg_zero_regions<real>(g, 1, a->max_iter, a->d_work, true, &r.z1, &r.n1_bytes, &r.z2, &r.n2_bytes)) return rc;
  }
  if (wiski_shard_active(a->shard)) {
    int32_t glo = 0, ghi = 0;
    if (int rc = wiski_shard_groups(g->d, a->shard->rank, a->shard->nranks, &glo, &ghi)) return rc;
    r.g_lo = glo; r.g_hi = ghi;
  } else {
    r.bin = a->d_bin; r.bin_bytes = a->bin_bytes;
  }
  return absorb(g, r, s);
}
// The refresh of the stream's mean: (Kt^-1 + A_half) U = b, one column, warm from (U, Z) -- with `carry` from the residual R the
// absorb kept current.  Reports and deferred-poll mode are the caller's.
template <typename real>
static PcgArgs<real> solve_args(const typename StreamArgs<real>::type* a, int carry, int first_check) {
  PcgArgs<real> p;
  p.A = a->d_A_half; p.a_sym = true; p.RHS = a->d_b; p.k = 1;
  p.tcol = a->d_tcol; p.kscale = a->kscale; p.evec = a->d_evec; p.evec2 = a->d_evec2; p.eval = a->d_eval; p.shift = a->shift; p.two_level = a->two_level;
  for (int q = 0; q < 3; ++q) p.keep[q] = a->keep[q];
  p.U = a->d_U; p.Z = a->d_Z; p.R = a->d_R; p.warm = carry ? 2 : 1;
  p.tol = a->tol; p.max_iter = a->max_iter; p.check_every = a->check_every; p.first_check = first_check;
  p.work = a->d_work; p.work_bytes = a->work_bytes;
  p.d_err = a->d_err;
  p.shard = a->shard;
  return p;
}

template <typename real>
static int stream_step_impl(const wiski_grid* grid, const typename StreamArgs<real>::type* a, const real* d_x, const real* d_y, const real* d_wa,
                            const real* d_wb, const real* d_noise, int64_t q, real* d_mean_out, int32_t carry, int32_t first_check, int32_t* h_iters,
                            double* h_relres, int32_t* h_err, void* stream, wiski_pcg_async* as, int32_t defer, int32_t* h_resumed) {
  if (!grid || !a || q < 0 || !a->d_A_half || !a->d_b || !a->d_U || !a->d_Z || !a->d_R) return WISKI_E_BADARG;
  if (q > 0 && (!d_x || !d_y || !d_wa || !d_wb || !d_noise)) return WISKI_E_BADARG;
  if (wiski_shard_active(a->shard) && q > 0 && !d_mean_out) return WISKI_E_BADARG;   // the sharded absorb is the mean-emitting kernel
  // first_check = -1: pcg() places the first poll where the handle's last finished solve first met the tolerance (first_ok).  The
  // solve below is queued after the RESUME of the pending one, so that is the hindsight of the solve just resumed.  Refused here
  // as pcg_validate would, before the absorb is queued
  if (first_check < -1 || (first_check == -1 && !as)) return WISKI_E_BADARG;
  int rc = WISKI_OK;
  if (h_resumed) *h_resumed = 0;
  if (sizeof(real) == 8 && a->d_tap_stage) return WISKI_E_BADARG;
  PcgArgs<real> solve = solve_args<real>(a, carry, first_check);   // this stream's solve, reporting into the caller's outputs
  solve.h_iters = h_iters; solve.h_relres = h_relres; solve.h_err = h_err; solve.handle = as;
  AbsorbArgs<real> batch;                    // the points of this call; absorb_batch adds the targets
  batch.x = d_x; batch.y = d_y; batch.wa = d_wa; batch.wb = d_wb; batch.noise = d_noise; batch.n = q; batch.mean_out = d_mean_out;
  bool absorbed = false;                     // the speculative absorb below has run
  if (as && as->state == 1) {
    // A solve the previous call started is pending.  It has to finish BEFORE anything reads U (the batch mean) or changes the
    // system (the absorb) -- but the host need not have SEEN it finish: queue this batch's absorb now, guarded on the device
    // by the verdict of the pending poll (it runs iff that poll finds the solve converged and the error flag clear, which
    // is exactly when RESUME below queues nothing more), and only then wait for the poll.  The absorb then executes while
    // the host reads the poll and queues the next solve.
    bool spec = false;
    if (q > 0 && d_mean_out) {
      const void* guard = nullptr;
      int64_t expect = 0;
      if (pcg_guard(as, &guard, &expect) == WISKI_OK) {
        AbsorbArgs<real> spec_batch = batch;
        spec_batch.guard = guard; spec_batch.guard_expect = expect;
        rc = absorb_batch<real>(grid, a, spec_batch, carry, 1, stream);
        if (rc) return rc;
        spec = true;
      }
    }
    {
      PcgArgs<real> resume = solve;                // RESUME with the shift the solve was started with (a->shift is the NEXT solve's)
      resume.shift = (real)as->shift;
      resume.mode = 2;
      rc = pcg(grid, resume, stream);
    }
    if (h_resumed) *h_resumed = 1;
    if (rc != WISKI_OK && rc != WISKI_E_NOTCONV) {
      if constexpr (sizeof(real) == 4) {           // the speculative absorb may have staged its batch: no solve of this call will fold it
        if (spec && step_tap_stage(grid, a, carry)) (void)tap_fold(a->d_tap_stage, a->d_b, a->d_cnt, a->d_R, grid_nodes(grid), stream);
      }
      return rc;
    }
    absorbed = spec && as->guard_ok;          // else the guarded kernel was a no-op (and RESUME may have queued more iterations)
    if (q == 0) return rc;
    if (!absorbed && h_err && *h_err) return rc;   // out-of-grid points in the previous batch: let the caller deal with them first
  } else if (q == 0 && as) {
    return WISKI_OK;
  }
  const int resumed_rc = rc;
  if (q > 0) {                                 // this call's absorb stages its tap adds (or has done so): its solve folds them
    solve.tap_stage = step_tap_stage(grid, a, carry);
    if (solve.tap_stage) { solve.tap_b = a->d_b; solve.tap_cnt = a->d_cnt; }
  }
  if (absorbed) {
    as->prezeroed = 1;
  } else if (q > 0) {
    if (d_mean_out) {
      // the absorb kernel forms w_p . U for the residual carry anyway: it is the predictive mean of the batch, so there is no
      // gather launch; with a handle the same kernel also zeroes what the solve below would zero in a launch of its own
      rc = absorb_batch<real>(grid, a, batch, carry, as ? 1 : 0, stream);
      if (rc) return rc;
      if (as) as->prezeroed = 1;           // nothing touches the solve's workspace between this kernel and the solve below
    } else {
      rc = absorb_batch<real>(grid, a, batch, carry, 0, stream);
      if (rc) return rc;
    }
  }
  if (!as) return pcg(grid, solve, stream);
  if (defer) {
    as->shift = (double)a->shift;
    solve.h_iters = nullptr; solve.h_relres = nullptr; solve.h_err = nullptr;           // outputs of THIS solve arrive with the next call
    solve.mode = 1;
    rc = pcg(grid, solve, stream);
    return rc == WISKI_PENDING ? (resumed_rc == WISKI_E_NOTCONV ? WISKI_E_NOTCONV : WISKI_PENDING) : rc;
  }
  // deferral switched off with a solve pending: the outputs below describe THIS step's synchronous solve; the resumed
  // one (finished above) is reported as *h_resumed = 2 -- "resumed, but its numbers were overwritten" -- and a resumed
  // solve that stopped at max_iter still surfaces through the return code
  if (h_resumed && *h_resumed == 1) *h_resumed = 2;
  rc = pcg(grid, solve, stream);
  return rc == WISKI_OK && resumed_rc == WISKI_E_NOTCONV ? WISKI_E_NOTCONV : rc;
}

extern "C" {
int wiski_stream_step_f32(const wiski_grid* grid, const wiski_stream_args_f32* a, const float* d_x, const float* d_y, const float* d_wa, const float* d_wb, const float* d_noise, int64_t q, float* d_mean_out, int32_t carry, int32_t first_check, int32_t* h_iters, double* h_relres, int32_t* h_err, void* stream, wiski_pcg_async* as, int32_t defer, int32_t* h_resumed) {
  return stream_step_impl<float>(grid, a, d_x, d_y, d_wa, d_wb, d_noise, q, d_mean_out, carry, first_check, h_iters, h_relres, h_err, stream, as, defer, h_resumed);
}
int wiski_stream_step_f64(const wiski_grid* grid, const wiski_stream_args_f64* a, const double* d_x, const double* d_y, const double* d_wa, const double* d_wb, const double* d_noise, int64_t q, double* d_mean_out, int32_t carry, int32_t first_check, int32_t* h_iters, double* h_relres, int32_t* h_err, void* stream, wiski_pcg_async* as, int32_t defer, int32_t* h_resumed) {
  return stream_step_impl<double>(grid, a, d_x, d_y, d_wa, d_wb, d_noise, q, d_mean_out, carry, first_check, h_iters, h_relres, h_err, stream, as, defer, h_resumed);
}
}
