// One streaming step behind ONE C-ABI call: the launches of
//   predictive mean of the incoming batch + absorb   wiski_scatter_stats_step (BFN:206-210, BFN:155-171 + URLT:58; carries the residual)
//   warm-started refresh of the mean                 wiski_pcg                (CG branch of BFN:368-383)
// are queued back to back on the caller's stream without returning to the host language in between (the Python
// front-end left the GPU idle for ~30 us between the gather and the scatter and ~40 us after the solver's last poll).
// With a deferred solve pending, the absorb of the NEXT batch is queued before the host has read that solve's convergence
// poll, guarded on the device by the poll's own verdict (wiski_pcg_async_guard): the GPU goes from the last iteration
// straight into the absorb instead of idling through the host's poll round trip (~20 us of a 220 us step).
// Pure host code: it only sequences the entry points above.
#include "absorb.h"

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
template <typename real>
static int absorb_batch(const wiski_grid* g, const typename StreamArgs<real>::type* a, AbsorbArgs<real> r, int carry, int zero, void* s) {
  r.b = a->d_b; r.A = a->d_A_half; r.half = true; r.cnt = a->d_cnt; r.stats = a->d_stats; r.err = a->d_err;
  r.u = carry || r.mean_out ? a->d_U : nullptr;
  r.res = carry ? a->d_R : nullptr;
  if (!r.mean_out) return absorb(g, r, s);
  if (zero) {
    int rc;
    if constexpr (sizeof(real) == 4) rc = wiski_pcg_zero_regions_f32(g, 1, a->max_iter, a->d_work, 1, &r.z1, &r.n1_bytes, &r.z2, &r.n2_bytes);
    else rc = wiski_pcg_zero_regions_f64(g, 1, a->max_iter, a->d_work, 1, &r.z1, &r.n1_bytes, &r.z2, &r.n2_bytes);
    if (rc) return rc;
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
static int pcg1(const wiski_grid* g, const wiski_stream_args_f32* a, int warm, int first_check, int32_t* it, double* rr, int32_t* herr, void* s,
                wiski_pcg_async* as, int mode) {
  return wiski_pcg_twolevel_f32(g, a->d_A_half, a->d_tcol, a->kscale, a->d_evec, a->d_evec2, a->d_eval, a->shift, a->d_b, 1, a->d_U, a->d_Z, warm, a->tol,
                                a->max_iter, a->check_every, first_check, a->d_work, a->work_bytes, it, rr, a->d_err, herr, 1, a->d_R, s, as, mode, a->shard,
                                a->two_level);
}
static int pcg1(const wiski_grid* g, const wiski_stream_args_f64* a, int warm, int first_check, int32_t* it, double* rr, int32_t* herr, void* s,
                wiski_pcg_async* as, int mode) {
  if (a->two_level) return WISKI_E_BADARG;
  return wiski_pcg_sharded_f64(g, a->d_A_half, a->d_tcol, a->kscale, a->d_evec, a->d_evec2, a->d_eval, a->shift, a->d_b, 1, a->d_U, a->d_Z, warm, a->tol,
                               a->max_iter, a->check_every, first_check, a->d_work, a->work_bytes, it, rr, a->d_err, herr, 1, a->d_R, s, as, mode, a->shard);
}

template <typename real>
static int stream_step_impl(const wiski_grid* grid, const typename StreamArgs<real>::type* a, const real* d_x, const real* d_y, const real* d_wa,
                            const real* d_wb, const real* d_noise, int64_t q, real* d_mean_out, int32_t carry, int32_t first_check, int32_t* h_iters,
                            double* h_relres, int32_t* h_err, void* stream, wiski_pcg_async* as, int32_t defer, int32_t* h_resumed) {
  if (!grid || !a || q < 0 || !a->d_A_half || !a->d_b || !a->d_U || !a->d_Z || !a->d_R) return WISKI_E_BADARG;
  if (q > 0 && (!d_x || !d_y || !d_wa || !d_wb || !d_noise)) return WISKI_E_BADARG;
  if (wiski_shard_active(a->shard) && q > 0 && !d_mean_out) return WISKI_E_BADARG;   // the sharded absorb is the mean-emitting kernel
  int rc = WISKI_OK;
  if (h_resumed) *h_resumed = 0;
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
      if (wiski_pcg_async_guard(as, &guard, &expect) == WISKI_OK) {
        AbsorbArgs<real> spec_batch = batch;
        spec_batch.guard = guard; spec_batch.guard_expect = expect;
        rc = absorb_batch<real>(grid, a, spec_batch, carry, 1, stream);
        if (rc) return rc;
        spec = true;
      }
    }
    {
      typename StreamArgs<real>::type ar = *a;     // RESUME with the shift the solve was started with (a->shift is the NEXT solve's)
      ar.shift = (real)as->shift;
      rc = pcg1(grid, &ar, 2, first_check, h_iters, h_relres, h_err, stream, as, 2);
    }
    if (h_resumed) *h_resumed = 1;
    if (rc != WISKI_OK && rc != WISKI_E_NOTCONV) return rc;
    absorbed = spec && as->guard_ok;          // else the guarded kernel was a no-op (and RESUME may have queued more iterations)
    if (q == 0) return rc;
    if (!absorbed && h_err && *h_err) return rc;   // out-of-grid points in the previous batch: let the caller deal with them first
  } else if (q == 0 && as) {
    return WISKI_OK;
  }
  const int resumed_rc = rc;
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
  if (!as) return pcg1(grid, a, carry ? 2 : 1, first_check, h_iters, h_relres, h_err, stream, nullptr, 0);
  if (defer) {
    int32_t it2 = 0, e2 = 0;
    double r2 = 0;
    as->shift = (double)a->shift;
    rc = pcg1(grid, a, carry ? 2 : 1, first_check, &it2, &r2, &e2, stream, as, 1);      // outputs of THIS solve arrive with the next call
    return rc == WISKI_PENDING ? (resumed_rc == WISKI_E_NOTCONV ? WISKI_E_NOTCONV : WISKI_PENDING) : rc;
  }
  // deferral switched off with a solve pending: the outputs below describe THIS step's synchronous solve; the resumed
  // one (finished above) is reported as *h_resumed = 2 -- "resumed, but its numbers were overwritten" -- and a resumed
  // solve that stopped at max_iter still surfaces through the return code
  if (h_resumed && *h_resumed == 1) *h_resumed = 2;
  rc = pcg1(grid, a, carry ? 2 : 1, first_check, h_iters, h_relres, h_err, stream, as, 0);
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
