// The absorb's contract: everything one statistics scatter
//   b += W^T D^-1 y,  A += W^T D^-1 W,  cnt += W^T wa,  stats += (y^T D^-1 y, logdet D)
// may be asked to do, as ONE named record.  Every member defaults to "off"; the extern "C" entry points of scatter_stats.hip
// and the streaming step (stream_step.hip) fill the fields they expose and call absorb().  Which combinations are refused is
// absorb_validate() in scatter_stats.hip; whoever writes another form of the absorb has to honour every group below.
// Seven half-stencil kernels stand behind it, besides the full-stencil k_scatter_stats and the owner form (where its workspace is
// given and applies): the atomic form (k_scatter_stats_sym), the derivative-observation form (`channels`, scatter_grad.h), its
// interval-site form (`clo`, scatter_grad_interval.h), the sliding-window form (`ring_*`, scatter_window.h), the site-revisiting form (`site_*`, scatter_revisit.h), the heteroscedastic form (`b2`, scatter_hetero.h) and the site-weighted form (k_scatter_stats_site, scatter_site.h), which is the
// outlier-robust (`inv_scale`, scatter_robust.h), the interval (`lo`, scatter_interval.h), the count (`count_y`, scatter_count.h) or
// the noisy-input absorb (`xvar`, scatter_input_noise.h) by the site it is given.  What they do per point -- the tap tables, the per-tap atomics, the pair loop that
// encodes the row-interleaved layout, the two scalars -- is stated once, in scatter_half.h.
// Every group from `channels` on is the single-output half-stencil atomic form only, with cnt and the carry (res and mean_out stay
// optional): it excludes each of the others, the guard, the zero regions, the shard and the owner workspace.
#pragma once
#include "wiski_common.h"

// strides (in elements) between the outputs of a batched launch; all zero for a single output
struct ScatterBatch {
  int64_t y_stride = 0;    // between the outputs' targets y
  int64_t w_stride = 0;    // between their wa / wb / noise (0: one weight vector shared by all outputs)
  int64_t vec_stride = 0;  // between their b / cnt / u / res: the grid's node count m, which absorb() fills in
  int64_t A_stride = 0;    // between their half stencils
};

template <typename real>
struct AbsorbArgs {
  // points
  const real* x = nullptr;      // [n, d] coordinates; a point outside the grid is flagged in err and contributes nothing at all
  const real* y = nullptr;      // [n] targets                                                       ([n][channels] with channels)
  const real* wa = nullptr;     // [n] weight a point enters A, cnt and the carried residual with    (likewise)
  const real* wb = nullptr;     // [n] weight it enters b and y^T D^-1 y with                        (likewise)
  const real* noise = nullptr;  // [n] its noise: stats[1] += log noise                              (likewise)
  int64_t n = 0;                // 0: nothing happens, whatever the other fields hold
  // targets
  real* b = nullptr;            // [m]
  real* A = nullptr;            // half: row-interleaved symmetric half stencil [(7^d + 1) / 2 * m], else offset-major [7^d, m]; NULL: no A at all
  bool half = false;            // every optional behaviour below except cnt needs the half-stencil form
  real* cnt = nullptr;          // [m] row sums of the increment (preconditioner density model); optional
  double* stats = nullptr;      // [2]: sum wb y^2 and sum log(noise) over the points inside the grid
  int32_t* err = nullptr;       // bit 0: any point outside the grid; bits 1..: number of points dropped
  // carry
  const real* u = nullptr;      // [m] current posterior mean on the grid
  real* res = nullptr;          // [m] res += W^T (wb y - wa (W u)): keeps res = b - z - A u exact under the increment
  real* mean_out = nullptr;     // [n] w_p . u, the predictive mean of the batch BEFORE this update (saves the gather launch of a step); [n][channels] with channels
  // tap stage: [m][4], node-major records {delta b, delta cnt, delta res, unused}, all zero on entry.  The per-tap adds of the atomic
  // form go into the node's record instead of b / cnt / res (scatter_half.h: half_tap_stage) and the caller folds the records in
  // afterwards (pcg.h: tap_fold, or the first kernel of the solve that follows).  fp32, d = 3, the plain single-output atomic form
  // with cnt, u and res, no shard, no channels; the owner-computes form, where it applies, adds directly and leaves the stage zero
  real* tap_stage = nullptr;
  // zero regions: two word arrays of the solve that follows in the same streaming step (its scalar block, its partial vector)
  void* z1 = nullptr;
  int64_t n1_bytes = 0;         // multiples of 4
  void* z2 = nullptr;
  int64_t n2_bytes = 0;
  // guard: speculative launch behind a solve whose convergence poll the host has not read yet (wiski_pcg_async_guard)
  const void* guard = nullptr;  // device int64 the poll's publishing block writes
  int64_t guard_expect = 0;     // the absorb happens iff *guard == guard_expect, decided on the device
  // owner workspace: selects the owner-computes form (scatter_owner.h) where it applies; the atomic form runs otherwise
  void* bin = nullptr;          // wiski_scatter_bin_bytes bytes, zero-initialised once by the caller
  int64_t bin_bytes = 0;
  // shard: the stencil groups [g_lo, g_hi) this replica owns (wiski_shard).  A rank of a stencil-sharded step scatters the tap
  // pairs of ITS groups only -- 1 / N of the atomics per point; b, cnt, res and the statistics stay replicated
  int g_lo = 0, g_hi = 1 << 30;
  // batch: several independent outputs in one launch -- same points, per-output y / weights / targets / statistics at `bt`
  int nout = 1;
  ScatterBatch bt;
  // channels: 0, or d + 1 scalar observations per point -- its value and its d partial derivatives, each with its own y / wa / wb /
  // noise (an absent one: wa = wb = 0, noise = 1) -- summed on chip into one atomic per tap pair (scatter_grad.h)
  int channels = 0;
  // robust: inv_scale != NULL Huber-weights every point against the posterior before the batch (scatter_robust.h):
  //   z = (y - w_p . u) inv_scale,  omega = min(1, huber_c / |z|);  wa, wb enter as omega wa, omega wb, log noise as log(noise / omega)
  // -- the absorb of the point at noise / omega.  inv_scale_p = 0 exempts a point (omega = 1).  Needs u, A, cnt, omega_out and a
  // finite huber_c > 0
  const real* inv_scale = nullptr;  // [n] 1 / scale of each point's innovation
  real huber_c = 0;
  real* omega_out = nullptr;        // [n] the weight each point entered with; 0 for a point outside the grid
  // ring: ring_x != NULL makes the absorb a sliding window (scatter_window.h): entering point j is absorbed, stored in slot
  // (ring_head + j) mod ring_cap, and the point that slot held is taken out again with its weights negated, all in one launch.
  // An empty slot holds wa = wb = 0, noise = 1; a point outside the grid is stored void (wa = wb = 0, noise = 1, y = 0, x = NaN) and
  // void_left counts the void slots that were overwritten.  Needs all five arrays, ring_cap >= 1, 0 <= ring_head < ring_cap,
  // n <= ring_cap (the slots of a launch are distinct), u, A, cnt and void_left
  real* ring_x = nullptr;           // [ring_cap, d]
  real* ring_y = nullptr;           // [ring_cap]
  real* ring_wa = nullptr;          // [ring_cap]
  real* ring_wb = nullptr;          // [ring_cap]
  real* ring_noise = nullptr;       // [ring_cap]
  int64_t ring_cap = 0, ring_head = 0;
  int32_t* void_left = nullptr;     // += number of overwritten slots that were void
  // interval: lo != NULL makes every point an interval observation lo <= f(x) + eps <= hi, moment-matched against the posterior
  // before the batch (scatter_interval.h): with mu = w_p . u, v = pvar, dn = sigma2 noise the site (ytilde, omega) follows from the
  // Gaussian mass of [lo, hi] under N(mu, v + dn), and the point enters as the target ytilde at noise / omega; y is ignored.  A
  // site with omega < WISKI_INTERVAL_OMEGA_MIN, lo > hi or a NaN bound is skipped: nothing anywhere, omega_out = 0, no flag in err.
  // Needs hi, pvar, u, A, cnt, the three outputs and a finite sigma2 > 0
  const real* lo = nullptr;         // [n] lower ends (-inf: none)
  const real* hi = nullptr;         // [n] upper ends (+inf: none); lo == hi: an exact value
  const real* pvar = nullptr;       // [n] posterior variance of f at the point before the batch, in the units of y^2 (negative: 0)
  double sigma2 = 0;                // the noise scale: the point's noise variance is sigma2 noise
  real* ytilde_out = nullptr;       // [n] the pseudo-target each point entered with; the predictive mean for a skipped point
  double* logz_out = nullptr;       // [n] log P(lo <= y <= hi) under the posterior before the batch  (omega_out: the robust group's field)
  // count: count_y != NULL makes every point a count observation (scatter_count.h): count_y successes / events at count_t trials /
  // exposure under the family's link, moment-matched against the posterior before the batch by a quadrature over the lanes of the
  // point's wave, and entered as the target ytilde at noise / omega, omega = sigma2 noise tau (not capped); y is ignored.  An
  // invalid datum (y < 0, t <= 0, y > t for the binomial, a NaN) and a site with omega < WISKI_COUNT_OMEGA_MIN are skipped, as in the
  // interval form, whose pvar / sigma2 / ytilde_out / omega_out / logz_out it shares and needs, with u, A and cnt
  const real* count_y = nullptr;    // [n] counts (non-integers allowed)
  const real* count_t = nullptr;    // [n] exposure (Poisson) / trials (binomial)
  int count_family = 0;             // WISKI_COUNT_POISSON, WISKI_COUNT_BINOMIAL
  // input noise: xvar != NULL makes every point an observation at an uncertain location, x_p + e_p with e_p ~ N(0, diag(xvar_p))
  // (scatter_input_noise.h): with g_k = (d w_p / d x_k) . u the slope of the predictive mean before the batch, the point enters as
  // its own target y at noise / omega, omega = dn / (dn + sum_k xvar_k (g_k^2 + max(gvar_k, 0))), dn = sigma2 noise.  A negative or
  // NaN xvar_k, a non-finite sum and an omega < WISKI_INPUT_NOISE_OMEGA_MIN are skipped, as in the interval form, whose pvar /
  // sigma2 / omega_out / logz_out it shares and needs, with y, u, A and cnt; ytilde_out is not used (ytilde = y)
  const real* xvar = nullptr;       // [n, d] variance of the location error per dim, in the grid's units squared
  const real* gvar = nullptr;       // [n, d] posterior variance of d f / d x_k before the batch, in y^2 per grid unit squared; NULL: 0
  real* grad_out = nullptr;         // [n, d] the slopes g as the wave reduced them (0 for a point outside the grid); optional
  // channel intervals: clo != NULL, with channels = d + 1, makes every present channel (wa != 0) of every point an interval
  // observation clo <= v_c . u + eps <= chi at noise sigma2 noise -- bounds on f and on its partial derivatives -- each moment-matched
  // as in the interval form against mu_c = v_c . u and cpvar, and entered as ytilde_c at noise / omega_c in the one launch of the
  // derivative form (scatter_grad_interval.h).  A group of its own, not the interval group's fields: besides its three arrays it
  // uses sigma2 and the outputs ytilde_out / omega_out / logz_out, which are [n][channels] here.  y is ignored.  Needs chi, cpvar, u,
  // A, cnt, the three outputs and a finite sigma2 > 0; excludes lo / hi / pvar and every other group
  const real* clo = nullptr;        // [n][channels] lower ends (-inf: none)
  const real* chi = nullptr;        // [n][channels] upper ends (+inf: none); clo == chi: an exact value
  const real* cpvar = nullptr;      // [n][channels] posterior variance of each channel before the batch (negative: 0)
  // hetero: b2 != NULL makes the absorb heteroscedastic (scatter_hetero.h): a second single-output model on the same grid -- the
  // second target set below, every member of it the counterpart of the first set's -- holds g = log of the noise multiplier, prior
  // mean g0.  With mu_g = g0 + w_p . u2, v_g = max(pvar2, 0), e = exp(mu_g + v_g / 2), the point enters the first set as its own
  // target y at noise noise / omega_f, omega_f = 1 / e (not capped), and its deflated squared residual enters the second set as a
  // log-variance site (ytilde_g - g0 at noise 1 / tau_g; that model's sigma2 = noise = wa = wb = 1).  A NaN y skips the point for
  // both sets (no flag); a point outside the grid is dropped for both and counted once; a noise site with tau < WISKI_COUNT_OMEGA_MIN
  // is skipped for the second set alone.  Shares the interval group's pvar / sigma2 / ytilde_out / omega_out / logz_out (the noise
  // site, tau in omega_out) and needs them, with y, u, A, cnt, b2, A2, cnt2, stats2, u2, pvar2, e_out, logzy_out and a finite g0;
  // res and res2 are optional
  real* b2 = nullptr;               // [m]
  real* A2 = nullptr;               // the second model's symmetric half stencil
  real* cnt2 = nullptr;             // [m]
  double* stats2 = nullptr;         // [2]
  const real* u2 = nullptr;         // [m] posterior mean of g - g0 on the grid
  real* res2 = nullptr;             // [m] the second model's carried residual; optional
  const real* pvar2 = nullptr;      // [n] posterior variance of g at the point before the batch (negative: 0)
  double g0 = 0;                    // prior mean of g
  real* e_out = nullptr;            // [n] the multiplier each point entered f with; 0 for a point outside the grid
  double* logzy_out = nullptr;      // [n] log N(y; mu_f, v_f + sigma2 noise e) under the posteriors before the batch
  // revisit: site_codes != NULL makes the launch an expectation-propagation sweep over a ring of stored sites (scatter_revisit.h).
  // The points ARE the ring's slots: x / wa / wb / noise are its arrays and n its capacity; y is not used.  Every slot whose form code
  // is site_form_code is re-matched against its cavity under (u, pvar), damped by site_damping, and enters with the difference of
  // its site; its new (ytilde, omega) are written back to the ring.  A group of its own that shares the interval group's pvar ([n],
  // at the slots), sigma2 and logz_out ([n], the fresh site's log Z against the cavity; NaN for a slot of the form that was left
  // alone) and needs them, with u, A, cnt, the whole group, a finite sigma2 > 0 and 0 <= site_damping <= 1; res is optional,
  // mean_out is not produced; err is never raised (a stored point the grid does not contain is left alone)
  const real* site_d0 = nullptr;    // [n] lower ends / counts
  const real* site_d1 = nullptr;    // [n] upper ends / exposure or trials
  real* site_ytilde = nullptr;      // [n] the pseudo-target each slot is in the statistics with; updated
  real* site_omega = nullptr;       // [n] its weight (0: the slot's point was skipped and nothing of it is in the statistics); updated
  const int32_t* site_codes = nullptr; // [n] WISKI_SITE_EMPTY / _INTERVAL / _POISSON / _BINOMIAL
  int site_form_code = 0;           // the form this launch revisits
  double site_damping = 0;          // delta; 0 changes nothing bit for bit and issues no atomic
  real* site_change_out = nullptr;  // [n] |omega_new - omega_old| / max(omega_new, omega_old) of the slots of the form; 0 for one left alone

  bool sharded() const { return g_lo > 0 || g_hi < (1 << 30); }
  bool windowed() const { return ring_x || ring_y || ring_wa || ring_wb || ring_noise || ring_cap || ring_head || void_left; }
  bool counted() const { return count_y || count_t || count_family != 0; }
  bool input_noise() const { return xvar || gvar || grad_out; }
  // (the fields the matched forms share belong to whichever of the count, input-noise, channel-interval, hetero and revisit groups is given, else to the interval group)
  bool grad_interval() const { return clo || chi || cpvar; }
  bool hetero() const { return b2 || A2 || cnt2 || stats2 || u2 || res2 || pvar2 || g0 != 0 || e_out || logzy_out; }
  bool revisit() const { return site_d0 || site_d1 || site_ytilde || site_omega || site_codes || site_form_code != 0 || site_damping != 0 || site_change_out; }
  bool interval() const { return lo || hi || (!counted() && !input_noise() && !grad_interval() && !hetero() && !revisit() && (pvar || sigma2 != 0 || ytilde_out || logz_out)); }
  bool site_form() const { return inv_scale || interval() || counted() || input_noise(); }   // the forms of k_scatter_stats_site (scatter_site.h)
};

// Validates, then queues the absorb on `stream`: WISKI_OK, WISKI_E_BADARG (nothing was launched) or WISKI_E_LAUNCH.
// Instantiated for float and double in scatter_stats.hip.
template <typename real>
int absorb(const wiski_grid* grid, const AbsorbArgs<real>& args, void* stream);
