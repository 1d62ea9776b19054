// The solve's contract: everything one preconditioned-CG solve
//   (Kt^-1 + A) U = RHS,  Kt = kscale * Kuu,  iterated in Z = Kt^-1 U
// may be asked to do, as ONE named record.  Every member defaults to "off"; the extern "C" wiski_pcg* entry points of solve.hip
// and the streaming step (stream_step.hip) fill the fields they expose and call pcg().  Which combinations are refused is
// pcg_validate() in solve.hip; where the workspace's buffers lie is PcgLayout below, and nowhere else.
#pragma once
#include "wiski_common.h"

template <typename real>
struct PcgArgs {
  // system
  const real* A = nullptr;        // a_sym: symmetric half stencil (the absorb's row-interleaved layout), else offset-major [7^d][m]
  bool a_sym = false;
  const real* RHS = nullptr;      // [k][m]
  int k = 0;                      // right-hand sides
  // prior and preconditioner: P = Kt (needs tcol), or with (evec, eval) the separable model (Kt^-1 + shift kron_q diag(t_q))^-1
  const real* tcol = nullptr;     // first columns of the per-dim Toeplitz factors of Kuu, concatenated
  real kscale = (real)0;
  const real* evec = nullptr;     // per-dim generalized eigenvectors X_q, concatenated row-major g_q x g_q
  const real* evec2 = nullptr;    // Z_q = diag(t_q) X_q; NULL: t_q = 1, X_q orthogonal
  const real* eval = nullptr;     // per-dim eigenvalues D_q >= 0, concatenated
  real shift = (real)0;           // density scale of the separable model
  const wiski_twolevel* two_level = nullptr;   // exact block on the dominant modes: fused fp32 path (d = 3, m % 4 == 0, eigen tables) only
  int keep[3] = {0, 0, 0};        // eigenmodes per dimension the preconditioner transforms (the rest: t = r, y = 0 -- spectral_keep.h); 0: all.
                                  // fused fp32 path, k = 1, multiples of 4 up to min(g_q, 24)
  // iterate
  real* U = nullptr;              // [k][m] solution, in place
  real* Z = nullptr;              // [k][m] its pre-image, U = Kt Z
  real* R = nullptr;              // [k][m] caller-owned residual RHS - Z - A U, current on return; NULL: workspace scratch
  int warm = 0;                   // 0: from zero; 1: from the given (U, Z); 2: likewise, and R already holds their residual (no A U product)
  // stopping
  double tol = 0;                 // every column: ||r|| / ||rhs|| < tol
  int max_iter = 0;
  int check_every = 0;            // iterations between two convergence polls; < 1: 10
  int first_check = 0;            // iterations before the first poll; 0: check_every; -1 (needs a handle): where the handle's previous
                                  // solve first met the tolerance (first_ok), check_every without such history
  // workspace
  void* work = nullptr;           // PcgLayout<real>::bytes(m, k, max_iter) bytes of device scratch
  int64_t work_bytes = 0;
  // reports (host pointers, each may be NULL) and the device flag that rides on the last poll into h_err
  int32_t* h_iters = nullptr;     // iterations run
  double* h_relres = nullptr;     // [k] final relative residuals
  const int32_t* d_err = nullptr; // device: the out-of-grid flag of the absorb / gather entry points
  int32_t* h_err = nullptr;       // its raw value as the last poll saw it
  int32_t* h_first_ok = nullptr;  // hindsight of the last poll: the first iteration slot at which every column had met the tolerance
                                  // (the largest over the columns of each column's first such slot; <= h_iters), -1: some column never did
  // deferred poll: 0 = run to convergence; 1 = START: queue the iterations up to the first poll, queue the poll, return
  // WISKI_PENDING without waiting for it; 2 = RESUME a started solve (same arguments): wait for that poll, finish with
  // synchronous polls if it had not converged.  Nothing but the resume call may use (U, Z, R, work) in between
  wiski_pcg_async* handle = nullptr;   // owns the poll buffer of a deferred solve; `prezeroed`: an earlier kernel zeroed both zero regions
  int mode = 0;
  // shard (wiski_shard, nranks > 1): A holds only this rank's groups of the half stencil; every A . v product is this rank's share,
  // summed over the ranks by ONE all-reduce of an m-vector (+ the p . Ap slots) on the solve's stream.  Preconditioner, vector
  // updates and scalars are replicated, so all ranks take identical iterations.  k = 1, half stencil, m % 4 == 0
  const wiski_shard* shard = nullptr;
  // tap stage (AbsorbArgs::tap_stage): the absorb queued before this solve left its per-tap adds on RHS, the density row sums and R
  // in tap_stage [m][4] instead of the three arrays.  The solve adds them in and zeroes the records before anything reads RHS or R:
  // inside its first kernel where that is the truncated forward transform of a carried residual (fp32, keep, warm = 2), else by a
  // launch of tap_fold() first.  Whatever pcg() returns -- a refusal included -- the records have been folded and are zero again.
  // fp32, k = 1, not RESUME; tap_b (the writable RHS) always, tap_cnt optional
  real* tap_stage = nullptr;
  real* tap_b = nullptr;
  real* tap_cnt = nullptr;
};

// Where everything lies in a solve's workspace: 20 slots of one 256-byte-aligned [k][m] vector each, then the scalar block.
template <typename real>
struct PcgLayout {
  static constexpr int SLOTS = 20;
  static int64_t align(int64_t v) { return (v + 255) / 256 * 256; }
  static int64_t bytes(int m, int k, int max_iter, int elem_size = (int)sizeof(real)) {
    return SLOTS * align((int64_t)k * m * elem_size) + align(PcgScal::doubles(k, max_iter) * 8);
  }
  real *r, *y, *p, *pt, *hp, *tmp;   // residual (unless the caller owns it), P r, search direction and its pre-image, A p (+ pt), Kron scratch
  real* part;                        // 8 slots: the partial vectors of the wide SpMV, the atomically accumulated one last
  real* ty;                          // 2 slots: [t | y] of the unfused spectral preconditioner
  real *sa, *sb;                     // 2 slots each: scratch of the spectral transforms
  PcgScal S;                         // the scalar block: ||rhs||^2, per-iteration rho / rn, poll ticket, dot-slot ring
  int64_t km;                        // elements of one [k][m] vector
  int64_t nscal;                     // doubles of S
  PcgLayout(int m, int k, int max_iter, void* work) : km((int64_t)k * m), nscal(PcgScal::doubles(k, max_iter)) {
    char* w = static_cast<char*>(work);
    const int64_t vec = align(km * (int64_t)sizeof(real));
    auto at = [&](int slot) { return reinterpret_cast<real*>(w + slot * vec); };
    r = at(0); y = at(1); p = at(2); pt = at(3); hp = at(4); tmp = at(5); part = at(6); ty = at(14); sa = at(16); sb = at(18);
    double* base = reinterpret_cast<double*>(at(SLOTS));
    S = PcgScal{base, k, base + PcgScal::scalars(k, max_iter)};
  }
  // The two regions that must be zero when a solve starts: all of S, and -- where the product leaves `nch` partial vectors of which
  // the last is accumulated atomically (`zl`) -- that vector.  The solve zeroes them in one launch of its own unless an earlier
  // kernel of the streaming step did (AbsorbArgs::z1 / z2, wiski_pcg_async::prezeroed): both sides read them here.
  double* zero1() const { return S.base; }
  int64_t zero1_count() const { return nscal; }
  real* zero2(int nch) const { return part + (int64_t)(nch > 0 ? nch - 1 : 0) * km; }
  int64_t zero2_count(int zl) const { return zl ? km : 0; }
};

// Validates, then queues the solve on `stream` and polls it: WISKI_OK, WISKI_E_NOTCONV (max_iter reached, result written),
// WISKI_PENDING (mode 1), WISKI_E_BADARG / WISKI_E_WORKSPACE (nothing was queued, the handle is untouched) or WISKI_E_LAUNCH.
// Instantiated for float and double in solve.hip.
template <typename real>
int pcg(const wiski_grid* grid, const PcgArgs<real>& args, void* stream);

// The zero regions (pointer, bytes) of a solve with these parameters on workspace `work`, for a caller that has an earlier kernel
// zero them; and the device word + value a kernel queued behind a started solve tests to learn that its poll found it converged
// (wiski_pcg_zero_regions, wiski_pcg_async_guard).
template <typename real>
int pcg_zero_regions(const wiski_grid* grid, int k, int max_iter, void* work, bool a_sym, void** p1, int64_t* n1_bytes, void** p2, int64_t* n2_bytes);
int pcg_guard(const wiski_pcg_async* handle, const void** d_guard, int64_t* expect);

// b += stage[.][0], cnt += stage[.][1], res += stage[.][2] (cnt, res: each may be NULL) with plain stores, and stage = 0: one launch
// on `stream`.  What a solve does with PcgArgs::tap_stage when its first kernel cannot.
int tap_fold(float* stage, float* b, float* cnt, float* res, int64_t m, void* stream);
