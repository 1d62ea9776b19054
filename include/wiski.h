/*
 * wiski.h -- C ABI of libwiski_hip.so: the MI355X (gfx950) implementation of the
 * WISKI streaming-update hot path of wjmaddox/online_gp.
 *
 * The reference has no FFI: its boundary is the Python object surface
 * (SURVEY.md section 8b).  Each entry point below replaces the torch/gpytorch
 * op sequence at the cited reference call site (paths relative to the
 * reference repo; BFN = online_gp/models/batched_fixed_noise_online_gp.py,
 * URLT = online_gp/lazy/updated_root_lazy_tensor.py,
 * BWM = online_gp/mlls/batched_woodbury_marginal_log_likelihood.py).
 *
 * Conventions
 *   - every function is `extern "C" int fn(..., void* stream)`; returns
 *     WISKI_OK or a negative WISKI_E_* code, never throws, never allocates
 *     memory the caller can see;
 *   - `stream` is a hipStream_t; work is enqueued asynchronously on it
 *     (wiski_pcg_* additionally synchronises the stream at its convergence
 *     checks);
 *   - pointers named d_* are DEVICE pointers borrowed for the call; all other
 *     pointers are HOST pointers (small per-dim arrays, outputs of wiski_pcg);
 *   - `_f32` / `_f64` suffix = scalar type of every `real` array;
 *   - dense vectors over the inducing grid are stored column-major as
 *     V[k][m] (k contiguous m-vectors); flat grid index has dim 0 slowest;
 *   - W^T D^-1 W is kept in block-stencil form A_st[o][i] = A[i, i+off(o)],
 *     o in 7^d relative offsets, i in [0, m)  (layout: o-major, m contiguous).
 */
#ifndef WISKI_H
#define WISKI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WISKI_OK 0
#define WISKI_E_BADARG (-1)   /* unsupported d / k / null pointer          */
#define WISKI_E_LAUNCH (-2)   /* hip launch or runtime error               */
#define WISKI_E_WORKSPACE (-3) /* workspace too small                      */
#define WISKI_E_NOTCONV (-4)  /* wiski_pcg hit max_iter (result still written) */
#define WISKI_PENDING 1       /* wiski_pcg_async / wiski_stream_step: the solve was started, its first poll is in flight */

#define WISKI_MAX_DIM 4

/* Inducing-grid geometry (host struct, passed by pointer, read at call time).
 * g0/h follow gpytorch's GridInterpolationKernel grid (BFN:114-120):
 * delta=(hi-lo)/(g-2), grid=linspace(lo-delta, hi+delta, g). */
typedef struct wiski_grid {
  int32_t d;                      /* 1..WISKI_MAX_DIM                      */
  int32_t g[WISKI_MAX_DIM];       /* points per dim (incl. 2 extension pts) */
  double g0[WISKI_MAX_DIM];       /* first grid point per dim               */
  double h[WISKI_MAX_DIM];        /* grid spacing per dim                   */
} wiski_grid;

int wiski_version(void);
/* A hipStream_t for work off the critical path (lazy/two_level.py: the refresh of the two-level block), at the device's lowest priority
 * when asked: beside a kernel of the caller's stream that fills every wave slot the dispatcher then serves the caller first. */
int wiski_side_stream_create(int32_t lowest_priority, void** out);

/* a1 -- replaces covar_module(X).evaluate_kernel() (BFN:143,205,261,421):
 * cubic (Keys a=-0.5) interpolation indices/values, T=4^d taps per point,
 * d_idx int32 [n][T], d_val real [n][T].  Out-of-grid points set *d_err != 0
 * (the reference raises RuntimeError there). */
int wiski_interp_f32(const wiski_grid* grid, const float* d_x, int64_t n, int32_t* d_idx, float* d_val, int32_t* d_err, void* stream);
int wiski_interp_f64(const wiski_grid* grid, const double* d_x, int64_t n, int32_t* d_idx, double* d_val, int32_t* d_err, void* stream);

/* a14 -- replaces left_interp(idx, val, pred_mean) (BFN:206-210,235), fused:
 * weights are recomputed from x on the fly, nothing but x and V is read.
 * d_out[n][k] = W(x) V,  V given as [k][m].  diag != 0: requires k == n and
 * writes d_out[p] = W(x_p) . V[p]  (per-query quadratic forms, BFN:222-228). */
int wiski_gather_f32(const wiski_grid* grid, const float* d_x, int64_t n, const float* d_V, int32_t k, int32_t diag, float* d_out, int32_t* d_err, void* stream);
int wiski_gather_f64(const wiski_grid* grid, const double* d_x, int64_t n, const double* d_V, int32_t k, int32_t diag, double* d_out, int32_t* d_err, void* stream);

/* Input gradient of the interpolation row (learned stems; streaming_partial_mll.py:20-36
 * differentiates through W):  d_out[n][d] = d/dx ( W(x_p) . V_c ), c = 0 (diag == 0, one
 * column d_V[m]) or c = p (diag != 0, d_V[n][m]). */
int wiski_gather_grad_f32(const wiski_grid* grid, const float* d_x, int64_t n, const float* d_V, int32_t diag, float* d_out, void* stream);
int wiski_gather_grad_f64(const wiski_grid* grid, const double* d_x, int64_t n, const double* d_V, int32_t diag, double* d_out, void* stream);

/* a14 with the dense operand stored ROW-major, d_Vr[m][ncols] (left_interp's own layout,
 * BFN:206-210): d_out[n][ncols] = W(x) Vr.  Every tap reads a contiguous row segment;
 * used for W* M with the cached dense posterior M of small grids (BFN:222-225). */
int wiski_gather_rows_f32(const wiski_grid* grid, const float* d_x, int64_t n, const float* d_Vr, int32_t ncols, float* d_out, int32_t* d_err, void* stream);
int wiski_gather_rows_f64(const wiski_grid* grid, const double* d_x, int64_t n, const double* d_Vr, int32_t ncols, double* d_out, int32_t* d_err, void* stream);
/* Input gradient (VJP) of wiski_gather_rows: d_gx[n][d] = sum_c d_G[p][c] * d/dx_p ( W(x_p) Vr )[c] for the upstream gradient d_G[n][ncols]
 * (same row-major d_Vr[m][ncols]).  Zero derivative in the one-hot boundary cells (as wiski_gather_grad); n = 0 is a no-op. */
int wiski_gather_rows_vjp_f32(const wiski_grid* grid, const float* d_x, int64_t n, const float* d_Vr, int32_t ncols, const float* d_G, float* d_gx, void* stream);
int wiski_gather_rows_vjp_f64(const wiski_grid* grid, const double* d_x, int64_t n, const double* d_Vr, int32_t ncols, const double* d_G, double* d_gx, void* stream);
/* Interpolated bilinear forms of a dense symmetric table (look-ahead acquisitions, csrc/lookahead.hip):
 * d_out[s][a][b] = w(xL[s][a])^T A w(xR[s][b]) for d_A [m][lda] (lda >= m), d_xL [nbatch][qL][d], d_xR [nbatch][qR][d], d_out [nbatch][qL][qR].
 * Symmetric mode (xR = xL) exactly when d_xR is NULL (qR must equal qL): one triangle is computed and mirrored (exactly symmetric output);
 * a non-NULL d_xR is always the general mode, also when it aliases d_xL (two independent inputs for the VJP).
 * Points outside the grid set *d_err (as wiski_gather_rows) and contribute zero.  nbatch, qL or qR = 0 is a no-op. */
int wiski_interp_bilinear_f32(const wiski_grid* grid, const float* d_A, int64_t lda, const float* d_xL, int32_t qL, const float* d_xR, int32_t qR, int64_t nbatch, float* d_out, int32_t* d_err, void* stream);
int wiski_interp_bilinear_f64(const wiski_grid* grid, const double* d_A, int64_t lda, const double* d_xL, int32_t qL, const double* d_xR, int32_t qR, int64_t nbatch, double* d_out, int32_t* d_err, void* stream);
/* Input gradient (VJP) of wiski_interp_bilinear for the upstream gradient d_G [nbatch][qL][qR] (A symmetric): d_gxL [nbatch][qL][d] and
 * d_gxR [nbatch][qR][d] (either may be NULL to skip it).  Symmetric mode (d_xR NULL): the whole gradient goes to d_gxL and d_gxR must be NULL.
 * Zero derivative in the one-hot boundary cells and outside the grid; fp64 accumulation in a fixed order (deterministic, no atomics). */
int wiski_interp_bilinear_vjp_f32(const wiski_grid* grid, const float* d_A, int64_t lda, const float* d_xL, int32_t qL, const float* d_xR, int32_t qR, int64_t nbatch, const float* d_G, float* d_gxL, float* d_gxR, void* stream);
int wiski_interp_bilinear_vjp_f64(const wiski_grid* grid, const double* d_A, int64_t lda, const double* d_xL, int32_t qL, const double* d_xR, int32_t qR, int64_t nbatch, const double* d_G, double* d_gxL, double* d_gxR, void* stream);

/* a14, ELL form -- same product from materialised (idx, val) rows of width T
 * (the layout InterpolatedLazyTensor keeps; BFN:206-210). k == 1 only. */
int wiski_gather_ell_f32(const int32_t* d_idx, const float* d_val, int64_t n, int32_t T, const float* d_v, float* d_out, void* stream);
int wiski_gather_ell_f64(const int32_t* d_idx, const double* d_val, int64_t n, int32_t T, const double* d_v, double* d_out, void* stream);
/* The same product for rows written by wiski_interp on `grid` (idx[tap] = base + sum_q c_q stride_q; T = 4^d): d_v is first
 * copied into a blocked layout (second-to-last dim in groups of 4, once per alignment of the stencil: csrc/gather_ell_dma.h) in which
 * every lane's four taps are one aligned group of four reals and a row touches ~5.5 cache lines instead of ~17.5 -- the gathers of v, not the
 * idx / val stream, bound the plain form.  d_vpack: scratch of
 * wiski_gather_ell_pack_elems(grid) reals, 16-byte aligned (0 elements: d = 1 or a grid too large -- pass NULL).  Small row
 * counts, d = 1, a NULL or misaligned scratch take wiski_gather_ell. */
int wiski_gather_ell_grid_f32(const wiski_grid* grid, const int32_t* d_idx, const float* d_val, int64_t n, const float* d_v, float* d_vpack, float* d_out, void* stream);
int wiski_gather_ell_grid_f64(const wiski_grid* grid, const int32_t* d_idx, const double* d_val, int64_t n, const double* d_v, double* d_vpack, double* d_out, void* stream);
int64_t wiski_gather_ell_pack_elems(const wiski_grid* grid);

/* a2+a3+a4+URLT:58 -- replaces _initialize_caches / _update_cache_dicts /
 * UpdatedRootLazyTensor.update's `tensor + V V^T` (BFN:31-60,155-171):
 *   d_b[m]      += W^T (y * wb)            interpolation_cache
 *   d_A_st      += W^T diag(wa) W          WtW (block stencil; may be NULL)
 *   d_stats[0]  += sum y^2 wb              response_cache      (double)
 *   d_stats[1]  += sum log(noise)          D_logdet            (double)
 * wa/wb/noise are per-point device arrays [n] (wb = 1/noise; wa = 1/noise at
 * initialisation, 1/max(noise,1e-7) on updates -- BFN:163). */
int wiski_scatter_stats_f32(const wiski_grid* grid, const float* d_x, const float* d_y, const float* d_wa, const float* d_wb, const float* d_noise, int64_t n, float* d_b, float* d_A_st, double* d_stats, int32_t* d_err, void* stream);
int wiski_scatter_stats_f64(const wiski_grid* grid, const double* d_x, const double* d_y, const double* d_wa, const double* d_wb, const double* d_noise, int64_t n, double* d_b, double* d_A_st, double* d_stats, int32_t* d_err, void* stream);

/* Same statistics with W^T diag(wa) W accumulated into the SYMMETRIC HALF stencil d_A_half --
 * the model's native WtW storage (replaces the dense m x m tensor of URLT:42,58).  Only stencil
 * offsets >= the centre are kept ((7^d+1)/2 * m reals: half the atomics of the full form, half the
 * bytes per product, and the buffer the data-parallel path all-reduces), in the "row-interleaved"
 * layout: with P the leading d-1 base-7 digits of an offset, s its innermost digit and
 * g = P - P_centre >= 0,
 *     g == 0 :  d_A_half[4 i + (s - 3)]                s = 3..6  (s = 3: the diagonal A[i,i])
 *     g >= 1 :  d_A_half[(7 g - 3) m + 7 i + s]        s = 0..6
 * holds A[i, i + off(P, s)].  (The 16 innermost-digit combinations of a tap pair then fall into one
 * 88-byte span, which is what the transaction-bound memory-side atomics want: 72 us vs 208 us per 4096
 * points at 50^3 against an offset-major half stencil.)  wiski_stencil_expand_add unpacks it into a
 * full offset-major stencil: A_st += expand(d_A_half), d_A_half = 0. */
int wiski_scatter_stats_sym_f32(const wiski_grid* grid, const float* d_x, const float* d_y, const float* d_wa, const float* d_wb, const float* d_noise, int64_t n, float* d_b, float* d_A_half, double* d_stats, int32_t* d_err, void* stream);
int wiski_scatter_stats_sym_f64(const wiski_grid* grid, const double* d_x, const double* d_y, const double* d_wa, const double* d_wb, const double* d_noise, int64_t n, double* d_b, double* d_A_half, double* d_stats, int32_t* d_err, void* stream);
/* One-launch form used by the model: as above (half != 0: d_A is the symmetric half stencil,
 * else the full offset-major one) and additionally
 *   d_cnt[m] += W^T wa      the row sums of the increment (the preconditioner's data-density statistic;
 *                           d_cnt may be NULL)
 *   d_res[m] += W^T (wb y - wa (W d_u))      (d_u / d_res: both or neither; half form only)
 * the residual carry-over: if d_res held b - z - A u for the current solution (u, z) of
 * (Kt^-1 + A) u = b, it still does after the increment, so the next wiski_pcg warm start (warm = 2)
 * needs no A u product. */
int wiski_scatter_stats_cnt_f32(const wiski_grid* grid, const float* d_x, const float* d_y, const float* d_wa, const float* d_wb, const float* d_noise, int64_t n, float* d_b, float* d_A, int32_t half, float* d_cnt, const float* d_u, float* d_res, double* d_stats, int32_t* d_err, void* stream);
int wiski_scatter_stats_cnt_f64(const wiski_grid* grid, const double* d_x, const double* d_y, const double* d_wa, const double* d_wb, const double* d_noise, int64_t n, double* d_b, double* d_A, int32_t half, double* d_cnt, const double* d_u, double* d_res, double* d_stats, int32_t* d_err, void* stream);
int wiski_stencil_expand_add_f32(const wiski_grid* grid, float* d_A_half, float* d_A_st, void* stream);
int wiski_stencil_expand_add_f64(const wiski_grid* grid, double* d_A_half, double* d_A_st, void* stream);

/* Adds W(x)^T as k = n one-hot-interpolated columns: d_out[p][idx] += val
 * (the sparse `wmat` of BFN:22-28 for a query batch, kept column-dense only
 * for the k right-hand sides of a solve). d_out must be zeroed by the caller. */
int wiski_wt_columns_f32(const wiski_grid* grid, const float* d_x, int64_t n, float* d_out, int32_t* d_err, void* stream);
int wiski_wt_columns_f64(const wiski_grid* grid, const double* d_x, int64_t n, double* d_out, int32_t* d_err, void* stream);

/* Jet rows J(x) = [w(x); d_1 w(x); ...; d_d w(x)], C = d + 1 channels (csrc/jet_rows.h): channel 0 is the value row, channel 1 + q has
 * dim q's four weights replaced by k'(s) / h_q and is identically zero where dim q's cell is a one-hot boundary cell (as
 * wiski_gather_grad).  A point outside the grid has all C rows zero and sets bit 0 of *d_err (as wiski_gather).  All three: n = 0 is a
 * no-op; a null pointer, k < 1, rows_per_point < 0 or ldm < m is WISKI_E_BADARG without a launch.
 * wiski_jet_quadform: d_out[p][c][c'] = sum_ab J_c(x_p)[a] d_M[idx_a][idx_b] J_c'(x_p)[b] for a row-major d_M [m][ldm] (ldm >= m), d_out
 *   [n][C][C].  Reads the 4^d x 4^d sub-block of the point's taps only; fp64 accumulation; the lower triangle is a copy of the upper. */
int wiski_jet_quadform_f32(const wiski_grid* grid, const float* d_x, int64_t n, const float* d_M, int64_t ldm, float* d_out, int32_t* d_err, void* stream);
int wiski_jet_quadform_f64(const wiski_grid* grid, const double* d_x, int64_t n, const double* d_M, int64_t ldm, double* d_out, int32_t* d_err, void* stream);
/* wiski_wt_columns_jet: row p C + c of the caller-zeroed d_out [n C][m] receives J_c(x_p) (plain stores); row p C is the column that
 *   wiski_wt_columns writes for x_p, bit for bit. */
int wiski_wt_columns_jet_f32(const wiski_grid* grid, const float* d_x, int64_t n, float* d_out, int32_t* d_err, void* stream);
int wiski_wt_columns_jet_f64(const wiski_grid* grid, const double* d_x, int64_t n, double* d_out, int32_t* d_err, void* stream);
/* wiski_gather_jet: rows_per_point = 0: d_V [k][m] is shared by all points, d_out[p][j][c] = J_c(x_p) . d_V[j], d_out [n][k][C].
 *   rows_per_point = B >= 1: d_V [n B][m], d_out[p][j][c] = J_c(x_p) . d_V[p B + j], d_out [n][B][C] (k is not used beyond k >= 1).
 *   fp64 accumulation. */
int wiski_gather_jet_f32(const wiski_grid* grid, const float* d_x, int64_t n, const float* d_V, int32_t k, int32_t rows_per_point, float* d_out, int32_t* d_err, void* stream);
int wiski_gather_jet_f64(const wiski_grid* grid, const double* d_x, int64_t n, const double* d_V, int32_t k, int32_t rows_per_point, double* d_out, int32_t* d_err, void* stream);

/* Box functionals c_b = int_box w(x) dx (csrc/box_rows.h): the Kronecker product of d per-dimension integrated rows.  Boxes d_lo, d_hi
 * [B][d].  A box is clipped to the grid's extent (w = 0 outside); a dimension with lo == hi evaluates at that coordinate instead of
 * integrating (its row is the value row of wiski_wt_columns, bit for bit, and its factor of the volume is 1).  A box not wholly
 * inside the grid sets bit 0 of *d_err; a NaN bound or lo > hi also gives a zero row.  All three: B = 0 is a no-op; a null pointer,
 * k < 1, rows_per_box < 0 or nsplit outside 1 .. 65535 is WISKI_E_BADARG without a launch.
 * wiski_box_tables: d_tab [B][sum_q g_q] the per-dimension rows (every entry written, evaluated in fp64 and rounded once), d_range
 *   [B][d][2] the node range [first, end) of each row's support, d_vol [B] the clipped volume (0 when nothing of the box is inside). */
int wiski_box_tables_f32(const wiski_grid* grid, const float* d_lo, const float* d_hi, int64_t B, float* d_tab, int32_t* d_range, float* d_vol, int32_t* d_err, void* stream);
int wiski_box_tables_f64(const wiski_grid* grid, const double* d_lo, const double* d_hi, int64_t B, double* d_tab, int32_t* d_range, double* d_vol, int32_t* d_err, void* stream);
/* wiski_wt_columns_box: row b of the caller-zeroed d_out [B][m] receives c_b (plain stores over the support). */
int wiski_wt_columns_box_f32(const wiski_grid* grid, const float* d_tab, const int32_t* d_range, int64_t B, float* d_out, void* stream);
int wiski_wt_columns_box_f64(const wiski_grid* grid, const double* d_tab, const int32_t* d_range, int64_t B, double* d_out, void* stream);
/* wiski_gather_box: rows_per_box = 0: d_V [k][m] is shared by all boxes, d_out[b][j] = c_b . d_V[j], d_out [B][k].  rows_per_box = R >= 1:
 *   d_V [B R][m], d_out[b][j] = c_b . d_V[b R + j], d_out [B][R] (k is not used beyond k >= 1).  fp64 accumulation.  nsplit blocks share
 *   the support of each (box, row); nsplit > 1 needs the workspace d_part [B rows][nsplit] doubles and adds a small second launch. */
int wiski_gather_box_f32(const wiski_grid* grid, const float* d_tab, const int32_t* d_range, int64_t B, const float* d_V, int32_t k, int32_t rows_per_box, int32_t nsplit, double* d_part, float* d_out, void* stream);
int wiski_gather_box_f64(const wiski_grid* grid, const double* d_tab, const int32_t* d_range, int64_t B, const double* d_V, int32_t k, int32_t rows_per_box, int32_t nsplit, double* d_part, double* d_out, void* stream);

/* replaces WtW._matmul (URLT:47-48) on the stencil form:
 * d_out[c] = beta * d_add[c] + A_st . d_V[c]   (d_add may be NULL).
 * d_A_st is offset-major [7^d][m]: offset o has the base-7 digits (dimension 0 slowest) digit - 3 = shift per dimension, entry
 * (o, i) is A[i, i + off(o)].  CONTRACT of both forms: an entry whose neighbour i + shift leaves the grid in any dimension must be
 * an exact zero, and every stored entry and every element of d_V (and d_add) finite -- the kernels clamp or wrap the neighbour
 * index of such entries instead of branching, so they multiply a zero with some other element of d_V.
 * Refused with WISKI_E_BADARG before anything is launched or written: a NULL d_A_st / d_A_half, d_V or d_out, k < 1, d_out == d_V
 * (both forms), a grid make_grid would refuse (d outside 1..4, a g[q] < 4, 2^31 nodes or more). */
int wiski_stencil_spmv_f32(const wiski_grid* grid, const float* d_A_st, const float* d_V, int32_t k, const float* d_add, float beta, float* d_out, void* stream);
int wiski_stencil_spmv_f64(const wiski_grid* grid, const double* d_A_st, const double* d_V, int32_t k, const double* d_add, double beta, double* d_out, void* stream);
/* Same product on the symmetric half stencil d_A_half (layout: wiski_scatter_stats_sym); every
 * stored entry is used for A[i,j] and A[j,i], so a product streams half the HBM bytes of the full
 * form.  d_out must not alias d_V. */
int wiski_stencil_spmv_sym_f32(const wiski_grid* grid, const float* d_A_half, const float* d_V, int32_t k, const float* d_add, float beta, float* d_out, void* stream);
int wiski_stencil_spmv_sym_f64(const wiski_grid* grid, const double* d_A_half, const double* d_V, int32_t k, const double* d_add, double beta, double* d_out, void* stream);
/* Which kernel the two products above take for k columns of elem_bytes (4 or 8) wide reals on the full (half == 0) or the half
 * stencil; launches nothing, reads the same once-per-process switches (WISKI_SYM_DMA, WISKI_SPMM_BCAST) as the launchers.
 *   0 k_stencil_spmv            full, m % 4 != 0                 *kc = 1, 2 or 4 columns per pass
 *   1 k_stencil_spmv4 (+ k_spmv_reduce)  full, m % 4 == 0        *kc = 1, 2, 4, 8; d = 2, 3 and k >= 8: k_stencil_spmm, *kc = 8 or 16
 *   2 k_stencil_spmv_sym        half, m % 4 != 0                 *kc = 1, 2 or 4
 *   3 k_stencil_spmv4_sym       half, m % 4 == 0, none of 4..7   *kc = 1, 2 or 4
 *   4 k_spmv_sym_dma            fp32, d = 3, k = 1, LDS <= 64 KB *kc = 1
 *   5 k_spmv_sym_dma_mc         fp32, d = 3, 2 <= k < 16, g[2] >= 4, LDS <= 64 KB   *kc = 2 (k < 4) or 4
 *   6 k_spmm_sym_bcast          k >= 16 (fp32) / 24 (fp64)       *kc = 64 (columns per slice)
 *   7 k_spmm_sym_cols           WISKI_SPMM_BCAST=0 and k >= 32   *kc = k rounded up to a multiple of 16
 * kc may be NULL.  WISKI_E_BADARG: k < 1, elem_bytes other than 4 or 8, a grid the products refuse. */
int wiski_stencil_spmv_path(const wiski_grid* grid, int32_t k, int32_t elem_bytes, int32_t half, int32_t* kc);

/* a8/a9/a11 -- replaces Kuu @ V (BFN:334-348,363-366) with
 * Kuu = kron_i SymToeplitz(tcol_i): d_out[c] = scale * Kuu d_V[c].
 * d_tcol = concatenated first columns (sum_i g[i] reals).  d_tmp: scratch of
 * k*m reals (ping-pong); d_out must not alias d_V. */
int wiski_kron_toeplitz_mm_f32(const wiski_grid* grid, const float* d_tcol, const float* d_V, int32_t k, float scale, float* d_tmp, float* d_out, void* stream);
int wiski_kron_toeplitz_mm_f64(const wiski_grid* grid, const double* d_tcol, const double* d_V, int32_t k, double scale, double* d_tmp, double* d_out, void* stream);

/* a17 backward -- gradient of bilinear forms in Kuu w.r.t. the Toeplitz columns
 * (what autograd computes through Kuu in BWM:19-51 / BFN:334-366):
 *   d_grad[sum g] += d/d tcol  sum_c X[c]^T (kron_q SymToeplitz(tcol_q)) Y[c]
 * d_tmp: 2*k*m reals of scratch; d_grad is double and is accumulated into. */
int wiski_kron_toeplitz_grad_f32(const wiski_grid* grid, const float* d_tcol, const float* d_X, const float* d_Y, int32_t k, float* d_tmp, double* d_grad, void* stream);
int wiski_kron_toeplitz_grad_f64(const wiski_grid* grid, const double* d_tcol, const double* d_X, const double* d_Y, int32_t k, double* d_tmp, double* d_grad, void* stream);

/* Spectral functions of Kt = kscale*Kuu in its Kronecker eigenbasis (d_evec/d_eval
 * as for wiski_pcg): d_out[c] = V diag(lam^pw / (1 + shift*lam)^rw) V^T d_V[c].
 * pw = 0.5, rw = 0 gives the symmetric root Kt^(1/2) (logdet(Q) by stochastic
 * Lanczos quadrature, BWM:27 inv_quad_logdet).  d_tmp: k*m reals.
 * The factors need not be orthogonal: d_evec holds d row-major g[q] x g[q] tables F_q (column = mode) and the
 * product is (kron F_q) diag(f) (kron F_q)^T d_V[c]; f is 0 where pw != 0 and lam <= 0.  Supported: 4 <= g[q] <= 128
 * in both precisions (a factor is held in g[q]^2 reals of LDS, 128 KB in fp64 at g = 128, requested per launch;
 * WISKI_E_LAUNCH if the device refuses it), k >= 1, d_out distinct from d_V; anything else returns WISKI_E_BADARG
 * before any launch.  wiski_kron_toeplitz_mm takes 4 <= g[q] <= 256. */
int wiski_kron_spectral_mm_f32(const wiski_grid* grid, const float* d_evec, const float* d_eval, float kscale, float shift, float pw, float rw, const float* d_V, int32_t k, float* d_tmp, float* d_out, void* stream);
int wiski_kron_spectral_mm_f64(const wiski_grid* grid, const double* d_evec, const double* d_eval, double kscale, double shift, double pw, double rw, const double* d_V, int32_t k, double* d_tmp, double* d_out, void* stream);

/* CG branch of a12 (BFN:368-383; gpytorch linear_cg under Q.inv_matmul),
 * moved to inducing space: solves (Kt^-1 + A) U = RHS, Kt = kscale*Kuu, for k
 * columns by preconditioned CG (no inverse of Kt is ever applied):
 *   U = M RHS,  M = (Kt^-1 + A)^-1  (SURVEY 3.5).
 * Preconditioner:
 *   d_evec == NULL : P = Kt                      (needs d_tcol)
 *   d_evec != NULL : P = (Kt^-1 + shift * kron_q diag(t_q))^-1, a separable model of A
 *     (t_q = per-dim data-density profile; t_q = 1 gives shift * I), applied through the
 *     per-dim generalized eigenproblems  K_q = X_q D_q X_q^T,  X_q^T diag(t_q) X_q = I:
 *     d_evec = concatenated row-major g_q x g_q matrices X_q, d_evec2 = Z_q = diag(t_q) X_q
 *     (NULL when t_q = 1: Z_q = X_q orthogonal), d_eval = concatenated D_q (>= 0);
 *     shift = density scale (d_tcol unused).
 * d_U/d_Z [k][m]: solution and its pre-image (U = Kt Z). warm != 0 starts
 * from the given (U, Z) (must satisfy U = Kt Z), else from zero.
 * Stops when every column has ||r||/||rhs|| < tol or at max_iter; the host polls the
 * residual norms after first_check iterations (< 1: check_every) and then every
 * check_every iterations.  A poll is a tiny publish kernel writing to host-mapped memory that
 * the host spins on (no stream synchronisation).  d_err (may be NULL): the out-of-grid flag of
 * the interp/scatter/gather entry points; its raw value (bit 0: some point was outside the grid; bits 1..:
 * number of training points the scatter kernels dropped for that reason) rides on the last poll into
 * *h_err, so the caller needs no separate device-to-host read to raise the reference's RuntimeError.
 * Host threads: the poll buffer is per device and held under a mutex for the duration of a solve, so
 * concurrent solves on one device from several host threads serialise (the calling thread's current
 * device must be the one the pointers live on).
 * a_sym != 0: d_A_st is the symmetric half stencil (wiski_scatter_stats_sym layout) instead of
 * the full offset-major [7^d][m] one.
 * d_R (k*m reals, may be NULL): caller-owned residual buffer used instead of workspace scratch; on return
 * it holds rhs - Z - A U for the returned (U, Z).  warm = 2 (needs d_R): d_R already holds that residual
 * for the incoming (U, Z) -- kept current across streaming updates by wiski_scatter_stats_cnt's d_res --
 * so the solve starts without an A U product.
 * workspace: wiski_pcg_workspace_bytes(...) bytes of device scratch.
 * h_iters (host, may be NULL): iterations run; h_relres (host, k doubles, may
 * be NULL): final relative residuals. */
int64_t wiski_pcg_workspace_bytes(const wiski_grid* grid, int32_t k, int32_t max_iter, int32_t elem_size);
int wiski_pcg_f32(const wiski_grid* grid, const float* d_A_st, const float* d_tcol, float kscale, const float* d_evec, const float* d_evec2, const float* d_eval, float shift, const float* d_RHS, int32_t k, float* d_U, float* d_Z, int32_t warm, double tol, int32_t max_iter, int32_t check_every, int32_t first_check, void* d_work, int64_t work_bytes, int32_t* h_iters, double* h_relres, const int32_t* d_err, int32_t* h_err, int32_t a_sym, float* d_R, void* stream);
int wiski_pcg_f64(const wiski_grid* grid, const double* d_A_st, const double* d_tcol, double kscale, const double* d_evec, const double* d_evec2, const double* d_eval, double shift, const double* d_RHS, int32_t k, double* d_U, double* d_Z, int32_t warm, double tol, int32_t max_iter, int32_t check_every, int32_t first_check, void* d_work, int64_t work_bytes, int32_t* h_iters, double* h_relres, const int32_t* d_err, int32_t* h_err, int32_t a_sym, double* d_R, void* stream);

/* Stencil-sharded replicas (multi-GPU step that DIVIDES the work).  Rank r of n owns the groups
 * [r G / n, (r + 1) G / n) of the symmetric half stencil (G = (7^(d-1) + 1) / 2 groups, wiski_shard_groups): it scatters only
 * the tap pairs of its groups (wiski_scatter_stats_step_sharded: 1 / n of the atomics per point; b, cnt, the statistics and
 * the carried residual stay replicated, so every rank must see every point) and computes only its groups' share of A p
 * (wiski_pcg_sharded), which ONE all-reduce(SUM) of an m-vector plus the p . Ap slots per product turns into the full
 * product on the solve's stream.  Vectors, preconditioner and scalars are replicated: all ranks take identical iterations.
 * comm != NULL: RCCL (an ncclComm_t, see wiski_comm_*); else `allreduce(ctx, d_vec, n_vec, elem_bytes, d_dots, n_dots, stream)`
 * is called -- in place, SUM, d_dots fp64, must be ordered after the work already queued on `stream` and before what is
 * queued next (tests route it through another transport).  One right-hand side, half stencil, m % 4 == 0; any d, fp32 and fp64
 * (d = 3 fp32: the LDS-DMA kernel on a part table; otherwise the LDS-window kernel on the replica's group range); the RCCL route
 * (comm != NULL) sums the vector in its own precision (ncclFloat32 / ncclFloat64). */
typedef int (*wiski_allreduce_fn)(void* ctx, void* d_vec, int64_t n_vec, int32_t elem_bytes, double* d_dots, int64_t n_dots, void* stream);
typedef struct wiski_shard {
  int32_t rank, nranks;
  void* comm;
  wiski_allreduce_fn allreduce;
  void* ctx;
} wiski_shard;
int wiski_shard_groups(int32_t d, int32_t rank, int32_t nranks, int32_t* g_lo, int32_t* g_hi);

/* Two-level preconditioner of the fused fp32 solve (d = 3).  The separable model
 * P = (Kt^-1 + a kron_q diag(t_q))^-1 is exact only for a separable data density; on road-like (line-clustered) streams
 * W^T D^-1 W is far from that and a warm CG step needs 6 iterations instead of 2.5.  In the generalized eigenbasis X of the
 * separable model (the tables wiski_pcg already transforms with: X^T (kron diag t) X = I, Kt = X^-T D X^-1) the system
 * matrix is D^-1 + X^T A X; the two-level form keeps the EXACT block N = (D_S^-1 + X_S^T A X_S)^-1 on the r modes of largest
 * prior eigenvalue D (the directions the data inform) and the diagonal model D / (1 + a D) on all others -- block Jacobi in
 * spectral coordinates, SPD.  The caller owns N (r x r, fp32) and refreshes it as the stream grows (projection of the new
 * points on X_S + a GEMM + an r x r Cholesky, off the critical path: a stale block only costs iterations, never accuracy).
 * The coupling crosses the dim-0 slabs of the fused slab kernel: the blocks that hold selected modes exchange their r
 * coefficients through d_cs (self-validating 64-bit words stamped with a per-launch number drawn on the host: a launch sequence
 * that uses a wiski_twolevel must not be captured into a graph and replayed), every block then forms the rows of N c it needs.
 * Modes are identified by their eigen-indices (i0, x, y) in the order of the eigen tables handed to the solve. */
typedef struct wiski_twolevel {
  int32_t r;                 /* modes in the exact block, 1 <= r <= 512 */
  int32_t nslab;             /* number of dim-0 eigen-indices i0 that hold at least one selected mode */
  const uint64_t* d_mask;    /* [g0][64]: bit y of d_mask[i0 * 64 + x] set <=> mode (i0, x, y) is selected */
  const int32_t* d_off;      /* [g0 + 1]: the selected modes of slab i0 are d_off[i0] .. d_off[i0 + 1] - 1 in block order */
  const uint16_t* d_pos;     /* [r]: x << 8 | y of every selected mode, block order (sorted by i0) */
  const float* d_N;          /* [r][r] row-major, symmetric positive definite, block order */
  uint64_t* d_cs;            /* [r + 1]: r exchange words {application number << 32 | fp32 bits} + one sticky count of exchange words that
                              * never arrived (their writer block was not co-resident: the application then used a stale coefficient --
                              * drop the block); zeroed ONCE by the caller.  Refused (WISKI_E_BADARG) where 2 g0 exceeds the CU count */
  float* d_mc;               /* [2][mc_cols][r] scratch of the multi-column form, or NULL: solves with k > 1 columns apply the block around the
                              * slab launch (two small launches per application: c_S = X_S^T r per column from the mode-0 image, d = N c_S;
                              * the slab kernel then substitutes d for the selected entries) -- no exchange words, no co-residency needed */
  int32_t mc_cols;           /* columns d_mc has room for; k > mc_cols (or d_mc == NULL with k > 1): WISKI_E_BADARG */
} wiski_twolevel;

/* Deferred convergence poll.  wiski_pcg_async_* = wiski_pcg_* plus a host-side handle (zero-initialised by the caller,
 * released with wiski_pcg_async_free) and a mode: 0 = as wiski_pcg; 1 = START: queue the iterations up to the first poll
 * (first_check), queue the poll, return WISKI_PENDING without waiting -- the host gets its time back while the GPU iterates;
 * 2 = RESUME with the same arguments: wait for that poll (normally long over), finish with synchronous polls if it had not
 * converged, fill h_iters / h_relres / h_err, return 0 / WISKI_E_NOTCONV.  Between START and RESUME nothing else may touch
 * (d_U, d_Z, d_R, d_work) or the system (d_A, d_RHS); the handle owns its own poll buffer.
 * first_check = -1 (needs a handle; every other negative value, and -1 without a handle, is WISKI_E_BADARG): the first poll goes
 * to max(1, handle->first_ok), where the solve this handle finished last first met the tolerance -- solves of one stream are
 * alike, so that poll neither fails (as one placed earlier would, at the price of a host round trip with the GPU idle) nor runs
 * iterations the solve does not need.  Without such history (first_ok_valid == 0) as first_check = 0. */
typedef struct wiski_pcg_async {
  int32_t state;   /* 0 idle, 1 a started solve is waiting to be resumed */
  int32_t it;      /* iterations queued so far */
  int64_t seq;     /* sequence number of the poll in flight */
  void* poll;      /* opaque: the handle's pinned poll buffer */
  int32_t prezeroed; /* set by wiski_stream_step when an earlier kernel of the step has zeroed the solve's scalar block and
                        accumulated partial vector (wiski_gather_zero): the next START / run skips its own zero launch */
  int32_t guard_ok;  /* set by RESUME: 1 when the poll it waited for found every column converged and no error flag, i.e. when a
                        kernel guarded by that poll (wiski_pcg_async_guard) has run */
  double shift;      /* wiski_stream_step: the preconditioner shift the pending solve was STARTed with -- its RESUME continues
                        with it even if the caller has meanwhile set the next step's shift in the argument struct */
  int32_t first_ok;        /* hindsight of the last solve this handle finished (RESUME, or mode 0 with a handle): the first iteration
                              at which every column had met the tolerance -- the largest over the columns of each column's first such
                              iteration, 0 when the start was already converged, <= h_iters -- or -1 when some column never did.
                              The poll publishes it beside the norms (the device keeps ||r_j||^2 of every iteration j; the scan
                              looks back at most 32 iterations), so a poll placed later than needed still tells where it was needed */
  int32_t first_ok_valid;  /* 1 when first_ok >= 0 describes a finished solve: what first_check = -1 places the next first poll by.
                              Set with first_ok, cleared by wiski_pcg_async_free (and in a zero-initialised handle) */
} wiski_pcg_async;
int wiski_pcg_async_f32(const wiski_grid* grid, const float* d_A_st, const float* d_tcol, float kscale, const float* d_evec, const float* d_evec2, const float* d_eval, float shift, const float* d_RHS, int32_t k, float* d_U, float* d_Z, int32_t warm, double tol, int32_t max_iter, int32_t check_every, int32_t first_check, void* d_work, int64_t work_bytes, int32_t* h_iters, double* h_relres, const int32_t* d_err, int32_t* h_err, int32_t a_sym, float* d_R, void* stream, wiski_pcg_async* handle, int32_t mode);
int wiski_pcg_async_f64(const wiski_grid* grid, const double* d_A_st, const double* d_tcol, double kscale, const double* d_evec, const double* d_evec2, const double* d_eval, double shift, const double* d_RHS, int32_t k, double* d_U, double* d_Z, int32_t warm, double tol, int32_t max_iter, int32_t check_every, int32_t first_check, void* d_work, int64_t work_bytes, int32_t* h_iters, double* h_relres, const int32_t* d_err, int32_t* h_err, int32_t a_sym, double* d_R, void* stream, wiski_pcg_async* handle, int32_t mode);
int wiski_pcg_async_free(wiski_pcg_async* handle);
/* Speculation across the poll of a started solve (state == 1): *d_guard is a device int64 that the poll's publishing block sets
 * to +*expect when it finds the solve converged and the error flag clear -- exactly when RESUME will report convergence from
 * that poll -- and to -*expect otherwise.  A kernel queued behind the solve that reads it can run or skip itself without the
 * host having seen the poll (wiski_scatter_stats_step); RESUME then tells through handle->guard_ok which of the two happened. */
int wiski_pcg_async_guard(const wiski_pcg_async* handle, const void** d_guard, int64_t* expect);
/* Support of wiski_stream_step: the two device regions (pointer, bytes) a solve with these parameters zeroes before its first
 * kernel, and a predictive-mean gather (k <= 4 columns, as wiski_gather with diag = 0) whose kernel zeroes them on the way when
 * it can (*zeroed = 1; d = 3 and n <= 65536) -- one launch less per streaming step. */
int wiski_pcg_zero_regions_f32(const wiski_grid* grid, int32_t k, int32_t max_iter, void* d_work, int32_t a_sym, void** p1, int64_t* n1_bytes, void** p2, int64_t* n2_bytes);
int wiski_pcg_zero_regions_f64(const wiski_grid* grid, int32_t k, int32_t max_iter, void* d_work, int32_t a_sym, void** p1, int64_t* n1_bytes, void** p2, int64_t* n2_bytes);
/* The absorb of a streaming step: wiski_scatter_stats_cnt (half-stencil form) that also (i) writes the predictive mean of every
 * point under the CURRENT posterior mean d_u into d_mean_out [n] (the w_p . u it forms for the residual carry anyway -- BFN:206-210
 * without a gather launch; d_res may be NULL when only the mean is wanted), and (ii) zeroes the two regions of
 * wiski_pcg_zero_regions on the way (n*_bytes = 0: none).  d_guard != NULL: the whole kernel (absorb, mean, zeroing) runs only
 * if *d_guard == guard_expect when it starts and is a no-op otherwise (wiski_pcg_async_guard: the absorb of the next batch is
 * queued behind a solve whose convergence poll the host has not read yet).
 * d_bin / bin_bytes (optional, d = 3): a workspace of at least wiski_scatter_bin_bytes(grid, n, sizeof(real)) bytes, zeroed ONCE
 * by the caller and then left alone.  With it, batches of 8192 points or more (WISKI_OWNER_MIN_POINTS) take the owner-computes
 * form -- points binned by cell, one block per grid line adds all contributions to its rows with plain read-modify-writes -- whose
 * cost is a sweep over the touched part of A_half instead of 19 ns of memory-side atomic transactions per point; results agree
 * with the atomic form up to the order of the fp additions. */
int64_t wiski_scatter_bin_bytes(const wiski_grid* grid, int64_t n, int32_t elem_size);
int wiski_scatter_stats_step_f32(const wiski_grid* grid, const float* d_x, const float* d_y, const float* d_wa, const float* d_wb, const float* d_noise, int64_t n, float* d_b, float* d_A_half, float* d_cnt, const float* d_u, float* d_res, float* d_mean_out, double* d_stats, int32_t* d_err, void* z1, int64_t n1_bytes, void* z2, int64_t n2_bytes, const void* d_guard, int64_t guard_expect, void* d_bin, int64_t bin_bytes, void* stream);
int wiski_scatter_stats_step_f64(const wiski_grid* grid, const double* d_x, const double* d_y, const double* d_wa, const double* d_wb, const double* d_noise, int64_t n, double* d_b, double* d_A_half, double* d_cnt, const double* d_u, double* d_res, double* d_mean_out, double* d_stats, int32_t* d_err, void* z1, int64_t n1_bytes, void* z2, int64_t n2_bytes, const void* d_guard, int64_t guard_expect, void* d_bin, int64_t bin_bytes, void* stream);
int wiski_gather_zero_f32(const wiski_grid* grid, const float* d_x, int64_t n, const float* d_V, int32_t k, float* d_out, int32_t* d_err, void* z1, int64_t n1_bytes, void* z2, int64_t n2_bytes, int32_t* zeroed, void* stream);
int wiski_gather_zero_f64(const wiski_grid* grid, const double* d_x, int64_t n, const double* d_V, int32_t k, double* d_out, int32_t* d_err, void* z1, int64_t n1_bytes, void* z2, int64_t n2_bytes, int32_t* zeroed, void* stream);

/* One streaming step in one call (single output, symmetric half stencil): the predictive mean of the incoming batch under
 * the CURRENT posterior mean d_U (written to d_mean_out [q]; skipped when NULL) and the absorb of the q points into b /
 * A_half / cnt / stats (with carry != 0 the residual d_R is kept equal to b - Z - A U) -- one kernel,
 * wiski_scatter_stats_step -- and wiski_pcg (refresh of (d_U, d_Z) for RHS = d_b, warm = 2 when carry != 0 else 1) are queued
 * back to back on `stream` -- what BFN:204-210, BFN:258-273 and BFN:368-383 do in three Python calls.  d_wa / d_wb /
 * d_noise [q]: the per-point weights 1/clamp(noise,1e-7), 1/noise and the noise itself (ones for unit noise).  The struct
 * carries the model-resident pointers and solver parameters (meaning as in wiski_pcg); first_check / h_iters / h_relres /
 * h_err as in wiski_pcg.
 * handle != NULL selects the deferred form: the call first RESUMEs the solve a previous call started (its iteration count,
 * residual and out-of-grid flag land in h_iters / h_relres / h_err; h_resumed = 1), then queues the absorb of the new
 * batch, then STARTs the new solve (defer != 0: returns WISKI_PENDING) or runs it to convergence (defer == 0: h_iters /
 * h_relres / h_err then describe THIS solve and h_resumed = 2 says a pending one was finished on the way).  q = 0 with
 * defer = 0 just finishes a pending solve.  So the host-language work between two steps overlaps the GPU's CG iterations.
 * (With a mean requested the absorb is in fact queued BEFORE the RESUME, guarded on the device by the verdict of the pending
 * poll -- wiski_pcg_async_guard -- and queued again unguarded only if that verdict was "not converged" or "error flag set";
 * the results are those of the order described above.)
 * first_check = -1 with a handle: the step places the first poll of its solve itself, at max(1, handle->first_ok) -- in a call
 * that RESUMEs a pending solve that is the hindsight this very RESUME produced, never one step old -- and as first_check = 0
 * while the handle has no history.  -1 without a handle and every other negative value: WISKI_E_BADARG, nothing queued. */
typedef struct wiski_stream_args_f32 {
  float* d_A_half; float* d_b; float* d_cnt; double* d_stats; int32_t* d_err;     /* statistics + out-of-grid flag      */
  float* d_U; float* d_Z; float* d_R;                                              /* posterior-mean state (in place)    */
  const float* d_tcol; float kscale; const float* d_evec; const float* d_evec2; const float* d_eval; float shift;
  double tol; int32_t max_iter; int32_t check_every; void* d_work; int64_t work_bytes;
  void* d_bin; int64_t bin_bytes;                 /* optional binning workspace of the absorb (wiski_scatter_bin_bytes), or NULL / 0 */
  const wiski_shard* shard;                      /* NULL, or: this replica owns a share of the half stencil (see wiski_shard) */
  const wiski_twolevel* two_level;               /* NULL, or: exact block on the dominant modes in the preconditioner (see wiski_twolevel) */
  int32_t keep[3];                               /* eigenmodes per dimension the preconditioner transforms (the last keep[q] columns of the
                                                  * eigen tables; on all others t = r and y = 0), or all 0: every mode.  See wiski_precond_keep_ok */
  float* d_tap_stage;                            /* NULL, or [m][4] floats, all zero: the absorb's tap adds on b / cnt / R go through it as one
                                                  * 16-byte record per node and the step's solve folds it in (wiski_absorb_staged_f32); all zero
                                                  * again when the call returns (in stream order).  d = 3, carry != 0, d_cnt, no shard; ignored otherwise */
} wiski_stream_args_f32;
typedef struct wiski_stream_args_f64 {
  double* d_A_half; double* d_b; double* d_cnt; double* d_stats; int32_t* d_err;
  double* d_U; double* d_Z; double* d_R;
  const double* d_tcol; double kscale; const double* d_evec; const double* d_evec2; const double* d_eval; double shift;
  double tol; int32_t max_iter; int32_t check_every; void* d_work; int64_t work_bytes;
  void* d_bin; int64_t bin_bytes;
  const wiski_shard* shard;
  const wiski_twolevel* two_level;               /* must be NULL (the two-level block exists for the fused fp32 path only) */
  int32_t keep[3];                               /* must be 0 (the truncated transforms exist for the fused fp32 path only) */
  double* d_tap_stage;                           /* must be NULL (the staged tap adds exist in fp32 only) */
} wiski_stream_args_f64;
int wiski_stream_step_f32(const wiski_grid* grid, const wiski_stream_args_f32* args, const float* d_x, const float* d_y, const float* d_wa, const float* d_wb, const float* d_noise, int64_t q, float* d_mean_out, int32_t carry, int32_t first_check, int32_t* h_iters, double* h_relres, int32_t* h_err, void* stream, wiski_pcg_async* handle, int32_t defer, int32_t* h_resumed);
int wiski_stream_step_f64(const wiski_grid* grid, const wiski_stream_args_f64* args, const double* d_x, const double* d_y, const double* d_wa, const double* d_wb, const double* d_noise, int64_t q, double* d_mean_out, int32_t carry, int32_t first_check, int32_t* h_iters, double* h_relres, int32_t* h_err, void* stream, wiski_pcg_async* handle, int32_t defer, int32_t* h_resumed);

/* Several independent outputs in ONE absorb launch (BFN:37-55 carries num_outputs as a batch dimension; the Dirichlet classifier has 2):
 * as wiski_scatter_stats_cnt on the half stencil, with output o reading d_y + o * y_stride, weights at + o * w_stride (0: one weight
 * vector shared by all outputs) and accumulating into d_b / d_cnt / d_res (+ d_u) at + o * m, d_A_half + o * A_stride, d_stats + 2 o.
 * A point outside the grid is dropped for every output and counted once. */
int wiski_scatter_stats_multi_f32(const wiski_grid* grid, const float* d_x, const float* d_y, const float* d_wa, const float* d_wb, const float* d_noise, int64_t n, int32_t nout, int64_t y_stride, int64_t w_stride, float* d_b, float* d_A_half, int64_t A_stride, float* d_cnt, const float* d_u, float* d_res, double* d_stats, int32_t* d_err, void* stream);
int wiski_scatter_stats_multi_f64(const wiski_grid* grid, const double* d_x, const double* d_y, const double* d_wa, const double* d_wb, const double* d_noise, int64_t n, int32_t nout, int64_t y_stride, int64_t w_stride, double* d_b, double* d_A_half, int64_t A_stride, double* d_cnt, const double* d_u, double* d_res, double* d_stats, int32_t* d_err, void* stream);

/* Derivative observations: values and gradients of f in ONE absorb launch.  Every point carries C = d + 1 scalar
 * observations, d_y / d_wa / d_wb / d_noise / d_mean_out being [n][C]: channel 0 is f(x_p), channel 1 + q is df/dx_q (x_p).  Under
 * the SKI model the latter is one more linear observation whose row of W is the value row with dim q's four weights replaced by
 * k'(.) / h_q (zero where dim q's cell is a one-hot boundary cell: the rows wiski_gather_grad differentiates with).  Per point
 *   b[a] += sum_c v_c[a] wb_c y_c,   A[a, b] += sum_c wa_c v_c[a] v_c[b],   stats += (sum_c wb_c y_c^2, sum_c log noise_c),
 * the sum over c formed on chip, so that a point with a full gradient issues the T (T + 1) / 2 tap-pair atomics of a point with a
 * value alone.  An absent channel is wa = wb = 0, noise = 1.  A present derivative channel in a boundary cell has a zero row: it
 * adds its wb y^2 and log noise only (the model calls it pure noise).  A point outside the grid is dropped for every channel and
 * counted once in d_err.  d_cnt (optional; feeds the preconditioner's density model only) += wa_0 v_0[a] + sum_{c >= 1} wa_c v_c[a]^2.
 * The carry (optional, d_u with d_res and / or d_mean_out): d_mean_out[p][c] = v_c . u, the predictive mean and gradient of the
 * point before the update, and d_res[a] += sum_c v_c[a] (wb_c y_c - wa_c (v_c . u)).  Symmetric half stencil, atomic form, d = 1..4.
 * Entry: wiski_absorb_f32 / _f64 below with channels = d + 1.  The form has no argument beyond the record, so it has no entry of its
 * own: a wiski_absorb_grad would be wiski_absorb under a second name. */

/* The absorb with every option it has, as one record: what each wiski_scatter_stats_* entry above fills a part of.  Pointers are
 * device pointers to float (wiski_absorb_f32) or double (wiski_absorb_f64) unless typed; a zeroed record with the points, d_b,
 * d_stats, d_err and nout = 1 set is the plain absorb.  half: d_A is the symmetric half stencil (else offset-major); channels: 0,
 * or d + 1 (derivative observations, above); g_hi = 0: every stencil group, else the groups [g_lo, g_hi) (wiski_scatter_stats_step_sharded);
 * nout / *_stride as wiski_scatter_stats_multi.  Combinations no form of the absorb implements return WISKI_E_BADARG before
 * anything is launched -- channels, for one, with a full stencil, a guard, zero regions, a shard or nout > 1.
 *
 * The observation forms below (wiski_absorb_robust, _window, _interval, _grad_interval, _count, _revisit, _hetero, _label,
 * _input_noise) each take this record plus the form's own few arguments; the record is the one way in, from C and from the Python
 * package alike.  The record is passed by pointer without a size field and has NOT grown a group per form: callers built against
 * today's header hand over records of today's size.  No entry fills in a field of the record for the caller.  Every form needs
 *   half = 1 and nout = 1 (label: nout = C), everything not named here zero;
 *   the points d_x / d_wa / d_wb / d_noise, n, and d_y where the form has targets of its own kind (robust, window, hetero,
 *     input_noise, derivative observations); the interval, grad_interval, count and label forms ignore d_y (it may be NULL);
 *   d_b, d_A (the half stencil), d_cnt, d_stats, d_err and d_u; d_res and d_mean_out are optional;
 *   grad_interval (as the derivative observations): channels = d + 1;
 *   label: w_stride = 0 (weights shared by the outputs) or n, A_stride = H * m (H the rows of a half stencil);
 *   revisit: d_x / d_y / d_wa / d_wb / d_noise / n are ignored (the ring's slots are the points), d_mean_out must be NULL.
 * A record that asks for more -- a guard, zero regions, a shard, an owner workspace, nout > 1 (but for label), channels (but for
 * grad_interval), a full stencil -- is WISKI_E_BADARG before a launch, as is a NULL record. */
typedef struct wiski_absorb_args {
  const void* d_x; const void* d_y; const void* d_wa; const void* d_wb; const void* d_noise; int64_t n;
  void* d_b; void* d_A; int32_t half; int32_t channels; void* d_cnt; double* d_stats; int32_t* d_err;
  const void* d_u; void* d_res; void* d_mean_out;
  void* z1; int64_t n1_bytes; void* z2; int64_t n2_bytes;
  const void* d_guard; int64_t guard_expect;
  void* d_bin; int64_t bin_bytes;
  int32_t g_lo; int32_t g_hi; int32_t nout; int32_t reserved;
  int64_t y_stride; int64_t w_stride; int64_t A_stride;
} wiski_absorb_args;
int wiski_absorb_f32(const wiski_grid* grid, const wiski_absorb_args* args, void* stream);
int wiski_absorb_f64(const wiski_grid* grid, const wiski_absorb_args* args, void* stream);

/* Staged tap adds.  The per-tap adds of a point on d_b, d_cnt and d_res are three runs of 16 bytes per tap row of 4:
 * 16 % of the atomic form's 64-byte memory-side requests for 8 % of its adds.  With d_tap_stage -- [m][4] floats, node-major records
 * {delta b, delta cnt, delta res, unused}, ALL ZERO on entry -- wiski_absorb_staged_f32 adds the three into the node's record instead
 * (one run of 64 bytes per tap row) and leaves d_b / d_cnt / d_res untouched; wiski_tap_fold_f32 then adds every record to the three
 * arrays with plain stores and zeroes it (d_cnt, d_res: each may be NULL).  Until the fold the three arrays lack the batch.
 * The record is that of wiski_absorb_f32; the plain single-output fp32 half-stencil atomic form at d = 3 with d_cnt, d_u and d_res, no
 * shard and channels = 0 only -- anything else, or d_tap_stage = NULL, is WISKI_E_BADARG before a launch.  A closed guard stages
 * nothing; a batch the owner-computes form takes (d_bin) is added directly, the stage stays zero.  wiski_stream_step_f32 does both
 * steps by itself (wiski_stream_args_f32.d_tap_stage), the fold inside the first kernel of its solve where that is the truncated
 * forward transform of a carried residual. */
int wiski_absorb_staged_f32(const wiski_grid* grid, const wiski_absorb_args* args, float* d_tap_stage, void* stream);
int wiski_tap_fold_f32(float* d_tap_stage, float* d_b, float* d_cnt, float* d_res, int64_t m, void* stream);

/* Outlier-robust absorb: every point is Huber-weighted against the posterior BEFORE the batch, inside the launch that absorbs it
 * (DESIGN.md 3.16).  The record (a value per point: d_y / d_wa / d_wb / d_noise / d_mean_out are [n]; half = 1, nout = 1) plus
 * d_inv_scale [n], huber_c and d_omega_out [n].  With u the posterior mean on the grid,
 *   z_p = (y_p - w_p . u) inv_scale_p,   omega_p = min(1, huber_c / |z_p|)      (exactly 1 for |z_p| <= huber_c),
 * and the point enters A, cnt and the carried residual with omega_p wa_p, b and sum wb y^2 with omega_p wb_p, log|D| with
 * log(noise_p / omega_p): the absorb of the same point at noise noise_p / omega_p, so everything downstream stays an exact GP.
 * d_omega_out receives omega_p (0 for a point outside the grid, which is flagged, counted and dropped as everywhere);
 * inv_scale_p = 0 exempts a point.  Required: d_u, d_A, d_cnt, d_omega_out, d_inv_scale, a finite huber_c > 0; d_res and
 * d_mean_out are optional.  Symmetric half stencil, atomic form, one output, d = 1..4; anything else is WISKI_E_BADARG before
 * a launch -- a NULL d_inv_scale and every record field the form has no use for (see wiski_absorb_args) included. */
int wiski_absorb_robust_f32(const wiski_grid* grid, const wiski_absorb_args* args, const float* d_inv_scale, float huber_c, float* d_omega_out, void* stream);
int wiski_absorb_robust_f64(const wiski_grid* grid, const wiski_absorb_args* args, const double* d_inv_scale, double huber_c, double* d_omega_out, void* stream);

/* Sliding-window absorb: the statistics of exactly the points in a device-resident ring.  The statistics are
 * sums, so a point leaves them by being absorbed once more with its weights negated.  The ring is five device arrays of `cap`
 * slots in the working precision -- d_x [cap, d], d_y, d_wa, d_wb, d_noise [cap] -- and `head`, kept by the host, is the slot of
 * the launch's first entering point.  An EMPTY slot holds wa = wb = 0, noise = 1 and a finite x: the caller creates the ring that
 * way.  In ONE launch, for entering point j of n, the wave of slot s = (head + j) mod cap
 *   1. reads the old occupant of s,
 *   2. writes the entering point into s -- a point outside the grid is flagged and counted in d_err as everywhere, contributes
 *      nothing, and is stored VOID: wa = wb = 0, noise = 1, y = 0, x = NaN (a point no grid contains, a grown one included),
 *   3. absorbs the entering point with (+wa, +wb); d_mean_out[j] is its predictive mean before the update,
 *   4. absorbs the old occupant, if it holds weight, with (-wa, -wb); a void or empty slot gives nothing back.
 * stats += (sum wb y^2, sum log noise) of the points that entered minus those of the points that left.  *d_void_left += the
 * number of overwritten slots that were void, so that a caller can keep its point count without reading the ring.  n <= cap is
 * required (the slots of one launch are then distinct: a slot has one reader and one writer, the same wave), as are d_u, d_A,
 * d_cnt and d_void_left; d_res and d_mean_out are optional.  Both sweeps use the same u, so the result does not depend on the
 * order of points or atomics.  The caller advances head by n (mod cap) afterwards.  Symmetric half stencil, atomic form, one
 * output, d = 1..4; anything else -- n > cap, head outside [0, cap), a missing ring array -- is WISKI_E_BADARG before a launch.
 * wiski_absorb_window takes the record (the entering points, as for the robust form) plus the ring and d_void_left. */
typedef struct wiski_window_ring {
  void* d_x; void* d_y; void* d_wa; void* d_wb; void* d_noise;
  int64_t cap; int64_t head;
} wiski_window_ring;
int wiski_absorb_window_f32(const wiski_grid* grid, const wiski_absorb_args* args, const wiski_window_ring* ring, int32_t* d_void_left, void* stream);
int wiski_absorb_window_f64(const wiski_grid* grid, const wiski_absorb_args* args, const wiski_window_ring* ring, int32_t* d_void_left, void* stream);

/* Interval and censored observations: y_p = f(x_p) + eps_p is only known to lie in [d_lo_p, d_hi_p].  Either end
 * may be infinite (a one-sided bound: censored data, a probit label); lo == hi is an exact value.  Every point is moment-matched
 * against the posterior BEFORE the batch, inside the launch that absorbs it (assumed-density filtering, all sites of a launch in
 * parallel).  With mu = w_p . u, v = max(d_pvar_p, 0) the posterior variance of f at x_p, dn = sigma2 noise_p, s^2 = v + dn,
 *   a = (lo - mu) / s,  b = (hi - mu) / s,  Z = Phi(b) - Phi(a),
 *   alpha = (phi(a) - phi(b)) / (s Z),   beta = alpha^2 + (b phi(b) - a phi(a)) / (s^2 Z),
 *   omega = min(1, dn beta / (1 - v beta)),   ytilde = mu + alpha / beta,
 * evaluated in double in both precisions, and the point enters as the target ytilde at noise noise_p / omega_p: A, cnt and the
 * carried residual with omega wa, b and sum wb y^2 with omega wb and ytilde, log|D| with log(noise / omega) -- so everything
 * downstream is the exact GP of the pseudo-observations.  lo == hi gives ytilde = lo and omega = 1 exactly.  A point is SKIPPED --
 * it enters nothing and is not flagged in d_err -- when omega < 1e-12 (WISKI_INTERVAL_OMEGA_MIN: (-inf, inf), a bound satisfied
 * by many standard deviations), when beta is not positive and finite, when lo > hi or when a bound is NaN.
 * Outputs, [n] each: d_ytilde_out (mu for a skipped point), d_omega_out (0 for a skipped point), d_logz_out (double in both
 * precisions): log Z, the log predictive probability of the interval -- the Gaussian log density for lo == hi, -inf for lo > hi,
 * NaN for a NaN bound.  A point outside the grid is flagged, counted and dropped as everywhere and reports (0, 0, 0).
 * wiski_absorb_interval takes the record as wiski_absorb_robust does (its d_y is ignored) plus the interval arguments.  Required:
 * d_lo, d_hi, d_pvar, d_u, d_A, d_cnt, the three outputs and a finite sigma2 > 0; d_res and d_mean_out are optional.  Symmetric
 * half stencil, atomic form, one output, d = 1..4; anything else is WISKI_E_BADARG before a launch. */
int wiski_absorb_interval_f32(const wiski_grid* grid, const wiski_absorb_args* args, const float* d_lo, const float* d_hi, const float* d_pvar, double sigma2, float* d_ytilde_out, float* d_omega_out, double* d_logz_out, void* stream);
int wiski_absorb_interval_f64(const wiski_grid* grid, const wiski_absorb_args* args, const double* d_lo, const double* d_hi, const double* d_pvar, double sigma2, double* d_ytilde_out, double* d_omega_out, double* d_logz_out, void* stream);

/* Interval observations of the value AND the partial derivatives of a point: the C = d + 1 channels of
 * the derivative observations (0: f(x_p), 1 + q: df/dx_q (x_p)), each present one (d_wa[p][c] != 0) an interval
 *   d_lo[p][c] <= (row_c . u) + eps <= d_hi[p][c]   at noise sigma2 d_noise[p][c]
 * -- "f increases in x_q" is d_lo = 0 on channel 1 + q, a slope bound is [-L, L].  Every channel is moment-matched as in
 * wiski_absorb_interval, against its own predictive mean row_c . u and its posterior variance d_pvar[p][c] before the
 * batch (the channels of a point independently of each other), and all of them enter in the one launch of the derivative
 * form: one atomic per tap pair.  The skip rules are those of the interval form, per channel; lo == hi is an exact value and
 * enters with omega = 1 exactly.  All per-point arrays, the three outputs and d_mean_out are [n][d + 1].  A skipped channel
 * reports (row_c . u, 0, log Z), an absent one and every channel of a point outside the grid (0, 0, 0); such a point is flagged
 * and counted once.  A derivative channel in a boundary cell of its dim has a zero row: its site is evaluated at mean 0 and
 * enters the two scalars only.  Required: d_hi, d_pvar, d_u, d_A, d_cnt, the three outputs and a finite sigma2 > 0; d_res
 * and d_mean_out are optional.  Symmetric half stencil, atomic form, one output, d = 1..4; anything else is WISKI_E_BADARG
 * before a launch.  wiski_absorb_grad_interval takes the record (its d_y is ignored, its channels must be d + 1) plus the
 * form's arguments. */
int wiski_absorb_grad_interval_f32(const wiski_grid* grid, const wiski_absorb_args* args, const float* d_lo, const float* d_hi, const float* d_pvar, double sigma2, float* d_ytilde_out, float* d_omega_out, double* d_logz_out, void* stream);
int wiski_absorb_grad_interval_f64(const wiski_grid* grid, const wiski_absorb_args* args, const double* d_lo, const double* d_hi, const double* d_pvar, double sigma2, double* d_ytilde_out, double* d_omega_out, double* d_logz_out, void* stream);

/* Count observations: point p carries a count d_y_p and a second number d_t_p.  `family`:
 *   WISKI_COUNT_POISSON   y ~ Poisson(t exp f(x)), t > 0 the exposure, y >= 0 (non-integers allowed: the constant is lgamma);
 *   WISKI_COUNT_BINOMIAL  y successes of t trials at success probability 1 / (1 + exp(-f(x))), 0 <= y <= t.
 * Every point is moment-matched against the posterior BEFORE the batch, inside the launch that absorbs it, as an interval
 * observation is.  With mu = w_p . u, v = max(d_pvar_p, 0) and l the likelihood,
 *   Z = int l(f) N(f; mu, v) df,   alpha = d log Z / d mu,   beta = -d^2 log Z / d mu^2,
 *   tau = beta / (1 - v beta),   ytilde = mu + alpha / beta,   omega = sigma2 noise_p tau,
 * evaluated in double in both precisions by a quadrature whose nodes are the 64 lanes of the point's wave (sectioning to the mode,
 * a bracket where the log integrand has fallen by 40, 64 Gauss-Legendre nodes on either side of the mode), and the point enters as
 * the target ytilde at noise noise_p / omega_p -- the effective noise variance 1 / tau.  omega is NOT capped at 1: a count has no
 * Gaussian noise of its own, callers pass noise = wa = wb = 1.  v = 0 gives the Laplace site at mu.  A point is SKIPPED -- it enters
 * nothing and is not flagged in d_err -- when omega < 1e-12 (WISKI_COUNT_OMEGA_MIN), when beta is not positive and finite, or when
 * the datum is invalid (y < 0, t <= 0, y > t for the binomial, a NaN: log Z = NaN).  Outputs and every other argument as
 * wiski_absorb_interval; d_logz_out is the log predictive probability of the count.  wiski_absorb_count takes the record
 * (its d_y is ignored: the counts are the argument d_y of the entry) plus the count arguments.
 * wiski_count_sites evaluates the sites alone, one wave per site and no scatter, from given means d_mu and variances d_pvar [n]:
 * d_omega_out receives tau (sigma2 noise = 1). */
#define WISKI_COUNT_POISSON 0
#define WISKI_COUNT_BINOMIAL 1
int wiski_absorb_count_f32(const wiski_grid* grid, const wiski_absorb_args* args, const float* d_y, const float* d_t, int family, const float* d_pvar, double sigma2, float* d_ytilde_out, float* d_omega_out, double* d_logz_out, void* stream);
int wiski_absorb_count_f64(const wiski_grid* grid, const wiski_absorb_args* args, const double* d_y, const double* d_t, int family, const double* d_pvar, double sigma2, double* d_ytilde_out, double* d_omega_out, double* d_logz_out, void* stream);
int wiski_count_sites_f32(const float* d_mu, const float* d_pvar, const float* d_y, const float* d_t, int family, int64_t n, float* d_ytilde_out, float* d_omega_out, double* d_logz_out, void* stream);
int wiski_count_sites_f64(const double* d_mu, const double* d_pvar, const double* d_y, const double* d_t, int family, int64_t n, double* d_ytilde_out, double* d_omega_out, double* d_logz_out, void* stream);

/* Revisiting stored sites: expectation-propagation sweeps over a ring of interval and count observations.  The
 * two forms above match a point once and never look at it again.  A ring of `cap` slots, nine device arrays the caller owns and
 * fills, remembers such points: d_x [cap, d], the two data numbers d_d0 / d_d1 [cap] ((lo, hi) of an interval, (count, exposure)
 * or (count, trials) of a count), d_noise / d_wa / d_wb [cap], the site d_ytilde / d_omega [cap] the point is in the statistics
 * with (omega = 0: it was skipped and nothing of it is there) -- all in the working precision -- and int32 d_form [cap], one of
 * the codes below.  ONE launch revisits the slots whose code is `form`; a sweep over a ring that holds several forms is one launch
 * per form, every one with the same d_u and d_pvar.  With dn = sigma2 noise, tau = omega / dn, nu = tau ytilde, mu = w . u and
 * v = d_pvar[s] the posterior variance of f at the slot's point under the CURRENT statistics,
 *   cavity:  p = 1 / v - tau,   v_ = 1 / p,   mu_ = v_ (mu / v - nu),
 *   fresh:   (ytilde', omega', log Z') = the site of wiski_absorb_interval / _count at (mu_, v_, dn),
 *   damped:  tau_new = (1 - damping) tau + damping omega' / dn,   nu_new = (1 - damping) nu + damping (omega' / dn) ytilde',
 *            omega_new = dn tau_new,   ytilde_new = nu_new / tau_new,
 * evaluated in double in both precisions, and the slot enters the statistics with the difference of its site: A, cnt with
 * wa (omega_new - omega_old), b with wb (omega_new ytilde_new - omega_old ytilde_old), the carried residual with that minus
 * wa (omega_new - omega_old) mu, stats[0] with wb (omega_new ytilde_new^2 - omega_old ytilde_old^2), stats[1] with
 * log(noise / omega_new) [omega_new > 0] - log(noise / omega_old) [omega_old > 0] -- the differences of the values as the ring holds
 * them, rounded to the working precision.  The new (ytilde, omega) are written back to the ring.  An omega_new below 1e-12 (the
 * forms' OMEGA_MIN) becomes exactly 0: the point leaves, ytilde_new = mu.  A slot with omega_old = 0 whose fresh site is positive
 * enters.  A slot is LEFT EXACTLY AS IT IS -- no atomic, no store to the ring, change 0 -- when it is empty or of another form
 * (neither output is written for it: the launches of a sweep may share them), when its point lies outside the grid (d_err is not
 * raised: a stored point), when it holds an exact value (lo == hi), when v is not positive and finite, when p <= 1e-4 / v (the
 * cavity is a difference of two precisions; below that relative size it is the rounding of d_pvar), or when damping = 0, which
 * changes nothing bit for bit.  All slots are taken against the same d_u and d_pvar: the result depends neither on the order of the
 * slots nor on the order of the atomics.
 * Outputs, per slot of the form: d_change_out [cap] = |omega_new - omega_old| / max(omega_new, omega_old) (0 for a slot left alone),
 * d_logz_out [cap] (double) = log Z' against the cavity (NaN for a slot left alone).  Required: every ring array, d_pvar, d_u,
 * d_A, d_cnt, d_b, d_stats, d_err, both outputs, a finite sigma2 > 0, 0 <= damping <= 1 and a known form; d_res is optional.
 * cap = 0 or a ring without a slot of the form does nothing and returns WISKI_OK.  Symmetric half stencil, atomic form, one output,
 * d = 1..4; anything else is WISKI_E_BADARG before a launch.  wiski_absorb_revisit takes the record (its points d_x / d_y / d_wa /
 * d_wb / d_noise / n are not looked at: the points are the ring's slots; its d_mean_out must be NULL) plus the revisit arguments. */
#define WISKI_SITE_EMPTY 0
#define WISKI_SITE_INTERVAL 1
#define WISKI_SITE_POISSON 2
#define WISKI_SITE_BINOMIAL 3
typedef struct wiski_site_ring {
  void* d_x; void* d_d0; void* d_d1; void* d_noise; void* d_wa; void* d_wb; void* d_ytilde; void* d_omega;
  int32_t* d_form;
  int64_t cap;
} wiski_site_ring;
int wiski_absorb_revisit_f32(const wiski_grid* grid, const wiski_absorb_args* args, const wiski_site_ring* ring, int form, const float* d_pvar, double sigma2, double damping, double* d_logz_out, float* d_change_out, void* stream);
int wiski_absorb_revisit_f64(const wiski_grid* grid, const wiski_absorb_args* args, const wiski_site_ring* ring, int form, const double* d_pvar, double sigma2, double damping, double* d_logz_out, double* d_change_out, void* stream);

/* Heteroscedastic absorb: the noise of a point is not known but learned, as a second field on the same grid:
 *   y_p = f(x_p) + eps_p,   eps_p ~ N(0, sigma2 noise_p exp g(x_p)),   g ~ GP(g0, k_g).
 * f and g are two single-output models with a set of statistics each: (d_b, d_A, d_cnt, d_stats, d_u, d_res) for f and
 * (d_b2, d_A2_half, d_cnt2, d_stats2, d_u2, d_res2) for g - g0.  Both are taken against their posteriors BEFORE the batch, inside the
 * one launch that absorbs it into both: with mu_f = w_p . u, v_f = max(d_pvar_p, 0), mu_g = g0 + w_p . u2, v_g = max(d_pvar2_p, 0),
 *   e     = exp(mu_g + v_g / 2)                      (the mean of the log-normal multiplier),   dn = sigma2 noise_p e,
 *   f     takes the point as its own target y_p at noise noise_p / omega_f, omega_f = 1 / e -- NOT capped at 1 --
 *         and d_logzy_out = log N(y; mu_f, v_f + dn);
 *   rho   = (y_p - mu_f)^2 / (sigma2 noise_p) * dn / (dn + v_f)
 *         (the last factor takes out the share of the residual that is f's own uncertainty and keeps the likelihood log-concave);
 *   g     takes the site of l(g) = (2 pi)^(-nu / 2) exp(-nu g / 2 - rho e^-g / 2), nu = 1, moment-matched against N(mu_g, v_g) by
 *         the quadrature of the count form as its family WISKI_COUNT_LOGVAR (y = rho, t = nu; valid for rho >= 0, nu > 0, both finite):
 *         the target ytilde_g - g0 at noise 1 / tau_g.  The noise model's own sigma2 = noise = wa = wb = 1, as for counts.
 * The site is evaluated in double in both precisions.  d_e_out [n] receives e, d_ytilde_out / d_omega_out / d_logz_out [n] the noise
 * site (ytilde_g including g0, tau_g, its log Z), d_mean_out (optional) mu_f.  rho = 0 has tau = 0: the noise site is SKIPPED by the
 * omega < 1e-12 rule (WISKI_COUNT_OMEGA_MIN), it reports ytilde = mu_g, omega = 0, and the point still enters f.  A y that is not
 * finite, a noise that is not positive and finite, or a multiplier e for which e or 1 / e is not positive and finite IN THE WORKING
 * PRECISION (|mu_g + v_g / 2| > 87 in fp32: the weight would be 0 or inf) skips the point for both models (both log Z = NaN, no flag
 * in d_err; d_e_out still reports e as rounded).  A point outside the grid is dropped for both, flagged and counted ONCE in d_err, and reports zeros.  d_stats2[0], the sum
 * of tau ytilde^2, is dominated by weak sites and is no evidence term: the evidence is the sum of the log Z.
 * d_u, d_A, d_cnt and the whole second set but d_res2 are required; d_res, d_res2 and d_mean_out are optional.  d = 1..4,
 * symmetric half stencil, atomic form, a single output.  wiski_absorb_hetero takes the record (the set of f and the points) plus
 * the hetero arguments (the set of g, the variances, the outputs).  Everything refused returns WISKI_E_BADARG before a launch; n = 0
 * does nothing.
 * wiski_hetero_sites evaluates the noise sites alone, one wave per site and no scatter, from given d_mu = mu_g, d_pvar = v_g, d_rho
 * and d_nu [n] (nu is general: replicated readings give a sample variance with nu degrees of freedom): d_omega_out receives tau.
 * It is wiski_count_sites of the family WISKI_COUNT_LOGVAR (the same kernel with the family fixed at compile time), which the count
 * absorb and wiski_count_sites themselves do not take.  n = 0 returns WISKI_OK from all three, whatever the other arguments hold. */
#define WISKI_COUNT_LOGVAR 2
int wiski_absorb_hetero_f32(const wiski_grid* grid, const wiski_absorb_args* args, const float* d_pvar, const float* d_pvar2, double sigma2, double g0, float* d_b2, float* d_A2_half, float* d_cnt2, const float* d_u2, float* d_res2, double* d_stats2, float* d_e_out, float* d_ytilde_out, float* d_omega_out, double* d_logz_out, double* d_logzy_out, void* stream);
int wiski_absorb_hetero_f64(const wiski_grid* grid, const wiski_absorb_args* args, const double* d_pvar, const double* d_pvar2, double sigma2, double g0, double* d_b2, double* d_A2_half, double* d_cnt2, const double* d_u2, double* d_res2, double* d_stats2, double* d_e_out, double* d_ytilde_out, double* d_omega_out, double* d_logz_out, double* d_logzy_out, void* stream);
int wiski_hetero_sites_f32(const float* d_mu, const float* d_pvar, const float* d_rho, const float* d_nu, int64_t n, float* d_ytilde_out, float* d_omega_out, double* d_logz_out, void* stream);
int wiski_hetero_sites_f64(const double* d_mu, const double* d_pvar, const double* d_rho, const double* d_nu, int64_t n, double* d_ytilde_out, double* d_omega_out, double* d_logz_out, void* stream);

/* Categorical observations: point p carries a label d_labels_p in {0 .. C - 1}, C = nout outputs.  The likelihood is
 * the multinomial probit, y = argmax_c (f_c(x) + eps_c), eps_c ~ N(0, s_c), s_c = sigma2[c] noise_c,p.  Every point is moment-matched
 * against the posterior BEFORE the batch, inside the launch that absorbs it: with mu_c = w_p . u_c (u is [C][m]), v_c = max(d_pvar[c][p], 0),
 * a_c = v_c + s_c, z_c(t) = (t - mu_c) / sqrt a_c, r = phi / Phi and E[.] the expectation under the normalised integrand of
 *   Z = P(y) = int N(t; mu_y, a_y) prod_{c != y} Phi(z_c(t)) dt,
 *   c = y:   alpha = (E t - mu_y) / a_y,          beta = 1 / a_y - Var t / a_y^2,
 *   c != y:  alpha = -E r(z_c) / sqrt a_c,        beta = (E[r (r + z_c)] - Var r) / a_c,
 *   tau_c = beta_c / (1 - v_c beta_c),   ytilde_c = mu_c + alpha_c / beta_c,   omega_c = s_c tau_c,
 * evaluated in double in both precisions by the quadrature of the count form (its nodes are the 64 lanes of the point's wave), and
 * output c takes the point as the target ytilde_c at noise noise_c,p / omega_c.  This is the one form that couples outputs: a kernel
 * of its own, one wave per point, which builds the point's stencil once, reduces the C means, and runs the atomics of every output
 * whose site enters into d_b / d_cnt / d_res at + c m, d_A + c A_stride, d_stats + 2 c; d_wa / d_wb / d_noise of output c are at
 * + c w_stride (0: shared by all outputs).  A site is SKIPPED for its output only when beta_c is not positive and finite or
 * omega_c < 1e-12 (WISKI_COUNT_OMEGA_MIN: a class far below the label's says nothing).  A label that is not an integer in [0, C),
 * or NaN, skips the point for every output (log Z = NaN, no flag in d_err).  A point outside the grid is dropped for every output,
 * counted once, and reports zeros.  d_ytilde_out / d_omega_out / d_pvar and the optional d_mean_out are [C][n] (a skipped site
 * reports ytilde = mu_c, omega = 0), d_logz_out [n] is log P(y_p); sigma2 [C] is a HOST array, every entry positive and finite.
 * d_u, d_A and d_cnt are required, d_res and d_mean_out optional.  2 <= nout <= WISKI_LABEL_MAX_CLASSES, d = 1..4, symmetric
 * half stencil, atomic form.  wiski_absorb_label takes the record (its d_y is ignored; nout = C, w_stride and A_stride are the
 * record's) plus the label arguments.  Everything refused returns WISKI_E_BADARG before a launch.
 * wiski_label_sites evaluates the sites alone, one wave per point and no scatter, from given means d_mu, latent variances d_pvar and
 * noise variances d_s, all [C][n]: d_omega_out receives tau.  wiski_label_proba writes P(y = k) for every k into d_proba_out [n][C]
 * (double): the same integral without its derivatives, once per class; the row is NOT normalised (its sum is 1 to quadrature error). */
#define WISKI_LABEL_MAX_CLASSES 16
int wiski_absorb_label_f32(const wiski_grid* grid, const wiski_absorb_args* args, const float* d_labels, const float* d_pvar, const double* sigma2, float* d_ytilde_out, float* d_omega_out, double* d_logz_out, void* stream);
int wiski_absorb_label_f64(const wiski_grid* grid, const wiski_absorb_args* args, const double* d_labels, const double* d_pvar, const double* sigma2, double* d_ytilde_out, double* d_omega_out, double* d_logz_out, void* stream);
int wiski_label_sites_f32(const float* d_mu, const float* d_pvar, const float* d_s, const float* d_labels, int32_t nout, int64_t n, float* d_ytilde_out, float* d_omega_out, double* d_logz_out, void* stream);
int wiski_label_sites_f64(const double* d_mu, const double* d_pvar, const double* d_s, const double* d_labels, int32_t nout, int64_t n, double* d_ytilde_out, double* d_omega_out, double* d_logz_out, void* stream);
int wiski_label_proba_f32(const float* d_mu, const float* d_pvar, const float* d_s, int32_t nout, int64_t n, double* d_proba_out, void* stream);
int wiski_label_proba_f64(const double* d_mu, const double* d_pvar, const double* d_s, int32_t nout, int64_t n, double* d_proba_out, void* stream);

/* Noisy-input observations: point p was taken at x_p + e_p, e_p ~ N(0, diag(d_xvar_p)), d_xvar [n, d] in the grid's units squared
 * (DESIGN.md 3.24).  To first order the location error is extra output noise grad f^T diag(xvar) grad f, with the slope taken under
 * the posterior BEFORE the batch, inside the launch that absorbs it.  With mu = w_p . u, g_k = (d w_p / d x_k) . u (zero in a
 * one-hot boundary cell of dim k, as in wiski_gather_grad), v = max(d_pvar_p, 0), gamma_k = max(d_gvar_p,k, 0) the posterior variance
 * of d f / d x_k (d_gvar [n, d]; NULL: 0, the rule of the posterior mean's slope alone) and dn = sigma2 noise_p,
 *   s_in = sum_k xvar_k (g_k^2 + gamma_k),   omega = dn / (dn + s_in),   log Z = log N(y; mu, v + dn + s_in),
 * evaluated in double in both precisions, and the point enters as its own target d_y_p at noise noise_p / omega_p.  xvar = 0 gives
 * omega = 1 exactly: the plain absorb.  A point is SKIPPED -- it enters nothing, reports omega = 0 and is not flagged in d_err --
 * when an xvar_k is negative or NaN or s_in is not finite (log Z = NaN), or when omega < 1e-12 (WISKI_INPUT_NOISE_OMEGA_MIN).
 * d_omega_out [n], d_logz_out [n] (double) and, optionally, d_grad_out [n, d] (the slopes g as reduced by the kernel) are written
 * for every point; a point outside the grid reports zeros.  Every other argument as wiski_absorb_interval.
 * wiski_absorb_input_noise takes the record (with d_y: the targets are the points' own) plus the group. */
int wiski_absorb_input_noise_f32(const wiski_grid* grid, const wiski_absorb_args* args, const float* d_xvar, const float* d_gvar, const float* d_pvar, double sigma2, float* d_omega_out, double* d_logz_out, float* d_grad_out, void* stream);
int wiski_absorb_input_noise_f64(const wiski_grid* grid, const wiski_absorb_args* args, const double* d_xvar, const double* d_gvar, const double* d_pvar, double sigma2, double* d_omega_out, double* d_logz_out, double* d_grad_out, void* stream);

/* The two halves of a stencil-sharded step on their own (wiski_stream_step uses them when args->shard is set): the absorb
 * restricted to the stencil groups [g_lo, g_hi) (same arguments as wiski_scatter_stats_step; always the atomic form), and
 * wiski_pcg_async with every A . v product summed over the ranks of `shard`. */
int wiski_scatter_stats_step_sharded_f32(const wiski_grid* grid, const float* d_x, const float* d_y, const float* d_wa, const float* d_wb, const float* d_noise, int64_t n, float* d_b, float* d_A_half, float* d_cnt, const float* d_u, float* d_res, float* d_mean_out, double* d_stats, int32_t* d_err, void* z1, int64_t n1_bytes, void* z2, int64_t n2_bytes, const void* d_guard, int64_t guard_expect, int32_t g_lo, int32_t g_hi, void* stream);
int wiski_scatter_stats_step_sharded_f64(const wiski_grid* grid, const double* d_x, const double* d_y, const double* d_wa, const double* d_wb, const double* d_noise, int64_t n, double* d_b, double* d_A_half, double* d_cnt, const double* d_u, double* d_res, double* d_mean_out, double* d_stats, int32_t* d_err, void* z1, int64_t n1_bytes, void* z2, int64_t n2_bytes, const void* d_guard, int64_t guard_expect, int32_t g_lo, int32_t g_hi, void* stream);
int wiski_pcg_sharded_f32(const wiski_grid* grid, const float* d_A_st, const float* d_tcol, float kscale, const float* d_evec, const float* d_evec2, const float* d_eval, float shift, const float* d_RHS, int32_t k, float* d_U, float* d_Z, int32_t warm, double tol, int32_t max_iter, int32_t check_every, int32_t first_check, void* d_work, int64_t work_bytes, int32_t* h_iters, double* h_relres, const int32_t* d_err, int32_t* h_err, int32_t a_sym, float* d_R, void* stream, wiski_pcg_async* handle, int32_t mode, const wiski_shard* shard);
int wiski_pcg_sharded_f64(const wiski_grid* grid, const double* d_A_st, const double* d_tcol, double kscale, const double* d_evec, const double* d_evec2, const double* d_eval, double shift, const double* d_RHS, int32_t k, double* d_U, double* d_Z, int32_t warm, double tol, int32_t max_iter, int32_t check_every, int32_t first_check, void* d_work, int64_t work_bytes, int32_t* h_iters, double* h_relres, const int32_t* d_err, int32_t* h_err, int32_t a_sym, double* d_R, void* stream, wiski_pcg_async* handle, int32_t mode, const wiski_shard* shard);
/* wiski_pcg_async / wiski_pcg_sharded with the two-level block (two_level may be NULL: then exactly wiski_pcg_sharded).
 * two_level != NULL needs the fused path: d = 3, every g_q <= 64, eigen tables given, k = 1 or 2 <= k <= two_level->mc_cols;
 * f64: WISKI_E_BADARG. */
int wiski_pcg_twolevel_f32(const wiski_grid* grid, const float* d_A_st, const float* d_tcol, float kscale, const float* d_evec, const float* d_evec2, const float* d_eval, float shift, const float* d_RHS, int32_t k, float* d_U, float* d_Z, int32_t warm, double tol, int32_t max_iter, int32_t check_every, int32_t first_check, void* d_work, int64_t work_bytes, int32_t* h_iters, double* h_relres, const int32_t* d_err, int32_t* h_err, int32_t a_sym, float* d_R, void* stream, wiski_pcg_async* handle, int32_t mode, const wiski_shard* shard, const wiski_twolevel* two_level);
/* Refresh of the block in ONE call, everything queued on `stream`: G (r x r fp64, caller-owned, running sum) += F^T F with
 * F = diag(d_scale) W(d_x) X_S for the n points absorbed since the last refresh (d_scale [n] = sqrt of the per-point weights, or
 * NULL for unit weights; d_V / kw / d_S: the per-dim eigenvector tables [g_q][kw] and index set [3][r] of X_S as for
 * wiski_basis_project), then d_N (r x r fp32) = (D_S^-1 + gscale G)^-1 with D_S = kscale * d_lam_unit, through the Cholesky factor
 * and inverse of C = I + (gscale D_S)^1/2 G (gscale D_S)^1/2.  gscale = 1: the block for the statistics as they are; > 1: for a
 * stream expected to have grown by that factor while the block is in use (the block is applied some steps after it was computed
 * and until the next one arrives; for a stationary stream G grows in proportion to the absorbed weight).  n = 0 just re-derives
 * N from G.  d_work: scratch of wiski_twolevel_refresh_workspace_bytes(r) bytes.  The verdict travels without a launch of the caller's:
 * *d_bad (device or pinned host int32, zeroed by the caller; may be NULL) |= 1 if the factorisation failed or N has a non-finite entry
 * (N is then poisoned with NaNs), |= 2 if *d_sticky != 0 (d_sticky: the time-out word wiski_twolevel.d_cs + r of the block, or NULL). */
int64_t wiski_twolevel_refresh_workspace_bytes(int32_t r);
int wiski_twolevel_refresh_f32(const wiski_grid* grid, const float* d_x, int64_t n, const float* d_scale, const double* d_V, int32_t kw, const int32_t* d_S, int32_t r, const double* d_lam_unit, double kscale, double gscale, double* d_G, void* d_work, int64_t work_bytes, float* d_N, const uint64_t* d_sticky, int32_t* d_bad, void* stream);
/* One application of the fused preconditioner on its own (what a CG iteration does to its residual; test and tooling entry):
 * d_y = P r, d_t = Kt^-1 P r, *d_rho (device double) += r . P r, for one m-vector d_r; d_w0 (m reals) and d_w1 (2 m reals)
 * are scratch.  two_level as above or NULL.  d = 3, every g_q <= 64, g_1 g_2 % 4 == 0. */
int wiski_precond_apply_f32(const wiski_grid* grid, const float* d_evec, const float* d_evec2, const float* d_eval, float kscale, float shift, const float* d_r, float* d_w0, float* d_w1, float* d_y, float* d_t, double* d_rho, const wiski_twolevel* two_level, void* stream);
/* The same application on the kept eigenmodes only: keep[q] = number of modes of dimension q (the last columns of the eigen tables:
 * eigenvalues ascend) that are transformed; every other mode passes t = r and contributes nothing to y.  Exact to below fp32
 * resolution when shift * lambda / (1 + shift * lambda) < 2^-30 on every dropped mode.  Each keep[q] a multiple of 4 in
 * [4, min(g_q, 24)], the selected modes of two_level inside the box, and wiski_precond_keep_ok(grid, keep, two_level != NULL) == 1
 * (a backward workgroup holds the whole coefficient cube twice -- 16 or 24 rows of keep[1] * keep[2] + 16 floats each -- beside its
 * images within 144 KB of LDS: (16, 16, 16) fits, (20, 20, 20) does not);
 * keep all 0: exactly wiski_precond_apply_f32.  wiski_stream_args_f32.keep hands the same counts to the streaming step's solve;
 * there they are refused (WISKI_E_BADARG) with fp64, off the fused path or outside these bounds. */
int wiski_precond_apply_keep_f32(const wiski_grid* grid, const float* d_evec, const float* d_evec2, const float* d_eval, float kscale, float shift, const float* d_r, float* d_w0, float* d_w1, float* d_y, float* d_t, double* d_rho, const wiski_twolevel* two_level, const int32_t* keep, void* stream);
int wiski_precond_keep_ok(const wiski_grid* grid, const int32_t* keep, int32_t with_two_level);
/* The same for k grid vectors at once (the multi-column kernels of the 64-column variance / probe solves): d_r, d_y, d_t [k][m],
 * d_w0 k m reals, d_w1 2 k m reals, d_rho [k] doubles (+=).  two_level with k > 1 needs its d_mc scratch (k <= mc_cols). */
int wiski_precond_apply_cols_f32(const wiski_grid* grid, const float* d_evec, const float* d_evec2, const float* d_eval, float kscale, float shift, const float* d_r, int32_t k, float* d_w0, float* d_w1, float* d_y, float* d_t, double* d_rho, const wiski_twolevel* two_level, void* stream);

/* Dense Woodbury-factor path for small grids (the reference's own regime, m <=
 * max_cholesky_size): a10 `Q = I + L^T Kuu L` GEMM (BFN:350-355), a12 Cholesky
 * solve `Q.inv_matmul` (BFN:375), a13 `pred_cov` (BFN:399-403), BWM:27 logdet.
 * Row-major matrices with explicit leading dimensions, all DEVICE pointers.
 *   wiski_gemm   C[M,N] = alpha op(A) op(B) + beta C   (ta/tb != 0: transposed operand), MFMA
 *   wiski_potrf  in-place lower Cholesky (upper triangle zeroed); *d_info |= 1 on a
 *                non-positive pivot (caller adds jitter and retries, like psd_safe_cholesky)
 *                n <= 512: ONE launch (cooperating workgroups: serial chain on one, one owner wave per trailing tile; 32-wide
 *                panels in LDS, MFMA trailing updates); 512 < n: two-level blocked -- diagonal blocks of 256..448 rows through that
 *                launch (which also inverts them), panel and trailing update as two MFMA GEMMs per block
 *   wiski_potrf_inverse  the same factorisation plus the explicit inverse X = L^-1 (n x n, ldx; n <= 480: the same launch, one
 *                workgroup per 32-column block trailing the factor; beyond: the diagonal blocks' inverses + two GEMMs per block
 *                row) -- what a consumer wants that solves against the factor many times (the spectral and the dense Woodbury
 *                factor: mean, variances, MLL terms are then single GEMM / GEMV launches)
 *   wiski_trsm   in-place solve  L X = B (trans = 0)  or  L^T X = B (trans = 1), B is n x nrhs
 *   wiski_logdiag  *d_out += sum_i log A[i,i]   (double)
 * wiski_gemm answers WISKI_E_BADARG for a NULL operand, K < 0, lda < (ta ? M : K), ldb < (tb ? K : N) or ldc < N and touches nothing;
 * M <= 0 or N <= 0 is WISKI_OK (nothing to do); K == 0 is legal and gives C = beta C (exact zeros for beta == 0: C is not read then,
 * whatever it holds).  Operands and C may be windows of larger matrices: any base pointer aligned to the element, any leading dimension
 * from the bounds above.  wiski_trsm references the lower triangle of L only (the strict upper triangle may hold anything). */
int wiski_gemm_f32(int32_t ta, int32_t tb, int32_t M, int32_t N, int32_t K, float alpha, const float* d_A, int32_t lda, const float* d_B, int32_t ldb, float beta, float* d_C, int32_t ldc, void* stream);
int wiski_gemm_f64(int32_t ta, int32_t tb, int32_t M, int32_t N, int32_t K, double alpha, const double* d_A, int32_t lda, const double* d_B, int32_t ldb, double beta, double* d_C, int32_t ldc, void* stream);
/* Which kernel wiski_gemm (and every internal product of the library) takes for an M x N output over K terms of elem_bytes (4 or 8) wide
 * reals; launches nothing, reads the same once-per-process switch (WISKI_GEMM32_MAX_TILES) as the launcher.  t64 = ceil(M/64) ceil(N/64),
 * t128 = ceil(M/128) ceil(N/128), tested in this order:
 *   2 k_gemm128 on 64 x 64 tiles, 8 waves    K >= 128 and 240 <= t64 <= 900 (fp64) / 110 <= t64 <= 800 (fp32)
 *   1 k_gemm32  (32 x 32 tiles)              K >= 64, M N >= 8192 and t64 < 500 (fp64) / 300 (fp32) (or WISKI_GEMM32_MAX_TILES)
 *   3 k_gemm128 on 128 x 128 tiles, 8 waves  K >= 256 and t128 >= 128 (fp64) / 32 (fp32)
 *   0 k_gemm    (64 x 64 tiles)              everything else
 * WISKI_E_BADARG: M < 1, N < 1, K < 0, elem_bytes other than 4 or 8. */
int wiski_gemm_path(int32_t M, int32_t N, int32_t K, int32_t elem_bytes);
int wiski_potrf_f32(int32_t n, float* d_A, int32_t lda, int32_t* d_info, void* stream);
int wiski_potrf_f64(int32_t n, double* d_A, int32_t lda, int32_t* d_info, void* stream);
int wiski_potrf_inverse_f32(int32_t n, float* d_A, int32_t lda, float* d_X, int32_t ldx, int32_t* d_info, void* stream);
int wiski_potrf_inverse_f64(int32_t n, double* d_A, int32_t lda, double* d_X, int32_t ldx, int32_t* d_info, void* stream);
int wiski_trsm_f32(int32_t trans, int32_t n, int32_t nrhs, const float* d_L, int32_t ldl, float* d_B, int32_t ldb, void* stream);
int wiski_trsm_f64(int32_t trans, int32_t n, int32_t nrhs, const double* d_L, int32_t ldl, double* d_B, int32_t ldb, void* stream);
int wiski_logdiag_f32(int32_t n, const float* d_A, int32_t lda, double* d_out, void* stream);
int wiski_logdiag_f64(int32_t n, const double* d_A, int32_t lda, double* d_out, void* stream);

/* The dense regime's posterior factor in ONE call (lazy/dense_woodbury.py; BFN:343-404 with Kt^(1/2) as the root, BWM:27 for the logdet):
 *   G = Kt^(1/2) (the Kronecker eigenbasis d_evec / d_eval of wiski_kron_spectral_mm applied to the identity),  B = I + sym(G A G),
 *   B = C C^T with X = C^-1 (wiski_potrf_inverse),  T = X G,  M = T^T T = (Kt^-1 + A)^-1,  *d_logdiag += sum_i log C[i,i].
 * d_A_half: the native half stencil; d_work: 4 m^2 reals; d_chol, d_M: [m, m] row-major outputs; *d_info |= 1 on a non-positive pivot (the
 * caller escalates jitter as psd_safe_cholesky does).  m <= 4096.  All launches are queued on `stream`; nothing is read back. */
int wiski_dense_factor_f32(const wiski_grid* grid, const float* d_A_half, const float* d_evec, const float* d_eval, float kscale, float* d_work, int64_t work_elems, float* d_chol, float* d_M, double* d_logdiag, int32_t* d_info, void* stream);
int wiski_dense_factor_f64(const wiski_grid* grid, const double* d_A_half, const double* d_evec, const double* d_eval, double kscale, double* d_work, int64_t work_elems, double* d_chol, double* d_M, double* d_logdiag, int32_t* d_info, void* stream);

/* a6 -- replaces UpdatedRootLazyTensor.collect_vector (URLT:69-119): in-place rank-q update of a root /
 * inverse-root pair.  On entry L L^T = A and R^T L = I (R = L^-T), both [m][r] row-major with leading
 * dimensions ldl / ldr; V [m][q] (ldv) holds the new columns (W^T scaled by 1/sqrt(noise), BFN:163-168).  On
 * return L L^T = A + V V^T and R^T L = I.  O(m r q) on the MFMA GEMM through the thin factor of
 * p = R^T V (the reference builds a full r x r U: O(m r^2)); the q x q eigenproblem of p^T p is solved on the
 * device (one-workgroup parallel Jacobi, fp64) for q <= 32 -- the call is then asynchronous on `stream` like every
 * other entry point -- and on the host beyond (one small copy and a stream synchronisation).  L differs from the
 * reference's L U S~ by a right orthogonal factor.  d_ws: wiski_root_update_workspace_elems(m, r, q) reals of device scratch. */
int64_t wiski_root_update_workspace_elems(int32_t m, int32_t r, int32_t q);
int wiski_root_update_f32(int32_t m, int32_t r, int32_t q, float* d_L, int32_t ldl, float* d_R, int32_t ldr, const float* d_V, int32_t ldv, float* d_ws, int64_t ws_elems, void* stream);
int wiski_root_update_f64(int32_t m, int32_t r, int32_t q, double* d_L, int32_t ldl, double* d_R, int32_t ldr, const double* d_V, int32_t ldv, double* d_ws, int64_t ws_elems, void* stream);

/* a10 / a12 / a13 / a17 in a reduced Kronecker eigenbasis -- replaces the reference's rank-limited root space (BFN:343-404 with
 * gpytorch's root_decomposition capped at max_root_decomposition_size, URLT:74-76) for smooth kernels.  With
 * K_q = V_q diag(ev_q) V_q^T per dim, basis function j is b_j = kron_q V_q[:, S[q][j]]; the r x r problem
 * G = B^T A B, C = I + Lam^1/2 G Lam^1/2 runs on wiski_gemm / wiski_potrf / wiski_trsm (fp64).  Not GEMMs:
 *   wiski_basis_project   F[p][j] = scale_p * colscale_j * (W B)[p][j]  for n points (row-major, leading dimension ldf);
 *                         d_V: per-dim eigenvector tables [g_q][kmax] (fp64, row-major), concatenated over dims; d_S [d][r]:
 *                         per-dim eigenvector index of basis function j (< kmax <= 32); d_scale [n] / d_colscale [r] optional;
 *                         d_prior [n] optional (needs d_tcol [sum g], the Toeplitz columns): prod_q w_q^T K_q w_q, the prior
 *                         variance w^T Kuu w of each point -- its excess over sum_j lam_j F[p][j]^2 bounds the truncation error
 *                         of a predictive variance.  Points outside the grid give zero rows and set bit 0 of *d_err.
 *   wiski_basis_pair_reduce   D[q][a][a'] += sum over pairs (j, j') equal in every dim but q with S[q][j] = a, S[q][j'] = a'
 *                         of Wt[j][j'] * prod_{p != q} ev[p][S[p][j]]  (Wt r x r row-major, ev [d][kmax], D [d][kmax][kmax] zeroed by
 *                         the caller): V_q D_q V_q^T summed along its lag diagonals is the gradient of
 *                         sum_jj' Wt[j][j'] b_j^T (kron_q SymToeplitz(tcol_q)) b_j' w.r.t. tcol_q -- the MLL backward (BWM:19-51). */
int wiski_basis_project_f32(const wiski_grid* grid, const float* d_x, int64_t n, const double* d_V, int32_t kmax, const int32_t* d_S, int32_t r, const float* d_scale, const double* d_colscale, const double* d_tcol, double* d_F, int64_t ldf, double* d_prior, int32_t* d_err, void* stream);
int wiski_basis_project_f64(const wiski_grid* grid, const double* d_x, int64_t n, const double* d_V, int32_t kmax, const int32_t* d_S, int32_t r, const double* d_scale, const double* d_colscale, const double* d_tcol, double* d_F, int64_t ldf, double* d_prior, int32_t* d_err, void* stream);
/* Input gradient (VJP) of wiski_basis_project through both outputs: d_gx[n][d] (the dtype of d_x) = d/dx_p of
 * sum_j d_GF[p][j] F[p][j] + d_Gprior[p] prior[p] for the upstream gradients d_GF [n, r] (fp64, leading dimension ldg) and d_Gprior [n]
 * (fp64, may be NULL; needs d_tcol).  Same d_V / kmax / d_S / d_scale / d_colscale as the forward (d_scale is a constant, not differentiated).
 * Zero derivative in the one-hot boundary cells and at points outside the grid; fp64 accumulation; deterministic (no atomics). */
int wiski_basis_project_vjp_f32(const wiski_grid* grid, const float* d_x, int64_t n, const double* d_V, int32_t kmax, const int32_t* d_S, int32_t r, const float* d_scale, const double* d_colscale, const double* d_tcol, const double* d_GF, int64_t ldg, const double* d_Gprior, float* d_gx, void* stream);
int wiski_basis_project_vjp_f64(const wiski_grid* grid, const double* d_x, int64_t n, const double* d_V, int32_t kmax, const int32_t* d_S, int32_t r, const double* d_scale, const double* d_colscale, const double* d_tcol, const double* d_GF, int64_t ldg, const double* d_Gprior, double* d_gx, void* stream);
/* h[j] += sum_p F[p][j] t_p with t_p = d_wby[p] (/ d_scale[p] when the rows of F carry that scale; NULL: none): W^T D^-1 y of a batch in the
 * basis of F (wiski_basis_project), the right-hand-side half of a streamed update of the spectral factor's statistics (BFN:160). */
int wiski_basis_absorb_h_f32(int64_t n, int32_t r, const double* d_F, int64_t ldf, const float* d_wby, const float* d_scale, double* d_h, void* stream);
int wiski_basis_absorb_h_f64(int64_t n, int32_t r, const double* d_F, int64_t ldf, const double* d_wby, const double* d_scale, double* d_h, void* stream);
/* The spectral factor's refresh after a hyper-parameter step in ONE host call: wiski_basis_eig_update_adaptive (niter = 2, resid_ok = 1e300:
 * wiski_basis_eig_update) -> wiski_basis_change -> G = T^T G_ref T -> wiski_woodbury_c -> wiski_potrf_inverse -> wiski_factor_tail, queued
 * back to back on `stream` (OSR:113-146 refreshes its caches after every optimiser step; here that is seven kernels' worth of launches and no
 * host work in between).  All products in one packed fp64 buffer d_out of off[14] doubles; off[0..13] (wiski_factor_refresh_layout) are the
 * offsets of Vout, ev, resid, Tq, TS, lam_kuu, GT, G, chol (C factorised in place), sqG, lam, sq, Linv, tail (as wiski_factor_tail's d_out).
 * nV = sum_q g_q kw; d_work / d_verdict as wiski_basis_change; d_info as wiski_potrf_inverse; verdict_event: NULL or a hipEvent_t recorded on
 * `stream` right behind the change of basis (the verdict can then be read without waiting for the factorisation). */
int wiski_factor_refresh_layout(int32_t d, int64_t nV, int32_t kw, int32_t r_ref, int32_t r, int64_t* off);
int wiski_factor_refresh(int32_t d, const int32_t* d_g, int64_t nV, const double* d_tcol, const double* d_Vin, int32_t kw, int32_t kuse, const double* d_Vref, int32_t kref, int32_t niter, double resid_ok, const int32_t* d_Sref, const int32_t* d_S, int32_t r_ref, int32_t r, double* d_work, double* d_verdict, const double* d_Gref, const double* d_href, double kscale, int32_t* d_info, double* d_out, void* verdict_event, void* stream);
int wiski_basis_pair_reduce(int32_t d, int32_t r, int32_t kmax, const double* d_Wt, const int32_t* d_S, const double* d_ev, double* d_D, void* stream);
/* Dominant eigenvectors of the d symmetric-Toeplitz factors after a small change of their first columns, refined ON THE DEVICE from
 * the previous ones (no host eigh, no device-to-host copy): d_tcol [sum g] the new columns, d_Vin / d_Vout per-dim tables [g_q][kw]
 * (row-major, concatenated; kw even, <= 32; g_q <= 64; d_g [d] on the device), d_ev [d][kw] Ritz values (descending), d_resid [d]
 * the largest residual |K v - theta v|_inf / theta_1 over the first kuse vectors.  Two subspace-iteration steps + Rayleigh-Ritz
 * (parallel Jacobi), fp64, one workgroup per dim. */
int wiski_basis_eig_update(int32_t d, const int32_t* d_g, const double* d_tcol, const double* d_Vin, int32_t kw, int32_t kuse, double* d_Vout, double* d_ev, double* d_resid,
                           const double* d_Vref, int32_t kref, double* d_Tq, void* stream);   /* d_Vref / d_Tq (both or neither): also T_q = Vref_q^T Vnew_q, [d][32][32] */
/* The same refresh, adaptive: Rayleigh-Ritz in the span of the previous vectors (after niter steps of subspace iteration, normally 0 -- one Adam step
 * leaves the new eigenvectors inside that span to ~1e-14); only if the relative residual exceeds resid_ok a second pass with two steps re-centres the span. */
int wiski_basis_eig_update_adaptive(int32_t d, const int32_t* d_g, const double* d_tcol, const double* d_Vin, int32_t kw, int32_t kuse, double* d_Vout, double* d_ev, double* d_resid, const double* d_Vref, int32_t kref, double* d_Tq, int32_t niter, double resid_ok, void* stream);
/* Companion of wiski_basis_eig_update, one launch: the Kronecker-structured change of basis d_TS [r_ref, r] from the reference basis
 * (index set d_Sref [d, r_ref]) to the refreshed one (d_S [d, r]) given d_Tq [d][32][32] = Vref_q^T Vnew_q from wiski_basis_eig_update, the eigenvalues d_lam [r]
 * of Kuu on the kept index set, and d_verdict [3] = { max eigen-residual, trace fraction the index set leaves out, eigenvalue-weighted
 * defect of the reference span }.  d_work: r + 1 doubles, ZERO on first use (the kernel leaves it zero). */
int wiski_basis_change(int32_t d, const int32_t* d_g, int32_t kref, int32_t kw, int32_t r_ref, int32_t r, const double* d_Tq, const int32_t* d_Sref, const int32_t* d_S, const double* d_ev, const double* d_tcol, const double* d_resid, double* d_TS, double* d_lam, double* d_work, double* d_verdict, void* stream);
/* d_out [sum g] = scale * lag sums of V_q D_q V_q^T (d_V tables [g_q][kw], d_D [d][kw][kw] from wiski_basis_pair_reduce): the gradient
 * w.r.t. the Toeplitz columns, one launch; g_q <= 64. */
int wiski_basis_lag_grad(int32_t d, const int32_t* d_g, int32_t kw, const double* d_V, const double* d_D, double scale, const double* d_scale, double* d_out, void* stream);   /* d_scale != NULL: the scale is read from the device (captured graphs) */
/* d_diag[j] = |d_Y[:, j]|^2 (d_Y [r, n]), d_tail[j] = max(d_prior[j] * kscale - |d_F[j, :]|^2, 0) (d_F [n, r]): the two parts of the
 * predictive variances of n queries from the spectral factor, one launch. */
int wiski_spectral_var(int32_t n, int32_t r, const double* d_Y, const double* d_F, const double* d_prior, double kscale, double* d_diag, double* d_tail, void* stream);
/* ---- the Adam step on the MLL for the standard parameterisation, without the framework's autograd (csrc/hyper_step.hip; recorded into a
 * HIP graph by models/_graphed_step.py).  Replaces, for (Scale of)* RBF | Matern kernels with a homoskedastic second noise, what
 * /root/reference/online_gp/models/online_ski_regression.py:135-147 does through torch autograd + torch.optim.Adam. */
#define WISKI_HYPER_MAX_PARAMS 6
typedef struct {
  void* raw;          /* the raw (unconstrained) parameter, numel elements of the parameter dtype */
  void* exp_avg;      /* Adam's first / second moments (parameter dtype) and step counter(s) (fp32; step_numel = 1 or numel) */
  void* exp_avg_sq;
  void* step;
  int32_t numel;
  int32_t step_numel;
  int32_t role;       /* 0 lengthscale (numel 1 or d), 1 a factor of the output scale, 2 the second noise sigma2 */
  int32_t kind;       /* 0: value = lower + softplus(raw); 1: value = lower + (upper - lower) sigmoid(raw) */
  double lower, upper;
} wiski_hyper_param;
typedef struct {
  int32_t count;
  int32_t reserved;
  wiski_hyper_param p[WISKI_HYPER_MAX_PARAMS];
} wiski_hyper_plan;
/* d_ell [1 or d], d_scale [1] (NULL without output scales), d_s2 [1] (and d_s2_f64, may be NULL) from the raw parameters; with d_tcol64 != NULL also
 * the Toeplitz columns [sum g] (kind 0 RBF, 1-3 Matern 1/2, 3/2, 5/2) in fp64 and, if d_tcol != NULL, in the parameter dtype. */
int wiski_hyper_columns_f32(const wiski_hyper_plan* plan, const wiski_grid* grid, int32_t kind, float* d_ell, float* d_scale, float* d_s2, double* d_s2_f64, double* d_tcol64, float* d_tcol, void* stream);
int wiski_hyper_columns_f64(const wiski_hyper_plan* plan, const wiski_grid* grid, int32_t kind, double* d_ell, double* d_scale, double* d_s2, double* d_s2_f64, double* d_tcol64, double* d_tcol, void* stream);
/* d_out [9] = { val, coef0, coef1, coef2, g = -1/n, g coef0, g coef1, loss = -val/n, 1/s2 } (wiski_mll_value's arithmetic; d_n the data count on the
 * device); d_loss (may be NULL) receives the loss as well. */
int wiski_hyper_mid_f32(const double* d_bMb, const double* d_logdet, const float* d_s2, const double* d_c, const double* d_ld, const double* d_n, double* d_out, double* d_loss, void* stream);
int wiski_hyper_mid_f64(const double* d_bMb, const double* d_logdet, const double* d_s2, const double* d_c, const double* d_ld, const double* d_n, double* d_out, double* d_loss, void* stream);
/* Chain rule to the raw parameters (d_gell, d_gscale from wiski_stationary_columns_grad, sigma2's from d_mid / d_gkap) and torch.optim.Adam's update
 * (no weight decay, no amsgrad) of every parameter of the plan, its moments and step counters.  The plan is held to what wiski_hyper_columns asks of it
 * (count 1..6, exactly one lengthscale and one noise, scalar scale factors, roles 0..2, kinds 0..1, at most 64 elements; only the lengthscale's numel
 * against the grid dimension is not known here) and, on top, needs the moments and counters (step_numel 1 or numel) of every entry and d_scale / d_gscale
 * when it has a role-1 entry: anything else is WISKI_E_BADARG and nothing is launched. */
int wiski_hyper_adam_f32(const wiski_hyper_plan* plan, const float* d_scale, const float* d_s2, const float* d_gell, const float* d_gscale, const double* d_mid, const double* d_gkap, const double* d_n, double lr, double beta1, double beta2, double eps, void* stream);
int wiski_hyper_adam_f64(const wiski_hyper_plan* plan, const double* d_scale, const double* d_s2, const double* d_gell, const double* d_gscale, const double* d_mid, const double* d_gkap, const double* d_n, double lr, double beta1, double beta2, double eps, void* stream);
/* count <= 12 fp64 segments dst[s][0 .. n[s]) = src[s][..] and one scalar store, in ONE launch (the staging of a factor state into the static
 * buffers of a captured hyper-parameter step: models/_graphed_step.py). */
#define WISKI_COPY_MAX_SEGMENTS 12
typedef struct {
  const void* src[WISKI_COPY_MAX_SEGMENTS];
  void* dst[WISKI_COPY_MAX_SEGMENTS];
  int64_t n[WISKI_COPY_MAX_SEGMENTS];
  int32_t count;
  int32_t reserved;
  double scalar;        /* written to scalar_dst[0] when scalar_dst != NULL */
  void* scalar_dst;
} wiski_copy_plan;
int wiski_multi_copy_f64(const wiski_copy_plan* plan, void* stream);
/* evaluate() of n <= 64 queries from the spectral factor (r <= 1024) in one launch (the reference loop scores every batch before absorbing it,
 * /root/reference/online_gp/models/online_ski_regression.py:56-78): d_F [n, r] = W B Lam^1/2 and d_prior [n] from wiski_basis_project,
 * d_Linv = chol^-1 [r, r] (ld ldl), d_t [r] = chol^-T chol^-1 Lam^1/2 h, d_s2 [1] the observation noise, d_y [n] the targets, d_err the
 * out-of-grid flag (may be NULL).  d_out (fp64 [4]) = { rmse, mean Gaussian nll, flag, max |mean| }; d_mean / d_var (may be NULL): the
 * means and LATENT variances in the data dtype.  d_ws: 200 doubles, zero on first use (left zero). */
int wiski_spectral_evaluate_f32(int32_t n, int32_t r, const double* d_F, const double* d_prior, const double* d_Linv, int32_t ldl, const double* d_t, double kscale, const float* d_s2, const float* d_y, const int32_t* d_err, double* d_ws, double* d_out, float* d_mean, float* d_var, void* stream);
int wiski_spectral_evaluate_f64(int32_t n, int32_t r, const double* d_F, const double* d_prior, const double* d_Linv, int32_t ldl, const double* d_t, double kscale, const double* d_s2, const double* d_y, const int32_t* d_err, double* d_ws, double* d_out, double* d_mean, double* d_var, void* stream);
/* The same for a larger batch (any n; one evaluate() chunk is <= 1024): d_Y [r, n] = chol^-1 d_F^T from wiski_gemm_f64; same outputs and workspace. */
int wiski_spectral_evaluate_y_f32(int32_t n, int32_t r, const double* d_Y, const double* d_F, const double* d_prior, const double* d_t, double kscale, const float* d_s2, const float* d_y, const int32_t* d_err, double* d_ws, double* d_out, float* d_mean, float* d_var, void* stream);
int wiski_spectral_evaluate_y_f64(int32_t n, int32_t r, const double* d_Y, const double* d_F, const double* d_prior, const double* d_t, double kscale, const double* d_s2, const double* d_y, const int32_t* d_err, double* d_ws, double* d_out, double* d_mean, double* d_var, void* stream);
/* After the factorisation, three launches: d_out (packed fp64, 6 r + 2) = hr [r] | c [r] | t [r] | coef [r] | zeta [r] | bMb | logdet | scratch [r]
 * with hr = T^T h_ref (d_TS [r_ref, r]), c = chol^-1 (sq o hr) (d_Linv = chol^-1, [r, r]), bMb = |c|^2, t = chol^-T c, coef = sq o t,
 * zeta = t / sq, logdet = 2 sum log diag d_chol. */
int wiski_factor_tail(int32_t r_ref, int32_t r, const double* d_TS, const double* d_href, const double* d_sq, const double* d_Linv, const double* d_chol, double* d_out, void* stream);
/* C = I + Lam^1/2 G Lam^1/2, lam = lam_kuu * kscale, sq = sqrt(lam)  (r x r, contiguous): the matrix the spectral factor factorises. */
int wiski_woodbury_c(int32_t r, const double* d_G, const double* d_lam_kuu, double kscale, double* d_C, double* d_lam, double* d_sq, double* d_sqG, void* stream);   /* d_sqG (may be NULL): Lam^1/2 G */
/* MLL backward: d_Wt = g_ld (G - P) + g_b zeta zeta^T (r x r), d_gkap = sum_i Wt[i,i] lam_kuu[i]; d_gb, d_gld device scalars.  One launch. */
int wiski_mll_weights(int32_t r, const double* d_G, const double* d_P, const double* d_zeta, const double* d_lam_kuu, const double* d_gb, const double* d_gld, double* d_Wt, double* d_gkap, void* stream);

/* (e) -- the one collective of the path: in-place RCCL all-reduce(SUM), grouped into one launch, of the
 * statistics that are sums over data points: the half-stencil delta of W^T D^-1 W (n_half reals), W^T D^-1 y (n_b), the
 * row-sum vector W^T D^-1 1 (n_cnt) and fp64 scalars ([y^T D^-1 y, log|D|] per output, point count, weight sums: n_scal
 * doubles).  Any pointer may be NULL / count 0.  `comm` is an ncclComm_t owned by the caller (one rank per GPU); librccl
 * is resolved with dlopen at the first call (WISKI_RCCL_LIB overrides its name), so the library has no link-time
 * dependency on it.  wiski_comm_* are thin bootstrap helpers for hosts without their own RCCL setup: rank 0 creates
 * wiski_comm_unique_id_bytes() bytes with wiski_comm_unique_id, ships them to the other ranks by any means, and every
 * rank calls wiski_comm_init_rank.  The reference has no distributed code. */
int wiski_comm_unique_id_bytes(void);
int wiski_comm_unique_id(void* id_out);
int wiski_comm_init_rank(const void* id_bytes, int32_t nranks, int32_t rank, void** comm_out);
int wiski_comm_destroy(void* comm);
/* What the loaded librccl reports: its version code (ncclGetVersion; e.g. 22203) and, for a communicator, the number of ranks
 * it joins and this rank's index (comm may be NULL: version only; any out pointer may be NULL).  bench.py prints these in
 * its JSON line so that a multi-GPU number says which RCCL carried it and how many ranks the communicator really saw. */
int wiski_comm_info(void* comm, int32_t* version_out, int32_t* nranks_out, int32_t* rank_out);
int wiski_allreduce_stats_f32(void* comm, float* d_half, int64_t n_half, float* d_b, int64_t n_b, float* d_cnt, int64_t n_cnt, double* d_scal, int64_t n_scal, void* stream);
int wiski_allreduce_stats_f64(void* comm, double* d_half, int64_t n_half, double* d_b, int64_t n_b, double* d_cnt, int64_t n_cnt, double* d_scal, int64_t n_scal, void* stream);

/* Value of a device int32 flag after everything already queued on `stream`, without a stream
 * synchronisation (a one-thread publish kernel + a host spin on pinned memory, a few microseconds once the
 * queue has drained).  Used for the out-of-grid flag after a query gather, where the reference raises
 * immediately (gpytorch's grid bounds check behind BFN:205). */
int wiski_read_flag(const int32_t* d_flag, int32_t* h_value, void* stream);

/* Measurement hook (bench.py roofline leg): every half-stencil SpMV launch gets a start/stop event pair
 * attached to its own dispatch packet (hipExtLaunchKernel), i.e. the kernel's execution time as rocprofv3
 * reports it, on the stream it runs on.  wiski_prof_stop returns the summed kernel time and launch count;
 * synchronise the stream before calling it. */
int wiski_prof_start(int32_t max_launches);
int wiski_prof_stop(double* total_ms, int64_t* launches);
/* Stamps taken INSIDE the kernel (k_spmv_sym_dma: 100 MHz wall clock, earliest wave start / latest wave end of each dispatch):
 * summed [first wave started -> last wave finished] time and the number of stamped dispatches.  EVERY such dispatch between
 * wiski_prof_start and wiski_prof_stop is stamped (no measurable cost), with or without the events of wiski_prof_enable.  The
 * event pair of wiski_prof_stop brackets [predecessor complete -> kernel complete] and so contains the dispatch latency in
 * front of the first wave (~2.4 us); this figure is the kernel alone.  Readable until the next wiski_prof_start, stream
 * synchronised. */
int wiski_prof_stamps(double* total_ms, int64_t* launches, double* each_us, int64_t each_cap);   /* each_us (may be NULL): the first each_cap dispatches one by one, microseconds */
/* the raw per-wave pairs of recorded dispatch i (tools/stamp_report.py): pairs[2w] = start | placement << 48 (simd(2) pipe(2)
 * cu(4) sh(1) se(3) xcc(4), low to high), pairs[2w+1] = end (0: padding workgroup), w = blockIdx.y * gridDim.x + blockIdx.x;
 * *nwaves = the dispatch's wave count (0: not stamped); at most cap pairs are copied (pairs may be NULL) */
int wiski_prof_stamps_raw(int64_t i, uint64_t* pairs, int64_t cap, int64_t* nwaves);
/* between start and stop: switch the event attachment off / on again without touching what has been recorded (sample some
 * steps of a pipelined loop, read all events once the loop has drained) */
int wiski_prof_enable(int32_t on);
/* the same clock on an EMPTY dispatch (average of n launches, microseconds; synchronises the stream): the per-dispatch
 * floor contained in every kernel time measured this way */
int wiski_prof_empty(int32_t n, double* avg_us, void* stream);

/* ---- hyper-parameter step glue (hyper_columns.hip): what the framework spends ~10 tiny launches each on, as single launches ----
 * wiski_stationary_columns      d_out [sum g] (fp64) = S * k(l h_q / ell_q): the Toeplitz columns of a Scale(RBF | Matern) kernel on the
 *                               grid (gpytorch: kernel(x1, x2, last_dim_is_batch=True) on the grid points, GridKernel / GridInterpolationKernel).
 *                               kind 0 RBF, 1 / 2 / 3 Matern-1/2, -3/2, -5/2; d_ell [nell] (nell = 1 isotropic or = d ARD), d_scale [1] or NULL,
 *                               both DEVICE pointers in the model's dtype (no host read of a hyper-parameter).
 * wiski_stationary_columns_grad d_gell [nell], d_gscale [1] (or NULL) = gradient of <d_gout, columns> w.r.t. lengthscales / outputscale.
 * wiski_gaussian_metrics        d_out [2] = { sqrt(mean (mu - y)^2), mean 1/2 ((mu - y)^2 / v + log v + log 2 pi) }, v = var + d_add_var[0]
 *                               (d_add_var may be NULL): the per-batch test metrics of the reference's regression loop
 *                               (online_ski_regression.py:88-111), n points, one launch. */
int wiski_stationary_columns_f32(const wiski_grid* grid, int32_t kind, const float* d_ell, int32_t nell, const float* d_scale, double* d_out, void* stream);
int wiski_stationary_columns_f64(const wiski_grid* grid, int32_t kind, const double* d_ell, int32_t nell, const double* d_scale, double* d_out, void* stream);
int wiski_stationary_columns_grad_f32(const wiski_grid* grid, int32_t kind, const float* d_ell, int32_t nell, const float* d_scale, const double* d_gout, float* d_gell, float* d_gscale, void* stream);
int wiski_stationary_columns_grad_f64(const wiski_grid* grid, int32_t kind, const double* d_ell, int32_t nell, const double* d_scale, const double* d_gout, double* d_gell, double* d_gscale, void* stream);
/* Scalar tail of the Woodbury MLL of one output (BWM:34-47), value and gradient, device scalars in and out:
 *   d_val  = -1/2 ((c - bMb) / s2 + logdet + ld + n log(2 pi) + n log s2)  (d_logdet may be NULL), d_coef [3] = { d val / d bMb, d val / d logdet, c - bMb };
 *   d_gs2  = g (1/2 coef[2] / s2^2 - 1/2 n / s2) - g_kap / s2^2   (d_gkap: gradient w.r.t. 1 / s2 through the factor, or NULL).
 * n: the data count by value, or from the device scalar d_n when that is not NULL (calls recorded into a hipGraph: the count moves on). */
int wiski_mll_value_f32(const double* d_bMb, const double* d_logdet, const float* d_s2, const double* d_c, const double* d_ld, double n, const double* d_n, double* d_val, double* d_coef, void* stream);
int wiski_mll_value_f64(const double* d_bMb, const double* d_logdet, const double* d_s2, const double* d_c, const double* d_ld, double n, const double* d_n, double* d_val, double* d_coef, void* stream);
int wiski_mll_s2_grad_f32(const double* d_g, const double* d_coef, const float* d_s2, double n, const double* d_n, const double* d_gkap, float* d_gs2, void* stream);
int wiski_mll_s2_grad_f64(const double* d_g, const double* d_coef, const double* d_s2, double n, const double* d_n, const double* d_gkap, double* d_gs2, void* stream);
int wiski_gaussian_metrics_f32(int64_t n, const float* d_mu, const float* d_var, const float* d_y, const float* d_add_var, float* d_out, void* stream);
int wiski_gaussian_metrics_f64(int64_t n, const double* d_mu, const double* d_var, const double* d_y, const double* d_add_var, double* d_out, void* stream);

/* ---- probe vectors of posterior sample paths (sample_paths.hip) ----
 * d_P [m][S] (probe-minor: the S probes of a grid node are contiguous) += sum_i sqrt(wa_i) eps(first_index + i, s) w(x_i) over the q points
 * d_x [q][d]; d_wa [q] is the weight point i enters W^T D^-1 W with, NULL = unit weights.  Then cov(P_s) = W^T diag(wa) W exactly, whatever
 * the hyper-parameters, and P is additive over batches and shards as long as every point has its own global index.  S even, 2..1024.
 * Points outside the grid set bit 0 of *d_err and contribute nothing; one-hot boundary cells as wiski_interp.  q = 0 is a no-op.
 * Precondition: every wa > 0 and finite (not checked: a negative or NaN weight gives NaN increments at the point's taps, without a flag).
 * Inside / outside is decided as wiski_scatter_stats decides it -- in the working precision, against g0 and the last grid point rounded to
 * it -- so that a point enters P exactly when it enters W^T D^-1 W; an fp32 point accepted within an ulp outside the fp64 grid is moved
 * onto the edge node before its weights are taken.  WHICH cell of a dim is a one-hot boundary cell is decided in fp64: a point within an
 * fp32 ulp of node 1 or node g - 2 may get the cubic's weights here and the one-hot weights in the fp32 absorb; the two agree at the node,
 * so the difference is of the order of that ulp.
 *
 * The standard normals are part of the ABI: eps(index, s) is a function of (seed, index, s) alone, so that the probes of a model can be
 * reproduced (and continued) from its seed and point count.  For probe pair j = s / 2:
 *   (w0, w1, w2, w3) = Philox4x32-10(counter = (index & 0xffffffff, index >> 32, j, 0), key = (seed & 0xffffffff, seed >> 32))
 *                      [multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85; counter 0, key 0 gives
 *                       6627e8d5 e169c58d bc57ac4c 9b00dbd8];
 *   u0 = ((w0 >> 5) * 2^26 + (w1 >> 6) + 1) * 2^-53,  u1 = ((w2 >> 5) * 2^26 + (w3 >> 6) + 1) * 2^-53      (both in (0, 1], exact in fp64);
 *   r = sqrt(-2 log u0), theta = 6.283185307179586 * u1;   eps(index, 2 j) = r cos(theta),  eps(index, 2 j + 1) = r sin(theta).
 * All of this, the interpolation weights and the product are evaluated in IEEE fp64 for both entry points, one rounding per operation (no
 * fused multiply-adds) in the order written here and in wiski_interp's rule: u = (x - g0) / h, t = u - floor(u), the Keys polynomials in
 * Horner form ((1.5 a - 2.5) a) a + 1 and ((-0.5 a + 2.5) a - 4) a + 2, w = ((w_0 w_1) w_2) w_3 over the dims, increment =
 * w * (sqrt(wa) * eps).  Each increment is rounded once to the working precision before its atomic add (the order of the adds, hence the
 * last bits of P, is not fixed).  A host implementation therefore reproduces every increment up to the last bits of log / cos / sin. */
int wiski_scatter_probes_f32(const wiski_grid* grid, const float* d_x, const float* d_wa, int64_t q, int64_t first_index, uint64_t seed, int32_t S, float* d_P, int32_t* d_err, void* stream);
int wiski_scatter_probes_f64(const wiski_grid* grid, const double* d_x, const double* d_wa, int64_t q, int64_t first_index, uint64_t seed, int32_t S, double* d_P, int32_t* d_err, void* stream);

/* ---- exponential forgetting of the streamed statistics (decay_stats.hip) ----
 * Scaling every statistic by gamma in (0, 1] is the same GP with the noise d_i of every absorbed point replaced by d_i / gamma.  ONE launch,
 * in place, plain loads and stores (16-byte vectors on the aligned body of every region, element-wise head and tail), no workspace:
 *   plan         up to WISKI_DECAY_MAX_REGIONS regions of `real`s, x <- factor x: the half-stencil pack, b, cnt with factor gamma, the probe
 *                vectors P [m][S] with sqrt(gamma) (cov(P_s) = A stays exact).  Each factor (in (0, 1], a double) is rounded ONCE to the working
 *                precision, so a scaled element is the correctly rounded product x * (real)factor.  Regions must not overlap; n = 0 is skipped.
 *   d_R, d_Z     (both or neither; n_res reals) the carried residual of wiski_pcg: R <- gamma R - (1 - gamma) Z keeps R = b - Z - A U for the
 *                decayed (b, A) -- Z = Kt^-1 U does not depend on the data -- so the next solve stays warm without an A U product.
 *   d_stats      [nout][2] fp64 (may be NULL with nout = 0): slot 0 (y^T D^-1 y) *= gamma, slot 1 (log|D|) -= h_count[o] log gamma, with
 *                h_count [nout] (HOST) the number of points output o has absorbed.  nout <= WISKI_DECAY_MAX_OUTPUTS per call.
 *   d_side       nside <= WISKI_DECAY_MAX_OUTPUTS further fp64 device scalars *= gamma (the model's noise-weight sums), or NULL / 0.
 * gamma = 1 returns without a launch; gamma outside (0, 1] or NaN (or such a factor): WISKI_E_BADARG. */
#define WISKI_DECAY_MAX_REGIONS 8
#define WISKI_DECAY_MAX_OUTPUTS 8
typedef struct wiski_decay_plan {
  void* ptr[WISKI_DECAY_MAX_REGIONS];      /* DEVICE pointers to `real`s */
  int64_t n[WISKI_DECAY_MAX_REGIONS];      /* elements */
  double factor[WISKI_DECAY_MAX_REGIONS];
  int32_t count, reserved;
} wiski_decay_plan;
int wiski_decay_stats_f32(const wiski_decay_plan* plan, double gamma, float* d_R, const float* d_Z, int64_t n_res, double* d_stats, int32_t nout, const double* h_count, double* d_side, int32_t nside, void* stream);
int wiski_decay_stats_f64(const wiski_decay_plan* plan, double gamma, double* d_R, const double* d_Z, int64_t n_res, double* d_stats, int32_t nout, const double* h_count, double* d_side, int32_t nside, void* stream);

/* ---- re-embedding of the streamed statistics on a grown / shifted / trimmed grid (regrid_stats.hip) ----
 * The new grid has the spacing of `grid` and g_new[q] = grid->g[q] + below[q] + above[q] nodes per dim (negative: removed); the old node j of
 * dim q is the new node j + below[q].  ONE launch copies every region of the plan, out of place: a region is k blocks of m nodes of w reals,
 * element (c, node i, s) at src[c m w + i w + s] goes to dst[c m' w + i' w + s].  Every destination element is written exactly once -- zero
 * where the old grid has no such node -- in destination order, 16-byte vectors where the phases allow (any alignment of src / dst to the
 * element size is accepted); src is never written.  The layouts of the model:
 *     half stencil, group 0          k = 1,          w = 4,  r0 = (7^d - 1) / 2            (src / dst: the stencil's first element)
 *     half stencil, groups >= 1      k = (H - 4)/7,  w = 7,  r0 = 7 ((7^(d-1) - 1)/2 + 1)  (src + 4 m, dst + 4 m')
 *     offset-major stencil rows      k = rows,       w = 1,  r0 = offset index of row 0    (0 for the full stencil, (7^d - 1)/2 for a half)
 *     vectors [k][m] (b, cnt, ...)   k,              w = 1,  r0 = -1
 *     probes [m][S]                  k = 1,          w = S,  r0 = -1
 * r0 >= 0 names a stencil region: element (c, i, s) is A[i, i + off] for the offset index r0 + c w + s (base-7 digits, dim 0 first), and it is
 * written as zero where that neighbour node lies outside the new grid (so that a trimmed A is the principal submatrix, in the same layout).
 * report[i] >= 0 (a stencil region that contains the diagonal, offset index (7^d - 1)/2) asks for the drop report: the kernel ADDS to
 * d_record[2 report] the number of source nodes without a destination whose A_ii != 0 and to d_record[2 report + 1] the sum of those A_ii
 * (fp64; d_record holds WISKI_REGRID_MAX_REPORTS pairs and is zeroed by the caller).  `above` may be NULL (then g_new alone decides).
 * WISKI_E_BADARG, with nothing launched: g_new[q] < 4; g_new[q] != g[q] + below[q] + above[q]; grids without a common node; a null or
 * misaligned pointer; k or w < 1; a stencil region beyond offset index 7^d; a region whose src and dst overlap. */
#define WISKI_REGRID_MAX_REGIONS 16
#define WISKI_REGRID_MAX_REPORTS 8
typedef struct wiski_regrid_plan {
  const void* src[WISKI_REGRID_MAX_REGIONS];   /* DEVICE pointers to `real`s */
  void* dst[WISKI_REGRID_MAX_REGIONS];
  int64_t k[WISKI_REGRID_MAX_REGIONS];
  int64_t r0[WISKI_REGRID_MAX_REGIONS];
  int32_t w[WISKI_REGRID_MAX_REGIONS];
  int32_t report[WISKI_REGRID_MAX_REGIONS];
  int32_t count, reserved;
} wiski_regrid_plan;
int wiski_regrid_stats_f32(const wiski_grid* grid, const int32_t* below, const int32_t* above, const int32_t* g_new, const wiski_regrid_plan* plan, double* d_record, void* stream);
int wiski_regrid_stats_f64(const wiski_grid* grid, const int32_t* below, const int32_t* above, const int32_t* g_new, const wiski_regrid_plan* plan, double* d_record, void* stream);

/* ---- checkpoint, restore and merge of the streamed statistics through their touched nodes (pack_stats.hip) ----
 * Regions as above: k blocks of m nodes of w reals, element (c, node i, s) at c m w + i w + s; in the COMPACT form of a region m is replaced
 * by n_sel, and its node j is the full region's node d_nodes[j].  Plain loads and stores, no workgroup waits for another.
 * wiski_stats_select: marks in d_flags [m] (int32, zeroed ONCE by the caller) every node at which any element of any plan->src region is not
 *   == 0 (a NaN is kept; dst and factor are not looked at).  With d_nodes != NULL it then writes d_nodes[0 .. n_sel), the ASCENDING list of
 *   the marked nodes (d_nodes holds m), and d_count[0] = n_sel: three more launches -- counts per 256 nodes into d_work, a one-workgroup scan
 *   of them, the write -- with d_work of work_elems >= ceil(m / 256) int32 (less: WISKI_E_WORKSPACE).  A table of more than
 *   WISKI_STATS_MAX_REGIONS regions takes several calls on the same d_flags, all but the last with d_nodes = NULL.
 * wiski_stats_gather:      dst[c n_sel w + j w + s] = src[c m w + d_nodes[j] w + s]
 * wiski_stats_scatter_add: dst[c m w + d_nodes[j] w + s] += f src[c n_sel w + j w + s], f = (real)factor rounded once; f == 1 is a plain
 *   add, otherwise a rounded product and a rounded add (never one fused multiply-add).  src_full != 0: src is a FULL region and is read at
 *   the index dst is written at (a merge straight from another cache).  The list must be free of duplicates (select's is).
 * Both check every node index in the kernel: one outside [0, m) is skipped and sets bit 0 of *d_err (may be NULL), so a bad list never
 * reads or writes out of bounds.  n_sel = 0 launches nothing.  16-byte vectors where w is a multiple of the vector and both pointers are
 * 16-byte aligned.  WISKI_E_BADARG, with nothing launched: a null or misaligned pointer, k or w < 1, k m w >= 2^31, m < 1, n_sel outside
 * [0, m], a region whose src and dst overlap (or whose dst overlaps d_nodes), a NaN factor, count outside 0 .. WISKI_STATS_MAX_REGIONS. */
#define WISKI_STATS_MAX_REGIONS 16
typedef struct wiski_stats_plan {
  const void* src[WISKI_STATS_MAX_REGIONS];    /* DEVICE pointers to `real`s */
  void* dst[WISKI_STATS_MAX_REGIONS];
  int64_t k[WISKI_STATS_MAX_REGIONS];
  int64_t w[WISKI_STATS_MAX_REGIONS];
  double factor[WISKI_STATS_MAX_REGIONS];      /* scatter_add only */
  int32_t count, reserved;
} wiski_stats_plan;
int wiski_stats_select_f32(const wiski_stats_plan* plan, int64_t m, int32_t* d_flags, int32_t* d_nodes, int32_t* d_count, int32_t* d_work, int64_t work_elems, void* stream);
int wiski_stats_select_f64(const wiski_stats_plan* plan, int64_t m, int32_t* d_flags, int32_t* d_nodes, int32_t* d_count, int32_t* d_work, int64_t work_elems, void* stream);
int wiski_stats_gather_f32(const wiski_stats_plan* plan, int64_t m, const int32_t* d_nodes, int64_t n_sel, int32_t* d_err, void* stream);
int wiski_stats_gather_f64(const wiski_stats_plan* plan, int64_t m, const int32_t* d_nodes, int64_t n_sel, int32_t* d_err, void* stream);
int wiski_stats_scatter_add_f32(const wiski_stats_plan* plan, int64_t m, const int32_t* d_nodes, int64_t n_sel, int32_t src_full, int32_t* d_err, void* stream);
int wiski_stats_scatter_add_f64(const wiski_stats_plan* plan, int64_t m, const int32_t* d_nodes, int64_t n_sel, int32_t src_full, int32_t* d_err, void* stream);

/* ---- polynomial trend with marginalised coefficients (trend.hip) ----
 * y_i = h(x_i)^T beta + w(x_i)^T u + eps_i with beta ~ N(0, tau^2 I): h(x) holds the p monomials of total degree <= deg (0, 1 or 2) in the
 * normalised coordinates t_k = (x_k - center[k]) / scale[k], graded lexicographic -- 1, t_1 .. t_d, t_1^2, t_1 t_2, .., t_1 t_d, t_2^2, ..
 * -- so p = 1, d + 1 or (d + 1)(d + 2) / 2 (at most 15).  d_center and d_scale are DEVICE arrays of d doubles for both entry points.
 *
 * wiski_scatter_trend: the trend's statistics, additive over points and batches, in ONE launch:
 *     d_C [m][p] (working precision, trend-minor)   += sum_i wa_i w(x_i) h(x_i)^T        one atomic add per non-zero tap and basis function
 *     d_G [p][p] (fp64; the UPPER triangle only)    += sum_i wa_i h_i h_i^T              the caller mirrors it
 *     d_g [p]    (fp64)                             += sum_i wby_i h_i
 * d_wa NULL: unit weights; d_wby [n] is wb_i y_i, as the absorb's followers receive it.  A point enters C, G and g exactly when it enters
 * W^T D^-1 W: inside / outside is decided as wiski_scatter_stats decides it, in the working precision (wiski_scatter_probes has the
 * details, including the fp64 choice of the one-hot boundary cells); a point outside sets bit 0 of *d_err and contributes nothing.
 * Everything is evaluated in IEEE fp64 for both entry points, one rounding per operation (no fused multiply-adds): the coordinates are
 * read in the working precision and widened, the weights follow wiski_interp's rule as written for wiski_scatter_probes,
 * w = ((w_0 w_1) w_2) w_3 over the dims, t_k as above, the products t_a t_b, and the increment (wa w) h_j, which is rounded once to the
 * working precision before its atomic add (the order of the adds, hence the last bits of C, is not fixed).  G and g are summed per
 * workgroup in fp64 -- products (wa h_a) h_b and wby h_a -- and added with one fp64 atomic per entry and workgroup.
 * n = 0 is a no-op (d_x and d_wby may then be NULL).  WISKI_E_BADARG: deg outside {0, 1, 2}, n < 0, a NULL pointer other than d_wa.
 *
 * wiski_trend_rows: the query rows of the trend, one fused gather:
 *     d_R [n][p] = h(x*) - sum_t w_t(x*) S[idx_t][:]       with d_S [m][p] trend-minor (S = M C, the caller's solve)
 *     d_H [n][p] = h(x*)                                   where d_H is not NULL
 * d_S NULL writes R = H.  Weights, basis and the sum are taken in fp64 as above (the sum over the taps in tap order, dim 0 slowest), the
 * results rounded once.  A point outside the grid sets bit 0 of *d_err and its row is h(x*).  n = 0 is a no-op (d_x and d_R may then be NULL);
 * WISKI_E_BADARG as above (d_S and d_H may be NULL). */
int wiski_scatter_trend_f32(const wiski_grid* grid, const float* d_x, const float* d_wa, const float* d_wby, int64_t n, int32_t deg, const double* d_center, const double* d_scale, float* d_C, double* d_G, double* d_g, int32_t* d_err, void* stream);
int wiski_scatter_trend_f64(const wiski_grid* grid, const double* d_x, const double* d_wa, const double* d_wby, int64_t n, int32_t deg, const double* d_center, const double* d_scale, double* d_C, double* d_G, double* d_g, int32_t* d_err, void* stream);
int wiski_trend_rows_f32(const wiski_grid* grid, const float* d_x, int64_t n, int32_t deg, const double* d_center, const double* d_scale, const float* d_S, float* d_R, float* d_H, int32_t* d_err, void* stream);
int wiski_trend_rows_f64(const wiski_grid* grid, const double* d_x, int64_t n, int32_t deg, const double* d_center, const double* d_scale, const double* d_S, double* d_R, double* d_H, int32_t* d_err, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WISKI_H */
