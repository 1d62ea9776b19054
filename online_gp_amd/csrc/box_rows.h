// Box functionals c_b = int_box w(x) dx: the integral of the interpolation row over an axis-aligned box is the
// Kronecker product of D short per-dimension rows, and the three kernels on them:
//   k_box_tables       the per-dimension integrated rows tab [B][sum_q g_q], their node ranges [B][D][2] and the clipped volume [B],
//   k_wt_columns_box   the B functionals as dense m-columns (right-hand sides of the matrix-free solves),
//   k_gather_box       out[b][j] = c_b . V[row(b, j)], weights formed on the fly from the tables, fp64 accumulation.
// Included from interp_gather.hip.  Per dimension (u = (x - g0) / h, cell j = [node j, node j + 1)): an interior cell spreads
// h (F_c(t_b) - F_c(t_a)) over its four nodes j - 1 .. j + 2, F_c the antiderivative of tap c of the Keys cubic; a boundary cell
// (j = 0, j = g - 2: one-hot on the nearest node) gives node j the part of [t_a, t_b] below 1/2 and node j + 1 the part above;
// outside the grid w = 0, so a box is clipped to the grid's extent; a dimension with lo == hi evaluates at that coordinate (the
// value row of dim_stencil, bit for bit) instead of integrating.  A box not wholly inside the grid raises bit 0 of err; a NaN bound
// or lo > hi also gives a zero row.
#pragma once
#include "wiski_common.h"

// Antiderivatives of the two branches of the Keys cubic, P_near on [0, 1] and P_far on [1, 2], Horner, every operation rounded
// on its own (the closed forms are differences of these: the error of a table entry is then a few eps64 of the polynomials' TERMS).
__device__ __forceinline__ double box_p_near(double a) {
#pragma clang fp contract(off)
  return (((0.375 * a - 2.5 / 3.0) * a) * a + 1.0) * a;
}
__device__ __forceinline__ double box_p_far(double a) {
#pragma clang fp contract(off)
  return (((-0.125 * a + 2.5 / 3.0) * a - 2.0) * a + 2.0) * a;
}
// int_0^t k(tau + 1 - c) dtau: the weight that tap c (node j - 1 + c) of an interior cell j collects over [0, t] of the cell.
__device__ __forceinline__ double box_tap_integral(int c, double t) {
#pragma clang fp contract(off)
  switch (c) {
    case 0: return box_p_far(1.0 + t) - box_p_far(1.0);
    case 1: return box_p_near(t);
    case 2: return box_p_near(1.0) - box_p_near(1.0 - t);
    default: return box_p_far(2.0) - box_p_far(2.0 - t);
  }
}

// One dimension of one box: kind, clipped ends in cell units, the cells they lie in and the node range of the support.
struct BoxDim {
  int kind;          // 0: zero row (invalid, or nothing of the box inside the grid), 1: evaluated at lo == hi, 2: integrated
  int j0;            // kind 1: lowest tap
  int ia, ib;        // kind 2: first and last cell met
  double ua, ub;     // kind 2: the clipped ends, (x - g0) / h
  double width;      // factor of the clipped volume: 0, 1 (kind 1) or the clipped width
  int jlo, jhi;      // support nodes [jlo, jhi)
  bool flag;         // not wholly inside the grid, or invalid
};

template <typename real>
__device__ __forceinline__ BoxDim box_dim(real a, real c, real g0, real h, real hi, int g, real w[4]) {
#pragma clang fp contract(off)
  BoxDim r;
  r.kind = 0; r.j0 = 0; r.ia = 0; r.ib = 0; r.ua = 0.0; r.ub = 0.0; r.width = 0.0; r.jlo = 0; r.jhi = 0;
  const bool valid = a <= c;                                  // false for a NaN bound
  r.flag = !(valid && a >= g0 && c <= hi);
  if (!valid) return r;
  if (a == c) {
    const int j0 = dim_stencil<real>(a, g0, h, hi, g, w);
    if (j0 < 0) return r;
    r.kind = 1; r.j0 = j0; r.width = 1.0; r.jlo = j0; r.jhi = j0 + 4;
    return r;
  }
  const double g0d = (double)g0, hd = (double)h;
  const double ac = (double)a > g0d ? (double)a : g0d, cc = (double)c < (double)hi ? (double)c : (double)hi;
  if (!(ac < cc)) return r;
  r.kind = 2;
  r.ua = (ac - g0d) / hd;
  r.ub = (cc - g0d) / hd;
  r.width = cc - ac;
  const int fa = (int)floor(r.ua), fb = (int)floor(r.ub);
  r.ia = fa < g - 2 ? fa : g - 2;
  r.ib = fb < g - 2 ? fb : g - 2;
  r.jlo = r.ia - 1 > 0 ? r.ia - 1 : 0;
  r.jhi = (r.ib + 2 < g - 1 ? r.ib + 2 : g - 1) + 1;
  return r;
}

// Entry j of an integrated row: the cells j - 2 .. j + 1 are the ones that have node j among their taps.
__device__ __forceinline__ double box_entry(const BoxDim& r, double hd, int g, int j) {
#pragma clang fp contract(off)
  double s = 0.0;
  const int i0 = j - 2 > r.ia ? j - 2 : r.ia, i1 = j + 1 < r.ib ? j + 1 : r.ib;
  for (int i = i0; i <= i1; ++i) {
    double ta = r.ua - (double)i, tb = r.ub - (double)i;
    ta = ta < 0.0 ? 0.0 : ta;
    tb = tb > 1.0 ? 1.0 : tb;
    if (!(ta < tb)) continue;
    if (i >= 1 && i <= g - 3) {
      const int c = j - (i - 1);
      s += box_tap_integral(c, tb) - box_tap_integral(c, ta);
    } else if (j == i) {
      const double lo = ta < 0.5 ? ta : 0.5, up = tb < 0.5 ? tb : 0.5;
      s += up - lo;
    } else if (j == i + 1) {
      const double lo = ta > 0.5 ? ta : 0.5, up = tb > 0.5 ? tb : 0.5;
      s += up - lo;
    }
  }
  return hd * s;
}

// ---------------------------------------------------------------------------------------------------------------- tables
// One block per box; the threads stride over the nodes of each dimension in turn and write every entry of the row (zero off the
// support), straight to global memory: a 1-D grid may have 10^5 nodes.  Evaluated in fp64 in both precisions from g0, h as
// GridDev<real> holds them and rounded once to real -- in fp32 a narrow box would otherwise lose eps32 / width to cancellation.
template <typename real, int D>
__global__ __launch_bounds__(256) void k_box_tables(GridDev<real> G, const real* __restrict__ lo, const real* __restrict__ hi, int gsum,
                                                    real* __restrict__ tab, int32_t* __restrict__ range, real* __restrict__ vol,
                                                    int32_t* __restrict__ err) {
  const int64_t b = blockIdx.x;
  double v = 1.0;
  bool flag = false;
  int off = 0;
#pragma unroll
  for (int q = 0; q < D; ++q) {
    real w[4];
    const int g = G.g[q];
    const BoxDim r = box_dim<real>(lo[b * D + q], hi[b * D + q], G.g0[q], G.h[q], G.hi[q], g, w);
    flag = flag || r.flag;
    v *= r.width;
    real* __restrict__ row = tab + b * (int64_t)gsum + off;
    const double hd = (double)G.h[q];
    for (int j = threadIdx.x; j < g; j += blockDim.x) {
      real e = (real)0;
      if (r.kind == 1) {
        const int c = j - r.j0;
        e = c == 0 ? w[0] : (c == 1 ? w[1] : (c == 2 ? w[2] : (c == 3 ? w[3] : (real)0)));
      } else if (r.kind == 2 && j >= r.jlo && j < r.jhi) {
        e = (real)box_entry(r, hd, g, j);
      }
      row[j] = e;
    }
    if (threadIdx.x == 0) {
      range[(b * D + q) * 2] = r.jlo;
      range[(b * D + q) * 2 + 1] = r.jhi;
    }
    off += g;
  }
  if (threadIdx.x == 0) {
    vol[b] = (real)v;
    if (flag) atomicOr(err, 1);
  }
}

template <typename real>
struct BoxVec4 {
  typedef real type __attribute__((ext_vector_type(4), aligned(sizeof(real))));
};

// The support of box b: per-dimension node ranges (clamped to the grid: they come from caller memory), its rows of the table,
// and the items that the streaming kernels walk -- an item is one choice of the outer dimensions' nodes and one group of four
// consecutive nodes of the last dimension.  There are at most m < 2^31 items, and a launch strides by less than 2^24: items are
// counted and decoded in 32-bit unsigned arithmetic.
template <typename real, int D>
struct BoxSupport {
  int jlo[D], n[D];
  const real* row[D];
  int groups;          // ceil(n[D - 1] / 4)
  unsigned items;

  __device__ __forceinline__ void load(const GridDev<real>& G, const real* __restrict__ tab, const int32_t* __restrict__ range, int gsum, int64_t b) {
    int off = 0;
    items = 1;
#pragma unroll
    for (int q = 0; q < D; ++q) {
      int a = range[(b * D + q) * 2], c = range[(b * D + q) * 2 + 1];
      a = a < 0 ? 0 : a;
      c = c > G.g[q] ? G.g[q] : c;
      jlo[q] = a;
      n[q] = c > a ? c - a : 0;
      row[q] = tab + b * (int64_t)gsum + off;
      off += G.g[q];
      if (q < D - 1) items *= (unsigned)n[q];
    }
    groups = (n[D - 1] + 3) >> 2;
    items *= (unsigned)groups;
  }

  // item -> flat index of its first node, the product of the outer dimensions' entries (fp64) and the last dimension's first node
  __device__ __forceinline__ void decode(const GridDev<real>& G, unsigned item, int* flat, double* outer, int* jl) const {
    const int gi = (int)(item % (unsigned)groups);
    unsigned rest = item / (unsigned)groups;
    int f = 0;
    double p = 1.0;
#pragma unroll
    for (int q = D - 2; q >= 0; --q) {
      const int j = jlo[q] + (int)(rest % (unsigned)n[q]);
      rest /= (unsigned)n[q];
      f += j * G.stride[q];
      p *= (double)row[q][j];
    }
    *jl = jlo[D - 1] + 4 * gi;
    *flat = f + *jl;
    *outer = p;
  }
};

// ------------------------------------------------------------------------------------------------------ W^T box columns
// out[b][i] = prod_q tab_q[b][i_q] over the support of box b, plain stores (the caller zeroes the buffer), four consecutive
// entries of the last dimension per store.  `per` consecutive blocks belong to a box and stride over its items together.  The product runs
// over the dimensions in order, in real: for a box degenerate in every dimension the row is the column of wiski_wt_columns.
template <typename real, int D>
__global__ __launch_bounds__(256) void k_wt_columns_box(GridDev<real> G, const real* __restrict__ tab, const int32_t* __restrict__ range, int gsum,
                                                        int per, real* __restrict__ out) {
  const int64_t b = blockIdx.x / per;
  const int share = blockIdx.x - (int)b * per;
  BoxSupport<real, D> S;
  S.load(G, tab, range, gsum, b);
  real* __restrict__ o = out + b * (int64_t)G.m;
  const int jend = S.jlo[D - 1] + S.n[D - 1];
  for (unsigned item = (unsigned)share * blockDim.x + threadIdx.x; item < S.items; item += (unsigned)per * blockDim.x) {
    const int gi = (int)(item % (unsigned)S.groups);
    unsigned rest = item / (unsigned)S.groups;
    int flat = 0;
    real p = (real)1;
    int jq[D];
#pragma unroll
    for (int q = D - 2; q >= 0; --q) {
      jq[q] = S.jlo[q] + (int)(rest % (unsigned)S.n[q]);
      rest /= (unsigned)S.n[q];
      flat += jq[q] * G.stride[q];
    }
#pragma unroll
    for (int q = 0; q < D - 1; ++q) p *= S.row[q][jq[q]];
    const int jl = S.jlo[D - 1] + 4 * gi;
    const real* __restrict__ last = S.row[D - 1];
    if (jl + 4 <= jend) {
      typename BoxVec4<real>::type v;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = p * last[jl + i];
      *reinterpret_cast<typename BoxVec4<real>::type*>(o + flat + jl) = v;
    } else {
      for (int j = jl; j < jend; ++j) o[flat + j] = p * last[j];
    }
  }
}

// ----------------------------------------------------------------------------------------------------------- box gather
// blockIdx.x is the (box, row) pair, blockIdx.y one of nsplit shares of the box's support: the blocks of a pair stride over its
// items together, so that a single domain-sized box (125 000 terms at 50^3) still fills the machine, while a cell-sized box costs
// its few items in share 0 and an empty loop in the others.  Per item one vector load of four consecutive entries of V along the
// last dimension, weights from the tables, fp64 accumulators, block reduction.  nsplit = 1 writes out directly; otherwise the
// share's fp64 partial goes to part[(pair) nsplit + share] and k_box_reduce sums the shares in order (no atomics: the result does
// not depend on the blocks' timing).  rows_per_box = 0: the k rows of V are shared by all boxes; R >= 1: box b reads rows b R ..
template <typename real, int D>
__global__ __launch_bounds__(256) void k_gather_box(GridDev<real> G, const real* __restrict__ tab, const int32_t* __restrict__ range, int gsum,
                                                    const real* __restrict__ V, int rows, int per_box, double* __restrict__ part,
                                                    real* __restrict__ out) {
  __shared__ double sm[16];
  const int64_t pair = blockIdx.x;
  const int64_t b = pair / rows;
  const int j = (int)(pair - b * rows);
  BoxSupport<real, D> S;
  S.load(G, tab, range, gsum, b);
  const real* __restrict__ v = V + (per_box ? pair : (int64_t)j) * (int64_t)G.m;
  const real* __restrict__ last = S.row[D - 1];
  const int jend = S.jlo[D - 1] + S.n[D - 1];
  double acc = 0.0;
  for (unsigned item = blockIdx.y * blockDim.x + threadIdx.x; item < S.items; item += gridDim.y * blockDim.x) {
    int flat, jl;
    double outer;
    S.decode(G, item, &flat, &outer, &jl);
    double s = 0.0;
    if (jl + 4 <= jend) {
      const typename BoxVec4<real>::type r = *reinterpret_cast<const typename BoxVec4<real>::type*>(v + flat);
      const typename BoxVec4<real>::type w = *reinterpret_cast<const typename BoxVec4<real>::type*>(last + jl);
#pragma unroll
      for (int i = 0; i < 4; ++i) s += (double)r[i] * (double)w[i];
    } else {
      for (int jj = jl; jj < jend; ++jj) s += (double)v[flat + (jj - jl)] * (double)last[jj];
    }
    acc += outer * s;
  }
  const double total = block_reduce_sum(acc, sm);
  if (threadIdx.x == 0) {
    if (gridDim.y == 1) out[pair] = (real)total;
    else part[pair * gridDim.y + blockIdx.y] = total;
  }
}

template <typename real>
__global__ __launch_bounds__(256) void k_box_reduce(const double* __restrict__ part, int64_t pairs, int nsplit, real* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pairs) return;
  double s = 0.0;
  for (int i = 0; i < nsplit; ++i) s += part[p * nsplit + i];
  out[p] = (real)s;
}

// ------------------------------------------------------------------------------------------------------------ launchers
// Length of a box's table row: the dimensions' rows one after the other.
template <typename real>
static int box_gsum(const GridDev<real>& G) {
  int gsum = 0;
  for (int q = 0; q < G.d; ++q) gsum += G.g[q];
  return gsum;
}

template <typename real>
static int box_tables_impl(const wiski_grid* grid, const real* d_lo, const real* d_hi, int64_t B, real* d_tab, int32_t* d_range, real* d_vol,
                           int32_t* d_err, void* stream) {
  GridDev<real> G;
  int rc = make_grid_dev<real>(grid, &G);
  if (rc) return rc;
  if (B < 0 || B >= (int64_t)1 << 31) return WISKI_E_BADARG;
  if (B == 0) return WISKI_OK;
  if (!d_lo || !d_hi || !d_tab || !d_range || !d_vol || !d_err) return WISKI_E_BADARG;
  const int gsum = box_gsum<real>(G);
#define CALL(DD) hipLaunchKernelGGL((k_box_tables<real, DD>), dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, G, d_lo, d_hi, gsum, d_tab, d_range, d_vol, d_err)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

template <typename real>
static int wt_columns_box_impl(const wiski_grid* grid, const real* d_tab, const int32_t* d_range, int64_t B, real* d_out, void* stream) {
  GridDev<real> G;
  int rc = make_grid_dev<real>(grid, &G);
  if (rc) return rc;
  if (B < 0 || B >= (int64_t)1 << 24) return WISKI_E_BADARG;
  if (B == 0) return WISKI_OK;
  if (!d_tab || !d_range || !d_out) return WISKI_E_BADARG;
  const int gsum = box_gsum<real>(G);
  const int64_t most = ((int64_t)G.m / G.g[G.d - 1]) * ((G.g[G.d - 1] + 3) / 4);      // the items of a domain-sized box
  int64_t bx = (most + 255) / 256;
  bx = bx < 1 ? 1 : (bx > 128 ? 128 : bx);
  dim3 grd((unsigned)(bx * B));
#define CALL(DD) hipLaunchKernelGGL((k_wt_columns_box<real, DD>), grd, dim3(256), 0, (hipStream_t)stream, G, d_tab, d_range, gsum, (int)bx, d_out)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

template <typename real>
static int gather_box_impl(const wiski_grid* grid, const real* d_tab, const int32_t* d_range, int64_t B, const real* d_V, int32_t k,
                           int32_t rows_per_box, int32_t nsplit, double* d_part, real* d_out, void* stream) {
  GridDev<real> G;
  int rc = make_grid_dev<real>(grid, &G);
  if (rc) return rc;
  if (B < 0 || k < 1 || rows_per_box < 0 || nsplit < 1 || nsplit > 65535) return WISKI_E_BADARG;
  if (B == 0) return WISKI_OK;
  if (!d_tab || !d_range || !d_V || !d_out || (nsplit > 1 && !d_part)) return WISKI_E_BADARG;
  const int rows = rows_per_box > 0 ? rows_per_box : k;
  const int64_t pairs = B * rows;
  if (pairs >= (int64_t)1 << 31) return WISKI_E_BADARG;
  const int gsum = box_gsum<real>(G);
  dim3 grd((unsigned)pairs, (unsigned)nsplit);
#define CALL(DD) hipLaunchKernelGGL((k_gather_box<real, DD>), grd, dim3(256), 0, (hipStream_t)stream, G, d_tab, d_range, gsum, d_V, rows, rows_per_box > 0, d_part, d_out)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  if (nsplit > 1) {
    hipLaunchKernelGGL((k_box_reduce<real>), dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_part, pairs, nsplit, d_out);
    WISKI_LAUNCH_CHECK();
  }
  return WISKI_OK;
}

extern "C" {
int wiski_box_tables_f32(const wiski_grid* g, const float* lo, const float* hi, int64_t B, float* tab, int32_t* range, float* vol, int32_t* err, void* s) { return box_tables_impl<float>(g, lo, hi, B, tab, range, vol, err, s); }
int wiski_box_tables_f64(const wiski_grid* g, const double* lo, const double* hi, int64_t B, double* tab, int32_t* range, double* vol, int32_t* err, void* s) { return box_tables_impl<double>(g, lo, hi, B, tab, range, vol, err, s); }
int wiski_wt_columns_box_f32(const wiski_grid* g, const float* tab, const int32_t* range, int64_t B, float* out, void* s) { return wt_columns_box_impl<float>(g, tab, range, B, out, s); }
int wiski_wt_columns_box_f64(const wiski_grid* g, const double* tab, const int32_t* range, int64_t B, double* out, void* s) { return wt_columns_box_impl<double>(g, tab, range, B, out, s); }
int wiski_gather_box_f32(const wiski_grid* g, const float* tab, const int32_t* range, int64_t B, const float* V, int32_t k, int32_t rows_per_box, int32_t nsplit, double* part, float* out, void* s) { return gather_box_impl<float>(g, tab, range, B, V, k, rows_per_box, nsplit, part, out, s); }
int wiski_gather_box_f64(const wiski_grid* g, const double* tab, const int32_t* range, int64_t B, const double* V, int32_t k, int32_t rows_per_box, int32_t nsplit, double* part, double* out, void* s) { return gather_box_impl<double>(g, tab, range, B, V, k, rows_per_box, nsplit, part, out, s); }
}
