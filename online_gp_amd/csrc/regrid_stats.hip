// Re-embedding of the streamed statistics on a grid changed by whole nodes: every region of a small table is copied,
// out of place and in ONE launch, from its layout on the old grid (g nodes per dim) to the same layout on the new one
// (g' = g + below + above nodes per dim, the old node j sitting at j + below).  A region is k blocks of m nodes of w reals: element
// (c, node i, s) lives at c m w + i w + s in the source and at c m' w + i' w + s in the destination -- the half-stencil group 0
// (k = 1, w = 4), its groups >= 1 (w = 7), vectors [k][m] (w = 1), probes [m][S] (w = S), offset-major stencils [rows][m] (w = 1).
//
// The kernel is DESTINATION ordered: every destination element is written exactly once, with the source value where the node (and,
// for a stencil entry A[i, i + off], the neighbour node) exists on both grids and with zero elsewhere; there is no memset pass and the
// source is never written.  Units are numbered and walked as in decay_stats.hip: 16-byte vectors on the aligned body of every
// destination region plus one edge unit per region (the up to V - 1 elements before and after the body), REGRID_UNROLL units per thread
// and pass with every load issued before the first store.  A destination vector whose V elements are V consecutive source elements on
// a 16-byte boundary is one 16-byte load (fp32 group 0 with aligned buffers: one vector per stencil row); otherwise its elements are
// loaded one by one.  Plain loads and stores only.
//
// Drop report: when nodes are removed, a second grid-stride pass reads the stencil diagonal A_ii of every SOURCE node without a
// destination and adds (number of those with A_ii != 0, sum of those A_ii in fp64) to the caller's record, one pair of atomics per
// wave and report slot.
#include "wiski_common.h"

namespace {

constexpr int REGRID_THREADS = 256;
constexpr int REGRID_UNROLL = 4;
constexpr int REGRID_MAX_BLOCKS = 2048;                     // 256 CUs x 8 blocks, the rest by grid stride

struct RegridGeom {
  int d;
  int g_old[WISKI_MAX_DIM], g_new[WISKI_MAX_DIM], below[WISKI_MAX_DIM];
  int stride_old[WISKI_MAX_DIM];                            // flat stride of dim q on the old grid (dim 0 slowest)
  int m_old, m_new;
  int trims;                                                // some source node has no destination
};

template <typename real>
struct RegridRegion {
  const real* src;
  real* dst;
  int64_t n;          // destination elements: k m' w
  int64_t nvec;       // 16-byte vectors of the aligned destination body
  int64_t first;      // number of the region's first unit; its units are nvec vectors, then the edge unit if head + tail > 0
  int64_t r0;         // stencil offset index of element (c, ., s) is r0 + c w + s (base 7, dim 0 first); < 0: not a stencil
  int64_t diag;       // source position c w m + s of the diagonal's (c, s) pair, i.e. A_ii sits at src[diag_c m w + i w + diag_s]
  int32_t head;       // elements before the first aligned vector
  int32_t w;
  int32_t mw_old, mw_new;
  int32_t report;     // slot of the drop record, < 0: none
  int32_t diag_s;
};

template <typename real>
struct RegridArgs {
  RegridRegion<real> r[WISKI_REGRID_MAX_REGIONS];
  RegridGeom G;
  int32_t count;
  int64_t units;
  double* record;     // [WISKI_REGRID_MAX_REPORTS][2]: (rows, mass)
};

template <typename T>
using global_ptr = __attribute__((address_space(1))) T*;
template <typename T>
__device__ __forceinline__ global_ptr<T> as_global(T* p) { return (global_ptr<T>)p; }

template <typename real>
struct Vec16;
template <>
struct Vec16<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <>
struct Vec16<double> { typedef double type __attribute__((ext_vector_type(2))); };

// Position of one destination element: block c, node multi-index j (new grid), slot s.
struct Cursor {
  int64_t c;
  int s;
  int j[WISKI_MAX_DIM];
};

template <typename real>
__device__ __forceinline__ Cursor decode(const RegridRegion<real>& R, const RegridGeom& G, int64_t e) {
  Cursor p;
  p.c = e / R.mw_new;
  const int rem = (int)(e - p.c * R.mw_new);
  int node = rem / R.w;
  p.s = rem - node * R.w;
#pragma unroll
  for (int q = WISKI_MAX_DIM - 1; q >= 0; --q) {
    p.j[q] = 0;
    if (q < G.d) {
      const int t = node / G.g_new[q];
      p.j[q] = node - t * G.g_new[q];
      node = t;
    }
  }
  return p;
}

__device__ __forceinline__ void advance(Cursor& p, int w, const RegridGeom& G) {
  if (++p.s < w) return;
  p.s = 0;
#pragma unroll
  for (int q = WISKI_MAX_DIM - 1; q >= 0; --q) {
    if (q < G.d) {
      if (++p.j[q] < G.g_new[q]) return;
      p.j[q] = 0;
    }
  }
  ++p.c;
}

// Source index of the destination element at p, or -1 where the destination holds zero: a node the old grid does not have, or a
// stencil entry whose neighbour node lies outside the new grid.
template <typename real>
__device__ __forceinline__ int64_t source_index(const RegridRegion<real>& R, const RegridGeom& G, const Cursor& p) {
  int node = 0;
  bool ok = true;
  int64_t r = R.r0 + p.c * R.w + p.s;
#pragma unroll
  for (int q = WISKI_MAX_DIM - 1; q >= 0; --q) {
    if (q < G.d) {
      const int jo = p.j[q] - G.below[q];
      ok = ok && jo >= 0 && jo < G.g_old[q];
      node += jo * G.stride_old[q];
      if (R.r0 >= 0) {
        const int64_t t = r / 7;
        const int nb = p.j[q] + (int)(r - 7 * t) - 3;
        ok = ok && nb >= 0 && nb < G.g_new[q];
        r = t;
      }
    }
  }
  return ok ? p.c * R.mw_old + (int64_t)node * R.w + p.s : -1;
}

template <typename real>
__device__ __forceinline__ real fetch(const RegridRegion<real>& R, const RegridGeom& G, int64_t e) {
  const int64_t f = source_index(R, G, decode(R, G, e));
  return f >= 0 ? as_global(R.src)[f] : (real)0;
}

template <typename real>
__global__ __launch_bounds__(REGRID_THREADS) void k_regrid_stats(const RegridArgs<real> A) {
  using vec = typename Vec16<real>::type;
  constexpr int V = 16 / (int)sizeof(real);
  __shared__ RegridRegion<real> s_r[WISKI_REGRID_MAX_REGIONS];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < WISKI_REGRID_MAX_REGIONS; ++i)
      if (i < A.count) s_r[i] = A.r[i];
  }
  __syncthreads();
  const RegridGeom& G = A.G;
  const int64_t stride = (int64_t)gridDim.x * REGRID_THREADS;
  const int64_t tid = (int64_t)blockIdx.x * REGRID_THREADS + threadIdx.x;
  const int last = A.count - 1;
  int reg = 0;                                     // the units of a thread only move forward through the table
  for (int64_t u0 = tid; u0 < A.units; u0 += stride * REGRID_UNROLL) {
    vec v[REGRID_UNROLL];
    real* dst[REGRID_UNROLL];
    bool live[REGRID_UNROLL];
#pragma unroll
    for (int j = 0; j < REGRID_UNROLL; ++j) {
      const int64_t u = u0 + j * stride;
      live[j] = false;
      if (u >= A.units) continue;
      while (reg < last && u >= s_r[reg + 1].first) ++reg;
      const RegridRegion<real>& R = s_r[reg];
      const int64_t loc = u - R.first;
      if (loc < R.nvec) {
        const int64_t e0 = R.head + loc * V;
        Cursor p = decode(R, G, e0);
        int64_t f[V];
        bool run = true;                           // V consecutive source elements
#pragma unroll
        for (int e = 0; e < V; ++e) {
          f[e] = source_index(R, G, p);
          run = run && f[e] >= 0 && f[e] == f[0] + e;
          advance(p, R.w, G);
        }
        dst[j] = R.dst + e0;
        live[j] = true;
        if (run && ((uintptr_t)(R.src + f[0]) & 15) == 0) {
          v[j] = *as_global(reinterpret_cast<const vec*>(R.src + f[0]));
        } else {
#pragma unroll
          for (int e = 0; e < V; ++e) v[j][e] = f[e] >= 0 ? as_global(R.src)[f[e]] : (real)0;
        }
      } else {
        // the edge unit: [0, head) and [head + nvec V, n), element by element (at most 2 (V - 1) elements in one lane per region)
        const int64_t tail0 = R.head + R.nvec * V;
        const global_ptr<real> de = as_global(R.dst);
        for (int64_t e = 0; e < R.head; ++e) de[e] = fetch(R, G, e);
        for (int64_t e = tail0; e < R.n; ++e) de[e] = fetch(R, G, e);
      }
    }
#pragma unroll
    for (int j = 0; j < REGRID_UNROLL; ++j)
      if (live[j]) *as_global(reinterpret_cast<vec*>(dst[j])) = v[j];
  }
  if (!G.trims) return;                            // (uniform over the launch)
  // the drop report: diagonals of the source nodes that have no destination
  for (int i = 0; i < A.count; ++i) {
    const RegridRegion<real>& R = s_r[i];
    if (R.report < 0) continue;                    // (uniform over the block)
    double rows = 0.0, mass = 0.0;
    for (int64_t node = tid; node < G.m_old; node += stride) {
      int t = (int)node;
      bool kept = true;
#pragma unroll
      for (int q = WISKI_MAX_DIM - 1; q >= 0; --q) {
        if (q < G.d) {
          const int t2 = t / G.g_old[q];
          const int jn = t - t2 * G.g_old[q] + G.below[q];
          kept = kept && jn >= 0 && jn < G.g_new[q];
          t = t2;
        }
      }
      if (!kept) {
        const real a = as_global(R.src)[R.diag + node * R.w + R.diag_s];
        if (a != (real)0) {
          rows += 1.0;
          mass += (double)a;
        }
      }
    }
    rows = wave_reduce_sum<double>(rows);
    mass = wave_reduce_sum<double>(mass);
    if ((threadIdx.x & 63) == 0 && rows != 0.0) {
      atomicAdd(A.record + 2 * R.report, rows);
      atomicAdd(A.record + 2 * R.report + 1, mass);
    }
  }
}

template <typename real>
int regrid_stats_impl(const wiski_grid* grid, const int32_t* below, const int32_t* above, const int32_t* g_new, const wiski_regrid_plan* plan,
                      double* d_record, void* stream) {
  constexpr int V = 16 / (int)sizeof(real);
  GridDev<real> Go;
  if (make_grid_dev<real>(grid, &Go) != WISKI_OK) return WISKI_E_BADARG;
  if (!below || !g_new || !plan || plan->count < 0 || plan->count > WISKI_REGRID_MAX_REGIONS) return WISKI_E_BADARG;
  RegridArgs<real> A;
  RegridGeom& G = A.G;
  G.d = Go.d;
  G.trims = 0;
  int64_t m_new = 1, R7 = 1;
  for (int q = 0; q < WISKI_MAX_DIM; ++q) {
    G.g_old[q] = Go.g[q];
    G.stride_old[q] = Go.stride[q];
    G.g_new[q] = 1;
    G.below[q] = 0;
    if (q >= Go.d) continue;
    if (g_new[q] < 4) return WISKI_E_BADARG;
    if (above && (int64_t)g_new[q] != (int64_t)Go.g[q] + below[q] + above[q]) return WISKI_E_BADARG;
    if (below[q] <= -Go.g[q] || below[q] >= g_new[q]) return WISKI_E_BADARG;       // the grids share no node in this dim
    G.g_new[q] = g_new[q];
    G.below[q] = below[q];
    if (below[q] < 0 || Go.g[q] + below[q] > g_new[q]) G.trims = 1;
    m_new *= g_new[q];
    R7 *= 7;
    if (m_new >= (int64_t)1 << 31) return WISKI_E_BADARG;
  }
  G.m_old = Go.m;
  G.m_new = (int)m_new;
  A.count = 0;
  A.units = 0;
  A.record = d_record;
  const int64_t centre = (R7 - 1) / 2;
  for (int i = 0; i < plan->count; ++i) {
    const real* src = (const real*)plan->src[i];
    real* dst = (real*)plan->dst[i];
    const int64_t k = plan->k[i], w = plan->w[i], r0 = plan->r0[i];
    const int32_t report = plan->report[i];
    if (!src || !dst || ((uintptr_t)src % sizeof(real)) || ((uintptr_t)dst % sizeof(real))) return WISKI_E_BADARG;
    if (k < 1 || w < 1 || w * m_new >= ((int64_t)1 << 31) || w * (int64_t)Go.m >= ((int64_t)1 << 31)) return WISKI_E_BADARG;
    if (r0 >= 0 && r0 + k * w > R7) return WISKI_E_BADARG;
    const int64_t n = k * w * m_new, n_src = k * w * (int64_t)Go.m;
    if ((uintptr_t)src < (uintptr_t)(dst + n) && (uintptr_t)dst < (uintptr_t)(src + n_src)) return WISKI_E_BADARG;   // out of place only
    RegridRegion<real>& R = A.r[A.count++];
    R.src = src;
    R.dst = dst;
    R.n = n;
    R.w = (int32_t)w;
    R.r0 = r0 >= 0 ? r0 : -1;
    R.mw_old = (int32_t)(w * Go.m);
    R.mw_new = (int32_t)(w * m_new);
    R.report = -1;
    R.diag = 0;
    R.diag_s = 0;
    if (report >= 0) {
      // the region that holds the diagonal reports: offset index `centre` = r0 + c w + s
      if (report >= WISKI_REGRID_MAX_REPORTS || !d_record || ((uintptr_t)d_record % sizeof(double))) return WISKI_E_BADARG;
      if (r0 < 0 || centre < r0 || centre >= r0 + k * w) return WISKI_E_BADARG;
      R.report = report;
      R.diag = (centre - r0) / w * R.mw_old;
      R.diag_s = (int32_t)((centre - r0) % w);
    }
    int64_t head = (int64_t)((16 - (uintptr_t)dst % 16) % 16 / sizeof(real));
    if (head > n) head = n;
    R.head = (int32_t)head;
    R.nvec = (n - head) / V;
    R.first = A.units;
    A.units += R.nvec + ((R.nvec * V != n) ? 1 : 0);
  }
  if (A.units == 0) return WISKI_OK;
  const int64_t per_block = (int64_t)REGRID_THREADS * REGRID_UNROLL;
  int64_t blocks = (A.units + per_block - 1) / per_block;
  blocks = blocks < 1 ? 1 : (blocks > REGRID_MAX_BLOCKS ? REGRID_MAX_BLOCKS : blocks);
  hipLaunchKernelGGL((k_regrid_stats<real>), dim3((unsigned)blocks), dim3(REGRID_THREADS), 0, (hipStream_t)stream, A);
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

}  // namespace

extern "C" {
int wiski_regrid_stats_f32(const wiski_grid* grid, const int32_t* below, const int32_t* above, const int32_t* g_new, const wiski_regrid_plan* plan,
                           double* d_record, void* stream) {
  return regrid_stats_impl<float>(grid, below, above, g_new, plan, d_record, stream);
}
int wiski_regrid_stats_f64(const wiski_grid* grid, const int32_t* below, const int32_t* above, const int32_t* g_new, const wiski_regrid_plan* plan,
                           double* d_record, void* stream) {
  return regrid_stats_impl<double>(grid, below, above, g_new, plan, d_record, stream);
}
}
