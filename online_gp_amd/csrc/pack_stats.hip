// Checkpoint, restore and merge of the streamed statistics through their touched nodes.  All three operations work on
// node regions as regrid_stats.hip describes them: k blocks of m nodes of w reals, element (c, node i, s) at c m w + i w + s; in the
// COMPACT form of a region m is replaced by n_sel and node j of it is node nodes[j] of the full one.
//
//   select       nodes[0 .. n_sel) = the ascending list of the nodes at which any element of any region is not == 0 (a NaN is kept).
//                Several ordinary launches, no workgroup waits for another: k_stats_flags marks the nodes (one pass over every region,
//                walked like decay_stats.hip: 16-byte vectors on the aligned body, one edge unit per region; a marked node gets a plain
//                store of 1, so the flags of several calls accumulate); k_stats_count counts the marks of every 256 nodes; k_stats_scan,
//                ONE workgroup, turns the block counts into exclusive offsets, 256 per pass with a running carry, and writes n_sel;
//                k_stats_write puts node b 256 + t at offsets[b] + (marks before it in the block, by wave ballots).  The order is that of
//                the nodes: deterministic.
//   gather       dst[c n_sel w + j w + s] = src[c m w + nodes[j] w + s]
//   scatter_add  dst[c m w + nodes[j] w + s] += f src[c n_sel w + j w + s]   (src_full: src is a full region, read at the dst's index)
//
// gather and scatter_add number the COMPACT elements of all regions consecutively and walk them grid-stride, PACK_UNROLL units per
// thread and pass with every load issued before the first store.  Consecutive lanes hold consecutive (node, slot) pairs of a block
// (w = 1: consecutive nodes): the compact side is one contiguous stream, the full side is contiguous within a node and ascending
// between nodes.  A region whose w is a multiple of the 16-byte vector and whose two pointers are 16-byte aligned (fp32 group 0, w = 4)
// moves by whole vectors.  Every node index is checked in the kernel: one outside [0, m) is skipped and sets bit 0 of *err, so a bad
// list never reads or writes out of bounds.  Plain loads and stores only (the ascending, duplicate-free list needs no atomics; the
// error bit is the one atomicOr the absorb kernels use for theirs).
//
// f is rounded ONCE to the working precision.  f == 1 is a plain add; otherwise a rounded product followed by a rounded add, never
// contracted into a fused multiply-add, so a two-operation host reference matches bit for bit.
#include "wiski_common.h"

namespace {

constexpr int PACK_THREADS = 256;
constexpr int PACK_UNROLL = 4;
constexpr int PACK_MAX_BLOCKS = 2048;                       // 256 CUs x 8 blocks, the rest by grid stride

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

// k, w >= 1 and k m w < 2^31 (m < 2^31: no product below overflows)
inline bool region_fits(int64_t k, int64_t m, int64_t w) {
  const int64_t lim = (int64_t)1 << 31;
  return k >= 1 && w >= 1 && k < lim && w < lim && k * m < lim && k * m * w < lim;
}

// ---------------------------------------------------------------------------------------------------------------- select: flags --
template <typename real>
struct FlagRegion {
  const real* ptr;
  int64_t n;          // elements: k m w
  int64_t nvec;       // 16-byte vectors of the aligned body
  int64_t first;      // number of the region's first unit; its units are nvec vectors, then the edge unit if head + tail > 0
  int32_t head;       // elements before the first aligned vector
  int32_t w;
  int32_t mw;         // m w
};

template <typename real>
struct FlagArgs {
  FlagRegion<real> r[WISKI_STATS_MAX_REGIONS];
  int32_t count;
  int64_t units;
  int32_t* flags;     // [m]
};

// element e of the region (e < k m w < 2^31: 32-bit arithmetic) holds x: mark its node unless x == 0 (a NaN is not == 0)
template <typename real>
__device__ __forceinline__ void mark(const FlagRegion<real>& R, global_ptr<int32_t> flags, int64_t e, real x) {
  if (!(x == (real)0)) {
    const uint32_t r = (uint32_t)e % (uint32_t)R.mw;
    flags[R.w == 1 ? r : r / (uint32_t)R.w] = 1;
  }
}

template <typename real>
__global__ __launch_bounds__(PACK_THREADS) void k_stats_flags(const FlagArgs<real> A) {
  using vec = typename Vec16<real>::type;
  constexpr int V = 16 / (int)sizeof(real);
  __shared__ FlagRegion<real> s_r[WISKI_STATS_MAX_REGIONS];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < WISKI_STATS_MAX_REGIONS; ++i)
      if (i < A.count) s_r[i] = A.r[i];
  }
  __syncthreads();
  const global_ptr<int32_t> flags = as_global(A.flags);
  const int64_t stride = (int64_t)gridDim.x * PACK_THREADS;
  const int last = A.count - 1;
  int reg = 0;                                     // the units of a thread only move forward through the table
  for (int64_t u0 = (int64_t)blockIdx.x * PACK_THREADS + threadIdx.x; u0 < A.units; u0 += stride * PACK_UNROLL) {
    vec v[PACK_UNROLL];
    int64_t e0[PACK_UNROLL];
    int which[PACK_UNROLL];                        // region of the unit's vector, -1: nothing loaded
#pragma unroll
    for (int j = 0; j < PACK_UNROLL; ++j) {
      const int64_t u = u0 + j * stride;
      which[j] = -1;
      if (u >= A.units) continue;
      while (reg < last && u >= s_r[reg + 1].first) ++reg;
      const FlagRegion<real>& R = s_r[reg];
      const int64_t loc = u - R.first;
      if (loc < R.nvec) {
        e0[j] = R.head + loc * V;
        v[j] = *as_global(reinterpret_cast<const vec*>(R.ptr + e0[j]));
        which[j] = reg;
      } else {                                     // the edge unit: [0, head) and [head + nvec V, n), element by element
        const global_ptr<const real> xe = as_global(R.ptr);
        for (int64_t e = 0; e < R.head; ++e) mark(R, flags, e, xe[e]);
        for (int64_t e = R.head + R.nvec * V; e < R.n; ++e) mark(R, flags, e, xe[e]);
      }
    }
#pragma unroll
    for (int j = 0; j < PACK_UNROLL; ++j) {
      if (which[j] < 0) continue;
      const FlagRegion<real>& R = s_r[which[j]];
#pragma unroll
      for (int e = 0; e < V; ++e) mark(R, flags, e0[j] + e, v[j][e]);
    }
  }
}

// ----------------------------------------------------------------------------------------------------------- select: compaction --
// marks of the block's 256 nodes before this thread's (exclusive), and the block's total, by wave ballots
__device__ __forceinline__ int block_rank(bool on, int* total) {
  __shared__ int s_wave[PACK_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long mask = __ballot(on);
  if (lane == 0) s_wave[wave] = __popcll(mask);
  __syncthreads();
  int before = __popcll(mask & ((1ull << lane) - 1ull)), sum = 0;
#pragma unroll
  for (int i = 0; i < PACK_THREADS / 64; ++i) {
    if (i < wave) before += s_wave[i];
    sum += s_wave[i];
  }
  *total = sum;
  return before;
}

__global__ __launch_bounds__(PACK_THREADS) void k_stats_count(const int32_t* __restrict__ flags, int32_t m, int32_t* __restrict__ counts) {
  const int64_t node = (int64_t)blockIdx.x * PACK_THREADS + threadIdx.x;
  int total;
  block_rank(node < m && flags[node] != 0, &total);
  if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// ONE workgroup: counts [nb] -> exclusive offsets, in place; n_sel to d_count[0].
__global__ __launch_bounds__(PACK_THREADS) void k_stats_scan(int32_t* __restrict__ counts, int64_t nb, int32_t* __restrict__ d_count) {
  __shared__ int s_scan[PACK_THREADS];
  int carry = 0;                                   // (the same in every thread)
  for (int64_t base = 0; base < nb; base += PACK_THREADS) {
    const int64_t i = base + threadIdx.x;
    const int c = i < nb ? counts[i] : 0;
    s_scan[threadIdx.x] = c;
    __syncthreads();
    for (int off = 1; off < PACK_THREADS; off <<= 1) {          // Hillis-Steele, inclusive
      const int add = threadIdx.x >= off ? s_scan[threadIdx.x - off] : 0;
      __syncthreads();
      s_scan[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < nb) counts[i] = carry + s_scan[threadIdx.x] - c;
    carry += s_scan[PACK_THREADS - 1];
    __syncthreads();                               // (the next pass overwrites s_scan)
  }
  if (threadIdx.x == 0) d_count[0] = carry;
}

__global__ __launch_bounds__(PACK_THREADS) void k_stats_write(const int32_t* __restrict__ flags, int32_t m, const int32_t* __restrict__ offsets,
                                                             int32_t* __restrict__ nodes) {
  const int64_t node = (int64_t)blockIdx.x * PACK_THREADS + threadIdx.x;
  const bool on = node < m && flags[node] != 0;
  int total;
  const int before = block_rank(on, &total);
  if (on) nodes[offsets[blockIdx.x] + before] = (int32_t)node;   // (offset + rank < n_sel <= m: inside d_nodes [m])
}

template <typename real>
int stats_select_impl(const wiski_stats_plan* plan, int64_t m, int32_t* d_flags, int32_t* d_nodes, int32_t* d_count, int32_t* d_work,
                      int64_t work_elems, void* stream) {
  constexpr int V = 16 / (int)sizeof(real);
  if (!plan || plan->count < 0 || plan->count > WISKI_STATS_MAX_REGIONS) return WISKI_E_BADARG;
  if (m < 1 || m >= ((int64_t)1 << 31) || !d_flags || ((uintptr_t)d_flags % sizeof(int32_t))) return WISKI_E_BADARG;
  const int64_t nb = (m + PACK_THREADS - 1) / PACK_THREADS;
  if (d_nodes) {
    if (!d_count || !d_work || ((uintptr_t)d_nodes % sizeof(int32_t)) || ((uintptr_t)d_count % sizeof(int32_t)) ||
        ((uintptr_t)d_work % sizeof(int32_t)))
      return WISKI_E_BADARG;
    if (work_elems < nb) return WISKI_E_WORKSPACE;
  }
  FlagArgs<real> A;
  A.count = 0;
  A.units = 0;
  A.flags = d_flags;
  for (int i = 0; i < plan->count; ++i) {
    const real* ptr = (const real*)plan->src[i];
    const int64_t k = plan->k[i], w = plan->w[i];
    if (!ptr || ((uintptr_t)ptr % sizeof(real)) || !region_fits(k, m, w)) return WISKI_E_BADARG;
    FlagRegion<real>& R = A.r[A.count++];
    R.ptr = ptr;
    R.n = k * m * w;
    R.w = (int32_t)w;
    R.mw = (int32_t)(m * w);
    int64_t head = (int64_t)((16 - (uintptr_t)ptr % 16) % 16 / sizeof(real));
    if (head > R.n) head = R.n;
    R.head = (int32_t)head;
    R.nvec = (R.n - head) / V;
    R.first = A.units;
    A.units += R.nvec + ((R.nvec * V != R.n) ? 1 : 0);
  }
  const hipStream_t st = (hipStream_t)stream;
  if (A.units > 0) {
    const int64_t per_block = (int64_t)PACK_THREADS * PACK_UNROLL;
    int64_t blocks = (A.units + per_block - 1) / per_block;
    blocks = blocks > PACK_MAX_BLOCKS ? PACK_MAX_BLOCKS : blocks;
    hipLaunchKernelGGL((k_stats_flags<real>), dim3((unsigned)blocks), dim3(PACK_THREADS), 0, st, A);
    WISKI_LAUNCH_CHECK();
  }
  if (!d_nodes) return WISKI_OK;                   // (a split plan: the compaction follows its last part)
  hipLaunchKernelGGL(k_stats_count, dim3((unsigned)nb), dim3(PACK_THREADS), 0, st, d_flags, (int32_t)m, d_work);
  WISKI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_stats_scan, dim3(1), dim3(PACK_THREADS), 0, st, d_work, nb, d_count);
  WISKI_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_stats_write, dim3((unsigned)nb), dim3(PACK_THREADS), 0, st, d_flags, (int32_t)m, d_work, d_nodes);
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

// ------------------------------------------------------------------------------------------------------- gather and scatter_add --
template <typename real>
struct MoveRegion {
  const real* src;
  real* dst;
  int64_t first;      // number of the region's first unit
  int32_t w;
  int32_t step;       // elements per unit: V (whole 16-byte vectors: w % V == 0, both pointers aligned) or 1
  int32_t full_mw;    // m w
  int32_t sel_mw;     // n_sel w
  int32_t unit_f;     // f == 1: a plain add
  real f;
};

template <typename real>
struct MoveArgs {
  MoveRegion<real> r[WISKI_STATS_MAX_REGIONS];
  int32_t count;
  int32_t m;
  int32_t src_full;   // scatter_add: src is a full region, read where dst is written
  int64_t units;
  const int32_t* nodes;
  int32_t* err;
};

// dst + f src in two rounded operations
template <typename T>
__device__ __forceinline__ T add_scaled(T d, T s, T f, bool unit_f) {
#pragma clang fp contract(off)
  if (unit_f) return d + s;
  const T p = s * f;
  return d + p;
}

template <typename real, bool SCATTER>
__global__ __launch_bounds__(PACK_THREADS) void k_stats_move(const MoveArgs<real> A) {
  using vec = typename Vec16<real>::type;
  constexpr int V = 16 / (int)sizeof(real);
  __shared__ MoveRegion<real> s_r[WISKI_STATS_MAX_REGIONS];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < WISKI_STATS_MAX_REGIONS; ++i)
      if (i < A.count) s_r[i] = A.r[i];
  }
  __syncthreads();
  const global_ptr<const int32_t> nodes = as_global(A.nodes);
  const int64_t stride = (int64_t)gridDim.x * PACK_THREADS;
  const int last = A.count - 1;
  int reg = 0;                                     // the units of a thread only move forward through the table
  bool bad = false;
  for (int64_t u0 = (int64_t)blockIdx.x * PACK_THREADS + threadIdx.x; u0 < A.units; u0 += stride * PACK_UNROLL) {
    vec a[PACK_UNROLL], b[PACK_UNROLL];            // a: what is read at the source; b (scatter): what the destination holds
    real* to[PACK_UNROLL];
    real f[PACK_UNROLL];
    int kind[PACK_UNROLL];                         // 0: nothing, 1: one element, 2: a vector; + 4: f == 1
#pragma unroll
    for (int j = 0; j < PACK_UNROLL; ++j) {
      const int64_t u = u0 + j * stride;
      kind[j] = 0;
      if (u >= A.units) continue;
      while (reg < last && u >= s_r[reg + 1].first) ++reg;
      const MoveRegion<real>& R = s_r[reg];
      const int32_t e = (int32_t)(u - R.first) * R.step;          // compact element (k n_sel w < 2^31)
      const int32_t c = e / R.sel_mw, rem = e - c * R.sel_mw;
      const int32_t jn = rem / R.w, s = rem - jn * R.w;
      const int32_t node = nodes[jn];
      if (node < 0 || node >= A.m) {               // never dereferenced
        bad = true;
        continue;
      }
      const int32_t full = c * R.full_mw + node * R.w + s;        // (k m w < 2^31)
      const real* from = R.src + (SCATTER && !A.src_full ? e : full);
      to[j] = R.dst + (SCATTER ? full : e);
      f[j] = R.f;
      if (R.step == V) {
        a[j] = *as_global(reinterpret_cast<const vec*>(from));
        if (SCATTER) b[j] = *as_global(reinterpret_cast<const vec*>(to[j]));
        kind[j] = 2 | (R.unit_f ? 4 : 0);
      } else {
        a[j][0] = *as_global(from);
        if (SCATTER) b[j][0] = *as_global((const real*)to[j]);
        kind[j] = 1 | (R.unit_f ? 4 : 0);
      }
    }
#pragma unroll
    for (int j = 0; j < PACK_UNROLL; ++j) {
      const bool unit_f = (kind[j] & 4) != 0;
      if ((kind[j] & 3) == 2) {
        vec o = a[j];
        if (SCATTER) {
#pragma unroll
          for (int e = 0; e < V; ++e) o[e] = add_scaled<real>(b[j][e], a[j][e], f[j], unit_f);
        }
        *as_global(reinterpret_cast<vec*>(to[j])) = o;
      } else if ((kind[j] & 3) == 1) {
        *as_global(to[j]) = SCATTER ? add_scaled<real>(b[j][0], a[j][0], f[j], unit_f) : a[j][0];
      }
    }
  }
  if (bad && A.err) atomicOr(A.err, 1);
}

inline bool overlap(const void* a, int64_t na, const void* b, int64_t nb) {
  return (uintptr_t)a < (uintptr_t)b + (uint64_t)nb && (uintptr_t)b < (uintptr_t)a + (uint64_t)na;
}

template <typename real, bool SCATTER>
int stats_move_impl(const wiski_stats_plan* plan, int64_t m, const int32_t* d_nodes, int64_t n_sel, int32_t src_full, int32_t* d_err, void* stream) {
  constexpr int V = 16 / (int)sizeof(real);
  if (!plan || plan->count < 0 || plan->count > WISKI_STATS_MAX_REGIONS) return WISKI_E_BADARG;
  if (m < 1 || m >= ((int64_t)1 << 31) || n_sel < 0 || n_sel > m) return WISKI_E_BADARG;
  if (d_err && ((uintptr_t)d_err % sizeof(int32_t))) return WISKI_E_BADARG;
  if (!SCATTER && src_full) return WISKI_E_BADARG;
  if (n_sel > 0 && (!d_nodes || ((uintptr_t)d_nodes % sizeof(int32_t)))) return WISKI_E_BADARG;
  MoveArgs<real> A;
  A.count = 0;
  A.units = 0;
  A.m = (int32_t)m;
  A.src_full = src_full ? 1 : 0;
  A.nodes = d_nodes;
  A.err = d_err;
  for (int i = 0; i < plan->count; ++i) {
    const real* src = (const real*)plan->src[i];
    real* dst = (real*)plan->dst[i];
    const int64_t k = plan->k[i], w = plan->w[i];
    const double fac = plan->factor[i];
    if (!src || !dst || ((uintptr_t)src % sizeof(real)) || ((uintptr_t)dst % sizeof(real))) return WISKI_E_BADARG;
    if (!region_fits(k, m, w)) return WISKI_E_BADARG;
    if (SCATTER && !(fac == fac)) return WISKI_E_BADARG;           // (NaN)
    const int64_t n_full = k * m * w, n_sel_el = k * n_sel * w;
    const int64_t n_src = (SCATTER && !A.src_full) ? n_sel_el : n_full, n_dst = SCATTER ? n_full : n_sel_el;
    if (overlap(src, n_src * (int64_t)sizeof(real), dst, n_dst * (int64_t)sizeof(real))) return WISKI_E_BADARG;
    if (d_nodes && (overlap(d_nodes, n_sel * 4, dst, n_dst * (int64_t)sizeof(real)))) return WISKI_E_BADARG;
    if (n_sel == 0) continue;
    MoveRegion<real>& R = A.r[A.count++];
    R.src = src;
    R.dst = dst;
    R.w = (int32_t)w;
    R.full_mw = (int32_t)(m * w);
    R.sel_mw = (int32_t)(n_sel * w);
    R.f = SCATTER ? (real)fac : (real)1;                           // rounded ONCE to the working precision
    R.unit_f = R.f == (real)1;
    const bool vec_ok = (w % V == 0) && ((uintptr_t)src % 16 == 0) && ((uintptr_t)dst % 16 == 0);
    R.step = vec_ok ? V : 1;
    R.first = A.units;
    A.units += n_sel_el / R.step;
  }
  if (A.units == 0) return WISKI_OK;                               // n_sel == 0 launches nothing
  const int64_t per_block = (int64_t)PACK_THREADS * PACK_UNROLL;
  int64_t blocks = (A.units + per_block - 1) / per_block;
  blocks = blocks > PACK_MAX_BLOCKS ? PACK_MAX_BLOCKS : blocks;
  hipLaunchKernelGGL((k_stats_move<real, SCATTER>), dim3((unsigned)blocks), dim3(PACK_THREADS), 0, (hipStream_t)stream, A);
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

}  // namespace

extern "C" {
int wiski_stats_select_f32(const wiski_stats_plan* plan, int64_t m, int32_t* d_flags, int32_t* d_nodes, int32_t* d_count, int32_t* d_work,
                           int64_t work_elems, void* stream) {
  return stats_select_impl<float>(plan, m, d_flags, d_nodes, d_count, d_work, work_elems, stream);
}
int wiski_stats_select_f64(const wiski_stats_plan* plan, int64_t m, int32_t* d_flags, int32_t* d_nodes, int32_t* d_count, int32_t* d_work,
                           int64_t work_elems, void* stream) {
  return stats_select_impl<double>(plan, m, d_flags, d_nodes, d_count, d_work, work_elems, stream);
}
int wiski_stats_gather_f32(const wiski_stats_plan* plan, int64_t m, const int32_t* d_nodes, int64_t n_sel, int32_t* d_err, void* stream) {
  return stats_move_impl<float, false>(plan, m, d_nodes, n_sel, 0, d_err, stream);
}
int wiski_stats_gather_f64(const wiski_stats_plan* plan, int64_t m, const int32_t* d_nodes, int64_t n_sel, int32_t* d_err, void* stream) {
  return stats_move_impl<double, false>(plan, m, d_nodes, n_sel, 0, d_err, stream);
}
int wiski_stats_scatter_add_f32(const wiski_stats_plan* plan, int64_t m, const int32_t* d_nodes, int64_t n_sel, int32_t src_full, int32_t* d_err,
                                void* stream) {
  return stats_move_impl<float, true>(plan, m, d_nodes, n_sel, src_full, d_err, stream);
}
int wiski_stats_scatter_add_f64(const wiski_stats_plan* plan, int64_t m, const int32_t* d_nodes, int64_t n_sel, int32_t src_full, int32_t* d_err,
                                void* stream) {
  return stats_move_impl<double, true>(plan, m, d_nodes, n_sel, src_full, d_err, stream);
}
}
