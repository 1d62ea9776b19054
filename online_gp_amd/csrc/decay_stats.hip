// Exponential forgetting: x <- f x, in place, over a small table of regions in ONE launch -- the half-stencil pack,
// b, cnt (f = gamma) and the probe vectors (f = sqrt(gamma)) -- plus the carried PCG residual R <- gamma R - (1 - gamma) Z and, by one
// thread of block 0 in fp64, stats[o] <- (gamma stats[o][0], stats[o][1] - n_o log gamma) and gamma times a few fp64 side scalars.
//
// The kernel is a read + write stream: every region is cut into 16-byte vectors on its aligned body and one "edge" unit that
// holds the up to V - 1 elements before the first and after the last aligned vector (views such as pack[o] or rows of an [out, m]
// tensor with odd m start off a 16-byte boundary as a rule).  The units of all regions are numbered consecutively and walked
// grid-stride, DECAY_UNROLL units per thread and pass with the loads of all its vectors issued before the first store; consecutive
// lanes hold consecutive units, so a wave instruction moves 1 KiB.  The edge unit is the exception: its lane updates the up to
// 2 (V - 1) elements one after the other, load and store, where it meets it (one lane per region and launch: at most 9).
// Plain loads and stores only: no atomics, no workspace.
//
// Pure scalings are ONE multiplication by the factor rounded once to the working precision, i.e. correctly rounded products
// (nothing here for the compiler to contract); the residual line may become a fused multiply-add.
#include <math.h>

#include "wiski_common.h"

namespace {

constexpr int DECAY_THREADS = 256;
constexpr int DECAY_UNROLL = 4;
constexpr int DECAY_MAX_BLOCKS = 2048;                      // 256 CUs x 8 blocks, the rest by grid stride
constexpr int DECAY_SLOTS = WISKI_DECAY_MAX_REGIONS + 1;    // the table's regions + the residual

template <typename real>
struct DecayRegion {
  real* ptr;          // first element of the region
  const real* z;      // residual region: Z (then x <- f x - g z); else NULL
  int64_t n;          // elements
  int64_t nvec;       // 16-byte vectors of the aligned body
  int64_t first;      // number of the region's first unit; its units are nvec vectors, then the edge unit if head + tail > 0
  int32_t head;       // elements before the first aligned vector
  int32_t z_vec;      // Z may be read with vector loads (same 16-byte phase as ptr)
  real f, g;
};

template <typename real>
struct DecayArgs {
  DecayRegion<real> r[DECAY_SLOTS];
  int32_t count;
  int32_t nout;                                   // rows of stats
  int64_t units;                                  // all regions together
  double* stats;                                  // [nout][2] or NULL
  double* side;                                   // fp64 scalars scaled by gamma, or NULL
  int32_t nside;
  double gamma;
  double shift[WISKI_DECAY_MAX_OUTPUTS];          // - n_o log gamma
};

// The table travels through LDS, where a pointer loses its address space and every access would become a flat one (which also
// waits on the LDS counter): say that these are global addresses.
template <typename T>
using global_ptr = __attribute__((address_space(1))) T*;
template <typename T>
__device__ __forceinline__ global_ptr<T> as_global(T* p) { return (global_ptr<T>)p; }

// 16 bytes of reals as a native vector (element-wise arithmetic, a scalar operand is broadcast)
template <typename real>
struct Vec16;
template <>
struct Vec16<float> { typedef float type __attribute__((ext_vector_type(4))); };
template <>
struct Vec16<double> { typedef double type __attribute__((ext_vector_type(2))); };

template <typename real>
__global__ __launch_bounds__(DECAY_THREADS) void k_decay_stats(const DecayArgs<real> A) {
  using vec = typename Vec16<real>::type;
  constexpr int V = 16 / (int)sizeof(real);
  __shared__ DecayRegion<real> s_r[DECAY_SLOTS];
  if (threadIdx.x == 0) {                          // (constant indices: the table is read from the kernel arguments, not from a scratch copy)
#pragma unroll
    for (int i = 0; i < DECAY_SLOTS; ++i)
      if (i < A.count) s_r[i] = A.r[i];
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    for (int o = 0; o < A.nout; ++o) {
      A.stats[2 * o] *= A.gamma;                   // y^T D^-1 y
      A.stats[2 * o + 1] += A.shift[o];            // log|D| of the inflated noise d_i / gamma
    }
    for (int j = 0; j < A.nside; ++j) A.side[j] *= A.gamma;
  }
  const int64_t stride = (int64_t)gridDim.x * DECAY_THREADS;
  const int last = A.count - 1;
  int reg = 0;                                     // the units of a thread only move forward through the table
  for (int64_t u0 = (int64_t)blockIdx.x * DECAY_THREADS + threadIdx.x; u0 < A.units; u0 += stride * DECAY_UNROLL) {
    vec v[DECAY_UNROLL], z[DECAY_UNROLL];
    real* dst[DECAY_UNROLL];
    real f[DECAY_UNROLL], g[DECAY_UNROLL];
    int kind[DECAY_UNROLL];                        // 0: nothing to store, 1: scaled vector, 2: residual vector
#pragma unroll
    for (int j = 0; j < DECAY_UNROLL; ++j) {
      const int64_t u = u0 + j * stride;
      kind[j] = 0;
      if (u >= A.units) continue;
      while (reg < last && u >= s_r[reg + 1].first) ++reg;
      const DecayRegion<real>& R = s_r[reg];
      const int64_t loc = u - R.first;
      f[j] = R.f;
      g[j] = R.g;
      if (loc < R.nvec) {
        dst[j] = R.ptr + R.head + loc * V;
        v[j] = *as_global(reinterpret_cast<const vec*>(dst[j]));
        kind[j] = 1;
        if (R.z) {
          const real* zp = R.z + R.head + loc * V;
          if (R.z_vec) {
            z[j] = *as_global(reinterpret_cast<const vec*>(zp));
          } else {
#pragma unroll
            for (int e = 0; e < V; ++e) z[j][e] = as_global(zp)[e];
          }
          kind[j] = 2;
        }
      } else {
        // the edge unit: [0, head) and [head + nvec V, n), element by element and in place, here in the load phase (at most 2 (V - 1)
        // dependent load / store pairs in one lane of the launch's at most 9 such units)
        const int64_t tail0 = R.head + R.nvec * V;
        const global_ptr<real> xe = as_global(R.ptr);
        const global_ptr<const real> ze = as_global(R.z);
        for (int64_t e = 0; e < R.head; ++e) xe[e] = R.z ? R.f * xe[e] - R.g * ze[e] : xe[e] * R.f;
        for (int64_t e = tail0; e < R.n; ++e) xe[e] = R.z ? R.f * xe[e] - R.g * ze[e] : xe[e] * R.f;
      }
    }
#pragma unroll
    for (int j = 0; j < DECAY_UNROLL; ++j) {
      if (kind[j] == 1) {
        *as_global(reinterpret_cast<vec*>(dst[j])) = v[j] * f[j];
      } else if (kind[j] == 2) {
        *as_global(reinterpret_cast<vec*>(dst[j])) = f[j] * v[j] - g[j] * z[j];
      }
    }
  }
}

template <typename real>
int add_region(DecayArgs<real>* A, real* ptr, const real* z, int64_t n, double f, double g) {
  if (n < 0) return WISKI_E_BADARG;
  if (n == 0) return WISKI_OK;
  if (!ptr || ((uintptr_t)ptr % sizeof(real)) || (z && ((uintptr_t)z % sizeof(real)))) return WISKI_E_BADARG;
  if (!(f > 0.0) || !(f <= 1.0)) return WISKI_E_BADARG;
  constexpr int V = 16 / (int)sizeof(real);
  DecayRegion<real>& R = A->r[A->count++];
  R.ptr = ptr;
  R.z = z;
  R.n = n;
  int64_t head = (int64_t)((16 - (uintptr_t)ptr % 16) % 16 / sizeof(real));
  if (head > n) head = n;
  R.head = (int32_t)head;
  R.nvec = (n - head) / V;
  R.z_vec = z && ((uintptr_t)z % 16 == (uintptr_t)ptr % 16);
  R.first = A->units;
  R.f = (real)f;                                    // rounded ONCE to the working precision
  R.g = (real)g;
  A->units += R.nvec + ((R.nvec * V != n) ? 1 : 0);
  return WISKI_OK;
}

template <typename real>
int decay_stats_impl(const wiski_decay_plan* plan, double gamma, real* d_R, const real* d_Z, int64_t n_res, double* d_stats, int32_t nout,
                     const double* h_count, double* d_side, int32_t nside, void* stream) {
  if (!(gamma > 0.0) || !(gamma <= 1.0)) return WISKI_E_BADARG;          // (NaN fails both comparisons)
  if (!plan || plan->count < 0 || plan->count > WISKI_DECAY_MAX_REGIONS) return WISKI_E_BADARG;
  if (nout < 0 || nout > WISKI_DECAY_MAX_OUTPUTS || (nout > 0 && (!d_stats || !h_count))) return WISKI_E_BADARG;
  if (nside < 0 || nside > WISKI_DECAY_MAX_OUTPUTS || (nside > 0 && !d_side)) return WISKI_E_BADARG;
  if ((d_R == nullptr) != (d_Z == nullptr) || n_res < 0) return WISKI_E_BADARG;
  if (gamma == 1.0) return WISKI_OK;                                      // nothing moves: no launch
  DecayArgs<real> A;
  A.count = 0;
  A.units = 0;
  for (int i = 0; i < plan->count; ++i) {
    const int rc = add_region<real>(&A, (real*)plan->ptr[i], nullptr, plan->n[i], plan->factor[i], 0.0);
    if (rc != WISKI_OK) return rc;
  }
  if (d_R) {
    const int rc = add_region<real>(&A, d_R, d_Z, n_res, gamma, 1.0 - gamma);
    if (rc != WISKI_OK) return rc;
  }
  A.stats = d_stats;
  A.nout = nout;
  A.side = d_side;
  A.nside = nside;
  A.gamma = gamma;
  const double lg = log(gamma);
  for (int o = 0; o < WISKI_DECAY_MAX_OUTPUTS; ++o) A.shift[o] = o < nout ? -h_count[o] * lg : 0.0;
  if (A.units == 0 && nout == 0 && nside == 0) return WISKI_OK;
  const int64_t per_block = (int64_t)DECAY_THREADS * DECAY_UNROLL;
  int64_t blocks = (A.units + per_block - 1) / per_block;
  blocks = blocks < 1 ? 1 : (blocks > DECAY_MAX_BLOCKS ? DECAY_MAX_BLOCKS : blocks);
  hipLaunchKernelGGL((k_decay_stats<real>), dim3((unsigned)blocks), dim3(DECAY_THREADS), 0, (hipStream_t)stream, A);
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

}  // namespace

extern "C" {
int wiski_decay_stats_f32(const wiski_decay_plan* plan, double gamma, float* d_R, const float* d_Z, int64_t n_res, double* d_stats, int32_t nout,
                          const double* h_count, double* d_side, int32_t nside, void* stream) {
  return decay_stats_impl<float>(plan, gamma, d_R, d_Z, n_res, d_stats, nout, h_count, d_side, nside, stream);
}
int wiski_decay_stats_f64(const wiski_decay_plan* plan, double gamma, double* d_R, const double* d_Z, int64_t n_res, double* d_stats, int32_t nout,
                          const double* h_count, double* d_side, int32_t nside, void* stream) {
  return decay_stats_impl<double>(plan, gamma, d_R, d_Z, n_res, d_stats, nout, h_count, d_side, nside, stream);
}
}
