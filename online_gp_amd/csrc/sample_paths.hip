// Probe vectors for posterior sample paths: P[m][S] += sum_i sqrt(wa_i) eps_{i,s} w(x_i).
//
// One workgroup per point.  The point's per-dim stencils and its S scaled normals are staged in LDS (both in fp64: the
// generator is part of the ABI, include/wiski.h, and a host implementation must be able to reproduce the increments), then
// the 4^d taps x S probes are walked with lanes over s: P is probe-minor, so a wave's 64 fire-and-forget atomics cover
// 64 consecutive reals -- 4 taps of the innermost dim x 16 probes, or one tap x 64 probes -- which is the shape the
// memory-side atomic units want (256 contiguous bytes per wave instruction in fp32).
//
// No fused multiply-adds in this file: the increments are DEFINED by their IEEE fp64 operation sequence (include/wiski.h), and
// the cubic's weights near their zeros are differences of O(1) intermediates -- a contraction the host cannot repeat would move
// them by far more than one rounding of the result.
#pragma clang fp contract(off)
#include "wiski_common.h"

namespace {

constexpr int PROBES_MAX = 1024;       // S normals of one point in LDS (8 KB)
constexpr int PROBE_THREADS = 256;

__device__ __forceinline__ void philox_round(uint32_t c[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
  const uint32_t n1 = (uint32_t)p1;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  const uint32_t n3 = (uint32_t)p0;
  c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

// Philox4x32-10 (Salmon et al., SC'11): counter c, key (k0, k1), ten rounds, the key bumped between rounds.
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// words -> two uniforms in (0, 1] with 53 random bits each -> one Box-Muller pair (include/wiski.h: part of the ABI)
__device__ __forceinline__ void probe_normal_pair(uint64_t index, uint64_t seed, uint32_t pair, double* n0, double* n1) {
  uint32_t c[4] = {(uint32_t)index, (uint32_t)(index >> 32), pair, 0u};
  philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  const double u0 = ((double)(c[0] >> 5) * 67108864.0 + (double)(c[1] >> 6) + 1.0) * (1.0 / 9007199254740992.0);
  const double u1 = ((double)(c[2] >> 5) * 67108864.0 + (double)(c[3] >> 6) + 1.0) * (1.0 / 9007199254740992.0);
  const double r = sqrt(-2.0 * log(u0));
  const double th = 6.283185307179586 * u1;
  *n0 = r * cos(th);
  *n1 = r * sin(th);
}

template <typename real, int D>
__global__ __launch_bounds__(PROBE_THREADS) void k_scatter_probes(GridDev<double> G, GridDev<real> Gr, const real* __restrict__ x, const real* __restrict__ wa, int64_t q,
                                                                  int64_t first_index, uint64_t seed, int S, real* __restrict__ P,
                                                                  int32_t* __restrict__ err) {
  constexpr int T = 1 << (2 * D);
  __shared__ double s_w[D][4];
  __shared__ int s_j0[D];
  __shared__ int s_ok;
  __shared__ double s_tapw[T];
  __shared__ int s_tapi[T];
  __shared__ double s_nrm[PROBES_MAX];
  const int tid = threadIdx.x;
  for (int64_t p = blockIdx.x; p < q; p += gridDim.x) {
    if (tid == 0) s_ok = 1;
    __syncthreads();
    if (tid < D) {
      double w[4];
      // inside / outside is the ABSORB's verdict: taken in the working precision against the grid as GridDev<real> rounds it, so that a
      // point enters P exactly when it enters A.  A point the absorb accepts within an ulp outside the fp64 grid is moved onto the edge
      // (it is in a one-hot boundary cell either way: weight 1 on the edge node)
      const real xr = x[p * D + tid];
      const bool inside = xr >= Gr.g0[tid] && xr <= Gr.hi[tid];
      double xd = (double)xr;
      xd = xd < G.g0[tid] ? G.g0[tid] : (xd > G.hi[tid] ? G.hi[tid] : xd);
      const int j = dim_stencil<double>(xd, G.g0[tid], G.h[tid], G.hi[tid], G.g[tid], w);
      if (!inside || j < 0) s_ok = 0;
      s_j0[tid] = j < 0 ? 0 : j;
#pragma unroll
      for (int c = 0; c < 4; ++c) s_w[tid][c] = w[c];
    }
    const double sw = wa ? sqrt((double)wa[p]) : 1.0;
    for (int j = tid; j < S / 2; j += PROBE_THREADS) {
      double n0, n1;
      probe_normal_pair((uint64_t)(first_index + p), seed, (uint32_t)j, &n0, &n1);
      s_nrm[2 * j] = sw * n0;
      s_nrm[2 * j + 1] = sw * n1;
    }
    __syncthreads();
    const bool ok = s_ok != 0;
    if (ok) {
      for (int t = tid; t < T; t += PROBE_THREADS) {
        double w = 1.0;
        int idx = 0;
#pragma unroll
        for (int d_ = 0; d_ < D; ++d_) {
          const int c = (t >> (2 * (D - 1 - d_))) & 3;
          w *= s_w[d_][c];
          idx += (s_j0[d_] + c) * G.stride[d_];
        }
        s_tapw[t] = w;
        s_tapi[t] = idx;
      }
    } else if (tid == 0) {
      atomicOr(err, 1);                  // outside the grid: the point contributes nothing (as in the absorb, which counts it)
    }
    __syncthreads();
    if (ok) {
      const int total = T * S;
      for (int e = tid; e < total; e += PROBE_THREADS) {
        const int t = e / S, s = e - t * S;
        const double w = s_tapw[t];
        if (w != 0.0) atomic_add_real(P + (int64_t)s_tapi[t] * S + s, (real)(w * s_nrm[s]));
      }
    }
    __syncthreads();
  }
}

template <typename real>
int scatter_probes_impl(const wiski_grid* grid, const real* d_x, const real* d_wa, int64_t q, int64_t first_index, uint64_t seed, int32_t S,
                        real* d_P, int32_t* d_err, void* stream) {
  GridDev<double> G;
  int rc = make_grid_dev<double>(grid, &G);
  if (rc != WISKI_OK) return rc;
  GridDev<real> Gr;
  rc = make_grid_dev<real>(grid, &Gr);
  if (rc != WISKI_OK) return rc;
  if (!d_x || !d_P || !d_err || q < 0 || first_index < 0 || S < 2 || (S & 1) || S > PROBES_MAX) return WISKI_E_BADARG;
  if ((int64_t)G.m * S >= ((int64_t)1 << 40)) return WISKI_E_BADARG;
  if (q == 0) return WISKI_OK;
  const unsigned blocks = (unsigned)(q < (int64_t)1 << 20 ? q : (int64_t)1 << 20);
#define CALL(DD) \
  hipLaunchKernelGGL((k_scatter_probes<real, DD>), dim3(blocks), dim3(PROBE_THREADS), 0, (hipStream_t)stream, G, Gr, d_x, d_wa, q, first_index, seed, (int)S, d_P, d_err)
  WISKI_DISPATCH_D(G.d, CALL)
#undef CALL
  WISKI_LAUNCH_CHECK();
  return WISKI_OK;
}

}  // namespace

extern "C" {
int wiski_scatter_probes_f32(const wiski_grid* grid, const float* d_x, const float* d_wa, int64_t q, int64_t first_index, uint64_t seed, int32_t S,
                             float* d_P, int32_t* d_err, void* stream) {
  return scatter_probes_impl<float>(grid, d_x, d_wa, q, first_index, seed, S, d_P, d_err, stream);
}
int wiski_scatter_probes_f64(const wiski_grid* grid, const double* d_x, const double* d_wa, int64_t q, int64_t first_index, uint64_t seed, int32_t S,
                             double* d_P, int32_t* d_err, void* stream) {
  return scatter_probes_impl<double>(grid, d_x, d_wa, q, first_index, seed, S, d_P, d_err, stream);
}
}
