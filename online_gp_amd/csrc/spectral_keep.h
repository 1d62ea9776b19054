// Truncated form of the fused fp32 preconditioner (one column, d = 3): transform only the eigenmodes that matter.
// Included by spectral.hip (uses its spec_f32x4, TwoLevelDev and KS dispatch); entered through launch_spectral_fused_cg when
// `keep` counts are given.
//
// The separable model scales mode (k0, k1, k2) of the t-half by f = 1 / (1 + a lam) = 1 - w and of the y-half by lam f = w / a,
// w = a lam / (1 + a lam).  For a smooth prior on a grid much finer than its lengthscale the per-dimension eigenvalues fall off
// super-exponentially, so all but a small box of modes -- the last K_q columns of every eigen table (eigenvalues ascend) --
// have w below 2^-30: there the t-half is the identity and the y-half zero to 64 times less than an fp32 ulp.  With X_L, Z_L the
// Kronecker products of the kept columns of evec / evec2 and c = X_L^T r (a K0 x K1 x K2 cube):
//     y = X_L cy,   t = r - Z_L ct,     cy = lam f c,  ct = w c       (w formed directly, never as 1 - f)
//     two-level block (its r modes lie inside the box):  cy_S = N c_S,  ct_S = c_S - D_S^-1 N c_S
//     rho = sum cy . c
// The identity on the dropped modes of t is essential: Z = Kt^-1 U converges on the rough modes only through it (Z X^T = I).
//
// Two launches, and no workgroup ever waits on another (the slab kernel's exchange of the block's coefficients between
// co-resident workgroups is gone: every backward workgroup holds the whole cube):
//   k_keep_fwd  (g0 x 2 workgroups, a contiguous half slab of r each): every duty of k_spec_mode0_mfma<.., 2> -- the previous
//               iteration's u / z / r update, the norms, the ring clear; at the head of a carried solve also the fold of the
//               absorb's tap stage into b, cnt and r (each element has exactly one owner: plain stores) -- then T[i0] = X1_L^T R[i0] X2_L of the updated slab; the
//               two halves of a slab write their partial sums side by side
//   k_keep_bwd  (g0 workgroups of 16 waves): c[k0] = sum_i0 X0[i0, k0] T[i0] straight from the partial sums, scaling, the block's
//               N c_S, rho (workgroup 0), this slab's row of mode 0 backward, Y = X1_L S_y X2_L^T and the t-correction with Z1, Z2,
//               p = y + beta p, pt = (r - correction) + beta pt; the r / p / pt loads are in flight under all but the first product
// (The middle as a launch of its own -- one workgroup, S_y / S_t through memory -- was built first and measured: 10.6 us without
//  and 15.2 us with the block for that launch, 26.8 us per application against 24.3 us for the full transforms.)
// All LDS images are zero padded, so the padded MFMA products are exact (as in spectral.hip).
#pragma once

constexpr int KEEP_MAX = 24;                        // cap of a kept count (a multiple of 4 each)
constexpr int KEEP_NS = 2;                          // forward / backward workgroups per slab
constexpr int KEEP_LDK = 48;                        // row stride of an image whose 16-lane groups read a row (the 4 k-rows of a step on disjoint bank quarters)
constexpr int KEEP_LDC = 36;                        // row stride of an image whose lanes walk a column (36 l mod 64: 16 distinct multiples of 4)
constexpr size_t KEEP_LDS_BUDGET = 144 * 1024;      // dynamic LDS the backward kernel may ask for

struct KeepDev {
  int K[3];   // kept modes per dimension
  int o[3];   // first kept column of the eigen tables: g_q - K_q
};

// row stride of the [k0][k1 k2] coefficient cubes: K1 K2 (a multiple of 16) made 16 or 48 mod 64
__host__ __device__ static inline int keep_cube_ld(int KK) { return (KK % 64 == 16 || KK % 64 == 48) ? KK : KK + 16; }
// dynamic LDS of k_keep_bwd: the X0 / Z0 images, the two cubes (or the output slab that later lies there), S, the images of dims 1
// and 2, the eigenvalues, the block's scratch
static inline size_t keep_bwd_lds(const int* K, bool tl) {
  const int ksk = (K[0] > 16 || K[1] > 16 || K[2] > 16) ? 6 : 4;
  const size_t cubes = (size_t)2 * 4 * ksk * keep_cube_ld(K[1] * K[2]), slab = 2 * 64 * SPEC_LDN;
  return ((size_t)64 * KEEP_LDK + 2 * 64 * KEEP_LDC + (cubes > slab ? cubes : slab) + 2 * 32 * KEEP_LDC + 4 * 64 * KEEP_LDC + 96 +
          (tl ? 4 * SPEC_TL_MAXR + 80 : 0)) * sizeof(float);
}
constexpr size_t KEEP_FWD_LDS = (size_t)(64 * SPEC_LDN + 3 * 64 * KEEP_LDK) * sizeof(float);

// Would a solve on G accept these counts?  (all zero = "full path" is not a kept set: false)
static bool keep_counts_ok(const GridDev<float>& G, const int* K, bool tl) {
  if (G.d != 3 || G.stride[0] % 4 != 0) return false;
  for (int q = 0; q < 3; ++q)
    if (G.g[q] > 64 || K[q] < 4 || K[q] % 4 != 0 || K[q] > KEEP_MAX || K[q] > G.g[q]) return false;
  return keep_bwd_lds(K, tl) <= KEEP_LDS_BUDGET;
}

// one 16 x 16 output tile, KS steps of 4: A(x, b) at pa[x sax + b sab], B(b, y) at pb[b sbb + y sby]; every operand word is read
// up front (spec_mfma_product)
template <int KS>
__device__ __forceinline__ spec_f32x4 keep_tile(const float* __restrict__ pa, int sax, int sab, const float* __restrict__ pb, int sbb, int sby, int lane) {
  const int l15 = lane & 15, l4 = lane >> 4;
  const float* qa = pa + l15 * sax + l4 * sab;
  const float* qb = pb + l4 * sbb + l15 * sby;
  float af[KS], bf[KS];
#pragma unroll
  for (int i = 0; i < KS; ++i) {
    af[i] = qa[4 * i * sab];
    bf[i] = qb[4 * i * sbb];
  }
  spec_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < KS; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[i], acc, 0, 0, 0);
  return acc;
}

// the kept columns [o, o + K) of a g x g eigen table -> registers, for an LDS image of 64 rows x W columns (W = 16 or 32, zero
// padded): element (row, col) of pass j is thread t + NT j
template <int W, int NT = 256>
struct KeepCols {
  static constexpr int NP = 64 * W / NT;
  float v[NP];
  __device__ __forceinline__ void issue(const float* __restrict__ M, int g, int o, int K) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int idx = (int)threadIdx.x + NT * j, row = idx / W, col = idx % W;
      const bool ok = row < g && col < K;
      const float x = M[ok ? row * g + o + col : 0];
      v[j] = ok ? x : 0.f;
    }
  }
  __device__ __forceinline__ void commit(float* __restrict__ dst, int ld) const {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
      const int idx = (int)threadIdx.x + NT * j;
      dst[(idx / W) * ld + idx % W] = v[j];
    }
  }
};

// the flat float4 range of a slab that workgroup h of KEEP_NS owns
__device__ __forceinline__ void keep_range(int n4, int h, int* lo, int* hi) {
  const int per = (n4 + KEEP_NS - 1) / KEEP_NS;
  *lo = h * per;
  *hi = *lo + per < n4 ? *lo + per : n4;
}

// ------------------------------------------------------------------ forward ---
template <int KS, int W>
__global__ __launch_bounds__(256) void k_keep_fwd(GridDev<float> G, KeepDev kp, const float* __restrict__ X1, const float* __restrict__ X2,
                                                  float* __restrict__ r, float* __restrict__ T, int it, int apply, double tol2,
                                                  const float* __restrict__ p, const float* __restrict__ pt, PcgScal S,
                                                  float* __restrict__ part, int nch, int zl, float* __restrict__ u, float* __restrict__ z,
                                                  float* __restrict__ stage, float* __restrict__ bw, float* __restrict__ cnt) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double s_red[16];
  float* sR = reinterpret_cast<float*>(smem);     // R[i1][i2], stride LDN: zero outside this workgroup's half
  float* sX1 = sR + 64 * SPEC_LDN;                // X1_L[i1][k1], stride LDK
  float* sX2 = sX1 + 64 * KEEP_LDK;               // X2_L[i2][k2]
  float* sC = sX2 + 64 * KEEP_LDK;                // C[i1][k2] = R X2_L
  const int g1 = G.g[1], g2 = G.g[2], m = G.m, sl = g1 * g2;
  const int K1 = kp.K[1], K2 = kp.K[2];
  const int i0 = blockIdx.x, h = blockIdx.y;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, l15 = lane & 15, l4 = lane >> 4;
  int lo, hi;
  keep_range(sl >> 2, h, &lo, &hi);
  for (int e = t; e < 64 * SPEC_LDN / 4; e += 256) reinterpret_cast<float4*>(sR)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
  KeepCols<W> c1, c2;
  c1.issue(X1, g1, kp.o[1], K1);
  c2.issue(X2, g2, kp.o[2], K2);
  float al = 0.f;
  if (apply == 1) {
    const double den = S.php_sum(it - 1, 0);
    if (i0 == 0 && h == 0) pcg_dot_clear(S.php(it), 0, 1, S.k);   // ring entry the SpMV of this iteration accumulates into
    if (pcg_active(S, it - 1, 0, tol2) && den > 0) al = (float)(S.rho(it - 1)[0] / den);
  }
  float4 tin[2];
  float rn_part = 0.f, rhs_part = 0.f;
#pragma unroll
  for (int q = 0; q < 2; ++q) {                     // <= 512 float4 per half slab (g <= 64)
    const int f = lo + t + 256 * q;
    const bool ok = f < hi;
    const int64_t e = ok ? (int64_t)i0 * sl + 4 * f : 0;
    tin[q] = *reinterpret_cast<const float4*>(r + e);
    if (!ok) tin[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (apply == 2 && ok) {                         // carried residual: ||r||^2 and ||rhs||^2 (`p` carries the right-hand side)
      float4 f4, rv = tin[q];
      if (stage) {
        // the tap stage (AbsorbArgs::tap_stage): records {delta b, delta cnt, delta res, -} of these four nodes.  bw is the right-hand
        // side again, writable (p is not read: it is the same memory).  Every load is issued before the first use -- cnt too, although
        // only a touched group needs it: behind the test it would be one more trip to memory; a group the batch did not touch stores nothing
        float4 sg[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) sg[j] = *reinterpret_cast<const float4*>(stage + 4 * (e + j));
        f4 = *reinterpret_cast<const float4*>(bw + e);
        float4 cv = *reinterpret_cast<const float4*>(cnt + e);
        unsigned any = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) any |= __float_as_uint(sg[j].x) | __float_as_uint(sg[j].y) | __float_as_uint(sg[j].z);
        if (any) {
          f4.x += sg[0].x; f4.y += sg[1].x; f4.z += sg[2].x; f4.w += sg[3].x;
          cv.x += sg[0].y; cv.y += sg[1].y; cv.z += sg[2].y; cv.w += sg[3].y;
          rv.x += sg[0].z; rv.y += sg[1].z; rv.z += sg[2].z; rv.w += sg[3].z;
          *reinterpret_cast<float4*>(bw + e) = f4;
          *reinterpret_cast<float4*>(cnt + e) = cv;
          *reinterpret_cast<float4*>(r + e) = rv;
#pragma unroll
          for (int j = 0; j < 4; ++j) *reinterpret_cast<float4*>(stage + 4 * (e + j)) = make_float4(0.f, 0.f, 0.f, 0.f);
          tin[q] = rv;
        }
      } else {
        f4 = *reinterpret_cast<const float4*>(p + e);
      }
      rhs_part += f4.x * f4.x + f4.y * f4.y + f4.z * f4.z + f4.w * f4.w;
      rn_part += rv.x * rv.x + rv.y * rv.y + rv.z * rv.z + rv.w * rv.w;
    }
    if (apply == 1 && ok) {                         // u += alpha p; z += alpha pt; r -= alpha (pt + sum_ch part[ch])
      const float4 pv = *reinterpret_cast<const float4*>(p + e), ptv = *reinterpret_cast<const float4*>(pt + e);
      float4 uv = *reinterpret_cast<const float4*>(u + e), zv = *reinterpret_cast<const float4*>(z + e);
      float4 pp[8];
#pragma unroll
      for (int ch = 0; ch < 8; ++ch)
        if (ch < nch) pp[ch] = *reinterpret_cast<const float4*>(part + (int64_t)ch * m + e);
      if (zl) *reinterpret_cast<float4*>(part + (int64_t)(nch - 1) * m + e) = make_float4(0.f, 0.f, 0.f, 0.f);   // consumed: re-zero
      float4 hv = ptv;
#pragma unroll
      for (int ch = 0; ch < 8; ++ch)
        if (ch < nch) { hv.x += pp[ch].x; hv.y += pp[ch].y; hv.z += pp[ch].z; hv.w += pp[ch].w; }
      uv.x += al * pv.x; uv.y += al * pv.y; uv.z += al * pv.z; uv.w += al * pv.w;
      zv.x += al * ptv.x; zv.y += al * ptv.y; zv.z += al * ptv.z; zv.w += al * ptv.w;
      float4 rv = tin[q];
      rv.x -= al * hv.x; rv.y -= al * hv.y; rv.z -= al * hv.z; rv.w -= al * hv.w;
      rn_part += rv.x * rv.x + rv.y * rv.y + rv.z * rv.z + rv.w * rv.w;
      *reinterpret_cast<float4*>(u + e) = uv;
      *reinterpret_cast<float4*>(z + e) = zv;
      *reinterpret_cast<float4*>(r + e) = rv;
      tin[q] = rv;
    }
  }
  if (apply) {                                      // block-uniform
    const double tot = block_reduce_sum((double)rn_part, s_red);
    if (t == 0) unsafeAtomicAdd(S.rn(it), tot);
    if (apply == 2) {
      const double tot0 = block_reduce_sum((double)rhs_part, s_red);
      if (t == 0) unsafeAtomicAdd(S.rn0(), tot0);
    }
  }
  __syncthreads();                                  // the zero fill of sR is complete
  c1.commit(sX1, KEEP_LDK);
  c2.commit(sX2, KEEP_LDK);
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int f = lo + t + 256 * q;
    if (f < hi) {
      const float v[4] = {tin[q].x, tin[q].y, tin[q].z, tin[q].w};
      int row = (4 * f) / g2, col = 4 * f - row * g2;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (col == g2) { col = 0; ++row; }
        sR[row * SPEC_LDN + col] = v[j];
        ++col;
      }
    }
  }
  __syncthreads();
  // C[i1][k2] = sum_i2 R[i1][i2] X2_L[i2][k2]: wave w owns rows [16 w, 16 w + 16) (all four: sC is read in full below)
#pragma unroll
  for (int ct = 0; ct < W / 16; ++ct) {
    const spec_f32x4 acc = keep_tile<KS>(sR + 16 * w * SPEC_LDN, SPEC_LDN, 1, sX2 + 16 * ct, KEEP_LDK, 1, lane);
#pragma unroll
    for (int q = 0; q < 4; ++q) sC[(16 * w + 4 * l4 + q) * KEEP_LDK + 16 * ct + l15] = acc[q];
  }
  __syncthreads();
  // T[k1][k2] = sum_i1 X1_L[i1][k1] C[i1][k2]: at most (W / 16)^2 <= 4 tiles, one per wave
  constexpr int NT1 = W / 16;
  if (w < NT1 * NT1) {
    const int mt = w / NT1, nt = w % NT1;
    const spec_f32x4 acc = keep_tile<KS>(sX1 + 16 * mt, 1, KEEP_LDK, sC + 16 * nt, KEEP_LDK, 1, lane);
    float* __restrict__ out = T + (int64_t)(i0 * KEEP_NS + h) * K1 * K2;
    const int k2 = 16 * nt + l15;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k1 = 16 * mt + 4 * l4 + q;
      if (k1 < K1 && k2 < K2) out[k1 * K2 + k2] = acc[q];
    }
  }
}

// ------------------------------------------------------- middle + backward ---
// One workgroup of 16 waves per slab i0.  Every workgroup forms the WHOLE cube for itself (c = X0_L^T T from the forward partial
// sums, scaling, the block's N c_S): 100 KB of T and the rows of N out of L2 per workgroup, a few hundred MFMAs -- less than the
// launch boundary and the single cold workgroup that a middle launch of its own costs (measured: 15.2 + 6.0 us as two launches).
// Of mode 0 backward it then needs only its own row: S[i0] = sum_k0 X0_L[i0][k0] c[k0].  rho is added by workgroup 0 alone.
// LDS regions are reused once dead: the X0 / Z0 images hold E = S X2_L^T later, the cubes the output slab.
template <int KS0, int KSK, bool TL>
__global__ __launch_bounds__(1024) void k_keep_bwd(GridDev<float> G, KeepDev kp, const float* __restrict__ X0, const float* __restrict__ Z0,
                                                   const float* __restrict__ X1, const float* __restrict__ X2, const float* __restrict__ Z1,
                                                   const float* __restrict__ Z2, const float* __restrict__ evals, float kscale, float shift,
                                                   const float* __restrict__ T, const float* __restrict__ r, float* __restrict__ p,
                                                   float* __restrict__ pt, int it, PcgScal S, double* __restrict__ rho, TwoLevelDev tl) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __shared__ double s_red[16];
  constexpr int KR = 4 * KSK;                      // rows of a coefficient cube (K0 <= KR; rows beyond K0 are exact zeros)
  constexpr int W = KSK == 4 ? 16 : 32;            // columns of the kept-column images of dims 1, 2
  const int g0 = G.g[0], g1 = G.g[1], g2 = G.g[2], sl = g1 * g2, n4 = sl >> 2;
  const int K0 = kp.K[0], K1 = kp.K[1], K2 = kp.K[2], KK = K1 * K2, ldc = keep_cube_ld(KK);
  const int i0 = blockIdx.x;
  float* sXt = reinterpret_cast<float*>(smem);     // X0_L[i0][k0], stride LDK (forward: A^T)
  float* sXn = sXt + 64 * KEEP_LDK;                // X0_L[i0][k0], stride LDC
  float* sZn = sXn + 64 * KEEP_LDC;                // Z0_L[i0][k0]
  float* sEh = sXt;                                // later: [2][32][LDT], E = S X2_L^T, [k1][i2]
  float* sCY = sZn + 64 * KEEP_LDC;                // cy[k0][k1 k2], stride ldc
  float* sCT = sCY + KR * ldc;                     // ct
  float* sO = sCY;                                 // later: [2][64][LDN], y | t-correction of the slab
  const int cube = 2 * KR * ldc > 2 * 64 * SPEC_LDN ? 2 * KR * ldc : 2 * 64 * SPEC_LDN;
  float* sS = sCY + cube;                          // [2][32][LDC]: S_y | S_t of this slab, [k1][k2]
  float* sM = sS + 2 * 32 * KEEP_LDC;              // [4][64][LDC]: X2_L | Z2_L | X1_L | Z1_L, [i][k]
  float* sE = sM + 4 * 64 * KEEP_LDC;              // kept eigenvalues of dims 0 | 1 | 2, 32 each, zero padded
  float* sCs = sE + 96;                            // TL: c_S [r]
  float* sD = sCs + SPEC_TL_MAXR;                  // TL: N c_S [r]
  float* sLam = sD + SPEC_TL_MAXR;                 // TL: lam of the selected modes
  int* sIdx = reinterpret_cast<int*>(sLam + SPEC_TL_MAXR);   // TL: position in the cubes, -1 outside the box
  int* sOff = sIdx + SPEC_TL_MAXR;                 // TL: tl.off [g0 + 1]
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, l15 = lane & 15, l4 = lane >> 4;
  const int nnt = KK / 16, ntile = ((KR + 15) / 16) * nnt;   // every row of the cubes is written (rows beyond K0: exact zeros)
  const int tr = TL ? (tl.r < SPEC_TL_MAXR ? tl.r : SPEC_TL_MAXR) : 0;
  // the vectors of the epilogue: one float4 per thread (g1 g2 / 4 <= 1024), requested behind the forward product (whose operands
  // need the registers) and in flight under everything after it
  const bool v_ok = t < n4;
  const int64_t ve = (int64_t)i0 * sl + (v_ok ? 4 * t : 0);
  KeepCols<W, 1024> cx2, cz2, cx1, cz1;            // the kept columns of dims 1 and 2
  cx2.issue(X2, g2, kp.o[2], K2);
  cz2.issue(Z2, g2, kp.o[2], K2);
  cx1.issue(X1, g1, kp.o[1], K1);
  cz1.issue(Z1, g1, kp.o[1], K1);
  for (int e = t; e < 2 * 32 * KEEP_LDC / 4; e += 1024) reinterpret_cast<float4*>(sS)[e] = make_float4(0.f, 0.f, 0.f, 0.f);
  // nothing below depends on another load: the mode positions (thread e holds mode e: r <= 512 < 1024), the slab offsets, the kept
  // columns of X0 / Z0 (thread t = (row, col) of two 32 x 32 passes) and the kept eigenvalues are in flight with the first tile's operand
  unsigned ppos = 0;
  if constexpr (TL) {
    if (t < tr) ppos = tl.pos[t];
    if (t <= g0) sOff[t] = tl.off[t];
  }
  float xi[2], zi[2], ev = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = t + 1024 * j, row = idx >> 5, col = idx & 31;
    const bool ok = row < g0 && col < K0;
    const float x = X0[ok ? row * g0 + kp.o[0] + col : 0], zv = Z0[ok ? row * g0 + kp.o[0] + col : 0];
    xi[j] = ok ? x : 0.f;
    zi[j] = ok ? zv : 0.f;
  }
  if (t < 96) {
    const int q = t >> 5, j = t & 31;
    const int base = q == 0 ? kp.o[0] : (q == 1 ? g0 + kp.o[1] : g0 + g1 + kp.o[2]);
    const bool ok = j < (q == 0 ? K0 : (q == 1 ? K1 : K2));
    const float e = evals[ok ? base + j : 0];
    ev = ok ? e : 0.f;
  }
  // the B operand of a forward tile straight from the partial sums: b[i] = sum_h T[4 i + l4][h][n]
  float bf[KS0];
  unsigned long long mrow[4];
  auto load_b = [&](int tile) {
    const int mt = tile / nnt, n = 16 * (tile - mt * nnt) + l15;
#pragma unroll
    for (int i = 0; i < KS0; ++i) {
      const int b0 = 4 * i + l4;
      const bool ok = b0 < g0;
      const float* q = T + (int64_t)(ok ? b0 : 0) * KEEP_NS * KK + n;
      float v = q[0];
#pragma unroll
      for (int hh = 1; hh < KEEP_NS; ++hh) v += q[hh * KK];
      bf[i] = ok ? v : 0.f;
    }
    if constexpr (TL) {
      const int k1 = n / K2;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int k0 = 16 * mt + 4 * l4 + q;
        mrow[q] = k0 < K0 ? tl.mask[(kp.o[0] + k0) * 64 + kp.o[1] + k1] : 0ull;
      }
    }
  };
  int tile = w;
  if (tile < ntile) load_b(tile);
  // two-level: this wave's rows of N (e = w, w + 16, ...; r <= 192: 12 rows, 3 chunks) do not depend on anything either, but they are
  // 147 KB per workgroup and vector-memory loads return in order: requested BEHIND the first tile's operand, which the product waits for
  constexpr int PF_ROWS = 12, PF_CH = 3;
  // (only in the K <= 16 variants: with 24-row cubes the 36 prefetch registers no longer fit under the 128 of a 1024-thread
  //  workgroup and would spill; those variants fetch the rows where they use them.  Compiler's resource remarks, gfx950 -O3: no
  //  scratch in any variant but <16, 4, true> -- g0 of 53..64 with the block -- which spills 7 registers, 28 bytes per lane)
  constexpr bool PF = TL && KSK == 4;
  float npf[PF ? PF_ROWS : 1][PF ? PF_CH : 1];
  const bool pf = PF && tr <= 64 * PF_CH && tr <= 16 * PF_ROWS;   // block-uniform
  if constexpr (PF) {
    if (pf) {
#pragma unroll
      for (int i = 0; i < PF_ROWS; ++i) {
        const int e = w + 16 * i;
        const float* __restrict__ nrow = tl.N + (int64_t)(e < tr ? e : 0) * tl.r;
#pragma unroll
        for (int j = 0; j < PF_CH; ++j) npf[i][j] = (e < tr && lane + 64 * j < tr) ? nrow[lane + 64 * j] : 0.f;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int idx = t + 1024 * j, row = idx >> 5, col = idx & 31;
    sXt[row * KEEP_LDK + col] = xi[j];
    sXn[row * KEEP_LDC + col] = xi[j];
    sZn[row * KEEP_LDC + col] = zi[j];
  }
  if (t < 96) sE[t] = ev;
  __syncthreads();
  float rho_lane = 0.f;
  while (tile < ntile) {                           // wave-uniform
    const int mt = tile / nnt, n = 16 * (tile - mt * nnt) + l15;
    spec_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    {
      const float* qa = sXt + l4 * KEEP_LDK + 16 * mt + l15;
      float af[KS0];
#pragma unroll
      for (int i = 0; i < KS0; ++i) af[i] = qa[4 * i * KEEP_LDK];
#pragma unroll
      for (int i = 0; i < KS0; ++i) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bf[i], acc, 0, 0, 0);
    }
    const int k1 = n / K2, k2 = n - k1 * K2;
    const float e1 = sE[32 + k1], e2 = sE[64 + k2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int k0 = 16 * mt + 4 * l4 + q;
      if (k0 < KR) {
        const float lam = kscale * sE[k0] * e1 * e2;   // 0 on the padding rows
        const float al = shift * lam, f1 = __frcp_rn(1.f + al);
        const float v = acc[q];
        float cy = (lam * f1) * v, ct = (al * f1) * v;
        bool sel = false;
        if constexpr (TL) sel = (mrow[q] >> (kp.o[2] + k2)) & 1ull;
        if (sel) cy = ct = v;                          // raw coefficient: the exact block below replaces both
        else rho_lane += cy * v;
        sCY[k0 * ldc + n] = cy;
        sCT[k0 * ldc + n] = ct;
      }
    }
    tile += 16;
    if (tile < ntile) load_b(tile);
  }
  __syncthreads();                                 // the cubes are complete
  const float4 rv = *reinterpret_cast<const float4*>(r + ve);
  float4 pv = make_float4(0.f, 0.f, 0.f, 0.f), ptv = pv;
  if (it > 0) {                                    // (it == 0: p and pt are not read)
    pv = *reinterpret_cast<const float4*>(p + ve);
    ptv = *reinterpret_cast<const float4*>(pt + ve);
  }
  if constexpr (TL) {
    // where mode e sits in the cubes (block order = sorted by slab: its slab is the last i0 with off[i0] <= e), its raw
    // coefficient and eigenvalue; a mode outside the box (the caller rules it out) stays out
    if (t < tr) {
      int lo_ = 0, hi_ = g0 - 1;
      while (lo_ < hi_) {
        const int mid = (lo_ + hi_ + 1) >> 1;
        if (sOff[mid] <= t) lo_ = mid;
        else hi_ = mid - 1;
      }
      const int x = ppos >> 8, y = ppos & 255u;
      const int k0 = lo_ - kp.o[0], k1 = x - kp.o[1], k2 = y - kp.o[2];
      const bool in = k0 >= 0 && k1 >= 0 && k1 < K1 && k2 >= 0 && k2 < K2;
      const int idx = in ? k0 * ldc + k1 * K2 + k2 : -1;
      sIdx[t] = idx;
      sCs[t] = in ? sCY[idx] : 0.f;
      sLam[t] = in ? kscale * sE[k0] * sE[32 + k1] * sE[64 + k2] : 1.f;
    }
    __syncthreads();
    bool rows_done = false;
    if constexpr (PF) {
     if (pf) {
      rows_done = true;
      float cq[PF_CH];
#pragma unroll
      for (int j = 0; j < PF_CH; ++j) cq[j] = lane + 64 * j < tr ? sCs[lane + 64 * j] : 0.f;
#pragma unroll
      for (int i = 0; i < PF_ROWS; ++i) {
        const int e = w + 16 * i;
        if (e < tr) {                                  // wave-uniform
          float d = 0.f;
#pragma unroll
          for (int j = 0; j < PF_CH; ++j) d += npf[i][j] * cq[j];
          d = wave_reduce_sum<float>(d);
          if (lane == 0) sD[e] = d;
        }
      }
     }
    }
    if (!rows_done) {
      for (int e = w; e < tr; e += 16) {
        const float* __restrict__ nrow = tl.N + (int64_t)e * tl.r;
        float d = 0.f;
        for (int q = lane; q < tr; q += 64) d += nrow[q] * sCs[q];
        d = wave_reduce_sum<float>(d);
        if (lane == 0) sD[e] = d;
      }
    }
    __syncthreads();
    for (int e = t; e < tr; e += 1024) {
      const int idx = sIdx[e];
      if (idx >= 0) {
        const float d = sD[e], cs = sCs[e];
        sCY[idx] = d;                                  // N c_S
        sCT[idx] = cs - d / sLam[e];                   // c_S - D_S^-1 N c_S
        rho_lane += cs * d;
      }
    }
  }
  // rho(it) of THIS application: every workgroup holds the same terms and sums them in the same order (S.rho(it) itself is being
  // written by workgroup 0 of this very launch: beta must not read it)
  {
    const double ws = wave_reduce_sum<double>((double)rho_lane);
    if (lane == 0) s_red[w] = ws;
  }
  __syncthreads();                                 // ... and the block's entries of the cubes
  double rho_it = 0;
#pragma unroll
  for (int i = 0; i < 16; ++i) rho_it += s_red[i];
  float bt = 0.f;
  if (it > 0) {
    const double den = S.rho(it - 1)[0];
    bt = (float)(den > 0 ? rho_it / den : 0.0);
  }
  // mode 0 backward, this slab's row only: S_y[n] = sum_k0 X0_L[i0][k0] cy[k0][n],  S_t with Z0_L and ct  (K1 K2 <= 576 threads)
  if (t < KK) {
    float sy = 0.f, st = 0.f;
    for (int k0 = 0; k0 < K0; ++k0) {
      sy += sXn[i0 * KEEP_LDC + k0] * sCY[k0 * ldc + t];
      st += sZn[i0 * KEEP_LDC + k0] * sCT[k0 * ldc + t];
    }
    const int k1 = t / K2, k2 = t - k1 * K2;
    sS[k1 * KEEP_LDC + k2] = sy;
    sS[32 * KEEP_LDC + k1 * KEEP_LDC + k2] = st;
  }
  cx2.commit(sM, KEEP_LDC);
  cz2.commit(sM + 64 * KEEP_LDC, KEEP_LDC);
  cx1.commit(sM + 2 * 64 * KEEP_LDC, KEEP_LDC);
  cz1.commit(sM + 3 * 64 * KEEP_LDC, KEEP_LDC);
  __syncthreads();                                 // S and the images of dims 1, 2; the X0 / Z0 images and the cubes are dead
  // E[hh][k1][i2] = sum_k2 S[hh][k1][k2] M2[hh][i2][k2]: 2 x (W / 16) x 4 tiles
  constexpr int MT = W / 16;
  for (int id = w; id < 2 * MT * 4; id += 16) {
    const int hh = id / (MT * 4), mt = (id / 4) % MT, ct = id % 4;
    const spec_f32x4 acc = keep_tile<KSK>(sS + hh * 32 * KEEP_LDC + 16 * mt * KEEP_LDC, KEEP_LDC, 1, sM + hh * 64 * KEEP_LDC + 16 * ct * KEEP_LDC, 1, KEEP_LDC, lane);
#pragma unroll
    for (int q = 0; q < 4; ++q) sEh[hh * 32 * SPEC_LDT + (16 * mt + 4 * l4 + q) * SPEC_LDT + 16 * ct + l15] = acc[q];
  }
  __syncthreads();
  // O[hh][i1][i2] = sum_k1 M1[hh][i1][k1] E[hh][k1][i2]
  for (int id = w; id < 2 * 4 * 4; id += 16) {
    const int hh = id / 16, rt = (id / 4) % 4, ct = id % 4;
    if (16 * rt >= g1) continue;                   // wave-uniform
    const spec_f32x4 acc = keep_tile<KSK>(sM + (2 + hh) * 64 * KEEP_LDC + 16 * rt * KEEP_LDC, KEEP_LDC, 1, sEh + hh * 32 * SPEC_LDT + 16 * ct, SPEC_LDT, 1, lane);
#pragma unroll
    for (int q = 0; q < 4; ++q) sO[hh * 64 * SPEC_LDN + (16 * rt + 4 * l4 + q) * SPEC_LDN + 16 * ct + l15] = acc[q];
  }
  __syncthreads();
  // p = y + beta p,  pt = (r - correction) + beta pt
  if (v_ok) {
    const float rr[4] = {rv.x, rv.y, rv.z, rv.w};
    const float po[4] = {pv.x, pv.y, pv.z, pv.w}, pto[4] = {ptv.x, ptv.y, ptv.z, ptv.w};
    float pn[4], ptn[4];
    int row = (4 * t) / g2, col = 4 * t - row * g2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (col == g2) { col = 0; ++row; }
      const float y = sO[row * SPEC_LDN + col], tv = rr[j] - sO[64 * SPEC_LDN + row * SPEC_LDN + col];
      pn[j] = it > 0 ? y + bt * po[j] : y;
      ptn[j] = it > 0 ? tv + bt * pto[j] : tv;
      ++col;
    }
    *reinterpret_cast<float4*>(p + ve) = make_float4(pn[0], pn[1], pn[2], pn[3]);
    *reinterpret_cast<float4*>(pt + ve) = make_float4(ptn[0], ptn[1], ptn[2], ptn[3]);
  }
  if (i0 == 0 && t == 0 && rho != nullptr) unsafeAtomicAdd(rho, rho_it);
}

// ------------------------------------------------------------------- launch ---
// w1: 2 m floats of scratch (T, the forward partial sums: 2 g0 K1 K2 <= 2 m)
static int launch_spectral_keep_cg(const GridDev<float>& G, const float* evec, const float* evec2, const float* evals, float kscale, float shift,
                                   float* r, float* w1, int it, int apply, double tol2, float* p, float* pt, float* part, int nch, int zl,
                                   float* u, float* z, PcgScal S, hipStream_t s, const float* rhs0, const wiski_twolevel* two_level, const int* keep,
                                   const TapFold<float>* fold = nullptr) {
  const int g0 = G.g[0], g1 = G.g[1], g2 = G.g[2];
  if (!keep_counts_ok(G, keep, two_level != nullptr) || S.k != 1 || nch > 8) return WISKI_E_BADARG;
  if (two_level && (two_level->r < 1 || two_level->r > SPEC_TL_MAXR || !two_level->d_mask || !two_level->d_off || !two_level->d_pos || !two_level->d_N))
    return WISKI_E_BADARG;
  if (rhs0 && apply) return WISKI_E_BADARG;
  if (fold && (!fold->stage || !fold->b || !fold->cnt || fold->b != rhs0)) return WISKI_E_BADARG;   // the fold rides on the norms of a carried residual
  float *const fstage = fold ? fold->stage : nullptr, *const fb = fold ? fold->b : nullptr, *const fcnt = fold ? fold->cnt : nullptr;
  if (!evec2) evec2 = evec;
  const float *X0 = evec, *X1 = evec + g0 * g0, *X2 = X1 + g1 * g1;
  const float *Z0 = evec2, *Z1 = evec2 + g0 * g0, *Z2 = Z1 + g1 * g1;
  KeepDev kp;
  for (int q = 0; q < 3; ++q) { kp.K[q] = keep[q]; kp.o[q] = G.g[q] - keep[q]; }
  TwoLevelDev tl{};
  if (two_level)
    tl = TwoLevelDev{two_level->r, two_level->nslab, (const unsigned long long*)two_level->d_mask, two_level->d_off, two_level->d_pos, two_level->d_N,
                     nullptr, 0u};
  const bool wide = keep[0] > 16 || keep[1] > 16 || keep[2] > 16;
  const size_t bwd_lds = keep_bwd_lds(keep, two_level != nullptr);
  const dim3 grd((unsigned)g0, KEEP_NS);
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return WISKI_E_LAUNCH;
#define KEEP_LDS_OPT_IN(fn, bytes)                                                                                                     \
  do {                                                                                                                                 \
    static size_t set_[16] = {0};   /* per device: the attribute belongs to the device's copy of the kernel */                         \
    if ((size_t)(bytes) > set_[dev & 15]) {                                                                                            \
      if (hipFuncSetAttribute((const void*)(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)) != hipSuccess) return WISKI_E_LAUNCH; \
      set_[dev & 15] = (bytes);                                                                                                        \
    }                                                                                                                                  \
  } while (0)
  // forward: the previous iteration's update + T = X1_L^T R X2_L per half slab
  {
    const int gm = g1 > g2 ? g1 : g2;
    const float* pin = rhs0 ? rhs0 : p;
    const int ap = rhs0 ? 2 : apply;
#define KEEP_FWD2(KS, WW)                                                                                                                  \
  do {                                                                                                                                     \
    KEEP_LDS_OPT_IN((k_keep_fwd<KS, WW>), KEEP_FWD_LDS);                                                                                   \
    hipLaunchKernelGGL((k_keep_fwd<KS, WW>), grd, dim3(256), KEEP_FWD_LDS, s, G, kp, X1, X2, r, w1, it, ap, tol2, pin, (const float*)pt, S, \
                       part, nch, zl, u, z, fstage, fb, fcnt);                                                                             \
  } while (0)
#define KEEP_FWD(KS, VW_UNUSED)          \
  do {                                   \
    if (wide) KEEP_FWD2(KS, 32);         \
    else KEEP_FWD2(KS, 16);              \
  } while (0)
    SPEC_DISPATCH_KS_VW(gm, true, KEEP_FWD);
#undef KEEP_FWD
#undef KEEP_FWD2
    if (hipGetLastError() != hipSuccess) return WISKI_E_LAUNCH;
  }
  // middle + backward: one workgroup per slab forms the cube, its row of mode 0 backward, modes 2 and 1 and the direction update
  {
#define KEEP_BWD3(KS, KSK, TLV)                                                                                                          \
  do {                                                                                                                                   \
    KEEP_LDS_OPT_IN((k_keep_bwd<KS, KSK, TLV>), bwd_lds);                                                                                \
    hipLaunchKernelGGL((k_keep_bwd<KS, KSK, TLV>), dim3((unsigned)g0), dim3(1024), bwd_lds, s, G, kp, X0, Z0, X1, X2, Z1, Z2, evals, kscale, \
                       shift, (const float*)w1, (const float*)r, p, pt, it, S, S.rho(it), tl);                                           \
  } while (0)
#define KEEP_BWD(KS, VW_UNUSED)                    \
  do {                                             \
    if (wide) {                                    \
      if (two_level) KEEP_BWD3(KS, 6, true);       \
      else KEEP_BWD3(KS, 6, false);                \
    } else {                                       \
      if (two_level) KEEP_BWD3(KS, 4, true);       \
      else KEEP_BWD3(KS, 4, false);                \
    }                                              \
  } while (0)
    SPEC_DISPATCH_KS_VW(g0, true, KEEP_BWD);
#undef KEEP_BWD
#undef KEEP_BWD3
  }
#undef KEEP_LDS_OPT_IN
  return hipGetLastError() == hipSuccess ? WISKI_OK : WISKI_E_LAUNCH;
}
