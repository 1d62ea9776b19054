"""Plain fp64 reference, layouts, data makers, case tables, a mirror of the kernel dispatch and seeded defects for the block-stencil
products of csrc/solve.hip:

  wiski_stencil_spmv       out[c, i] = beta add[c, i] + sum_o A[o, i] V[c, i + off(o)]          (full stencil, offset-major [R][m])
  wiski_stencil_spmv_sym   the same product from the symmetric half stencil A_h (native layout)  (every stored entry used twice)

numpy only; tests/test_stencil_reference_host.py checks this file without a GPU and tests/test_stencil_products_gpu.py holds the
eight kernels behind the two entries to it.  Everything here is written from the comments of csrc/solve.hip and include/wiski.h
(not from online_gp_amd.grid_ops, whose packers the GPU test checks against these):

  offsets      R = 7^d of them; offset o has d base-7 digits, dimension 0 slowest, digit - 3 = shift along that dimension;
               off(o) = sum_q shift_q stride_q, stride of the last dimension 1.  Centre ctr = (R - 1) / 2, H = (R + 1) / 2.
  in-grid      entry (o, i) is in the grid iff every coordinate of node i plus its shift stays in [0, g_q).  All other entries
               of a stencil are exact +0.0: that is the contract the kernels rely on (they clamp the neighbour index and multiply).
  full         A[o * m + i]                                                               (offset-major [R][m])
  half, om     a(oh, i) = A[ctr + oh, i], oh = 0 .. H - 1                                 (offset-major half [H][m])
  half, native group 0 (oh < 4, the centre prefix, innermost digits 3..6): A_h[4 i + oh]; group g >= 1 (oh = 7 g - 3 + s,
               s = 0..6): A_h[(7 g - 3) m + 7 i + s]                                      (what the scatter accumulates)

Two kinds of data.  INTEGER: every in-grid coefficient is a nonzero integer of [-8, 8], V and add integers of [-8, 8], beta = -2;
every partial sum of any summation order is an integer of magnitude <= 7^4 64 + 16 = 153 680 < 2^24, so fp32 and fp64, plain sums,
FMAs and the atomically accumulated partial all give THE result, and the comparison is bit for bit.  REAL: coefficients U(-1, 1),
V and add N(0, 1), drawn in the kernel's type and upcast exactly, so there is no input-rounding term; every element is held to

  |out - ref|_e <= gamma_n absref_e,   gamma_n = n u / (1 - n u),  u = 2^-24 or 2^-53,
  absref = |beta| |add| + sum |A| |V|   (Higham, Accuracy and Stability of Numerical Algorithms, 3.1)

with n counted from the kernels and no other constant.  The count (`spmv_n`): an output is a sum of at most R = 7^d products and
beta add, and whatever the kernel's order -- registers, the wave's LDS window, the atomic partial, k_spmv_reduce -- a term meets one
rounding for its product and one per addition on its way to the output; additions to an exact zero (fresh accumulators, the zeroed
window and partial) round nothing.  Per path, n = R + P + 2 with P the partial vectors k_spmv_reduce sums and 2 for beta add (its
product, its addition):

  code 0  k_stencil_spmv        one accumulator per row                                            P = 0
  code 1  k_stencil_spmv4 / k_stencil_spmm    one partial per leading digit                        P = 7 (d >= 2), 1 (d = 1)
  code 2  k_stencil_spmv_sym    one accumulator per row, both terms                                P = 0
  code 3  k_stencil_spmv4_sym   min(groups, 7) direct partials + the accumulated one               P = min((7^(d-1) + 1) / 2, 7) + 1
  code 4  k_spmv_sym_dma        4 parts + the accumulated one                                      P = 5
  code 5  k_spmv_sym_dma_mc     4 parts + the accumulated one                                      P = 5
  code 6  k_spmm_sym_bcast      one finished vector                                                P = 1
  code 7  k_spmm_sym_cols       one finished vector                                                P = 1

(R + 1 would already bound any order; the P + 1 on top is the count the kernels' structure gives without that argument.)  The fp64
reference obeys the same kind of bound with u = 2^-53: nothing next to an fp32 kernel, a share of the budget next to an fp64 one
that no constant is added for."""
import functools
import itertools
import zlib

import numpy as np

F64, F32 = np.float64, np.float32
INT_BETA = -2.0
INT_BOUND = 7 ** 4 * 64 + 16            # largest magnitude any partial sum of the integer data can reach (d = 4)
OLD_FP32_TOL = 2e-5                     # the max-norm tolerance of the three older stencil tests of tests/test_hip_ops.py


def unit(real):
    return 2.0 ** -24 if np.dtype(real) == np.dtype(F32) else 2.0 ** -53


def gamma(n, real):
    nu = n * unit(real)
    return nu / (1.0 - nu)


def ratio(out, ref, bound):
    """max_e |out - ref|_e / bound_e; an element that is not finite, or wrong where the bound is 0, counts as infinite."""
    out = np.asarray(out, F64)
    err = np.abs(out - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(out), r, np.inf)
    return float(r.max())


# ------------------------------------------------------------------------------------------------------------- geometry --
def strides(gs):
    st = [1] * len(gs)
    for q in range(len(gs) - 2, -1, -1):
        st[q] = st[q + 1] * gs[q + 1]
    return st


class Geometry:
    def __init__(self, gs):
        self.gs, self.d = tuple(gs), len(gs)
        self.st = strides(gs)
        self.m = int(np.prod(gs))
        self.R = 7 ** self.d
        self.ctr, self.H = (self.R - 1) // 2, (self.R + 1) // 2
        o = np.arange(self.R)
        self.shifts = np.stack([(o // 7 ** (self.d - 1 - q)) % 7 - 3 for q in range(self.d)], axis=1)      # [R, d], dimension 0 slowest
        self.offs = self.shifts @ np.asarray(self.st)                                                       # [R]
        i = np.arange(self.m)
        self.coords = np.stack([(i // self.st[q]) % gs[q] for q in range(self.d)], axis=1)                  # [m, d]
        # ok[q][digit][i]: coordinate q of node i plus (digit - 3) stays inside [0, g_q)
        ok = [[(self.coords[:, q] + s >= 0) & (self.coords[:, q] + s < gs[q]) for s in range(-3, 4)] for q in range(self.d)]
        mask = np.ones((self.R, self.m), bool)
        for q in range(self.d):
            mask &= np.stack(ok[q])[self.shifts[:, q] + 3]
        self.mask = mask                                                                                    # [R, m] the in-grid mask
        self.band = (3 * sum(self.st) + 1024 + 63) // 64 * 64       # guard band of the GPU test: wider than any window, 256-byte steps


@functools.lru_cache(maxsize=6)
def geometry(gs):
    return Geometry(tuple(gs))


# -------------------------------------------------------------------------------------------------------------- layouts --
def half_om_from_full(gs, A_full):
    """The stored half of a full stencil: a(oh, i) = A[ctr + oh, i]."""
    G = geometry(gs)
    return np.array(A_full[G.ctr:], copy=True)


def pack_half(gs, A_om):
    """Offset-major half [H, m] -> the native flat layout (H m reals)."""
    G = geometry(gs)
    m, H = G.m, G.H
    flat = np.empty(H * m, A_om.dtype)
    for oh in range(min(H, 4)):
        flat[oh:4 * m:4] = A_om[oh]
    for oh in range(4, H):
        g, s = (oh + 3) // 7, (oh + 3) % 7
        flat[(7 * g - 3) * m + s:(7 * g + 4) * m:7] = A_om[oh]
    return flat


def unpack_half(gs, flat):
    """The inverse of pack_half."""
    G = geometry(gs)
    m, H = G.m, G.H
    A_om = np.empty((H, m), flat.dtype)
    for oh in range(min(H, 4)):
        A_om[oh] = flat[oh:4 * m:4]
    for oh in range(4, H):
        g, s = (oh + 3) // 7, (oh + 3) % 7
        A_om[oh] = flat[(7 * g - 3) * m + s:(7 * g + 4) * m:7]
    return A_om


def expand_half(gs, A_om):
    """Half -> the symmetric full stencil: A[ctr + oh, i] = a(oh, i) and its mirror image A[ctr - oh, i + off] = a(oh, i) at every
    in-grid entry; everything else +0.0."""
    G = geometry(gs)
    full = np.zeros((G.R, G.m), A_om.dtype)
    for oh in range(G.H):
        o = G.ctr + oh
        i = np.flatnonzero(G.mask[o])
        full[o, i] = A_om[oh, i]
        if oh:
            full[G.ctr - oh, i + G.offs[o]] = A_om[oh, i]
    return full


# ------------------------------------------------------------------------------------------------------------ reference --
def product(gs, A_full, V, add=None, beta=0.0):
    """(ref, absref) in fp64, [k, m], summed over the in-grid entries only."""
    G = geometry(gs)
    A, V = np.asarray(A_full, F64), np.asarray(V, F64)
    k = V.shape[0]
    # V on the grid inside a margin of three zeros per side: a neighbour is addressed by its coordinates, never by a flat index, so an
    # entry whose neighbour leaves the grid meets a zero whatever coefficient it holds
    Vp = np.zeros((k,) + tuple(g + 6 for g in gs))
    Vp[(slice(None),) + tuple(slice(3, 3 + g) for g in gs)] = V.reshape((k,) + tuple(gs))
    aVp = np.abs(Vp)
    ref, absref = np.zeros((k,) + tuple(gs)), np.zeros((k,) + tuple(gs))
    for o in range(G.R):
        nb = (slice(None),) + tuple(slice(3 + s, 3 + s + g) for s, g in zip(G.shifts[o], gs))
        a = A[o].reshape(gs)
        ref += a * Vp[nb]
        absref += np.abs(a) * aVp[nb]
    ref, absref = ref.reshape(k, G.m), absref.reshape(k, G.m)
    if add is not None:
        add = np.asarray(add, F64)
        ref += beta * add
        absref += abs(beta) * np.abs(add)
    return ref, absref


def dense_matrix(gs, A_full):
    """The m x m matrix of a full stencil, assembled node by node from coordinates (an independent route for the host test)."""
    m, d = int(np.prod(gs)), len(gs)
    D = np.zeros((m, m))
    for i, ci in enumerate(itertools.product(*[range(g) for g in gs])):
        for o, sh in enumerate(itertools.product(range(-3, 4), repeat=d)):
            cj = [a + b for a, b in zip(ci, sh)]
            if all(0 <= c < g for c, g in zip(cj, gs)):
                D[i, int(np.ravel_multi_index(cj, gs))] = A_full[o, i]
    return D


def sym_groups(d):
    return (7 ** (d - 1) + 1) // 2


def partials(gs, code):
    """Partial vectors k_spmv_reduce sums on the path `code` (the table of the module docstring)."""
    d = len(gs)
    return {0: 0, 1: 7 if d >= 2 else 1, 2: 0, 3: min(sym_groups(d), 7) + 1, 4: 5, 5: 5, 6: 1, 7: 1}[code]


def spmv_n(gs, code):
    return 7 ** len(gs) + partials(gs, code) + 2


def bound(gs, code, absref, real):
    return gamma(spmv_n(gs, code), real) * absref


# ---------------------------------------------------------------------------------------------------------- data makers --
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


@functools.lru_cache(maxsize=6)
def _grid_data(gs, kmax, kind, real_name, symmetric):
    """The data of one grid at its widest column count, with its reference: drawn and multiplied once, shared by every case of the
    grid (a case takes the first k columns; the columns of a product are independent)."""
    G, real = geometry(gs), np.dtype(real_name).type
    rng = _rng(gs, kind, real_name, symmetric)
    rows = G.H if symmetric else G.R
    msk = G.mask[G.ctr:] if symmetric else G.mask
    if kind == "int":
        c = rng.integers(1, 9, (rows, G.m)) * rng.choice([-1, 1], (rows, G.m))
        V, add, beta = rng.integers(-8, 9, (kmax, G.m)), rng.integers(-8, 9, (kmax, G.m)), INT_BETA
    else:
        c = rng.uniform(-1.0, 1.0, (rows, G.m))
        V, add, beta = rng.standard_normal((kmax, G.m)), rng.standard_normal((kmax, G.m)), float(np.asarray(0.6, real))
    c = np.where(msk, c, 0.0).astype(real)
    D = {"V": V.astype(real), "add": add.astype(real), "beta": beta}
    if symmetric:
        D["half"], D["full"] = pack_half(gs, c), expand_half(gs, c)
    else:
        D["half"], D["full"] = None, c
    D["ref"], D["absref"] = product(gs, D["full"], D["V"], D["add"], beta)
    for v in D.values():
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return D


def make_data(gs, k, kind, real, symmetric=True):
    """kind "int" or "real" (module docstring).  symmetric: draws on the stored half, `full` its expansion; otherwise independent
    draws at all R offsets (full form only: `half` is None).  Out-of-grid entries are exact +0.0.  Returns a dict of read-only arrays
    in `real`: half (native flat), full [R, m], V, add [k, m]; beta (a Python float that `real` holds exactly); and in fp64
    ref, absref [k, m] = product(gs, full, V, add, beta)."""
    gs = tuple(gs)
    kmax = max([k] + [kk for g, kk in CASES if g == gs])
    D = _grid_data(gs, kmax, kind, np.dtype(real).name, bool(symmetric))
    return {key: (v[:k] if key in ("V", "add", "ref", "absref") else v) for key, v in D.items()}


def keys_weights(t):
    """Cubic-convolution (Keys, a = -0.5) weights of the four nodes around a point at fraction t of its cell."""
    return np.stack([(-t ** 3 + 2 * t ** 2 - t) / 2, (3 * t ** 3 - 5 * t ** 2 + 2) / 2, (-3 * t ** 3 + 4 * t ** 2 + t) / 2, (t ** 3 - t ** 2) / 2], axis=-1)


def interpolation_stencil(gs, n, seed=0):
    """W^T W of n random interior points with cubic interpolation weights, as a full stencil [R, m] in fp64: the statistics the three
    older tests of tests/test_hip_ops.py draw their coefficients from."""
    G = geometry(gs)
    rng, d = np.random.default_rng(seed), G.d
    A = np.zeros((G.R, G.m))
    x = np.stack([rng.uniform(1.0, g - 2.0, n) for g in gs], axis=1)           # in node units; the 4 taps floor - 1 .. floor + 2 are nodes
    cell = np.minimum(np.floor(x).astype(int), np.asarray(gs) - 3)
    w1 = keys_weights(x - cell)                                                 # [n, d, 4]
    taps = np.asarray(list(itertools.product(range(4), repeat=d)))              # [4^d, d]
    node = sum((cell[:, None, q] - 1 + taps[None, :, q]) * G.st[q] for q in range(d))      # [n, T]
    w = np.prod(np.stack([w1[:, q, taps[:, q]] for q in range(d)]), axis=0)                 # [n, T]
    for a in range(len(taps)):
        for b in range(len(taps)):
            o = sum((taps[b, q] - taps[a, q] + 3) * 7 ** (d - 1 - q) for q in range(d))
            np.add.at(A[o], node[:, a], w[:, a] * w[:, b])
    return A


# ----------------------------------------------------------------------------------------------------- dispatch mirror --
SYMDMA_TILE = 7 * 256
LDS_LIMIT = 64 * 1024


def symdma_w4(g2):
    return ((256 + 6 * g2 + 10 + 3) // 4) | 1


def symdma_wp(g2):
    return (4 * symdma_w4(g2) + 63) & ~63


def symdma_vwf(g2):
    need = 256 + 6 * g2 + 10 + 3
    n128 = need // 256
    return 256 * n128 + 64 * ((need - 256 * n128 + 63) // 64)


def symdma_lds_bytes(g2, nst=2):
    return (nst * SYMDMA_TILE + 256 + symdma_vwf(g2) + symdma_wp(g2)) * 4


def symdma_mc_lds_bytes(g2, kc):
    return (2 * SYMDMA_TILE + kc * (256 + symdma_vwf(g2) + symdma_wp(g2))) * 4


def lds_handover(lds_bytes):
    """The largest innermost g for which the kernel's LDS still fits LDS_LIMIT (lds_bytes never decreases with g)."""
    g = 4
    while lds_bytes(g + 1) <= LDS_LIMIT:
        g += 1
    return g


def window_cap(es, kc):
    """launch_spmv4_sym: the widest window span a block of two waves keeps within 64 KB; a span 6 stride[d - 2] above it is shrunk."""
    return (LDS_LIMIT // (2 * es) - 7 * 256) // kc - 256 - 32


def kc3(k):
    return 4 if k >= 4 else 2 if k >= 2 else 1


def expected_path(gs, k, es, half, sym_dma=True, spmm_bcast=True):
    """(code, kc) of wiski_stencil_spmv_path, from the predicates of csrc/solve.hip (sym_use_cols, sym_use_bcast, sym_use_dma,
    sym_use_dma_mc, m % 4); sym_dma / spmm_bcast are the WISKI_SYM_DMA / WISKI_SPMM_BCAST switches."""
    d, m = len(gs), int(np.prod(gs))
    if not half:
        if m % 4:
            return 0, kc3(k)
        if k >= 8 and d in (2, 3):
            return 1, 16 if es == 4 and k >= 16 else 8
        return 1, 8 if k >= 8 else kc3(k)
    if m % 4:
        return 2, kc3(k)
    if k >= ((16 if es == 4 else 24) if spmm_bcast else 32):
        return (6, 64) if spmm_bcast else (7, (k + 15) // 16 * 16)
    if es == 4 and sym_dma and d == 3:
        if k == 1 and symdma_lds_bytes(gs[2]) <= LDS_LIMIT:
            return 4, 1
        if k >= 2 and gs[2] >= 4 and symdma_mc_lds_bytes(gs[2], 4 if k >= 4 else 2) <= LDS_LIMIT:
            return 5, 4 if k >= 4 else 2
    return 3, kc3(k)


# ----------------------------------------------------------------------------------------------------------- case tables --
COLS_ALL = [1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 23, 24, 25, 31, 32, 33, 63, 64, 65, 100]
COLS_EDGE = [1, 2, 5, 16, 24]             # KC 1 / 2 / 4 with a tail, the fp32 and the fp64 broadcast thresholds
ALL_COLS_GRIDS = [(7, 9), (4, 4, 4), (8, 5, 9), (4, 4, 4, 4)]
# the LDS hand-over points (largest innermost g that kernels 4 / 5 still take, the LDS-window kernel above): lds_handover() of
# symdma_lds_bytes and symdma_mc_lds_bytes; tests/test_stencil_reference_host.py re-derives them
HANDOVER = {"dma": 1000, "mc2": 467, "mc4": 200}
HANDOVER_K = {"dma": 1, "mc2": 2, "mc4": 4}
# window-shrink threshold of kernel 3 (d = 2: span = 6 g[1] against window_cap): fp64 with four columns 288 = 6 * 48, fp32 with four 1312 >= 6 * 218
SHRINK = {"f64": (8, 4, 48), "f32": (4, 4, 218)}
GRIDS = {
    1: [(4,), (7,), (64,), (255,), (256,), (1000,)],
    2: [(4, 4), (7, 9), (30, 10), (5, 64), (4, 48), (4, 49), (4, 218), (4, 219)],
    3: [(4, 4, 4), (8, 5, 9), (6, 10, 14), (5, 7, 64), (7, 5, 9), (20, 24, 50)],
    4: [(4, 4, 4, 4), (4, 5, 4, 6), (5, 5, 5, 5)],
}


def _cases():
    out = []
    for d in (1, 2, 3, 4):
        for gs in GRIDS[d]:
            if gs in ALL_COLS_GRIDS:
                ks = COLS_ALL
            elif gs in ((4, 48), (4, 49), (4, 218), (4, 219)):
                ks = [4]
            elif gs == (20, 24, 50):
                ks = [1, 2, 4]
            else:
                ks = COLS_EDGE
            out += [(gs, k) for k in ks]
        if d == 3:
            for name in ("dma", "mc2", "mc4"):
                out += [((4, 4, HANDOVER[name] + e), HANDOVER_K[name]) for e in (0, 1)]
    return out


CASES = _cases()


def cases_of(d):
    return [c for c in CASES if len(c[0]) == d]


def case_id(case):
    return "x".join(map(str, case[0])) + f"-k{case[1]}"


# -------------------------------------------------------------------------------------------------------- seeded defects --
DEFECTS = ["corner_groups", "transposed_row", "centre_stride7", "diag_twice", "clamp_last_row", "last_row_block", "last_column", "add_column0",
           "beta_ignored", "flat_wrap", "slice_boundary"]


def emulate_half(gs, half, V, add=None, beta=0.0, defect=None):
    """A half-stencil product as the kernels form it -- every stored entry used for the direct term out[i] += a(oh, i) v[i + off] and,
    oh > 0, the transposed one out[i] += a(oh, i - off) v[i - off]; neighbour indices clamped, not masked (the out-of-grid entries
    are zeros) -- in fp64 from the native flat layout, with one defect of DEFECTS seeded:

      corner_groups    the groups whose two leading shifts are both +-3 are skipped (d >= 3)
      transposed_row   the transposed term takes a(oh, i) for a(oh, i - off)
      centre_stride7   the centre group is read with the row stride 7 of the later groups
      diag_twice       the diagonal is applied in the transposed term as well
      clamp_last_row   the neighbour index is clamped to m - 2
      last_row_block   the ragged last block of 256 rows is not computed (left zero)
      last_column      column k - 1 is not computed when k % 4 != 0
      add_column0      add of column 0 is used for every column
      beta_ignored     beta taken as 1
      flat_wrap        an entry whose neighbour is inside [0, m) by its flat index but outside the grid counts as in-grid: it carries
                       a coefficient (1, where the contract has a zero) and is multiplied like any other
      slice_boundary   a 64-column slice ends one column early: columns c % 64 == 63 are not computed"""
    G = geometry(gs)
    m, d = G.m, G.d
    flat, V = np.asarray(half, F64), np.asarray(V, F64)
    k = V.shape[0]
    i = np.arange(m)
    out = np.zeros((k, m))
    for oh in range(G.H):
        o = G.ctr + oh
        off, sh = int(G.offs[o]), G.shifts[o]
        if defect == "corner_groups" and d >= 3 and abs(sh[0]) == 3 and abs(sh[1]) == 3:
            continue
        if oh < 4:
            a = flat[np.minimum((7 if defect == "centre_stride7" else 4) * i + oh, flat.size - 1)]
        else:
            g, s = (oh + 3) // 7, (oh + 3) % 7
            a = flat[(7 * g - 3) * m + 7 * i + s]
        if defect == "flat_wrap":
            a = np.where((i + off >= 0) & (i + off < m) & ~G.mask[o], 1.0, a)
        j = np.clip(i + off, 0, m - 2 if defect == "clamp_last_row" else m - 1)
        out += a * V[:, j]
        if oh or defect == "diag_twice":
            jt = i - off
            okt = (jt >= 0) & (jt < m)
            jt = np.clip(jt, 0, m - 1)
            at = np.where(okt, a if defect == "transposed_row" else a[jt], 0.0)
            out += at * V[:, jt]
    if defect == "last_row_block" and m % 256:
        out[:, m // 256 * 256:] = 0.0
    if defect == "last_column" and k % 4:
        out[k - 1] = 0.0
    if defect == "slice_boundary":
        out[63::64] = 0.0
    if add is not None:
        add = np.asarray(add, F64)
        out += (1.0 if defect == "beta_ignored" else beta) * (add[:1] if defect == "add_column0" else add)
    return out


# the smallest table case at which each defect is caught (bit-inequality of the integer data, an element outside gamma_n absref of
# the real data); tests/test_stencil_reference_host.py checks every row
DEFECT_CASE = {
    "corner_groups": ((4, 4, 4), 1), "transposed_row": ((4,), 1), "centre_stride7": ((4,), 1), "diag_twice": ((4,), 1), "clamp_last_row": ((4,), 1),
    "last_row_block": ((4,), 1), "last_column": ((4,), 1), "add_column0": ((4,), 2), "beta_ignored": ((4,), 1), "flat_wrap": ((4, 4), 1),
    "slice_boundary": ((4, 4, 4), 64),
}
