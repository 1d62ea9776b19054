"""Plain fp64 references, derived error bounds, fp32 emulations and seeded defects for the Kronecker mode products of csrc/solve.hip:

  wiski_kron_toeplitz_mm   out = scale (kron_q T_q) V,  T_q[i, j] = tcol_q[|i - j|]
                           (k_toeplitz_line_shfl on the innermost mode when g <= 64, k_toeplitz_mode otherwise)
  wiski_kron_spectral_mm   out = (kron_q F_q) diag(f) (kron_q F_q)^T V,  lam = kscale prod_q evals_q[i_q],
                           f = (power != 0 ? (lam > 0 ? lam^power : 0) : 1) (rpower != 0 ? (1 + shift lam)^-rpower : 1)
                           (k_dense_mode<., 0> twice per mode, k_spectral_scale between the two transforms)

numpy only; tests/test_kron_reference_host.py checks this file without a GPU and tests/test_kron_products_gpu.py holds the kernels to it.

The bound is componentwise and derived, not fitted.  With u the unit roundoff of the kernel's type (2^-24, 2^-53) and
gamma_n = n u / (1 - n u), a chain of n roundings on every path from an input to an output gives

  |out - ref|_e <= gamma_n absref_e,

absref being the same product with every factor, every scaling and V replaced by its absolute value (Higham, Accuracy and Stability
of Numerical Algorithms, 3.1 and 3.5: gamma_a + gamma_b + gamma_a gamma_b <= gamma_{a+b} carries the bound of one mode through the
next).  The counts n are next to `toeplitz_n` and `spectral_n`.  The references take the tensors and the scalars that the kernel is
given, upcast (exactly) to fp64, so the bound has no input-rounding term.  The fp64 reference itself obeys the same kind of bound with
u = 2^-53: nothing next to an fp32 kernel, and a share of the budget next to an fp64 one that no constant is added for."""
import functools
import zlib

import numpy as np

F64, F32 = np.float64, np.float32
LINE_MAX = 64          # launch_kron: the shuffle kernel takes the innermost mode up to this g
LINE_BLOCKS = 2048     # ... with at most this many blocks of four waves, one line per wave and trip
SPECTRAL_PARAMS = [    # (power, rpower, shift, kscale)
    (0.5, 0.0, 0.0, 1.0), (0.5, 0.0, 0.0, 0.37), (1.0, 1.0, 0.8, 1.3), (0.0, 1.0, 0.8, 1.3), (0.0, 0.0, 0.8, 1.3), (-0.5, 0.0, 0.0, 1.0)]
TOEPLITZ_GRIDS = [(4,), (63,), (64,), (65,), (256,), (5, 64), (64, 5), (7, 65), (65, 7), (4, 256), (4, 4, 4), (6, 5, 63), (5, 7, 64),
                  (9, 4, 65), (96, 96, 4), (4, 5, 6, 7), (4, 4, 4, 64)]
TOEPLITZ_CASES = [(gs, k) for gs in TOEPLITZ_GRIDS for k in (1, 3)] + [((5, 7, 64), 17)]
SPECTRAL_GRIDS = [(4,), (64,), (90,), (91,), (128,), (65, 5), (5, 65), (128, 4), (6, 5, 7), (8, 8, 8), (4, 5, 6, 7)]
SPECTRAL_KINDS = ["eigen", "dense"]     # kron_eigen's orthogonal tables with one zero eigenvalue / random dense factors
SPECTRAL_CASES = [(gs, k, kind) for gs in SPECTRAL_GRIDS for k in (1, 3) for kind in SPECTRAL_KINDS]
PROBE_GRIDS = [(64,), (5, 7, 64), (65,)]
TOEPLITZ_SCALE = 1.3


def case_id(case):
    return "-".join("x".join(map(str, c)) if isinstance(c, tuple) else f"k{c}" if isinstance(c, int) else str(c) for c in case)


def unit(real):
    return 2.0 ** -24 if np.dtype(real) == np.dtype(F32) else 2.0 ** -53


def gamma(n, real):
    nu = n * unit(real)
    return nu / (1.0 - nu)


def toeplitz_n(gs):
    """Roundings between an input and an output of the Toeplitz product.  Per mode: the g multiply-adds of one accumulator (a product
    and at most g - 1 additions after it; the first addition, to 0 or of t_0 v_i, is exact) and, in the line kernel only, the sum
    up + dn; then the final scale, once (the other modes multiply by 1, exactly).  k_toeplitz_mode has no up + dn and a fused
    multiply-add has one rounding less per term, so the count covers both kernels, contracted or not."""
    return sum(g + 1 for g in gs) + 1


def spectral_n(gs):
    """Roundings of the spectral product.  Two transforms of g multiply-adds per mode (2 sum g); lam = kscale e_0 ... e_{d-1} is d
    products (d), and f depends on lam with |d log f / d log lam| <= 1 at every row of SPECTRAL_PARAMS, so lam's error enters f
    once; the two pow results rounded to `real` (2), their product (1) and v *= f (1)."""
    return 2 * sum(gs) + len(gs) + 4


def toeplitz_bound(gs, absref, real):
    return gamma(toeplitz_n(gs), real) * absref


def spectral_bound(gs, absref, real):
    return gamma(spectral_n(gs), real) * absref


def ratio(out, ref, bound):
    """max_e |out - ref|_e / bound_e; an element that is not finite, or wrong where the bound is 0, counts as infinite."""
    out = np.asarray(out, F64)
    err = np.abs(out - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    r = np.where(np.isfinite(out), r, np.inf)
    return float(r.max())


def strides(gs):
    st = [1] * len(gs)
    for q in range(len(gs) - 2, -1, -1):
        st[q] = st[q + 1] * gs[q + 1]
    return st


def split(gs, flat, square=False):
    """The per-dimension pieces of a concatenated table: g_q entries each, or g_q x g_q row-major matrices."""
    out, off = [], 0
    for g in gs:
        n = g * g if square else g
        out.append(np.asarray(flat[off:off + n]).reshape((g, g) if square else (g,)))
        off += n
    return out


def sym_toeplitz(col):
    g = len(col)
    return np.asarray(col, F64)[np.abs(np.arange(g)[:, None] - np.arange(g)[None, :])]


def mode_apply(mats, X):
    """X [k, *gs] with mats[q] applied along dimension q (dimension 0 slowest): out[.., i, ..] = sum_j mats[q][i, j] X[.., j, ..]."""
    for q, M in enumerate(mats):
        X = np.moveaxis(np.tensordot(M, X, axes=(1, q + 1)), 0, q + 1)
    return X


def toeplitz_ref(gs, tcol, V, scale):
    """(ref, absref), both [k, m] fp64: scale (kron T_q) V and |scale| (kron |T_q|) |V|."""
    k = V.shape[0]
    T = [sym_toeplitz(c) for c in split(gs, tcol)]
    X = np.asarray(V, F64).reshape((k,) + tuple(gs))
    ref = float(scale) * mode_apply(T, X)
    absref = abs(float(scale)) * mode_apply([np.abs(t) for t in T], np.abs(X))
    return ref.reshape(k, -1), absref.reshape(k, -1)


def spectral_factor(gs, evals, kscale, shift, power, rpower):
    """(lam, f) on the grid, flattened: k_spectral_scale's rule, in fp64."""
    lam = np.full((1,) * len(gs), float(kscale))
    for q, e in enumerate(split(gs, evals)):
        lam = lam * np.asarray(e, F64).reshape([-1 if r == q else 1 for r in range(len(gs))])
    lam = lam.reshape(-1)
    f = np.ones_like(lam)
    if power != 0:
        f = np.where(lam > 0, np.power(np.where(lam > 0, lam, 1.0), float(power)), 0.0)
    if rpower != 0:
        f = f * np.power(1.0 + float(shift) * lam, -float(rpower))
    return lam, f


def spectral_ref(gs, F, evals, V, kscale, shift, power, rpower):
    """(ref, absref), both [k, m] fp64: (kron F_q) diag(f) (kron F_q)^T V and the same with |F_q|, |f|, |V|."""
    k = V.shape[0]
    Fq = [np.asarray(f, F64) for f in split(gs, F, square=True)]
    _, f = spectral_factor(gs, evals, kscale, shift, power, rpower)
    f = f.reshape(gs)
    X = np.asarray(V, F64).reshape((k,) + tuple(gs))
    ref = mode_apply(Fq, mode_apply([m.T for m in Fq], X) * f)
    absref = mode_apply([np.abs(m) for m in Fq], mode_apply([np.abs(m).T for m in Fq], np.abs(X)) * np.abs(f))
    return ref.reshape(k, -1), absref.reshape(k, -1)


def kron_dense(mats):
    """The dense Kronecker product, dimension 0 slowest (the brute-force check of the references; m <= 4096)."""
    return functools.reduce(np.kron, mats)


# ------------------------------------------------------------------------------------------------------------- inputs --
def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def toeplitz_inputs(case, real):
    """tcol [sum g], V [k, m] in `real` and the scale as the kernel receives it.  The columns are signed and drawn per dimension, so
    that every lag of every mode is its own number (the kernel does not need a positive definite column)."""
    gs, k = case
    rng = _rng("toeplitz", gs, k)
    tcol = rng.standard_normal(sum(gs)).astype(real)
    V = rng.standard_normal((k, int(np.prod(gs)))).astype(real)
    return dict(tcol=tcol, V=V, scale=float(np.asarray(TOEPLITZ_SCALE, real)))


class _Gs:
    def __init__(self, gs):
        self.g = list(gs)


def spectral_inputs(case, real):
    """F [sum g^2], evals [sum g], V [k, m] in `real`.  "eigen": grid_ops.kron_eigen of an RBF column with its own length scale per
    dimension (0.8 .. 1.25 grid steps: eigenvalues within [2e-3, 4] per dimension, so no product leaves fp32's normal range), and
    the smallest eigenvalue of dimension 0 set to exactly 0: a whole slab of modes has lam = 0.  "dense": random dense factors,
    random positive eigenvalues; nothing about them is orthogonal or symmetric."""
    gs, k, kind = case
    rng = _rng("spectral", gs, k, kind)
    V = rng.standard_normal((k, int(np.prod(gs)))).astype(real)
    if kind == "eigen":
        import torch

        from online_gp_amd import grid_ops

        tcol = np.concatenate([np.exp(-0.5 * (np.arange(g) * (0.8 + 0.15 * q)) ** 2) for q, g in enumerate(gs)])
        tdt = torch.float32 if np.dtype(real) == np.dtype(F32) else torch.float64
        evec, evals = grid_ops.kron_eigen(_Gs(gs), torch.tensor(tcol, dtype=torch.float64), dtype=tdt)
        F, evals = evec.numpy().copy(), evals.numpy().copy()
        evals[0] = 0
    else:
        F = np.concatenate([rng.standard_normal(g * g) / np.sqrt(g) for g in gs]).astype(real)
        evals = rng.uniform(0.5, 2.0, sum(gs)).astype(real)
    return dict(F=F, evals=evals, V=V)


def spectral_params(params, real):
    """(power, rpower, shift, kscale) as the kernel receives them (0.8, 1.3 and 0.37 are rounded to `real` at the call)."""
    return tuple(float(np.asarray(p, real)) for p in params)


def probes(gs):
    """Exact probes of the innermost mode's line ends: tcol = e_s there and e_0 on the other modes, V = e_j within one line per
    column, scale 1; the product is e_{j-s} + e_{j+s} (e_j when s = 0) with the terms outside the line dropped, and every operation in
    it is exact in any precision.  Yields (s, tcol, V, expected) with one column per j in (0, 1, g - 2, g - 1)."""
    g, m = gs[-1], int(np.prod(gs))
    nlines = m // g
    for s in (0, 1, g - 1):
        tcol = np.concatenate([np.eye(gq)[s if q == len(gs) - 1 else 0] for q, gq in enumerate(gs)])
        js = (0, 1, g - 2, g - 1)
        V, want = np.zeros((len(js), m)), np.zeros((len(js), m))
        for c, j in enumerate(js):
            base = ((3 * c + 1) % nlines) * g
            V[c, base + j] = 1.0
            for i in ({j} if s == 0 else {j - s, j + s}):
                if 0 <= i < g:
                    want[c, base + i] = 1.0
        yield s, tcol, V, want


# ------------------------------------------------------------------------------- emulations in the kernels' operation order --
def _mac(acc, a, b, fma):
    """acc + a b in acc's type; fma: one rounding (the fp32 product is exact in fp64)."""
    if fma and acc.dtype == np.dtype(F32):
        return (acc.astype(F64) + np.asarray(a, F64) * np.asarray(b, F64)).astype(F32)
    return acc + a * b


def _emu_strided(coef, g, post, X, sc, fma):
    """k_toeplitz_mode / k_dense_mode: one thread and one accumulator per output e, i = (e / post) % g, sum over j of
    coef[i, j] * in[e - i post + j post], then * sc.  Flat indices as in the kernel (an index past m, which only a defect can make,
    reads 0)."""
    k, m = X.shape
    e = np.arange(m)
    i = (e // post) % g
    base = e - i * post
    acc = np.zeros((k, m), X.dtype)
    inside = int(base.max()) + (g - 1) * post < m
    for j in range(g):
        idx = base + j * post
        x = X[:, idx] if inside else np.where(idx < m, X[:, np.minimum(idx, m - 1)], X.dtype.type(0))
        acc = _mac(acc, coef[i, j][None, :], x, fma)
    return acc * X.dtype.type(sc)


def _emu_line(tc, g, X, sc, fma, mutant):
    """k_toeplitz_line_shfl: 64 lanes per line; up / dn move one lane per step with zeros entering at lanes 0 and 63 (a shuffle from
    outside the wave returns the lane's own value)."""
    k, m = X.shape
    real = X.dtype.type
    nlines, lanes = m // g, min(g, 64)
    v = np.zeros((k, nlines, 64), X.dtype)
    v[:, :, :lanes] = X.reshape(k, nlines, g)[:, :, :lanes]
    acc = tc[0] * v
    up, dn = v.copy(), v.copy()
    for sft in range(1, g):
        up = np.concatenate([up[..., :1], up[..., :-1]], axis=-1)
        dn = np.concatenate([dn[..., 1:], dn[..., -1:]], axis=-1)
        if mutant != "no zero at lane 0":
            up[..., 0] = 0
        if mutant != "no zero at lane 63":
            dn[..., 63] = 0
        acc = _mac(acc, tc[sft - 1] if mutant == "tcol[sft-1]" else tc[sft], up + dn, fma)
    acc = acc * real(sc)
    out = np.zeros((k, nlines, g), X.dtype)          # what a defect leaves unwritten reads 0
    out[:, :, :lanes] = acc[:, :, :lanes]
    if mutant == "no grid-stride loop":
        out[:, 4 * LINE_BLOCKS:] = 0
    return out.reshape(k, m)


def emu_toeplitz(gs, tcol, V, scale, fma=True, mutant=None):
    """launch_kron in V's precision: the same kernel choice, coefficient offsets, strides and placement of the scale."""
    d, st = len(gs), strides(gs)
    if mutant == "strides of two modes swapped" and d >= 3:
        st[0], st[1] = st[1], st[0]
    src, toff = V, 0
    for q, g in enumerate(gs):
        sc = scale if (q == d - 1 or mutant == "scale on every mode") else 1.0
        off = 0 if mutant == "mode q's coefficients at offset 0" else toff
        tc = tcol[off:off + g]
        if st[q] == 1 and (g <= LINE_MAX or (mutant == "line kernel at g = 65" and g == 65)):
            src = _emu_line(tc, g, src, sc, fma, mutant)
        else:
            src = _emu_strided(tc[np.abs(np.arange(g)[:, None] - np.arange(g)[None, :])], g, st[q], src, sc, fma)
        toff += g
    return src


def _emu_scale(gs, evals, m, real, kscale, shift, power, rpower, mutant):
    """k_spectral_scale: lam in `real`, the two powers in double and rounded to `real`, their product in `real`."""
    e = np.arange(m)
    lam = np.full(m, real(kscale))
    eoff = 0
    for q, (g, s) in enumerate(zip(gs, strides(gs))):
        lam = lam * evals[(eoff + (e // s) % g) % len(evals)]        # a defective offset wraps here, it reads foreign memory there
        eoff += g * g if mutant == "eigenvalue offset += g^2" else g
    f = np.ones(m, real)
    lam64 = lam.astype(F64)
    with np.errstate(divide="ignore", invalid="ignore"):
        if power != 0:
            p = np.power(lam64, float(real(power)))
            f = (p if mutant == "no lam > 0 guard" else np.where(lam > 0, p, 0.0)).astype(real)
        if rpower != 0:
            sh = 0.0 if mutant == "shift ignored" else float(real(shift))
            rw = float(real(rpower))
            f = f * np.power(1.0 + sh * lam64, rw if mutant == "sign of rpower" else -rw).astype(real)
    return f


def emu_spectral(gs, F, evals, V, kscale, shift, power, rpower, fma=True, mutant=None):
    """spectral_mm_impl in V's precision: d transposed mode products, the scaling, d plain mode products."""
    d, st, real = len(gs), strides(gs), V.dtype.type
    Fq = split(gs, F, square=True)
    f = _emu_scale(gs, evals, V.shape[1], real, kscale, shift, power, rpower, mutant)
    scale_after = d if mutant == "scaling one step late" else d - 1
    cur = V
    with np.errstate(invalid="ignore", over="ignore"):       # a defect may put an infinity into f
        for step in range(2 * d):
            q = step % d
            transposed = (step < d) != (mutant == "transposed flags swapped")
            cur = _emu_strided(Fq[q].T if transposed else Fq[q], gs[q], st[q], cur, 1.0, fma)
            if step == scale_after:
                cur = cur * f[None, :]
    return cur


# name -> product.  Each is one wrong variant of the emulations above; the host test shows that every one leaves the bound at some
# case of the tables, and which cases those are.
MUTANTS = {
    "no zero at lane 63": "toeplitz", "no zero at lane 0": "toeplitz", "tcol[sft-1]": "toeplitz", "scale on every mode": "toeplitz",
    "mode q's coefficients at offset 0": "toeplitz", "strides of two modes swapped": "toeplitz", "no grid-stride loop": "toeplitz",
    "line kernel at g = 65": "toeplitz",
    "transposed flags swapped": "spectral", "scaling one step late": "spectral", "eigenvalue offset += g^2": "spectral",
    "no lam > 0 guard": "spectral", "sign of rpower": "spectral", "shift ignored": "spectral",
}
