"""Test infrastructure of the dense regime's edge tests (no GPU needed, nothing shared with the kernels):

  * `window` / `outside_unchanged`: operands and outputs as windows of larger parent buffers -- a leading dimension larger than
    the row, a base pointer off the 16-byte grid -- with everything outside the window compared BITWISE afterwards;
  * fp64 references of the GEMM, the Cholesky factorisation, the triangular solves and the rank-q root update, always from the
    inputs CAST to the tested dtype (the kernel and the reference then start from the same numbers);
  * `int_operands`: integer-valued matrices whose products are exact in fp32, for comparisons without a tolerance;
  * two SPD families (`well`: R R^T / n + I, condition ~5; `graded`: Q diag(lambda) Q^T with lambda log-spaced in [1, kappa]) and
    two non-PD constructions whose failing pivot is known (`first_pivot_fails`, `last_pivot_fails`);
  * `eta`, `rho`, `skeel`: the normalised backward errors of a factor and of a solve (Higham, Accuracy and Stability of Numerical
    Algorithms, Thm 10.3 / Thm 8.5) and the Skeel condition number of the factor that bounds a solve through explicit inverses
    (Du Croz & Higham, Stability of methods for matrix inversion, 1992), and `lapack_same_precision`, the yardstick the GPU
    figures are judged against: LAPACK's own factor and solve in the tested dtype on the same matrix.
"""
import functools

import numpy as np
import torch

U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}          # unit roundoff
KAPPA = {torch.float32: 1e4, torch.float64: 1e10}                   # condition number of the graded family, per dtype
_INT = {torch.float32: torch.int32, torch.float64: torch.int64}


# ------------------------------------------------------------------------------------------------ windows ---
def window(rows, cols, ld, lead, dtype, fill, device="cpu"):
    """(parent, view): a 1-D parent buffer and the [rows, cols] view into it with row stride `ld`, starting `lead` elements
    into the body.  fill = "nan": the parent is all NaN (an operand: a read outside the window poisons the result).
    fill = "pattern": the parent holds the finite pattern -(1000 + index % 97) (an output: a stray write shows), with a canary
    of NaN before and after the body (a multiple of four elements, so that lead = 0 keeps the view 16-byte aligned).  The body
    is lead + rows * ld elements: the last row has its padding too."""
    assert ld >= cols >= 0 and rows >= 0 and lead >= 0 and fill in ("nan", "pattern")
    canary = 0 if fill == "nan" else -(-max(ld, 1) // 4) * 4
    total = canary + lead + rows * ld + canary + 4
    if fill == "nan":
        parent = torch.full((total,), float("nan"), dtype=dtype)
    else:
        parent = (-(1000.0 + torch.arange(total, dtype=torch.float64) % 97)).to(dtype)
        parent[:canary] = float("nan")
        parent[total - canary - 4:] = float("nan")
    parent = parent.to(device)
    return parent, parent.as_strided((rows, cols), (ld, 1), canary + lead)


def bits(t):
    return t.view(_INT[t.dtype])


def outside_mask(parent, view):
    m = torch.ones(parent.numel(), dtype=torch.bool, device=parent.device)
    m.as_strided(tuple(view.shape), view.stride(), view.storage_offset()).fill_(False)
    return m


def outside_unchanged(parent_before, parent_after, view):
    """True when every element of the parent outside `view` has the same BITS before and after (NaN canaries compare equal
    to themselves, and a NaN overwritten by a NaN of another payload does not)."""
    m = outside_mask(parent_after, view)
    return bool(torch.equal(bits(parent_before)[m], bits(parent_after)[m]))


# --------------------------------------------------------------------------------------------- references ---
def gemm_ref(alpha, A, ta, B, tb, beta, C, dtype):
    """alpha op(A) op(B) + beta C in fp64 from the values the kernel gets (operands and coefficients cast to `dtype`)."""
    a, b = (float(torch.tensor(v, dtype=dtype)) for v in (alpha, beta))
    P = (A.t() if ta else A).double() @ (B.t() if tb else B).double()
    return a * P + (b * C.double() if b != 0.0 else 0.0)


def chol_ref(A):
    return torch.linalg.cholesky(A.double())


def solve_ref(L, B, trans):
    L, B = L.double(), B.double()
    return torch.linalg.solve_triangular(L.t() if trans else L, B, upper=bool(trans))


def root_update_ref(L, V):
    """The Gram matrix a rank-q root update must reach: L L^T + V V^T (roots are only defined up to a right orthogonal factor)."""
    return L.double() @ L.double().t() + V.double() @ V.double().t()


def int_exact(K, amax=8):
    """Products of K terms bounded by amax^2, plus one more operand of size amax, stay below 2^24: exact in fp32 in any order."""
    return K * amax * amax + amax < 2 ** 24


def int_operands(shape, rng, amax=8, K=None):
    """Integer-valued fp64 matrix in [-amax, amax]; K: the length of the sums it takes part in (default: its longest side)."""
    K = max(shape) if K is None else K
    assert int_exact(K, amax), (K, amax)
    return torch.as_tensor(rng.integers(-amax, amax + 1, size=shape).astype(np.float64))


# ------------------------------------------------------------------------------------------ SPD families ---
def well(n, seed=0):
    g = torch.Generator(device="cpu").manual_seed(1000 + n + 7919 * seed)
    R = torch.randn(n, n, generator=g, dtype=torch.float64)
    return R @ R.t() / n + torch.eye(n, dtype=torch.float64)


def graded(n, kappa, seed=0):
    """Q diag(lambda) Q^T, lambda log-spaced in [1, kappa], Q from the QR of a seeded Gaussian (fp64, symmetric to the bit)."""
    rng = np.random.default_rng(4000 + n + 7919 * seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(0.0, np.log10(kappa), n) if n > 1 else np.ones(1)
    A = (Q * lam[None, :]) @ Q.T
    return torch.as_tensor(0.5 * (A + A.T))


def rhs(n, nrhs, seed=0):
    g = torch.Generator(device="cpu").manual_seed(50000 + 31 * n + nrhs + 7919 * seed)
    return torch.randn(n, nrhs, generator=g, dtype=torch.float64)


def first_pivot_fails(A):
    A = A.clone()
    A[0, 0] = -1.0
    return A


def last_pivot_fails(A, dtype):
    """A (fp64, SPD) with A[n-1, n-1] halved until the last Schur complement of the matrix CAST to dtype is negative by at least
    1 % of the quantity it is the difference of; the leading (n-1) minor is untouched and stays positive definite."""
    A = A.clone()
    n = A.shape[0]
    assert n >= 2
    Ac = A.to(dtype).double().numpy()
    L11 = np.linalg.cholesky(Ac[:n - 1, :n - 1])                    # raises if the minor is not PD
    w = np.linalg.solve(L11, Ac[n - 1, :n - 1])
    ww = float(w @ w)
    ann = float(A[n - 1, n - 1])
    while float(torch.tensor(ann, dtype=dtype)) - ww >= -1e-2 * ww:
        ann *= 0.5
    A[n - 1, n - 1] = ann
    return A


def failing_pivot(A):
    """Index of the first non-positive pivot of the fp64 factorisation of A (numpy, unblocked), or -1."""
    a = A.double().numpy().copy()
    n = a.shape[0]
    for k in range(n):
        if not a[k, k] > 0:
            return k
        a[k, k] = np.sqrt(a[k, k])
        a[k + 1:, k] /= a[k, k]
        a[k + 1:, k + 1:] -= np.outer(a[k + 1:, k], a[k + 1:, k])
    return -1


# ------------------------------------------------------------------------------------------------- errors ---
def eta(A, L, u, Lref=None):
    """max_ij |A - L L^T|_ij / ((n + 1) u (|Lref| |Lref^T|)_ij): the componentwise backward error of a Cholesky factor in units
    of the bound of Higham Thm 10.3 (<= 1 for the textbook algorithm up to second order), Lref the fp64 factor of A."""
    A, L = A.double(), L.double()
    Lref = chol_ref(A) if Lref is None else Lref.double()
    n = A.shape[0]
    den = (n + 1) * u * (Lref.abs() @ Lref.abs().t())
    return float(((A - L @ L.t()).abs() / den).max())


def rho(L, X, B, u, Lref, Xref):
    """max |L X - B| / (n u (|Lref| |Xref|)), per element: the residual of a triangular solve in units of the bound of
    substitution (Higham Thm 8.5)."""
    L, X, B, Lref, Xref = (t.double() for t in (L, X, B, Lref, Xref))
    n = L.shape[0]
    den = n * u * (Lref.abs() @ Xref.abs())
    return float(((L @ X - B).abs() / den).max())


def skeel(Lref):
    """|| |Lref^-1| |Lref| ||_inf: what a solve through explicit inverses may lose over substitution (Du Croz & Higham)."""
    Lref = Lref.double()
    Li = torch.linalg.solve_triangular(Lref, torch.eye(Lref.shape[0], dtype=torch.float64, device=Lref.device), upper=False)
    return float((Li.abs() @ Lref.abs()).sum(1).max())


@functools.lru_cache(maxsize=None)
def graded_case(n, dtype, nrhs=5):
    """The conditioning case of size n in `dtype`, everything on the CPU and computed once: the cast matrix A and right-hand sides B,
    the fp64 factor and solution, and the figures of the same-precision LAPACK factor / solve (`eta_ref`, `rho_ref`)."""
    u = U[dtype]
    A = graded(n, KAPPA[dtype]).to(dtype)
    B = rhs(n, nrhs).to(dtype)
    Lref = chol_ref(A)
    Xref = solve_ref(Lref, B, False)
    Llp = torch.linalg.cholesky(A)                                   # LAPACK potrf in the tested dtype
    Xlp = torch.linalg.solve_triangular(Llp, B, upper=False)         # LAPACK / BLAS trsm in the tested dtype
    return dict(A=A, B=B, Lref=Lref, Xref=Xref, u=u, eta_ref=eta(A, Llp, u, Lref), rho_ref=rho(Llp, Xlp, B, u, Lref, Xref),
                skeel=skeel(Lref))


# ------------------------------------------------------------------------------------- the GEMM case table ---
# (dtypes, (M, N, K), kernel): 0 k_gemm, 1 k_gemm32, 2 k_gemm128 on 64-tiles, 3 k_gemm128 on 128-tiles -- the smallest shapes on
# either side of every threshold of the dispatch (online_gp_amd/csrc/dense.hip: gemm_path), plus the degenerate ones.
BOTH = (torch.float32, torch.float64)
F32, F64 = (torch.float32,), (torch.float64,)
GEMM_TABLE = [
    (BOTH, (1, 1, 1), 0),
    (BOTH, (1, 200, 70), 0),
    (BOTH, (200, 1, 70), 0),
    (BOTH, (64, 127, 64), 0),          # M N < 8192
    (BOTH, (64, 128, 63), 0),
    (BOTH, (64, 128, 64), 1),
    (BOTH, (130, 70, 0), 0),
    (BOTH, (130, 70, 1), 0),
    (BOTH, (130, 70, 17), 0),
    (F64, (960, 1024, 127), 1),
    (F64, (960, 1024, 128), 2),        # 240 tiles
    (F64, (1920, 1920, 128), 2),       # 900 tiles
    (F64, (1920, 1984, 128), 0),
    (F64, (1920, 1984, 255), 0),
    (F64, (1920, 1984, 256), 3),
    (F32, (640, 704, 127), 1),
    (F32, (640, 704, 128), 2),         # 110 tiles
    (F32, (1600, 2048, 128), 2),       # 800 tiles
    (F32, (1728, 1920, 255), 0),
    (F32, (1728, 1920, 256), 3),
]
GEMM_CASES = [(dt, shape, path) for dts, shape, path in GEMM_TABLE for dt in dts]
INT_COEFFS = [(1.0, 0.0), (1.0, 1.0), (-1.0, 1.0), (0.5, 0.0)]


def old_gemm_dispatch(M, N, K, elem_bytes, small_max_env=0):
    """The conditions of launch_gemm as they stood before the selection moved into one host function, written out again."""
    f64 = elem_bytes == 8
    nb64 = ((N + 63) // 64) * ((M + 63) // 64)
    p_min, p_max = (240, 900) if f64 else (110, 800)
    if p_min <= nb64 <= p_max and K >= 128:
        return 2
    small_max = small_max_env if small_max_env > 0 else (500 if f64 else 300)
    if nb64 < small_max and K >= 64 and M * N >= 32 * 32 * 8:
        return 1
    nb = ((N + 127) // 128) * ((M + 127) // 128)
    if nb >= (128 if f64 else 32) and K >= 256:
        return 3
    return 0
