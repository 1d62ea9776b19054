"""TEST INFRASTRUCTURE -- analytic reference of the cubic interpolation rows and of their derivative w.r.t. the points, plus the
case builders shared by tests/test_interp_reference_host.py (checks of this reference, no GPU) and
tests/test_interp_derivatives_gpu.py (the five derivative kernels against it).

Everything here is a plain restatement on the CPU of the documented rules, independent of every kernel and of grid_ops' wrappers:

* grid of dim q: nodes ``g0[q] + j h[q]``, j = 0 .. g[q] - 1 (``GridSpec``); dim 0 is the slowest of the flat index;
* value weights: the Keys cubic (a = -0.5) on the four nodes ``floor(u) - 1 .. floor(u) + 2``, ``u = (x - g0) / h``;
* one-hot boundary rule (oracle/spec.py:interp_1d_dense): a point in the first or the last cell of a dim (``floor(u) < 1`` or
  ``floor(u) >= g - 2``) has weight 1 on its nearest node of that dim.  Cell convention: a cell is ``[node j, node j+1)``, so a
  point exactly on node 1 belongs to the first interior cell and a point exactly on node g - 2 to the last (boundary) cell;
* derivative weights: ``k'(s) / h`` on the same four nodes, ZERO in dim q when the point is in a boundary cell of dim q (the
  kernels' stated convention: the one-hot rule is piecewise constant);
* a point outside the grid (``x < g0`` or ``x > g0 + h (g - 1)`` in any dim) has a zero row and a zero gradient.

The functions run in the dtype of ``x``: fp64 is the reference; in fp32 (``g0``, ``h`` rounded to fp32 as ``GridDev<float>``
receives them, ``u`` and the polynomials in fp32) they are the "fp32 restatement" from which the fp32 tolerance is measured.
"""
import numpy as np
import torch

EPS64 = 2.0 ** -52
EPS32 = 2.0 ** -23
C_ROUND = 8.0            # the few roundings inside each weight (d cubic polynomials, one division by h)
ROW_LDS_BYTES = 32768    # the row form of the bilinear kernels needs its K rows in this much LDS
SPB_KMAX = 32


# ------------------------------------------------------------------------------------------------------ the piecewise cubic
def keys(s):
    a = s.abs()
    near = ((1.5 * a - 2.5) * a) * a + 1.0
    far = ((-0.5 * a + 2.5) * a - 4.0) * a + 2.0
    return torch.where(a <= 1.0, near, torch.where(a < 2.0, far, torch.zeros_like(a)))


def keys_deriv(s):
    """d/ds of :func:`keys`, written out: sign(s) (4.5 a^2 - 5 a) for a <= 1, sign(s) (-1.5 a^2 + 5 a - 4) for 1 < a < 2."""
    a = s.abs()
    sg = torch.where(s < 0, -torch.ones_like(s), torch.ones_like(s))
    near = (4.5 * a - 5.0) * a
    far = (-1.5 * a + 5.0) * a - 4.0
    return torch.where(a <= 1.0, sg * near, torch.where(a < 2.0, sg * far, torch.zeros_like(a)))


def keys_terms(s):
    """:func:`keys` with every term of the polynomial replaced by its absolute value: the magnitude that the roundings inside a
    weight are relative to.  Near a node the off-node weights vanish by cancellation (k(1) = k(2) = 0 with terms of size 2..24), so
    their rounding error is eps times THIS, not eps times their value."""
    a = s.abs()
    near = ((1.5 * a + 2.5) * a) * a + 1.0
    far = ((0.5 * a + 2.5) * a + 4.0) * a + 2.0
    return torch.where(a <= 1.0, near, torch.where(a < 2.0, far, torch.zeros_like(a)))


def rows_1d(g0, h, g, x, terms=False):
    """Dense value rows W [n, g], derivative rows dW [n, g] and the inside mask [n] of one dim, in x's dtype.  terms=True: the
    cubic value weights replaced by keys_terms (the one-hot weights are exact and stay)."""
    dt = x.dtype
    g0 = torch.tensor(float(g0), dtype=torch.float64).to(dt)
    h = torch.tensor(float(h), dtype=torch.float64).to(dt)
    hi = g0 + h * torch.tensor(float(g - 1), dtype=dt)
    n = x.shape[0]
    u = (x - g0) / h
    fl = torch.floor(u)
    t = u - fl
    inside = (x >= g0) & (x <= hi)
    j0 = torch.where(inside, fl, torch.zeros_like(fl)).to(torch.int64) - 1
    interior = inside & (j0 >= 0) & (j0 <= g - 4)
    bnd = inside & ~interior
    c = torch.arange(4, dtype=dt)
    s = (t[:, None] + 1.0) - c[None, :]
    zero = torch.zeros((n, 4), dtype=dt)
    taps = torch.where(interior[:, None], keys_terms(s) if terms else keys(s), zero)
    dtaps = torch.where(interior[:, None], keys_deriv(s) / h, zero)
    idx = (j0[:, None] + torch.arange(4)[None, :]).clamp(0, g - 1)
    W = torch.zeros((n, g), dtype=dt).scatter_add_(1, idx, taps)
    dW = torch.zeros((n, g), dtype=dt).scatter_add_(1, idx, dtaps)
    base = torch.where(j0 < 0, torch.zeros_like(j0), torch.full_like(j0, g - 4))
    dist = (g0 + h * (base[:, None] + torch.arange(4)[None, :]).to(dt) - x[:, None]).abs()
    best = base + torch.argmin(dist, dim=1)
    W[bnd, best[bnd]] = 1.0
    return W, dW, inside


def rows_per_dim(grid, x, terms=False):
    """([W_q [n, g_q]], [dW_q [n, g_q]]) with the rows of a point outside the grid (in any dim) zeroed in every dim."""
    parts = [rows_1d(grid.g0[q], grid.h[q], grid.g[q], x[:, q], terms) for q in range(grid.d)]
    ok = torch.stack([p[2] for p in parts], 0).all(0)
    Ws = [torch.where(ok[:, None], p[0], torch.zeros_like(p[0])) for p in parts]
    dWs = [torch.where(ok[:, None], p[1], torch.zeros_like(p[1])) for p in parts]
    return Ws, dWs


def _kron_rows(fs):
    out = fs[0]
    for f in fs[1:]:
        out = (out[:, :, None] * f[:, None, :]).reshape(out.shape[0], -1)
    return out


def dense_rows(grid, x):
    """W [n, m]: the interpolation rows (product of the per-dim rows, dim 0 slowest)."""
    return _kron_rows(rows_per_dim(grid, x)[0])


def dense_row_grads(grid, x):
    """dW [n, d, m]: d W[p, :] / d x[p, q] -- k'(s) / h in dim q times the other dims' value weights."""
    Ws, dWs = rows_per_dim(grid, x)
    return torch.stack([_kron_rows([dWs[o] if o == q else Ws[o] for o in range(grid.d)]) for q in range(grid.d)], 1)


def dense_both(grid, x):
    """(W, dW) as fp64 tensors, evaluated in x's dtype (weights and their products across dims in that dtype)."""
    Ws, dWs = rows_per_dim(grid, x)
    dW = torch.stack([_kron_rows([dWs[o] if o == q else Ws[o] for o in range(grid.d)]) for q in range(grid.d)], 1)
    return _kron_rows(Ws).double(), dW.double()


# ------------------------------------------------------------------------------------- the five operations, by dense matmuls
# Each takes fp64 operands; called once with the operands (the result) and once with their absolute values (S_abs).
def op_gather_grad(dW, V, diag):
    return torch.einsum("pqm,pm->pq", dW, V) if diag else dW @ V.reshape(-1)


def op_gather_rows(W, Vr):
    return W @ Vr


def op_gather_rows_vjp(dW, Vr, G):
    n, d, m = dW.shape
    return ((dW.reshape(n * d, m) @ Vr).reshape(n, d, -1) * G[:, None, :]).sum(-1)


def op_bilinear(WL, A, WR):
    return WL @ A @ WR.transpose(-1, -2)


def op_bilinear_vjp_left(dWL, A, WR, G):
    """gL[s, a, k] = sum_b G[s, a, b] dW_L[s, a, k] A W_R[s, b]."""
    return torch.einsum("sakm,smb,sab->sak", dWL, A @ WR.transpose(-1, -2), G)


def op_bilinear_vjp_right(WL, A, dWR, G):
    """gR[s, b, k] = sum_a G[s, a, b] W_L[s, a] A dW_R[s, b, k]."""
    return torch.einsum("sam,sbkm,sab->sbk", WL @ A, dWR, G)


def op_basis(Ws, dWs, Vs, Ks, S, scale, colscale, GF, Gprior):
    """(F [n, r], prior [n], gx [n, d]) of the tensor-product basis projection, from the per-dim 1-D rows."""
    d, n = len(Ws), Ws[0].shape[0]
    P = [Ws[q] @ Vs[q] for q in range(d)]
    dP = [dWs[q] @ Vs[q] for q in range(d)]
    Pj = [P[q][:, S[q]] for q in range(d)]
    dPj = [dP[q][:, S[q]] for q in range(d)]
    sc = scale[:, None] * colscale[None, :]
    F = sc.clone()
    for q in range(d):
        F = F * Pj[q]
    qf = [((Ws[q] @ Ks[q]) * Ws[q]).sum(1) for q in range(d)]
    dqf = [2.0 * ((dWs[q] @ Ks[q]) * Ws[q]).sum(1) for q in range(d)]
    prior = torch.ones(n, dtype=torch.float64)
    for q in range(d):
        prior = prior * qf[q]
    gx = torch.zeros((n, d), dtype=torch.float64)
    for q in range(d):
        t = sc * GF * dPj[q]
        tp = Gprior * dqf[q]
        for o in range(d):
            if o != q:
                t = t * Pj[o]
                tp = tp * qf[o]
        gx[:, q] = t.sum(1) + tp
    return F, prior, gx


# ----------------------------------------------------------------------------------------------------------------- tolerances
class Ref:
    """Reference result, its S_abs (the same expression with every factor replaced by its absolute value), the number N of
    accumulated terms and, for fp32 cases, the fp32 restatement of the reference."""

    def __init__(self, ref, sabs, N, ref32=None, s1=None):
        self.ref, self.sabs, self.N, self.ref32, self.s1 = ref, sabs, N, ref32, s1

    def bound64(self):
        """8 N eps64 S_abs.  The two forwards that are single products of weights (basis_project's F, interp_bilinear) carry s1 and
        get 8 eps64 (N S_abs + S_1): S_1 is first order in the roundings inside the weights -- the sum, over one cubic weight at a
        time, of S_abs with THAT weight replaced by keys_terms (the size of its polynomial's terms, which its rounding is relative
        to) and every other factor by its absolute value.  S_1 is about 30 S_abs per weight in the product, so the bound stays within
        a small factor of 8 N eps64 S_abs (about 8.5 for F, below 5 for the bilinear form) in every dimension."""
        return C_ROUND * EPS64 * (self.N * self.sabs + (0 if self.s1 is None else self.s1))

    def dev32(self):
        return float((self.ref32 - self.ref).abs().max())

    def tol32(self):
        return C_ROUND * max(self.dev32(), EPS32 * float(self.sabs.max()))


def check(got, R, label):
    """fp64 (R.ref32 None): |got - ref| <= 8 N eps64 S_abs per element (Ref.bound64: plus the first-order weight term for the two
    forwards, where the ratio to 8 N eps64 S_abs alone is printed too).  fp32: max|got - ref| <= 8 max(dev32, eps32 max S_abs).
    Always: finite, and exactly zero wherever S_abs is zero (boundary-cell dims, points outside the grid).  Prints the head-room."""
    got = got.detach().double().cpu()
    assert got.shape == R.ref.shape, (label, got.shape, R.ref.shape)
    assert bool(torch.isfinite(got).all()), label
    assert float(R.sabs.max()) > 0, label
    assert bool((got[R.sabs == 0] == 0).all()), label + ": non-zero where the reference is identically zero"
    err = (got - R.ref).abs()
    if R.ref32 is None:
        bound = R.bound64()
        lit = float((err / (C_ROUND * R.N * EPS64 * R.sabs).clamp_min(1e-300)).max())
        ratio = float((err / bound.clamp_min(1e-300)).max())
        print(f"{label}: fp64 max err/bound {ratio:.3f} (N = {R.N}; against 8 N eps64 S_abs alone {lit:.3f})")
        assert bool((err <= bound).all()), f"{label}: err/bound {ratio:.3f}"
        return ratio
    dev, tol = R.dev32(), R.tol32()
    e = float(err.max())
    print(f"{label}: fp32 max err {e:.3e}  dev32 {dev:.3e}  got/dev32 {e / max(dev, 1e-300):.3f}  err/tol {e / tol:.3f}")
    assert e <= tol, f"{label}: {e:.3e} > {tol:.3e}"
    return e / max(dev, 1e-300)


# ------------------------------------------------------------------------------------------------------------- grids, points
GRIDS = {
    "d1g37": ([[-0.3, 2.0]], (37,)),
    "d2g9x31": ([[0.0, 1.0], [-4.0, 7.0]], (9, 31)),
    "d3g20x5x11": ([[-1.0, 1.0], [0.0, 0.25], [10.0, 13.0]], (20, 5, 11)),
    "d4g5x7x4x6": ([[-2.0, 1.0], [0.5, 0.75], [100.0, 108.0], [-0.01, 0.02]], (5, 7, 4, 6)),
}
BIG_GRIDS = {
    "d2g50": ([[-1.0, 1.0]] * 2, (50, 50)),       # m = 2500
    "d3g12": ([[-1.0, 1.0]] * 3, (12, 12, 12)),   # m = 1728
}
ALL_GRIDS = dict(GRIDS, **BIG_GRIDS)
DTYPES = {"f64": torch.float64, "f32": torch.float32}


def make_grid(name):
    from online_gp_amd import grid_ops

    gb, g = ALL_GRIDS[name]
    return grid_ops.GridSpec(torch.tensor(gb, dtype=torch.float64), list(g))


def seed_of(*parts):
    """A stable seed from the parts of a case id (Python's hash() of a str changes between runs)."""
    s = 0
    for ch in "|".join(str(p) for p in parts):
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


MARGIN = 1e-2      # interior coordinates stay this far (in units of h) from node 1, node g - 2 and the boundary cells' midpoints


def _interior_u(rng, g):
    return rng.uniform(1.0 + MARGIN, g - 2.0 - MARGIN)


def _boundary_u(rng, g):
    """A coordinate strictly inside the first or the last cell, away from its two nodes and from its midpoint (where the nearest
    node changes: the one-hot rule is discontinuous there, as at node 1 and node g - 2)."""
    t = rng.uniform(0.05, 0.45) if rng.random() < 0.5 else rng.uniform(0.55, 0.95)
    return t if rng.random() < 0.5 else g - 2.0 + t


KINDS = ("interior", "node1", "nodes_some", "nodes_all", "boundary_some", "interior", "switch")


def make_points(grid, n, rng, dtype, outside=False):
    """[n, d] points in `dtype` (built in fp64, rounded), rows cycling through KINDS:
    interior       random interior coordinates in every dim;
    node1 / nodes_some / nodes_all
                   exactly on an interior node (g0 + j h as GridSpec.grid_points computes it, 2 <= j <= g - 3) in one / all but
                   one / all dims, interior elsewhere (a dim with g = 4 has no such node and stays interior);
    boundary_some  inside a boundary cell in a random non-empty subset of the dims (a proper subset when d > 1), interior elsewhere;
    switch         fp64 only: exactly on node 1 or node g - 2 of one dim (fp32 rows of this kind are interior: the function is
                   discontinuous there, so fp32 inputs keep 1e-3 h away -- here MARGIN = 1e-2 h).
    outside=True: every third row (i % 3 == 1, k = i // 3) is additionally moved out of the grid in dim (k // 2) % d, below the first
    node (k even) or above the last (k odd); n >= 6 d covers both sides of every dim."""
    d = grid.d
    nodes = grid.grid_points()
    x = np.empty((n, d))
    for i in range(n):
        kind = KINDS[i % len(KINDS)]
        for q in range(d):
            x[i, q] = grid.g0[q] + grid.h[q] * _interior_u(rng, grid.g[q])
        perm = rng.permutation(d)
        if kind in ("node1", "nodes_some", "nodes_all"):
            k = {"node1": 1, "nodes_some": max(1, d - 1), "nodes_all": d}[kind]
            for q in perm[:k]:
                if grid.g[q] >= 5:
                    x[i, q] = float(nodes[q][int(rng.integers(2, grid.g[q] - 2))])
        elif kind == "boundary_some":
            k = 1 if d == 1 else int(rng.integers(1, d))
            for q in perm[:k]:
                x[i, q] = grid.g0[q] + grid.h[q] * _boundary_u(rng, grid.g[q])
        elif kind == "switch" and dtype == torch.float64:
            q = int(perm[0])
            x[i, q] = float(nodes[q][1 if rng.random() < 0.5 else grid.g[q] - 2])
        if outside and i % 3 == 1:
            k = i // 3
            q = (k // 2) % d
            x[i, q] = grid.g0[q] - 0.3 * grid.h[q] if k % 2 == 0 else grid.g0[q] + grid.h[q] * (grid.g[q] - 1 + 0.3)
    return torch.as_tensor(x, dtype=torch.float64).to(dtype)


def normal(rng, shape, dtype):
    return torch.as_tensor(rng.standard_normal(shape), dtype=torch.float64).to(dtype)


def _refs(dtype, f, x):
    """(W, dW) in fp64 on the (rounded) points, and the fp32 restatement when the case is fp32."""
    W, dW = f(x.double())
    if dtype == torch.float32:
        return W, dW, f(x)
    return W, dW, None


# ------------------------------------------------------------------------------------------------------------- case builders
GATHER_GRAD_N = (1, 255, 256, 257, 5000)


def gather_grad_case(gname, dname, n, diag, outside=False):
    grid, dtype = make_grid(gname), DTYPES[dname]
    rng = np.random.default_rng(seed_of("gg", gname, dname, n, diag, outside))
    x = make_points(grid, n, rng, dtype, outside)
    V = normal(rng, (n, grid.m) if diag else (grid.m,), dtype)
    W, dW, r32 = _refs(dtype, lambda xx: dense_both(grid, xx), x)
    Vd = V.double()
    R = Ref(op_gather_grad(dW, Vd, diag), op_gather_grad(dW.abs(), Vd.abs(), diag), grid.T,
            None if r32 is None else op_gather_grad(r32[1], Vd, diag))
    return dict(grid=grid, x=x, V=V, R=R)


ROWS_VJP_NCOLS = (1, 2, 63, 64, 65, 256, 257, 600)
ROWS_VJP_N = (1, 97)


def gather_rows_vjp_case(gname, dname, n, ncols, outside=False):
    grid, dtype = make_grid(gname), DTYPES[dname]
    rng = np.random.default_rng(seed_of("grv", gname, dname, n, ncols, outside))
    x = make_points(grid, n, rng, dtype, outside)
    Vr = normal(rng, (grid.m, ncols), dtype)
    G = normal(rng, (n, ncols), dtype)
    W, dW, r32 = _refs(dtype, lambda xx: dense_both(grid, xx), x)
    Vd, Gd = Vr.double(), G.double()
    R = Ref(op_gather_rows_vjp(dW, Vd, Gd), op_gather_rows_vjp(dW.abs(), Vd.abs(), Gd.abs()), grid.T * ncols,
            None if r32 is None else op_gather_rows_vjp(r32[1], Vd, Gd))
    return dict(grid=grid, x=x, Vr=Vr, G=G, R=R)


def sym_table(rng, m, dtype, lda=None):
    """A symmetric, indefinite table with entries of varying magnitude: D (B + B^T) D, D = diag(10 ** uniform(-2, 2)).  Rounded to
    `dtype` (rounding keeps it symmetric).  With lda > m: the leading m columns of an [m, lda] buffer whose padding is NaN."""
    B = rng.standard_normal((m, m))
    D = 10.0 ** rng.uniform(-2, 2, m)
    A = torch.as_tensor(D[:, None] * (B + B.T) * D[None, :], dtype=torch.float64).to(dtype)
    if lda is None:
        return A, A
    buf = torch.full((m, lda), float("nan"), dtype=dtype)
    buf[:, :m] = A
    return A, buf


def grid_sizes(gname):
    """(d, m, T) of a named grid, by arithmetic alone (usable while tests are collected, before the package is imported)."""
    g = ALL_GRIDS[gname][1]
    return len(g), int(np.prod(g)), 4 ** len(g)


def bilinear_forms(gname, dtype, qL, qR):
    """('pair' | 'row') of the forward, the left VJP and the right VJP: the two inequalities of use_row_form -- more (other point,
    tap) pairs than table columns, and the K rows (1 in the forward, d in the VJP) fit in 32 KiB of LDS."""
    size = 8 if dtype == torch.float64 else 4
    d, m, T = grid_sizes(gname)

    def form(n_other, K):
        return "row" if n_other * T > m and K * m * size <= ROW_LDS_BYTES else "pair"

    return form(qR, 1), form(qR, d), form(qL, d)


def bilinear_shapes(gname):
    """(qL, qR, nb, sym) per grid: with k = m // T, c in {k-1, k, k+1} puts c T one step below m, on it (or on the last multiple of
    T below it) and above it -- as the number of other points of the forward / left VJP (qR = c) and of the right VJP (qL = c),
    and as q of the symmetric mode; d = 4 adds qR in {1, 2, 3, 5}; the large tables take a qR that needs the row form."""
    d, m, T = grid_sizes(gname)
    if gname in BIG_GRIDS:
        c = m // T + 4
        return [(2, c, 1, False), (c, 3, 1, False), (c, c, 1, True)]
    k = m // T
    cs = [c for c in (k - 1, k, k + 1) if c >= 1]
    if d == 4:
        cs = sorted(set(cs) | {1, 2, 3, 5})
    out = []
    for i, c in enumerate(cs):
        for shape in ((2, c, (1, 7)[i % 2], False), (c, 3, (7, 1)[i % 2], False), (c, c, (1, 7)[i % 2], True)):
            if shape[:2] + shape[3:] not in [o[:2] + o[3:] for o in out]:
                out.append(shape)
    return out


def bilinear_case(gname, dname, qL, qR, nb, sym, lda_pad=0, outside=False):
    grid, dtype = make_grid(gname), DTYPES[dname]
    rng = np.random.default_rng(seed_of("bil", gname, dname, qL, qR, nb, sym, lda_pad, outside))
    m, d = grid.m, grid.d
    A, Abuf = sym_table(rng, m, dtype, m + lda_pad if lda_pad else None)
    xL = make_points(grid, nb * qL, rng, dtype, outside).reshape(nb, qL, d)
    xR = None if sym else make_points(grid, nb * qR, rng, dtype, outside).reshape(nb, qR, d)
    G = normal(rng, (nb, qL, qR), dtype)

    def rows(xx):
        W, dW = dense_both(grid, xx.reshape(-1, d))
        return W.reshape(nb, -1, m), dW.reshape(nb, -1, d, m)

    def rows_one_term(xx):
        """sum over the dims of the value rows with that one dim's cubic weights replaced by keys_terms, the others absolute."""
        Ws = [w.abs() for w in rows_per_dim(grid, xx.reshape(-1, d))[0]]
        Wt = rows_per_dim(grid, xx.reshape(-1, d), True)[0]
        return sum(_kron_rows([Wt[o] if o == q else Ws[o] for o in range(d)]) for q in range(d)).reshape(nb, -1, m)

    xRr = xL if sym else xR
    WL, dWL = rows(xL.double())
    WR, dWR = rows(xRr.double())
    Ad, Gd = A.double(), G.double()
    T2 = grid.T * grid.T

    def three(WL, dWL, WR, dWR, A, G):
        gl, gr = op_bilinear_vjp_left(dWL, A, WR, G), op_bilinear_vjp_right(WL, A, dWR, G)
        return op_bilinear(WL, A, WR), gl, gr

    r = three(WL, dWL, WR, dWR, Ad, Gd)
    s = three(WL.abs(), dWL.abs(), WR.abs(), dWR.abs(), Ad.abs(), Gd.abs())
    s1 = None                       # the forward's first-order weight term: needed by the fp64 bound only
    if dtype == torch.float64:
        s1 = op_bilinear(rows_one_term(xL), Ad.abs(), WR.abs()) + op_bilinear(WL.abs(), Ad.abs(), rows_one_term(xRr))
    r32 = (None, None, None)
    if dtype == torch.float32:
        WL3, dWL3 = rows(xL)
        WR3, dWR3 = rows(xRr)
        r32 = three(WL3, dWL3, WR3, dWR3, Ad, Gd)
    out = dict(grid=grid, A=A, Abuf=Abuf, xL=xL, xR=xR, G=G, fwd=Ref(r[0], s[0], T2, r32[0], s1))
    if sym:           # the whole gradient of x (both roles) in one output: 2 T^2 q terms
        out["gL"] = Ref(r[1] + r[2], s[1] + s[2], 2 * T2 * qR, None if r32[1] is None else r32[1] + r32[2])
    else:
        out["gL"] = Ref(r[1], s[1], T2 * qR, r32[1])
        out["gR"] = Ref(r[2], s[2], T2 * qL, r32[2])
    return out


BASIS_NR = ((1, 129), (3, 200), (64, 129), (64, 128), (65, 129), (301, 40), (16387, 24))
BASIS_KMAX = (1, 8, 32)


def basis_shapes(gname):
    """(n, r, kmax, use_scale, use_colscale, use_prior) per grid: every (n, r) with kmax and the three optional operands cycling,
    then every kmax with all and with none of the operands at (3, 200) (four waves per point) and (65, 129) (one wave per point)."""
    d = len(GRIDS[gname][1])
    out = []
    for i, (n, r) in enumerate(BASIS_NR):
        f = (3 * i + d) % 8
        out.append((n, r, BASIS_KMAX[(i + d) % 3], bool(f & 1), bool(f & 2), bool(f & 4)))
    for n, r in ((3, 200), (65, 129)):
        for kmax in BASIS_KMAX:
            for on in (True, False):
                out.append((n, r, kmax, on, on, on))
    return sorted(set(out))


def basis_tables(grid, kmax, rng):
    """Per-dim tables V_q [g_q, kmax] (leading eigenvectors of the RBF Toeplitz factor; zero columns beyond g_q), the factors K_q
    and their first columns."""
    from oracle import spec

    cols = spec.toeplitz_columns("rbf", np.array(grid.h), np.array(grid.g), np.array(grid.h) * 2.5, 0.8)
    Vs, Ks = [], []
    for c in cols:
        g = len(c)
        K = c[np.abs(np.arange(g)[:, None] - np.arange(g)[None, :])]
        _, E = np.linalg.eigh(K)
        V = np.zeros((g, kmax))
        k = min(g, kmax)
        V[:, :k] = E[:, ::-1][:, :k]
        if kmax > g:                               # unused by a real model; random so that a wrong column cannot hide
            V[:, g:] = rng.standard_normal((g, kmax - g)) / np.sqrt(g)
        Vs.append(torch.as_tensor(V.copy()))
        Ks.append(torch.as_tensor(K.copy()))
    return Vs, Ks, torch.as_tensor(np.concatenate(cols))


def basis_case(gname, dname, n, r, kmax, use_scale, use_colscale, use_prior, outside=False):
    """Per-dim 1-D rows only (never [n, m]).  x, scale in `dtype`; tables, cotangents, F and the prior are fp64 (the kernels compute
    the weights in fp64 from the up-cast points).  The fp32 restatement is therefore the fp64 reference on the rounded points with
    the gradient rounded to fp32 on output; F and the prior are held to the fp64 bound in both dtypes."""
    grid, dtype = make_grid(gname), DTYPES[dname]
    rng = np.random.default_rng(seed_of("bp", gname, dname, n, r, kmax, use_scale, use_colscale, use_prior, outside))
    d = grid.d
    x = make_points(grid, n, rng, dtype, outside)
    Vs, Ks, tcol = basis_tables(grid, kmax, rng)
    S = rng.integers(0, kmax, (d, r))
    S[:, -1] = kmax - 1                                          # the last table column, in every dim
    if r >= 3:
        S[:, 1] = S[:, 0]                                        # a repeated basis column
    S = torch.as_tensor(S.astype(np.int32))
    scale = torch.as_tensor(rng.uniform(0.5, 2.0, n)).to(dtype) if use_scale else None
    colscale = torch.as_tensor(rng.uniform(0.5, 2.0, r)) if use_colscale else None
    GF = normal(rng, (n, r), torch.float64)
    Gp = normal(rng, (n,), torch.float64) if use_prior else None
    Ws, dWs = rows_per_dim(grid, x.double())
    sc = scale.double() if use_scale else torch.ones(n, dtype=torch.float64)
    cs = colscale if use_colscale else torch.ones(r, dtype=torch.float64)
    gp = Gp if use_prior else torch.zeros(n, dtype=torch.float64)
    Sl = S.long()
    F, prior, gx = op_basis(Ws, dWs, Vs, Ks, Sl, sc, cs, GF, gp)
    Fa, pa, ga = op_basis([w.abs() for w in Ws], [w.abs() for w in dWs], [v.abs() for v in Vs], [k.abs() for k in Ks], Sl, sc, cs,
                          GF.abs(), gp.abs())
    Pa = [Ws[q].abs() @ Vs[q].abs() for q in range(d)]          # F's first-order weight term: one dim's weights by keys_terms
    Wt = rows_per_dim(grid, x.double(), True)[0]
    F1 = torch.zeros_like(F)
    for q in range(d):
        t = sc[:, None] * cs[None, :] * (Wt[q] @ Vs[q].abs())[:, Sl[q]]
        for o in range(d):
            if o != q:
                t = t * Pa[o][:, Sl[o]]
        F1 += t
    gx32 = gx.float().double() if dtype == torch.float32 else None
    return dict(grid=grid, x=x, Vtab=torch.cat([v.reshape(-1) for v in Vs]), S=S, tcol=tcol, scale=scale, colscale=colscale, GF=GF, Gp=Gp,
                F=Ref(F, Fa, 4 * d, None, F1), prior=Ref(prior, pa, 16 * d),
                gx=Ref(gx, ga, d * r + (16 * d if use_prior else 0), gx32))
