"""TEST INFRASTRUCTURE -- fp64 CPU reference of the box functionals c = int_box w(x) dx and of the posterior of box integrals
(DESIGN.md 3.21), shared by tests/test_box_integral_host.py (checks of this reference, no GPU) and tests/test_box_integral_gpu.py
(the three box kernels and ``posterior_integral`` against it).  Independent of every kernel and of grid_ops' wrappers.

Per dimension (grid nodes ``g0 + j h``, ``u = (x - g0) / h``, cell j = [node j, node j + 1)):

* interior cell (1 <= j <= g - 3): the four Keys weights sit on nodes j - 1 .. j + 2.  With the antiderivatives of the two branches,
  ``P_near(a) = 0.375 a^4 - (2.5/3) a^3 + a`` and ``P_far(a) = -0.125 a^4 + (2.5/3) a^3 - 2 a^2 + 2 a``, tap c collects over [0, t]
  ``P_far(1 + t) - P_far(1)``, ``P_near(t)``, ``P_near(1) - P_near(1 - t)``, ``P_far(2) - P_far(2 - t)`` (c = 0 .. 3), times h;
* boundary cell (j = 0 or g - 2: one-hot on the nearest node): node j receives the part of [t_a, t_b] below 1/2, node j + 1 the rest;
* outside the grid w = 0: a box is clipped to the grid's extent;
* a dimension with lo == hi evaluates at that coordinate (``interp_reference.rows_1d``) and contributes factor 1 to the volume
  (factor 0 when the coordinate is outside the grid: the row is zero);
* a NaN bound or lo > hi gives a zero row; a box not wholly inside the grid (or invalid) is flagged.

``dtype``: fp64 is the reference.  With fp32, ``g0`` and ``h`` are rounded to fp32 and the last node ``g0 + h (g - 1)`` is formed in
fp32, as ``GridDev<float>`` holds them; everything else stays fp64 (the kernel evaluates its tables in fp64 in both precisions),
except a degenerate dimension, which is ``rows_1d`` in fp32."""
import numpy as np
import scipy.linalg as sla
import torch

import interp_reference as ir

C3 = 2.5 / 3.0


def p_near(a, terms=False):
    s = 1.0 if terms else -1.0
    return 0.375 * a ** 4 + s * C3 * a ** 3 + a


def p_far(a, terms=False):
    s = 1.0 if terms else -1.0
    return s * 0.125 * a ** 4 + C3 * a ** 3 + s * 2.0 * a ** 2 + 2.0 * a


def tap_integral(c, t, terms=False):
    """int_0^t k(tau + 1 - c) dtau.  terms=True: every term of the two polynomial evaluations by its absolute value."""
    s = 1.0 if terms else -1.0
    if c == 0:
        return p_far(1.0 + t, terms) + s * p_far(1.0, terms)
    if c == 1:
        return p_near(t, terms)
    if c == 2:
        return p_near(1.0, terms) + s * p_near(1.0 - t, terms)
    return p_far(2.0, terms) + s * p_far(2.0 - t, terms)


def _geometry(g0, h, g, dtype):
    dt = dtype
    g0t = torch.tensor(float(g0), dtype=torch.float64).to(dt)
    ht = torch.tensor(float(h), dtype=torch.float64).to(dt)
    hit = g0t + ht * torch.tensor(float(g - 1), dtype=dt)
    return float(g0t), float(ht), float(hit)


def box_rows_1d(g0, h, g, lo, hi, dtype=torch.float64, terms=False):
    """Integrated rows [B, g], the clipped widths [B], the flags [B] (not wholly inside, or invalid) and the node ranges [B, 2] of
    one dimension, as fp64 numpy arrays.  terms=True: the rows with every term of the closed forms replaced by its absolute value
    (the magnitude that the roundings of an entry are relative to; for a degenerate dimension ``rows_1d(terms=True)``)."""
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1), np.asarray(hi, dtype=np.float64).reshape(-1)
    g0d, hd, hid = _geometry(g0, h, g, dtype)
    B = lo.shape[0]
    rows, width, flag, rng = np.zeros((B, g)), np.zeros(B), np.zeros(B, dtype=bool), np.zeros((B, 2), dtype=np.int64)
    for b in range(B):
        a, c = lo[b], hi[b]
        valid = bool(a <= c)
        flag[b] = not (valid and a >= g0d and c <= hid)
        if not valid:
            continue
        if a == c:
            W, _, inside = ir.rows_1d(g0, h, g, torch.tensor([a], dtype=torch.float64).to(dtype), terms)
            if bool(inside[0]):
                rows[b], width[b] = W[0].double().numpy(), 1.0
                j0 = _lowest_tap(g0, h, g, a, dtype)
                rng[b] = (j0, j0 + 4)
            continue
        ac, cc = max(a, g0d), min(c, hid)
        if not ac < cc:
            continue
        ua, ub = (ac - g0d) / hd, (cc - g0d) / hd
        width[b] = cc - ac
        ia, ib = min(int(np.floor(ua)), g - 2), min(int(np.floor(ub)), g - 2)
        rng[b] = (max(ia - 1, 0), min(ib + 2, g - 1) + 1)
        for i in range(g - 1):
            ta, tb = max(ua - i, 0.0), min(ub - i, 1.0)
            if not ta < tb:
                continue
            if 1 <= i <= g - 3:
                for k in range(4):
                    rows[b, i - 1 + k] += hd * (tap_integral(k, tb, terms) + (1.0 if terms else -1.0) * tap_integral(k, ta, terms))
            else:
                below = (min(tb, 0.5) + min(ta, 0.5)) if terms else (min(tb, 0.5) - min(ta, 0.5))
                above = (max(tb, 0.5) + max(ta, 0.5)) if terms else (max(tb, 0.5) - max(ta, 0.5))
                if min(tb, 0.5) > min(ta, 0.5):
                    rows[b, i] += hd * below
                if max(tb, 0.5) > max(ta, 0.5):
                    rows[b, i + 1] += hd * above
    return rows, width, flag, rng


def _lowest_tap(g0, h, g, x, dtype):
    """Lowest of the four nodes that the point rule keeps for a coordinate inside the grid: floor(u) - 1, moved into [0, g - 4]."""
    g0t = torch.tensor(float(g0), dtype=torch.float64).to(dtype)
    ht = torch.tensor(float(h), dtype=torch.float64).to(dtype)
    u = (torch.tensor(float(x), dtype=torch.float64).to(dtype) - g0t) / ht
    return min(max(int(torch.floor(u)) - 1, 0), g - 4)


def box_rows_per_dim(grid, lo, hi, dtype=torch.float64, terms=False):
    """([rows_q [B, g_q]], vol [B], flag [B], range [B, d, 2]) of boxes lo, hi [B, d]."""
    lo, hi = np.asarray(lo, dtype=np.float64).reshape(-1, grid.d), np.asarray(hi, dtype=np.float64).reshape(-1, grid.d)
    parts = [box_rows_1d(grid.g0[q], grid.h[q], grid.g[q], lo[:, q], hi[:, q], dtype, terms) for q in range(grid.d)]
    vol = np.prod(np.stack([p[1] for p in parts], 0), 0)
    flag = np.stack([p[2] for p in parts], 0).any(0)
    return [p[0] for p in parts], vol, flag, np.stack([p[3] for p in parts], 1)


def kron_rows(fs):
    out = fs[0]
    for f in fs[1:]:
        out = (out[:, :, None] * f[:, None, :]).reshape(out.shape[0], -1)
    return out


def box_rows(grid, lo, hi, dtype=torch.float64):
    """The functionals as dense rows C [B, m] (dim 0 slowest), and the clipped volumes [B]."""
    rows, vol, _, _ = box_rows_per_dim(grid, lo, hi, dtype)
    return kron_rows(rows), vol


# ---------------------------------------------------------------------------------------------- brute-force quadrature
GL_X, GL_W = np.polynomial.legendre.leggauss(4)          # exact to degree 7: a cubic piece, or a constant one


def gl_pieces_1d(g0, h, g, a, c):
    """4-point Gauss-Legendre nodes and weights on every smooth piece of [a, c] clipped to the grid: the pieces end at the nodes and
    at the midpoints of the two boundary cells.  A degenerate dimension (a == c) is the point itself with weight 1."""
    if a == c:
        return np.array([a]), np.array([1.0])
    hi = g0 + h * (g - 1)
    ac, cc = max(a, g0), min(c, hi)
    if not ac < cc:
        return np.zeros(0), np.zeros(0)
    cuts = [g0 + h * j for j in range(g)] + [g0 + 0.5 * h, g0 + h * (g - 1.5)]
    pts = sorted([ac, cc] + [x for x in cuts if ac < x < cc])
    xs, ws = [], []
    for p, q in zip(pts[:-1], pts[1:]):
        xs.append(0.5 * (p + q) + 0.5 * (q - p) * GL_X)
        ws.append(0.5 * (q - p) * GL_W)
    return np.concatenate(xs), np.concatenate(ws)


def gl_box(grid, lo, hi):
    """Tensor-product quadrature points [N, d] and weights [N] of one box."""
    parts = [gl_pieces_1d(grid.g0[q], grid.h[q], grid.g[q], float(lo[q]), float(hi[q])) for q in range(grid.d)]
    X = np.stack([m.reshape(-1) for m in np.meshgrid(*[p[0] for p in parts], indexing="ij")], 1)
    W = np.ones(X.shape[0])
    for q, m in enumerate(np.meshgrid(*[p[1] for p in parts], indexing="ij")):
        W = W * m.reshape(-1)
    return X, W


# -------------------------------------------------------------------------------------------------- the posterior itself
class GridOf:
    """The geometry of an ``oracle.dataspace.DataSpaceGP`` under the names the functions above use."""

    def __init__(self, gp):
        self.d, self.g0, self.h, self.g = gp.d, [float(v) for v in gp.g0], [float(v) for v in gp.h], [int(v) for v in gp.g]
        self.m = int(np.prod(self.g))


class BoxGP:
    """Posterior of box integrals of a fitted ``DataSpaceGP``, in data space: the test rows of ``predict`` replaced by the
    integrated rows, K(box, x) = prod_q c_q^T K_q w_q(x) and K(box, box') = prod_q c_q^T K_q c'_q, on ``Kd``, ``chol``, ``alpha``."""

    def __init__(self, gp):
        self.gp, self.grid = gp, GridOf(gp)

    def integral(self, lo, hi, average=False):
        """(mean [B], covariance [B, B], clipped volume [B]); average: divided by the volumes (zero where the volume is zero)."""
        gp = self.gp
        rows, vol, _, _ = box_rows_per_dim(self.grid, lo, hi)
        Wd, _ = gp._WK(gp.X)
        Kbx, Kbb = np.ones((rows[0].shape[0], gp.X.shape[0])), np.ones((rows[0].shape[0],) * 2)
        for q in range(gp.d):
            CK = rows[q] @ gp.Kd[q]
            Kbx *= CK @ Wd[q].T
            Kbb *= CK @ rows[q].T
        mean = Kbx @ gp.alpha
        V = sla.solve_triangular(gp.chol[0], Kbx.T, lower=True)
        cov = Kbb - V.T @ V
        if average:
            s = np.where(vol > 0, 1.0 / np.where(vol > 0, vol, 1.0), 0.0)
            mean, cov = mean * s, cov * s[:, None] * s[None, :]
        return mean, cov, vol

    def stats_space(self):
        """(Sigma_u [m, m], u_bar [m]) from the statistics A = Phi^T D^-1 Phi, b = Phi^T D^-1 y of the fitted points: the dense
        restatement of what the model holds, Sigma_u = (I + Kt A)^-1 K and u_bar = (I + Kt A)^-1 Kt b with Kt = K / sigma2."""
        gp = self.gp
        Wd, _ = gp._WK(gp.X)
        Phi = kron_rows(Wd)
        K = np.ones((1, 1))
        for Kq in gp.Kd:
            K = np.kron(K, Kq)
        A, b = Phi.T @ (Phi / gp.noise[:, None]), Phi.T @ (gp.y / gp.noise)
        Kt = K / gp.sigma2
        lu = sla.lu_factor(np.eye(K.shape[0]) + Kt @ A)
        return sla.lu_solve(lu, K), sla.lu_solve(lu, Kt @ b)


# ------------------------------------------------------------------------------------------------------------------ boxes
def make_boxes(grid, rng):
    """(lo, hi [B, d] fp64, kinds [B]) covering the ways the kernels can go wrong, in units of each dim's own nodes.  Coordinates keep
    1e-2 h away from the points where a floor or the one-hot rule switches, except where a kind asks for a face exactly on a node."""
    d, g = grid.d, grid.g
    node = lambda q, u: grid.g0[q] + grid.h[q] * u
    last = lambda q: g[q] - 1

    def interior_span(q):
        a, c = sorted(rng.uniform(1.02, g[q] - 2.02, 2))
        return (a, c) if c - a > 0.05 else (a, min(a + 0.3, g[q] - 2.02))

    def one_cell(q):                       # inside one interior cell
        j = int(rng.integers(1, g[q] - 2))
        return j + rng.uniform(0.05, 0.4), j + rng.uniform(0.6, 0.95)

    def half_boundary(q):                  # inside one half of a boundary cell
        j = 0 if rng.random() < 0.5 else g[q] - 2
        o = 0.0 if rng.random() < 0.5 else 0.5
        return j + o + 0.05, j + o + 0.45

    def straddle_mid(q):
        j = 0 if rng.random() < 0.5 else g[q] - 2
        return j + rng.uniform(0.1, 0.4), j + rng.uniform(0.6, 0.9)

    def on_nodes(q):
        a = int(rng.integers(0, g[q] - 1))
        return float(a), float(rng.integers(a + 1, g[q]))

    def across(q):                         # spans the boundary and the interior regimes
        return rng.uniform(0.1, 0.9), rng.uniform(1.1, g[q] - 2.02) if rng.random() < 0.5 else g[q] - 2 + rng.uniform(0.1, 0.9)

    def partly_out(q):
        return (-0.7, rng.uniform(0.2, 1.8)) if rng.random() < 0.5 else (rng.uniform(g[q] - 2.8, g[q] - 1.2), last(q) + 0.6)

    def wholly_out(q):
        return (-2.5, -0.5) if rng.random() < 0.5 else (last(q) + 0.25, last(q) + 1.5)

    def point(q):
        u = rng.uniform(0.05, last(q) - 0.05)
        return u, u

    def odd_last(q):                       # a last-dim support of 4 + 1, 4 + 2, 4 + 3 nodes where the dim has room, else what fits
        n = int(rng.integers(5, 8))
        j = int(rng.integers(1, max(2, g[q] - n)))
        return j + 0.3, min(j + (n - 3) - 0.3, g[q] - 2.02)

    full = lambda q: (0.0, float(last(q)))
    plan = [("domain", [full] * d), ("domain", [full] * d)]
    for name, f in (("one_cell", one_cell), ("half_boundary", half_boundary), ("straddle_mid", straddle_mid), ("on_nodes", on_nodes),
                    ("across", across), ("interior", interior_span)):
        i = len(plan)
        plan += [(name, [f] * d), (name, [f if q == i % d else interior_span for q in range(d)])]
    plan += [("partly_out", [partly_out if q == i % d else interior_span for q in range(d)]) for i in range(2)]
    plan += [("wholly_out", [wholly_out if q == (i + 1) % d else interior_span for q in range(d)]) for i in range(2)]
    plan += [("degenerate_one", [point if q == i % d else interior_span for q in range(d)]) for i in range(2)]
    plan += [("degenerate_all", [point] * d), ("degenerate_all_boundary", [half_boundary if q == 0 else point for q in range(d)])]
    plan += [("odd_last", [odd_last if q == d - 1 else one_cell for q in range(d)]) for _ in range(3)]
    lo, hi, kinds = np.zeros((len(plan), d)), np.zeros((len(plan), d)), []
    for b, (name, fs) in enumerate(plan):
        kinds.append(name)
        for q, f in enumerate(fs):
            a, c = f(q)
            if name == "degenerate_all_boundary" and q == 0:
                c = a
            lo[b, q], hi[b, q] = node(q, a), node(q, c)
    return lo, hi, kinds
