"""TEST INFRASTRUCTURE -- fp64 CPU reference of the jet posterior, shared by tests/test_jet_host.py (checks of this
reference, no GPU) and tests/test_jet_gpu.py (the three jet kernels and ``posterior_jet`` against it).

The jet rows of a point are J(x) = [w(x); d_1 w(x); ..; d_d w(x)], C = d + 1 channels: ``interp_reference.dense_rows`` and
``dense_row_grads`` (zero in a dim whose cell is a one-hot boundary cell, all zero outside the grid).  The three kernel operations
are dense contractions of J, returned as ``interp_reference.Ref`` objects (reference, S_abs = the same expression with every factor
replaced by its absolute value, term count N, and for fp32 the fp32 restatement).  The model reference is the data-space GP of
``grad_obs_reference.GradObsGP``: with Phi the stacked rows of the present observations,

    Sigma_u = K - K Phi^T (Phi K Phi^T + sigma2 D)^-1 Phi K,   mean J u_bar,   covariance J Sigma_u J^T,

and the same from the statistics A = Phi^T D^-1 Phi, b = Phi^T D^-1 y: Sigma_u = (I + Kt A)^-1 K, u_bar = (I + Kt A)^-1 Kt b."""
import numpy as np
import scipy.linalg as sla
import torch

import grad_obs_reference as gr
import interp_reference as ir


def jet_rows(grid, x):
    """J [n, C, m] as fp64, evaluated in x's dtype."""
    W, dW = ir.dense_both(grid, x)
    return torch.cat([W[:, None], dW], 1)


# ------------------------------------------------------------------------------------------ the three operations, densely
def op_quadform(J, M):
    return torch.einsum("pca,ab,pdb->pcd", J, M, J)


def op_gather(J, V, per_point):
    """V [k, m] shared (out [n, k, C]) or V [n, B, m] per point (out [n, B, C])."""
    return torch.einsum("pcm,pjm->pjc", J, V) if per_point else torch.einsum("pcm,jm->pjc", J, V)


def _case(tag, gname, dname, n, outside, *extra):
    grid, dtype = ir.make_grid(gname), ir.DTYPES[dname]
    rng = np.random.default_rng(ir.seed_of(tag, gname, dname, n, outside, *extra))
    x = ir.make_points(grid, n, rng, dtype, outside)
    J = jet_rows(grid, x.double())
    J32 = jet_rows(grid, x) if dtype == torch.float32 else None
    return grid, dtype, rng, x, J, J32


def quadform_case(gname, dname, n, outside=False, pad=0):
    """N = 4^d 4^d terms per entry."""
    grid, dtype, rng, x, J, J32 = _case("jq", gname, dname, n, outside, pad)
    M, Mbuf = ir.sym_table(rng, grid.m, dtype, grid.m + pad if pad else None)
    Md = M.double()
    R = ir.Ref(op_quadform(J, Md), op_quadform(J.abs(), Md.abs()), grid.T * grid.T, None if J32 is None else op_quadform(J32, Md))
    return dict(grid=grid, x=x, M=M, Mbuf=Mbuf, R=R)


def gather_case(gname, dname, n, k, per_point, outside=False):
    """N = 4^d terms per entry.  per_point: V [n k, m], k rows for each point."""
    grid, dtype, rng, x, J, J32 = _case("jg", gname, dname, n, outside, k, per_point)
    V = ir.normal(rng, (n * k, grid.m) if per_point else (k, grid.m), dtype)
    Vd = V.double().reshape(n, k, grid.m) if per_point else V.double()
    R = ir.Ref(op_gather(J, Vd, per_point), op_gather(J.abs(), Vd.abs(), per_point), grid.T, None if J32 is None else op_gather(J32, Vd, per_point))
    # for the two kernels that gather_jet fuses (their weights are evaluated with fused multiply-adds): the first-order weight term
    s1 = op_gather(rows_first_order(grid, x.double()), Vd.abs(), per_point) if dtype == torch.float64 else None
    return dict(grid=grid, x=x, V=V, R=R, s1=s1)


def _deriv_terms_1d(g0, h, g, x):
    """Dense [n, g] rows of dim q with every term of the derivative polynomial k'(s) / h replaced by its absolute value (the
    magnitude its rounding is relative to: k'(2) = 0 by cancellation of terms of size 6, 10 and 4); zero where the derivative row
    is identically zero."""
    dt = x.dtype
    a0 = torch.tensor(float(g0), dtype=torch.float64).to(dt)
    hh = torch.tensor(float(h), dtype=torch.float64).to(dt)
    u = (x - a0) / hh
    fl = torch.floor(u)
    inside = (x >= a0) & (x <= a0 + hh * torch.tensor(float(g - 1), dtype=dt))
    j0 = torch.where(inside, fl, torch.zeros_like(fl)).to(torch.int64) - 1
    interior = inside & (j0 >= 0) & (j0 <= g - 4)
    a = (((u - fl)[:, None] + 1.0) - torch.arange(4, dtype=dt)[None, :]).abs()
    t = torch.where(a <= 1.0, (4.5 * a + 5.0) * a, torch.where(a < 2.0, (1.5 * a + 5.0) * a + 4.0, torch.zeros_like(a))) / hh
    t = torch.where(interior[:, None], t, torch.zeros_like(t))
    idx = (j0[:, None] + torch.arange(4)[None, :]).clamp(0, g - 1)
    return torch.zeros((x.shape[0], g), dtype=dt).scatter_add_(1, idx, t)


def rows_first_order(grid, x, support=False):
    """S_1 [n, C, m] (fp64, evaluated in x's dtype) of the rows themselves: the sum, over one dim at a time, of |J| with THAT dim's factor replaced
    by the size of its polynomial's terms (``interp_reference.keys_terms`` for a value factor, :func:`_deriv_terms_1d` for the
    derivative factor).  A row entry is a single product of d weights, so its rounding error is first order in the roundings inside
    each weight, which are relative to the terms, not to the weight (tests/test_interp_derivatives_gpu.py on the two forwards).
    support=True: also the product of the terms of ALL d factors -- positive exactly where a row entry is not zero by construction
    (two outer taps next to a node in two dims can both round to zero in the reference: their product is second order)."""
    d = grid.d
    Ws, dWs = ir.rows_per_dim(grid, x)
    Wt = ir.rows_per_dim(grid, x, True)[0]
    ok = torch.stack([ir.rows_1d(grid.g0[q], grid.h[q], grid.g[q], x[:, q])[2] for q in range(d)], 0).all(0)
    dWt = [torch.where(ok[:, None], _deriv_terms_1d(grid.g0[q], grid.h[q], grid.g[q], x[:, q]), torch.zeros(1, dtype=x.dtype)) for q in range(d)]
    out, sup = [], []
    for c in range(d + 1):                                   # channel c: derivative factor in dim c - 1 (none for c = 0)
        fac = [(dWs[o] if o == c - 1 else Ws[o]).abs() for o in range(d)]
        trm = [dWt[o] if o == c - 1 else Wt[o] for o in range(d)]
        out.append(sum(ir._kron_rows([trm[o] if o == q else fac[o] for o in range(d)]) for q in range(d)))
        sup.append(ir._kron_rows(trm))
    return (torch.stack(out, 1).double(), torch.stack(sup, 1).double()) if support else torch.stack(out, 1).double()


def columns_case(gname, dname, n, outside=False):
    """The rows as wt_columns_jet writes them, [n C, m]: single products (N = 1), with the first-order weight term in fp64.
    S_abs is |J| + eps64 S_1 + eps64^2 (product of all d factors' terms): next to a node the reference's own outer weights round to exactly zero ((t + 1) - c loses t) where
    the true weight is about t / 2, so |J| alone would call an entry identically zero that is not; S_1 vanishes exactly where a row
    is zero by construction -- off the taps, in a boundary cell's derivative channel, at the other nodes of a one-hot cell, for a
    point outside the grid; the product of the terms is positive exactly off that set."""
    grid, dtype, rng, x, J, J32 = _case("jc", gname, dname, n, outside)
    m = grid.m
    s1, sup = (t.reshape(-1, m) for t in rows_first_order(grid, x.double(), support=True))
    # fp32: a point within an fp32 rounding of a node can take its four taps one node further along in fp32 than in fp64 (floor(u)
    # differs); the support of the fp32 restatement counts too
    if dtype == torch.float32:
        sup = sup + rows_first_order(grid, x, support=True)[1].reshape(-1, m)
    mask = s1 + ir.EPS64 * sup
    R = ir.Ref(J.reshape(-1, m), J.abs().reshape(-1, m) + ir.EPS64 * mask, 1, None if J32 is None else J32.reshape(-1, m),
               s1 if dtype == torch.float64 else None)
    return dict(grid=grid, x=x, R=R)


# ----------------------------------------------------------------------------------------------------- the jet posterior
class JetGP:
    """Jet posterior of a fitted ``GradObsGP``: ``data_space`` and ``stats_space`` give (Sigma_u [m, m], u_bar [m]); ``jet`` the
    mean [n, C] and the joint covariance [n C, n C] (point-major) at query points."""

    def __init__(self, gp):
        self.gp = gp

    def data_space(self):
        gp = self.gp
        return gp.K - gp.PK.T @ sla.cho_solve(gp.chol, gp.PK), gp.PK.T @ gp.alpha

    def stats_space(self):
        gp = self.gp
        wt = 1.0 / gp.nz
        A, b = gp.Phi.T @ (gp.Phi * wt[:, None]), gp.Phi.T @ (wt * gp.y)
        Kt = gp.K / gp.sigma2
        lu = sla.lu_factor(np.eye(gp.grid.m) + Kt @ A)
        return sla.lu_solve(lu, gp.K), sla.lu_solve(lu, Kt @ b)

    def jet(self, Xs, space="data"):
        S, u = self.data_space() if space == "data" else self.stats_space()
        J = gr.stacked_rows(self.gp.grid, Xs)                            # [n, C, m]
        n, C, m = J.shape
        Jf = J.reshape(n * C, m)
        cov = Jf @ S @ Jf.T
        return J @ u, 0.5 * (cov + cov.T)

    def kpost(self, Xa, Xb):
        """Posterior covariance of the VALUES between two point sets: w(Xa) Sigma_u w(Xb)^T."""
        S, _ = self.data_space()
        g = self.gp.grid
        return ir.dense_rows(g, torch.as_tensor(Xa)).numpy() @ S @ ir.dense_rows(g, torch.as_tensor(Xb)).numpy().T


def blocks_of(cov, n, C):
    return cov.reshape(n, C, n, C)[np.arange(n), :, np.arange(n), :]


def f_true(X):
    return np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.5 * X[:, -1]


def df_true(X):
    G = np.zeros_like(X)
    G[:, 0] = 2 * np.cos(2 * X[:, 0]) * np.cos(X[:, 1])
    G[:, 1] = -np.sin(2 * X[:, 0]) * np.sin(X[:, 1])
    G[:, -1] += 0.5
    return G


def model_data(grid, seed=0, n_val=40, n_jet=16, n_query=23):
    """40 points with values, 16 with values and gradients, 23 queries of which the last sits in a boundary cell of dim 0 (the
    grid's first cell, 0.3 spacings from its first node: away from both nodes and from the midpoint)."""
    d = grid.d
    rng = np.random.default_rng(seed)
    n = n_val + n_jet
    X = rng.uniform(-0.95, 0.95, (n, d))
    Y = np.concatenate([f_true(X)[:, None], df_true(X)], 1) + 0.05 * rng.standard_normal((n, d + 1))
    noise = rng.uniform(0.5, 2.0, (n, d + 1))
    present = np.ones((n, d + 1), dtype=bool)
    present[:n_val, 1:] = False
    Xs = rng.uniform(-0.7, 0.7, (n_query, d))
    Xs[-1, 0] = grid.g0[0] + 0.3 * grid.h[0]
    return dict(X=X, Y=Y, noise=noise, present=present, Xs=Xs, n_val=n_val)
