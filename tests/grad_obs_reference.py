"""TEST INFRASTRUCTURE -- fp64 reference of a GP conditioned on values AND gradients under the SKI model, shared by
tests/test_grad_obs_host.py (no GPU) and tests/test_grad_obs_gpu.py.

A point x_p carries C = d + 1 scalar observations ("channels"): channel 0 observes f(x_p), channel 1 + q observes df/dx_q (x_p).
Under the SKI model f(x) = w(x)^T u with u ~ N(0, Kuu), every channel is one linear observation of u: its row is the interpolation
row w(x_p) (``interp_reference.dense_rows``) or that row's derivative (``interp_reference.dense_row_grads``, zero in a dim whose
cell is a one-hot boundary cell).  Stacking the present channels' rows into Phi gives the data-space GP

    y ~ N(0, Phi Kuu Phi^T + sigma2 D)

from which mean, variance, predicted gradient and the marginal log-likelihood follow by dense linear algebra (:class:`GradObsGP`),
independent of every cache formula.  Kuu is the Kronecker product of the oracle's Toeplitz factors (``oracle/spec.py``).  The same
posterior from the streamed statistics (A, b) is :meth:`GradObsGP.stats_space`; the dense statistics a single absorb launch must
produce are :func:`dense_absorb`, in the half-stencil layout of ``regrid_reference.pack_half``.
"""
import numpy as np
import scipy.linalg as sla
import torch

import interp_reference as ir
import regrid_reference as rr
from oracle import spec


class Grid:
    """g0, h, g per dim as interp_reference reads them."""

    def __init__(self, g0, h, g):
        self.g0, self.h, self.g = [float(v) for v in g0], [float(v) for v in h], [int(v) for v in g]
        self.d, self.m = len(self.g), int(np.prod(self.g))

    @classmethod
    def from_bounds(cls, grid_bounds, grid_size):
        return cls(*spec.make_grid(grid_bounds, grid_size))


def stacked_rows(grid, X):
    """Phi [n, C, m] fp64: channel 0 the value row of each point, channel 1 + q its derivative in dim q."""
    X = torch.as_tensor(np.asarray(X, dtype=np.float64)).reshape(-1, grid.d)
    return torch.cat([ir.dense_rows(grid, X)[:, None], ir.dense_row_grads(grid, X)], 1).numpy()


def inside(grid, X):
    X = np.asarray(X, dtype=np.float64).reshape(-1, grid.d)
    g0, hi = np.array(grid.g0), np.array(grid.g0) + np.array(grid.h) * (np.array(grid.g) - 1)
    return ((X >= g0) & (X <= hi)).all(1)


def dense_kuu(grid, kind="rbf", lengthscale=spec.SOFTPLUS0, outputscale=spec.SOFTPLUS0):
    K = np.ones((1, 1))
    for c in spec.toeplitz_columns(kind, np.array(grid.h), np.array(grid.g), lengthscale, outputscale):
        K = np.kron(K, sla.toeplitz(c))
    return K


class GradObsGP:
    def __init__(self, grid, Kuu, sigma2=1.0):
        self.grid, self.K, self.sigma2 = grid, Kuu, float(sigma2)

    def fit(self, X, Y, noise, present):
        """X [n, d]; Y, noise [n, C]; present bool [n, C].  Only the present channels exist for the model."""
        pres = np.asarray(present, dtype=bool)
        self.Phi = stacked_rows(self.grid, X)[pres]                      # [N, m]
        self.y = np.asarray(Y, dtype=np.float64)[pres]
        self.nz = np.asarray(noise, dtype=np.float64)[pres]
        self.PK = self.Phi @ self.K
        Kd = self.PK @ self.Phi.T
        Kd[np.diag_indices_from(Kd)] += self.sigma2 * self.nz
        self.chol = sla.cho_factor(Kd, lower=True)
        self.alpha = sla.cho_solve(self.chol, self.y)
        return self

    @property
    def N(self):
        return self.y.shape[0]

    def predict(self, Xs):
        """(mean [ns], variance [ns], gradient of the mean [ns, d]) at Xs."""
        R = stacked_rows(self.grid, Xs)                                  # [ns, C, m]
        u = self.PK.T @ self.alpha                                      # posterior mean of the grid values
        Ks = R[:, 0] @ self.PK.T
        V = sla.solve_triangular(self.chol[0], Ks.T, lower=True)
        prior = np.einsum("im,mk,ik->i", R[:, 0], self.K, R[:, 0])
        return R[:, 0] @ u, prior - np.einsum("ij,ij->j", V, V), R[:, 1:] @ u

    def mll(self):
        """-(1/2)[quad + logdet + N log 2 pi] / N over the N scalar observations."""
        quad = float(self.y @ self.alpha)
        logdet = 2.0 * float(np.sum(np.log(np.diag(self.chol[0]))))
        return -0.5 * (quad + logdet + self.N * np.log(2.0 * np.pi)) / self.N

    def stats_space(self, Xs):
        """(mean, variance, gradient, mll) from the streamed statistics alone: A = Phi^T D^-1 Phi, b = Phi^T D^-1 y, c = y^T D^-1 y,
        ld = log|D|, with Kt = Kuu / sigma2:  u = (I + Kt A)^-1 Kt b,  cov u = (I + Kt A)^-1 Kuu."""
        wt = 1.0 / self.nz
        A, b = self.Phi.T @ (self.Phi * wt[:, None]), self.Phi.T @ (wt * self.y)
        c, ld = float(self.y @ (wt * self.y)), float(np.log(self.nz).sum())
        Kt = self.K / self.sigma2
        B = np.eye(self.grid.m) + Kt @ A
        lu = sla.lu_factor(B)
        u = sla.lu_solve(lu, Kt @ b)
        R = stacked_rows(self.grid, Xs)
        var = np.einsum("im,mi->i", R[:, 0], sla.lu_solve(lu, self.K @ R[:, 0].T))
        logdet = float(np.sum(np.log(np.abs(np.diag(lu[0])))))
        N = self.N
        mll = -0.5 * ((c - b @ u) / self.sigma2 + logdet + ld + N * np.log(self.sigma2) + N * np.log(2.0 * np.pi)) / N
        return R[:, 0] @ u, var, R[:, 1:] @ u, mll


def dense_absorb(grid, X, Y, wa, wb, noise, u=None):
    """What one absorb launch adds, densely: dict of A [m, m], A_half (flat, ``regrid_reference.pack_half``), b, cnt [m],
    stats [2], err (bit 0 | 2 x dropped points), and with u [m] mean_out [n, C] and res [m].  All [n, C] inputs as the kernel takes
    them (an absent channel: wa = wb = 0, noise = 1)."""
    Phi = stacked_rows(grid, X)                                          # rows of a point outside the grid are zero
    Y, wa, wb, noise = (np.asarray(t, dtype=np.float64) for t in (Y, wa, wb, noise))
    ok = inside(grid, X)
    A = np.einsum("pca,pc,pcb->ab", Phi, wa, Phi)
    A = np.triu(A) + np.triu(A, 1).T
    out = {"A": A, "A_half": rr.pack_half(torch.as_tensor(A), grid.g).numpy(), "b": np.einsum("pca,pc->a", Phi, wb * Y),
           "cnt": Phi[:, 0].T @ wa[:, 0] + np.einsum("pca,pc->a", Phi[:, 1:] ** 2, wa[:, 1:]),
           "stats": np.array([(wb * Y * Y)[ok].sum(), np.log(noise)[ok].sum()]),
           "err": int((~ok).any()) + 2 * int((~ok).sum())}
    if u is not None:
        u = np.asarray(u, dtype=np.float64)
        out["mean_out"] = Phi @ u
        out["res"] = np.einsum("pca,pc->a", Phi, wb * Y - wa * out["mean_out"])
    return out
