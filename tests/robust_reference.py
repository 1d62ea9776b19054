"""TEST INFRASTRUCTURE -- fp64 reference of the outlier-robust absorb, shared by tests/test_robust_host.py (no GPU)
and tests/test_robust_gpu.py.

A batch is Huber-weighted against the posterior grid mean u BEFORE it: with w_i the interpolation row of point i
(``interp_reference.dense_rows``; zero for a point outside the grid),

    z_i = (y_i - w_i . u) inv_scale_i,     omega_i = min(1, c / |z_i|),

and point i enters the statistics as the same point at noise d_i / omega_i: A, cnt and the carried residual take omega_i wa_i, b and
sum wb y^2 take omega_i wb_i, log|D| takes log noise_i - log omega_i.  A point outside the grid is dropped, counted in err and
reports omega = 0.  Dense numpy, independent of the kernel and of the model; the half-stencil layout is
``regrid_reference.pack_half``, as in ``grad_obs_reference.dense_absorb``.
"""
import numpy as np
import torch

import interp_reference as ir
import regrid_reference as rr
from grad_obs_reference import Grid, inside  # noqa: F401  (Grid: g0, h, g per dim as interp_reference reads them)


def huber_weights(y, mean, inv_scale, c):
    """(omega, z) of targets y against the predictive means `mean`."""
    z = (np.asarray(y, dtype=np.float64) - np.asarray(mean, dtype=np.float64)) * np.asarray(inv_scale, dtype=np.float64)
    az = np.abs(z)
    return np.where(az > c, c / np.where(az > 0, az, 1.0), 1.0), z


def dense_absorb(grid, X, y, wa, wb, noise, inv_scale, c, u):
    """What one robust absorb launch adds, densely: dict of omega, z, mean_out [n], A [m, m], A_half (flat), b, cnt, res [m],
    stats [2] and err (bit 0 | 2 x dropped points)."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, grid.d)
    W = ir.dense_rows(grid, torch.as_tensor(X)).numpy()                  # rows of a point outside the grid are zero
    y, wa, wb, noise, u = (np.asarray(t, dtype=np.float64) for t in (y, wa, wb, noise, u))
    ok = inside(grid, X)
    mean = W @ u
    omega, z = huber_weights(y, mean, inv_scale, c)
    omega = np.where(ok, omega, 0.0)
    wae, wbe = wa * omega, wb * omega
    A = W.T @ (W * wae[:, None])
    A = np.triu(A) + np.triu(A, 1).T
    return {"omega": omega, "z": z, "mean_out": mean, "A": A, "A_half": rr.pack_half(torch.as_tensor(A), grid.g).numpy(),
            "b": W.T @ (wbe * y), "cnt": W.T @ wae, "res": W.T @ (wbe * y - wae * mean),
            "stats": np.array([(wbe * y * y)[ok].sum(), (np.log(noise[ok]) - np.log(omega[ok])).sum()]),
            "err": int((~ok).any()) + 2 * int((~ok).sum())}
