"""TEST INFRASTRUCTURE -- fp64 reference of the interval-observation absorb, shared by tests/test_interval_host.py
(no GPU) and tests/test_interval_gpu.py.

Point i says y_i = f(x_i) + eps_i lies in [lo_i, hi_i].  Against the posterior BEFORE the batch -- predictive mean mu_i = w_i . u,
posterior variance v_i of f, noise dn_i = sigma2 noise_i, s^2 = v + dn, a = (lo - mu) / s, b = (hi - mu) / s --

    Z = Phi(b) - Phi(a),   alpha = (phi(a) - phi(b)) / (s Z),   beta = alpha^2 + (b phi(b) - a phi(a)) / (s^2 Z),
    omega = min(1, dn beta / (1 - v beta)),   ytilde = mu + alpha / beta,

and the point enters the statistics as the target ytilde at noise noise_i / omega_i.  lo == hi is an exact value (ytilde = lo,
omega = 1, log Z the Gaussian log density).  A point is skipped (omega = 0, ytilde = mu, nothing enters) when omega < OMEGA_MIN, when
beta is not positive and finite, when lo > hi (log Z = -inf) or when a bound is NaN (log Z = NaN).  A point outside the grid is
dropped, counted in err and reports (ytilde, omega, log Z) = (0, 0, 0).

The evaluation is the plain one: a one-sided bound through the inverse Mills ratio h(z) = phi(z) / Phi(z) = sqrt(2 / pi) /
erfcx(-z / sqrt 2) and log_ndtr, a two-sided interval through an ndtr difference after mirroring its centre below the mean.  Dense
numpy and scipy.special, independent of the kernel and of the model; the half-stencil layout is ``regrid_reference.pack_half``.
"""
import numpy as np
import torch
from scipy import special as sp

import interp_reference as ir
import regrid_reference as rr
from grad_obs_reference import Grid, inside  # noqa: F401  (Grid: g0, h, g per dim as interp_reference reads them)

OMEGA_MIN = 1e-12


def _phi(z):
    return np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi)


def _site(lo, hi, mu, v, dn):
    """One point, python floats: (ytilde, omega, log_z, alpha, beta); alpha = beta = nan where they are not defined."""
    nan = float("nan")
    if np.isnan(lo) or np.isnan(hi):
        return mu, 0.0, nan, nan, nan
    if lo > hi or (lo == hi and np.isinf(lo)):
        return mu, 0.0, -np.inf, nan, nan
    v = max(v, 0.0)
    s = np.sqrt(v + dn)
    if lo == hi:
        z = (lo - mu) / s
        return lo, 1.0, -0.5 * z * z - np.log(s) - 0.5 * np.log(2.0 * np.pi), z / s, 1.0 / (s * s)
    if np.isinf(lo) and np.isinf(hi):
        return mu, 0.0, 0.0, 0.0, 0.0
    if np.isinf(hi) or np.isinf(lo):
        sign = 1.0 if np.isinf(hi) else -1.0                             # a lower bound pushes the mean up
        z = (mu - lo) / s if np.isinf(hi) else (hi - mu) / s
        h = np.sqrt(2.0 / np.pi) / sp.erfcx(-z / np.sqrt(2.0))
        alpha, beta, log_z = sign * h / s, h * (h + z) / (s * s), float(sp.log_ndtr(z))
    else:
        a, b = (lo - mu) / s, (hi - mu) / s
        sign = 1.0
        if a + b > 0:
            a, b, sign = -b, -a, -1.0
        Z = float(sp.ndtr(b) - sp.ndtr(a))
        with np.errstate(divide="ignore", invalid="ignore"):
            alpha = sign * (_phi(a) - _phi(b)) / (s * Z)
            beta = alpha * alpha + (b * _phi(b) - a * _phi(a)) / (s * s * Z)
            log_z = float(np.log(Z))
    if not (beta > 0.0 and np.isfinite(beta)):
        return mu, 0.0, log_z, alpha, beta
    den = 1.0 - v * beta
    omega = min(1.0, dn * beta / den) if den > 0.0 else 1.0
    if not omega >= OMEGA_MIN:
        return mu, 0.0, log_z, alpha, beta
    return mu + alpha / beta, omega, log_z, alpha, beta


def sites(lo, hi, mean, pvar, dn):
    """The sites of interval observations against predictive means `mean` and posterior variances `pvar` at noise `dn` (all [n], or
    scalars broadcast): dict of ytilde, omega, log_z, alpha, beta [n] and skipped (bool [n]: omega == 0)."""
    lo, hi, mean, pvar, dn = np.broadcast_arrays(*(np.asarray(t, dtype=np.float64) for t in (lo, hi, mean, pvar, dn)))
    out = np.array([_site(*(float(t) for t in row)) for row in zip(lo.ravel(), hi.ravel(), mean.ravel(), pvar.ravel(), dn.ravel())]).reshape(-1, 5)
    r = {k: out[:, i].reshape(lo.shape) for i, k in enumerate(("ytilde", "omega", "log_z", "alpha", "beta"))}
    r["skipped"] = r["omega"] == 0.0
    return r


def dense_absorb(grid, X, lo, hi, wa, wb, noise, pvar, sigma2, u):
    """What one interval absorb launch adds, densely: dict of ytilde, omega, log_z, skipped, mean_out [n], A [m, m], A_half (flat), b,
    cnt, res [m], stats [2] and err (bit 0 | 2 x dropped points)."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, grid.d)
    W = ir.dense_rows(grid, torch.as_tensor(X)).numpy()                  # rows of a point outside the grid are zero
    lo, hi, wa, wb, noise, pvar, u = (np.asarray(t, dtype=np.float64) for t in (lo, hi, wa, wb, noise, pvar, u))
    ok = inside(grid, X)
    mean = W @ u
    st = sites(lo, hi, mean, pvar, sigma2 * noise)
    omega = np.where(ok, st["omega"], 0.0)
    yt = np.where(ok, st["ytilde"], 0.0)
    log_z = np.where(ok, st["log_z"], 0.0)
    ent = omega > 0.0
    wae, wbe = wa * omega, wb * omega
    A = W.T @ (W * wae[:, None])
    A = np.triu(A) + np.triu(A, 1).T
    return {"ytilde": yt, "omega": omega, "log_z": log_z, "skipped": ok & ~ent, "mean_out": mean, "A": A,
            "A_half": rr.pack_half(torch.as_tensor(A), grid.g).numpy(), "b": W.T @ (wbe * yt), "cnt": W.T @ wae, "res": W.T @ (wbe * yt - wae * mean),
            "stats": np.array([(wbe * yt * yt)[ent].sum(), (np.log(noise[ent]) - np.log(omega[ent])).sum()]),
            "err": int((~ok).any()) + 2 * int((~ok).sum())}
