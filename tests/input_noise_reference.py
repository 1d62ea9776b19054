"""TEST INFRASTRUCTURE -- fp64 reference of the noisy-input absorb, shared by tests/test_input_noise_host.py (no GPU)
and tests/test_input_noise_gpu.py.

Point i was taken at x_i + e_i with e_i ~ N(0, diag(xvar_i)).  Against the posterior BEFORE the batch -- predictive mean mu_i = w_i . u,
its slope g_ik = (d w_i / d x_k) . u, posterior variance v_i of f and gamma_ik of d f / d x_k, noise dn_i = sigma2 noise_i --

    s_in = sum_k xvar_k (g_k^2 + max(gamma_k, 0)),   omega = dn / (dn + s_in),   log Z = log N(y; mu, max(v, 0) + dn + s_in),

and the point enters the statistics as its own target y at noise noise_i / omega_i.  gvar None is gamma = 0, the rule of the mean's
slope alone.  A point is skipped (omega = 0, nothing enters) when an xvar_k is negative or NaN or s_in is not finite (log Z = NaN), or
when omega < OMEGA_MIN (log Z stays the density).  A point outside the grid is dropped, counted in err and reports zeros.

Rows and derivative rows are ``interp_reference.dense_both`` (the derivative row of dim k is zero in a one-hot boundary cell of that
dim); the half-stencil layout is ``regrid_reference.pack_half``.  Dense numpy, independent of the kernel and of the model.
``DenseStream`` is a small data-space GP on the SKI kernel that absorbs a stream batch by batch with these sites.
"""
import numpy as np
import scipy.linalg as sla
import torch

import interp_reference as ir
import regrid_reference as rr
from grad_obs_reference import Grid, dense_kuu, inside  # noqa: F401  (Grid: g0, h, g per dim as interp_reference reads them)

OMEGA_MIN = 1e-12
EPS32 = float(np.finfo(np.float32).eps)


def sites(y, mean, grad, pvar, gvar, dn, xvar):
    """The sites of noisy-input observations: y, mean, pvar, dn [n]; grad, xvar [n, d]; gvar [n, d] or None.  Dict of omega, log_z,
    s_in [n] and skipped (bool [n]: omega == 0)."""
    y, mean, pvar, dn = (np.asarray(t, dtype=np.float64).reshape(-1) for t in np.broadcast_arrays(y, mean, pvar, dn))
    grad = np.asarray(grad, dtype=np.float64).reshape(y.shape[0], -1)
    xvar = np.broadcast_to(np.asarray(xvar, dtype=np.float64), grad.shape)
    gam = np.zeros_like(grad) if gvar is None else np.asarray(gvar, dtype=np.float64).reshape(grad.shape)
    gam = np.where(gam > 0.0, gam, 0.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        s_in = (xvar * (grad * grad + gam)).sum(1)
        valid = (xvar >= 0.0).all(1) & np.isfinite(s_in)
        s2 = np.where(pvar > 0.0, pvar, 0.0) + dn + s_in
        log_z = -0.5 * (y - mean) ** 2 / s2 - 0.5 * np.log(s2) - 0.5 * np.log(2.0 * np.pi)
        omega = dn / (dn + s_in)
    log_z = np.where(valid, log_z, np.nan)
    omega = np.where(valid & (omega >= OMEGA_MIN), omega, 0.0)
    return {"omega": omega, "log_z": log_z, "s_in": s_in, "skipped": omega == 0.0}


def rows(grid, X):
    """(W [n, m], dW [n, d, m]) as fp64 numpy (``interp_reference.dense_both``)."""
    W, dW = ir.dense_both(grid, torch.as_tensor(np.asarray(X, dtype=np.float64).reshape(-1, grid.d)))
    return W.numpy(), dW.numpy()


def dense_absorb(grid, X, y, xvar, gvar, wa, wb, noise, pvar, sigma2, u):
    """What one noisy-input absorb launch adds, densely: dict of omega, log_z, skipped, mean_out [n], grad [n, d], A [m, m], A_half
    (flat), b, cnt, res [m], stats [2] and err (bit 0 | 2 x dropped points); abs_mean [n] = |w| . |u| and abs_grad [n, d] =
    |d w / d x_k| . |u|, the magnitudes the rounding errors of the kernel's dot products are relative to (``fp32_bounds``)."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, grid.d)
    W, dW = rows(grid, X)                                         # rows of a point outside the grid are zero
    y, wa, wb, noise, pvar, u = (np.asarray(t, dtype=np.float64) for t in (y, wa, wb, noise, pvar, u))
    ok = inside(grid, X)
    mean, grad = W @ u, dW @ u
    st = sites(y, mean, grad, pvar, gvar, sigma2 * noise, xvar)
    omega = np.where(ok, st["omega"], 0.0)
    log_z = np.where(ok, st["log_z"], 0.0)
    ent = omega > 0.0
    wae, wbe = wa * omega, wb * omega
    A = W.T @ (W * wae[:, None])
    A = np.triu(A) + np.triu(A, 1).T
    return {"omega": omega, "log_z": log_z, "s_in": st["s_in"], "skipped": ok & ~ent, "mean_out": mean, "grad": grad, "A": A,
            "A_half": rr.pack_half(torch.as_tensor(A), grid.g).numpy(), "b": W.T @ (wbe * y), "cnt": W.T @ wae, "res": W.T @ (wbe * y - wae * mean),
            "stats": np.array([(wbe * y * y)[ent].sum(), (np.log(noise[ent]) - np.log(omega[ent])).sum()]),
            "err": int((~ok).any()) + 2 * int((~ok).sum()), "abs_mean": np.abs(W) @ np.abs(u), "abs_grad": np.abs(dW) @ np.abs(u)}


def fp32_bounds(ref, y, xvar, pvar, dn, d):
    """Per point, how far an fp32 launch may lie from `ref` (a dense_absorb): the running error
    bound of an fp32 dot product over the T = 4^d taps, (T + 2) eps32 sum_a |v[a] u[a]|, for mu and for every g_k; propagated through
    s_in = sum_k xvar_k (g_k^2 + gamma_k) -- d s_in <= sum_k xvar_k (2 |g_k| dg_k + dg_k^2) -- into omega = dn / (dn + s_in), exactly:
    |omega(s + e) - omega(s)| <= dn e / ((dn + s)(dn + s - e)), with d omega / d mu = 0; and to first order into log Z through
    d log Z / d mu = (y - mu) / S and d log Z / d s_in = (y - mu)^2 / 2 S^2 - 1 / 2 S, S = v + dn + s_in; plus 4 eps32 |value| for the
    final rounding.  Dict of grad [n, d], omega [n], log_z [n]."""
    T = 4 ** d
    d_mu = (T + 2) * EPS32 * ref["abs_mean"]
    d_g = (T + 2) * EPS32 * ref["abs_grad"]
    g, s_in = ref["grad"], ref["s_in"]
    xi = np.where(np.isfinite(xvar) & (xvar >= 0), xvar, 0.0)
    d_s = (xi * (2.0 * np.abs(g) * d_g + d_g * d_g)).sum(1)
    tot = dn + np.where(np.isfinite(s_in), s_in, 0.0)
    d_om = dn * d_s / (tot * np.maximum(tot - d_s, 1e-300))
    S = np.where(pvar > 0, pvar, 0.0) + tot
    z = y - ref["mean_out"]
    d_lz = np.abs(z) / S * d_mu + np.abs(0.5 * z * z / (S * S) - 0.5 / S) * d_s
    return {"grad": d_g + 4 * EPS32 * np.abs(g), "omega": d_om + 4 * EPS32 * ref["omega"],
            "log_z": d_lz + 4 * EPS32 * np.abs(np.where(np.isfinite(ref["log_z"]), ref["log_z"], 0.0))}


# ------------------------------------------------------------------------------------------------- the batch of the kernel tests
KGRIDS = {"d1": [8], "d2": [8, 8], "d3": [8, 8, 8], "d4": [6, 6, 6, 6]}
N = 37                                                            # three blocks of 16; the last pass of the last block holds one point
KS2 = 0.7                                                         # sigma2 of the kernel cases
ZERO, NANXI, HUGE, OUTSIDE, PVAR0, PVARNEG, RLO, RHI = (0, 1, 2), 3, 6, 10, 5, 7, 8, 9
_cases = {}


def kernel_case(name):
    """Grid, 37 points (fp64 values that are exact in fp32) and the dense fp64 references with and without gvar; built once.
      0, 1, 2: xvar = 0   3: a NaN xvar_k   6: xvar so large that omega < 1e-12   10: outside the grid   5: pvar = gvar = 0 exactly
      7: pvar and gvar slightly negative   4 + q, 20 + q: a boundary cell of dim q   12 .. 16 share one interior cell (colliding atomics)
      the others: xvar such that s_in / dn (with gvar) is log-uniform in [1e-3, 1e3], 8 and 9 at the two ends."""
    if name in _cases:
        return _cases[name]
    from online_gp_amd import grid_ops                               # (GridSpec: geometry only, no device)

    g = KGRIDS[name]
    d = len(g)
    rng = np.random.default_rng(300 + d)
    grid = grid_ops.GridSpec([[-1.0, 1.0 + 0.25 * q] for q in range(d)], g)
    cell = np.stack([rng.integers(1, gq - 2, N) for gq in g], 1).astype(np.float64)
    frac = 0.5 + rng.choice([-1.0, 1.0], (N, d)) * rng.uniform(0.05, 0.45, (N, d))      # away from nodes and cell midpoints
    for q in range(d):
        cell[4 + q, q] = 0                                          # first (boundary) cell of dim q
        cell[20 + q, q] = g[q] - 2                                  # last (boundary) cell of dim q
    cell[12:17] = 1
    X = np.array(grid.g0) + np.array(grid.h) * (cell + frac)
    X[OUTSIDE, 0] = grid.g0[0] - 1.0
    f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
    X = f32(X)
    noise = f32(rng.uniform(0.5, 2.0, N))
    wa = f32(1.0 / noise)
    pvar, gvar = f32(rng.uniform(0.0, 2.0, N)), f32(rng.uniform(0.0, 2.0, (N, d)))
    pvar[PVAR0], gvar[PVAR0] = 0.0, 0.0
    pvar[PVARNEG], gvar[PVARNEG] = f32(-1e-3), f32(-1e-3)
    u = f32(rng.standard_normal(grid.m))
    zero = dense_absorb(grid, X, np.zeros(N), np.zeros((N, d)), gvar, wa, wa, noise, pvar, KS2, u)
    mean, grad = zero["mean_out"], zero["grad"]
    dn = KS2 * noise
    ratio = 10.0 ** rng.uniform(-3.0, 3.0, N)
    ratio[RLO], ratio[RHI] = 1e-3, 1e3
    e2 = grad * grad + np.maximum(gvar, 0.0)
    xvar = (ratio * dn / d)[:, None] / np.where(e2 > 0, e2, 1.0)      # (e2 = 0: a boundary cell of the dim at a point without slope variance)
    xvar[list(ZERO)] = 0.0
    xvar[NANXI, d - 1] = np.nan
    xvar[HUGE] = 1e20
    xvar[OUTSIDE] = 0.01
    xvar = f32(xvar)
    y = f32(mean + np.sqrt(np.maximum(pvar, 0) + dn) * rng.uniform(-2.0, 2.0, N))
    c = dict(grid=grid, X=X, y=y, xvar=xvar, gvar=gvar, wa=wa, noise=noise, pvar=pvar, u=u, dn=dn, d=d, ok=inside(grid, X))
    for key, gv in (("ref", gvar), ("ref_mean", None)):
        c[key] = dense_absorb(grid, X, y, xvar, gv, wa, wa, noise, pvar, KS2, u)
    _cases[name] = c
    return c


class DenseStream:
    """A GP on the SKI kernel W Kuu W^T held in data space (n x n work), fed batch by batch.  `slope`: "posterior" inflates the noise
    of an entering point by xvar E[(d f)^2] under the posterior before the batch, "mean" by xvar (E d f)^2, None not at all (the
    plain model).  Forgetting ages the effective noise of what is held by 1 / gamma before a batch."""

    def __init__(self, grid_bounds, grid_size, lengthscale, outputscale, sigma2, kind="rbf", slope="posterior", gamma=None, grid=None):
        self.grid = grid if grid is not None else Grid.from_bounds(grid_bounds, grid_size)
        self.K = dense_kuu(self.grid, kind, lengthscale, outputscale)
        self.sigma2, self.slope, self.gamma = float(sigma2), slope, gamma
        m = self.grid.m
        self.W, self.y, self.eff = np.zeros((0, m)), np.zeros(0), np.zeros(0)
        self.last = None

    def _factor(self):
        S = self.W @ self.K @ self.W.T + self.sigma2 * np.diag(self.eff)
        return sla.cho_factor(S, lower=True) if self.y.size else None

    def jet(self, X):
        """(mean [n], grad [n, d], pvar [n], gvar [n, d]) of f and its partial derivatives at X under the current posterior."""
        Wq, dWq = rows(self.grid, X)
        R = np.concatenate([Wq[:, None], dWq], 1)                         # [n, 1 + d, m]
        RK = R @ self.K
        var = np.einsum("ncm,ncm->nc", RK, R)
        mean = np.zeros(var.shape)
        ch = self._factor()
        if ch is not None:
            C = RK @ self.W.T                                            # [n, 1 + d, N]
            mean = C @ sla.cho_solve(ch, self.y)
            V = sla.solve_triangular(ch[0], C.reshape(-1, C.shape[-1]).T, lower=True)
            var = var - (V * V).sum(0).reshape(var.shape)
        return mean[:, 0], mean[:, 1:], var[:, 0], var[:, 1:]

    def predict(self, X):
        mean, _, var, _ = self.jet(X)
        return mean, var

    def predict_noisy_input(self, X, xvar):
        """Prediction at an uncertain query: the mean unchanged, the variance plus sum_k xvar_k (E[g_k]^2 + Var g_k)."""
        mean, grad, var, gvar = self.jet(X)
        return mean, var + (np.broadcast_to(np.asarray(xvar, dtype=np.float64), grad.shape) * (grad * grad + np.maximum(gvar, 0.0))).sum(1)

    def absorb(self, X, y, noise=None, xvar=0.0, plain=False):
        """plain: this batch enters at its declared noise whatever the rule (initial data)."""
        X = np.asarray(X, dtype=np.float64).reshape(-1, self.grid.d)
        y = np.asarray(y, dtype=np.float64).reshape(-1)
        noise = np.ones(y.shape[0]) if noise is None else np.broadcast_to(np.asarray(noise, dtype=np.float64), y.shape).copy()
        if self.gamma is not None and not plain:
            self.eff = self.eff / self.gamma
        if self.slope is None or plain:
            omega = np.ones(y.shape[0])
            self.last = None
        else:
            mean, grad, pvar, gvar = self.jet(X)
            st = sites(y, mean, grad, pvar, gvar if self.slope == "posterior" else None, self.sigma2 * noise, xvar)   # xvar: scalar, [d] or [n, d]
            omega = st["omega"]
            self.last = dict(st, grad=grad, mean=mean)
        ent = omega > 0.0
        self.W = np.concatenate([self.W, rows(self.grid, X[ent])[0]])
        self.y = np.concatenate([self.y, y[ent]])
        self.eff = np.concatenate([self.eff, noise[ent] / omega[ent]])
        return self

    def mll(self):
        """-(1/2)[quad + logdet + n log 2 pi] / n of the pseudo-data, as oracle.dataspace.DataSpaceGP.mll."""
        ch, n = self._factor(), self.y.shape[0]
        quad = float(self.y @ sla.cho_solve(ch, self.y))
        return -0.5 * (quad + 2.0 * float(np.log(np.diag(ch[0])).sum()) + n * np.log(2.0 * np.pi)) / n


# ------------------------------------------------------------------------------------------------------------- the toy problem
# (grid_bounds are the interior bounds of gpytorch's convention: one node lies 1.3 / 48 beyond either, so the 48 nodes span [-0.15, 1.15])
TOY = dict(bounds=[[-0.15 + 1.3 / 48, 1.15 - 1.3 / 48]], size=[48], ell=[0.08], osc=1.0, sigma_y=0.05, sigma_x=0.03, batches=8, q=16, ntest=200)


def toy_truth(x):
    return np.tanh(12.0 * (np.asarray(x) - 0.5))


def toy_stream(seed):
    """(X recorded [128, 1], y [128], Xs [200, 1]): the true locations are uniform on [0, 1], the recorded ones carry N(0, sigma_x^2),
    the readings N(0, sigma_y^2); clean test points on a regular mesh over [0.02, 0.98]."""
    rng = np.random.default_rng(seed)
    X, y = [], []
    for _ in range(TOY["batches"]):                                     # (per batch: the true locations, the readings, the recorded locations)
        xt = rng.uniform(0.0, 1.0, TOY["q"])
        y.append(toy_truth(xt) + TOY["sigma_y"] * rng.standard_normal(TOY["q"]))
        X.append(xt + TOY["sigma_x"] * rng.standard_normal(TOY["q"]))
    return np.concatenate(X)[:, None], np.concatenate(y), np.linspace(0.02, 0.98, TOY["ntest"])[:, None]


def toy_run(seed, slope, true_slope=False):
    """The stream of `seed` through DenseStream from a cold start: (NLPD, RMSE) of the noise-free truth at the test points under the
    latent posterior, and the model.  true_slope: the oracle -- the noise inflated by the true slope at the recorded location."""
    X, y, Xs = toy_stream(seed)
    s2 = TOY["sigma_y"] ** 2
    M = DenseStream(TOY["bounds"], TOY["size"], TOY["ell"], TOY["osc"], s2, slope=None if true_slope else slope)
    for k in range(TOY["batches"]):
        sl = slice(k * TOY["q"], (k + 1) * TOY["q"])
        if true_slope:
            g = 12.0 * (1.0 - toy_truth(X[sl, 0]) ** 2)
            M.absorb(X[sl], y[sl], noise=1.0 + TOY["sigma_x"] ** 2 * g * g / s2)
        else:
            M.absorb(X[sl], y[sl], xvar=TOY["sigma_x"] ** 2)
    mean, var = M.predict(Xs)
    return nlpd(toy_truth(Xs[:, 0]), mean, var), float(np.sqrt(np.mean((mean - toy_truth(Xs[:, 0])) ** 2))), M


def nlpd(truth, mean, var):
    var = np.maximum(var, 1e-12)
    return float(np.mean(0.5 * (truth - mean) ** 2 / var + 0.5 * np.log(2.0 * np.pi * var)))
