"""TEST INFRASTRUCTURE -- fp64 reference of the heteroscedastic absorb, shared by tests/test_hetero_host.py (no GPU)
and tests/test_hetero_gpu.py.

    y_p = f(x_p) + eps_p,   eps_p ~ N(0, sigma2 noise_p exp g(x_p)),   g ~ GP(g0, k_g)

f and g are two models on one grid.  Against the two posteriors BEFORE the batch -- mu_f = w_p . u_f, v_f = max(pvar_f, 0),
mu_g = g0 + w_p . u_g, v_g = max(pvar_g, 0) --

    e     = exp(mu_g + v_g / 2),   dn = sigma2 noise_p e,
    f     takes y_p at noise noise_p e (weight omega_f = 1 / e, not capped),   log Z_y = log N(y; mu_f, v_f + dn),
    rho   = (y_p - mu_f)^2 / (sigma2 noise_p) * dn / (dn + v_f),
    g     takes the site (ytilde_g, tau_g) of l(g) = (2 pi)^(-nu / 2) exp(-nu g / 2 - rho e^-g / 2), nu = 1, matched against N(mu_g, v_g),
          as the target ytilde_g - g0 at noise 1 / tau_g (the noise model's own sigma2 = noise = wa = wb = 1).

A noise site is skipped (tau = 0, ytilde = mu_g) when tau < OMEGA_MIN or beta is not positive and finite -- rho = 0 is -- and the point
still enters f.  A y that is not finite skips the point for both (both log Z = NaN); a point outside the grid is dropped for both,
counted once in err and reports zeros.

``sites`` is the reference of the noise site: a composite trapezoid of 6001 nodes between the points where the log integrand has
fallen by 60 from its maximum, found by bisection, as in count_reference -- plain numpy, nothing shared with the kernel but the
definitions; pinned to 50-digit mpmath.quad in tests/test_hetero_host.py.  ``DenseStream`` is the estimator as a dense stream on the
grid (both posteriors by dense solves), for the property test.
"""
import math

import numpy as np
import torch

import interp_reference as ir
import regrid_reference as rr
from count_reference import deviation, moments  # noqa: F401  (what the posterior receives from a site: the same for every family)
from grad_obs_reference import Grid, dense_kuu, inside  # noqa: F401

OMEGA_MIN = 1e-12
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
NREF, DROP_REF = 6001, 60.0


# ------------------------------------------------------------------------------------------------------------ the likelihood
def log_lik(rho, nu, g):
    with np.errstate(over="ignore"):
        return -nu * HALF_LOG_2PI - 0.5 * (nu * g + rho * np.exp(-g))


def d_log_lik(rho, nu, g):
    with np.errstate(over="ignore"):
        return 0.5 * (rho * np.exp(-g) - nu)


def d2_log_lik(rho, nu, g):
    with np.errstate(over="ignore"):
        return -0.5 * rho * np.exp(-g)


def valid(rho, nu):
    return rho == rho and nu == nu and rho >= 0 and nu > 0 and not math.isinf(rho) and not math.isinf(nu)


def _finish(mu, tau, alpha, beta, log_z):
    """(ytilde, tau, log_z, alpha, beta) with the skip rule applied."""
    if not (beta > 0.0 and math.isfinite(beta)) or not (tau >= OMEGA_MIN and math.isfinite(tau)):
        return mu, 0.0, log_z, alpha, beta
    return mu + alpha / beta, tau, log_z, alpha, beta


def mode(rho, nu, mu, v):
    """The tilted mode by bisection of h' on [mu, mu + v l'(mu)] (l' decreases: the mode lies between)."""
    d0 = float(d_log_lik(rho, nu, mu))
    a, b = (mu, mu + v * d0) if d0 >= 0 else (mu + v * d0, mu)
    for _ in range(200):
        c = 0.5 * (a + b)
        if float(d_log_lik(rho, nu, c)) - (c - mu) / v > 0:
            a = c
        else:
            b = c
    return 0.5 * (a + b)


def _site_ref(rho, nu, mu, v):
    nan = float("nan")
    if not valid(rho, nu) or not (mu == mu and v == v):
        return mu, 0.0, nan, nan, nan
    v = max(v, 0.0)
    if v == 0.0:
        l0, l1, l2 = (float(fn(rho, nu, mu)) for fn in (log_lik, d_log_lik, d2_log_lik))
        return _finish(mu, -l2, l1, -l2, l0)
    h = lambda g: log_lik(rho, nu, g) - (g - mu) ** 2 / (2.0 * v)
    c = mode(rho, nu, mu, v)
    hc = float(h(c))

    def edge(sign):
        lo, hi = 0.0, math.sqrt(2.0 * DROP_REF * v) * 1.001 + 1e-300      # -h'' >= 1 / v: the drop is reached within this
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            if hc - float(h(c + sign * mid)) < DROP_REF:
                lo = mid
            else:
                hi = mid
        return c + sign * hi

    L, R = edge(-1.0), edge(1.0)
    g = np.linspace(L, R, NREF)
    w = np.exp(h(g) - hc)
    w[0] *= 0.5
    w[-1] *= 0.5
    S0 = w.sum()
    x = g - c
    m1 = (w * x).sum() / S0
    V = (w * (x - m1) ** 2).sum() / S0
    l1c = float(d_log_lik(rho, nu, c))
    dl = d_log_lik(rho, nu, g) - l1c
    El = (w * dl).sum() / S0
    Vl = (w * (dl - El) ** 2).sum() / S0
    beta_w = -(w * d2_log_lik(rho, nu, g)).sum() / S0 - Vl
    log_z = hc + math.log(S0 * (R - L) / (NREF - 1)) - 0.5 * math.log(v) - HALF_LOG_2PI
    if v * beta_w < 0.25:                                                # a weak site: 1 / V - 1 / v would cancel
        beta, alpha = beta_w, l1c + El
        tau = beta / (1.0 - v * beta)
    else:                                                                # a sharp one: -E l'' - Var l' would
        tau = 1.0 / V - 1.0 / v
        beta, alpha = (v - V) / (v * v), (c + m1 - mu) / v
    return _finish(mu, tau, alpha, beta, log_z)


def sites(rho, nu, mu, v):
    """The reference noise sites of rho (sum of squares of nu residuals in units of the known noise) against N(mu, v) of the log
    multiplier (all [n], or scalars broadcast): dict of ytilde, tau, omega (= tau), log_z, alpha, beta [n] and skipped (tau == 0)."""
    rho, nu, mu, v = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (rho, nu, mu, v)))
    out = np.array([_site_ref(*(float(a) for a in row)) for row in zip(rho.ravel(), nu.ravel(), mu.ravel(), v.ravel())]).reshape(-1, 5)
    r = {k: out[:, i].reshape(rho.shape) for i, k in enumerate(("ytilde", "tau", "log_z", "alpha", "beta"))}
    r["omega"] = r["tau"]
    r["skipped"] = r["tau"] == 0.0
    return r


# --------------------------------------------------------------------------------------------------------------- the box
def box_cases(n, seed):
    """(rho, nu, mu, v) [n] on the specified box: mu_g in [-8, 8], v_g log-uniform in [1e-4, 9] (every 20th exactly 0), nu in {1, 4} in
    turn, zeta = rho exp(-mu_g) log-uniform in [1e-6, 400]."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-8.0, 8.0, n)
    v = np.exp(rng.uniform(math.log(1e-4), math.log(9.0), n))
    v[::20] = 0.0
    nu = np.where(np.arange(n) % 2 == 0, 1.0, 4.0)
    zeta = np.exp(rng.uniform(math.log(1e-6), math.log(400.0), n))
    return zeta * np.exp(mu), nu, mu, v


# ------------------------------------------------------------------------------------------------------------- the point rule
def point_sites(y, mu_f, pvar_f, wug, pvar_g, noise, sigma2, g0):
    """What a point inside the grid makes of its datum: dict of e, omega_f, log_zy, rho, enters (bool) and the noise site's ytilde, tau,
    log_z, skipped [n].  wug = w . u_g (without g0)."""
    y, mu_f, pvar_f, wug, pvar_g, noise = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (y, mu_f, pvar_f, wug, pvar_g, noise)))
    v_f, v_g = np.maximum(pvar_f, 0.0), np.maximum(pvar_g, 0.0)
    mu_g = g0 + wug
    e = np.exp(mu_g + 0.5 * v_g)
    kn = sigma2 * noise
    dn = kn * e
    enters = np.isfinite(y) & np.isfinite(mu_f) & (dn > 0) & np.isfinite(dn) & (kn > 0)
    s = v_f + dn
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.where(enters, y - mu_f, 0.0)
        log_zy = np.where(enters, -HALF_LOG_2PI - 0.5 * np.log(s) - 0.5 * d * d / s, np.nan)
        rho = np.where(enters, d * d / kn * (dn / s), np.nan)
    st = sites(np.where(enters, rho, 0.0), 1.0, mu_g, v_g)
    tau = np.where(enters, st["tau"], 0.0)
    return {"e": e, "omega_f": np.where(enters, 1.0 / e, 0.0), "log_zy": log_zy, "rho": rho, "enters": enters, "ytilde": np.where(enters, st["ytilde"], mu_g),
            "tau": tau, "log_z": np.where(enters, st["log_z"], np.nan), "skipped": enters & (tau == 0.0)}


# ------------------------------------------------------------------------------------------------------------- the dense absorb
def _dense_set(grid, W, wa, wb, target, mean, ent, log_noise):
    A = W.T @ (W * wa[:, None])
    A = np.triu(A) + np.triu(A, 1).T
    return {"A": A, "A_half": rr.pack_half(torch.as_tensor(A), grid.g).numpy(), "b": W.T @ (wb * target), "cnt": W.T @ wa,
            "res": W.T @ (wb * target - wa * mean), "stats": np.array([(wb * target * target)[ent].sum(), log_noise[ent].sum()])}


def dense_absorb(grid, X, y, wa, wb, noise, pvar, pvar2, sigma2, g0, u, u2):
    """What one heteroscedastic absorb launch adds, densely: dict of "f" and "g" (each a dict of A [m, m], A_half (flat), b, cnt, res [m],
    stats [2]), the per-point e, ytilde, tau, log_z, log_zy, entered_f, entered_g, mean_out [n], and err (bit 0 | 2 x dropped points)."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, grid.d)
    W = ir.dense_rows(grid, torch.as_tensor(X)).numpy()                  # rows of a point outside the grid are zero
    y, wa, wb, noise, pvar, pvar2, u, u2 = (np.asarray(a, dtype=np.float64) for a in (y, wa, wb, noise, pvar, pvar2, u, u2))
    ok = inside(grid, X)
    mean, wug = W @ u, W @ u2
    ps = point_sites(y, mean, pvar, wug, pvar2, noise, sigma2, g0)
    in_f = ok & ps["enters"]
    in_g = in_f & (ps["tau"] > 0)
    of = np.where(in_f, ps["omega_f"], 0.0)
    tau = np.where(in_g, ps["tau"], 0.0)
    y0 = np.where(in_f, y, 0.0)
    tg = np.where(in_g, ps["ytilde"] - g0, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ldf = np.where(in_f, np.log(noise * ps["e"]), 0.0)
        ldg = np.where(in_g, -np.log(np.where(in_g, tau, 1.0)), 0.0)
    zero = lambda a: np.where(ok, a, 0.0)
    return {"f": _dense_set(grid, W, wa * of, wb * of, y0, mean, in_f, ldf), "g": _dense_set(grid, W, tau, tau, tg, wug, in_g, ldg),
            "e": zero(ps["e"]), "ytilde": zero(ps["ytilde"]), "tau": tau, "log_z": zero(ps["log_z"]), "log_zy": zero(ps["log_zy"]),
            "entered_f": in_f, "entered_g": in_g, "skipped": in_f & ~in_g, "mean_out": mean, "err": int((~ok).any()) + 2 * int((~ok).sum())}


# ---------------------------------------------------------------------------------------------------------------- the stream
def sigma_true(x):
    """The noise standard deviation of the property stream."""
    return 0.05 + 0.45 * np.asarray(x, dtype=np.float64) ** 2


def f_true(x):
    return np.sin(6.0 * np.asarray(x, dtype=np.float64))


STREAM = dict(grid_bounds=[(0.0, 1.0)], grid_size=40, sigma2=0.04, g0=0.0, ell_f=0.2, os_f=1.0, ell_g=0.3, os_g=4.0, batches=20, batch=32, held_out=4000)


def stream_data(seed, n_batches=STREAM["batches"], batch=STREAM["batch"], held_out=STREAM["held_out"]):
    """(X [B, q], Y [B, q], Xt [T], Yt [T]) of the property stream: x uniform in [0.02, 0.98], f = sin 6x, sigma(x) = 0.05 + 0.45 x^2."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.02, 0.98, (n_batches, batch))
    Y = f_true(X) + sigma_true(X) * rng.standard_normal(X.shape)
    Xt = rng.uniform(0.02, 0.98, held_out)
    Yt = f_true(Xt) + sigma_true(Xt) * rng.standard_normal(held_out)
    return X, Y, Xt, Yt


class DenseStream:
    """The estimator as a dense stream on the grid: statistics (A, b) of f and of g, both posteriors by dense solves on the m nodes.
    hetero False: the plain model at the noise it is given (the true-noise and constant-noise baselines)."""

    def __init__(self, grid, sigma2, ell_f, os_f, ell_g=None, os_g=None, g0=0.0, hetero=True):
        self.grid, self.sigma2, self.g0, self.hetero = grid, float(sigma2), float(g0), hetero
        m = grid.m
        self.Kf = dense_kuu(grid, "rbf", ell_f, os_f)
        self.Af, self.bf = np.zeros((m, m)), np.zeros(m)
        if hetero:
            self.Kg = dense_kuu(grid, "rbf", ell_g, os_g)
            self.Ag, self.bg = np.zeros((m, m)), np.zeros(m)
        self.skipped = 0
        self.sites = []

    @staticmethod
    def _post(K, A, b, s2):
        """(u, Sigma): mean and covariance of the grid values under the statistics (A, b) at noise scale s2."""
        M = np.linalg.solve(s2 * np.eye(K.shape[0]) + A @ K, np.column_stack([b, A @ K]))
        return K @ M[:, 0], K - K @ M[:, 1:]

    def rows(self, X):
        return ir.dense_rows(self.grid, torch.as_tensor(np.asarray(X, dtype=np.float64).reshape(-1, self.grid.d))).numpy()

    def posterior_f(self, W):
        u, S = self._post(self.Kf, self.Af, self.bf, self.sigma2)
        return u, W @ u, np.einsum("ij,jk,ik->i", W, S, W)

    def posterior_g(self, W):
        u, S = self._post(self.Kg, self.Ag, self.bg, 1.0)
        return u, self.g0 + W @ u, np.einsum("ij,jk,ik->i", W, S, W)

    def absorb(self, X, y, noise=None):
        W = self.rows(X)
        y = np.asarray(y, dtype=np.float64)
        noise = np.ones_like(y) if noise is None else np.asarray(noise, dtype=np.float64)
        if not self.hetero:
            self.Af += W.T @ (W / noise[:, None])
            self.bf += W.T @ (y / noise)
            return None
        _, mu_f, v_f = self.posterior_f(W)
        ug, mu_g, v_g = self.posterior_g(W)
        ps = point_sites(y, mu_f, v_f, mu_g - self.g0, v_g, noise, self.sigma2, self.g0)
        wf = ps["omega_f"] / noise
        self.Af += W.T @ (W * wf[:, None])
        self.bf += W.T @ (wf * y)
        self.Ag += W.T @ (W * ps["tau"][:, None])
        self.bg += W.T @ (ps["tau"] * (ps["ytilde"] - self.g0))
        self.skipped += int(ps["skipped"].sum())
        self.sites.append(ps)
        return ps

    def predictive(self, X, noise=None):
        """(mean, variance of y): the latter with the noise the model predicts (hetero) or is given (relative to sigma2)."""
        W = self.rows(X)
        _, mu_f, v_f = self.posterior_f(W)
        noise = np.ones(W.shape[0]) if noise is None else np.asarray(noise, dtype=np.float64)
        if self.hetero:
            _, mu_g, v_g = self.posterior_g(W)
            noise = noise * np.exp(mu_g + 0.5 * np.maximum(v_g, 0.0))
        return mu_f, np.maximum(v_f, 0.0) + self.sigma2 * noise


def nlpd(y, mean, var):
    return float(np.mean(0.5 * np.log(2.0 * np.pi * var) + 0.5 * (y - mean) ** 2 / var))


CONSTANT_NOISES = tuple(float(s) ** 2 for s in np.geomspace(0.03, 0.6, 25))     # the candidates of the best-constant baseline (variances)


def stream_report(het_predictive, seed):
    """The figures of conditions (a)-(c) for a heteroscedastic model given as ``het_predictive(Xt) -> (mean, var)`` AFTER it has taken the
    stream of ``seed``; the two baselines are dense streams here.  Returns dict of nlpd_het, nlpd_true, nlpd_const, cover_lo, cover_hi."""
    X, Y, Xt, Yt = stream_data(seed)
    grid = Grid.from_bounds(STREAM["grid_bounds"], STREAM["grid_size"])
    s2 = STREAM["sigma2"]
    true = DenseStream(grid, s2, STREAM["ell_f"], STREAM["os_f"], hetero=False)
    consts = [DenseStream(grid, c, STREAM["ell_f"], STREAM["os_f"], hetero=False) for c in CONSTANT_NOISES]
    for xb, yb in zip(X, Y):
        true.absorb(xb, yb, sigma_true(xb) ** 2 / s2)
        for m in consts:
            m.absorb(xb, yb)
    mean, var = het_predictive(Xt)
    mean, var = np.asarray(mean, dtype=np.float64), np.asarray(var, dtype=np.float64)
    z = 1.6448536269514722
    hit = np.abs(Yt - mean) <= z * np.sqrt(var)
    return dict(nlpd_het=nlpd(Yt, mean, var), nlpd_true=nlpd(Yt, *true.predictive(Xt, sigma_true(Xt) ** 2 / s2)),
                nlpd_const=min(nlpd(Yt, *m.predictive(Xt)) for m in consts), cover_lo=float(hit[Xt < 0.5].mean()), cover_hi=float(hit[Xt >= 0.5].mean()))


def stream_conditions(r):
    """Conditions (a) and (b) on a ``stream_report``."""
    a = r["nlpd_het"] - r["nlpd_true"] <= 0.25 * (r["nlpd_const"] - r["nlpd_true"])
    b = all(0.86 <= r[k] <= 0.94 for k in ("cover_lo", "cover_hi"))
    return a, b
