"""TEST INFRASTRUCTURE -- fp64 reference of the count-observation absorb, shared by tests/test_count_host.py (no GPU)
and tests/test_count_gpu.py.

Point i carries a count y_i and a second number t_i: y ~ Poisson(t exp f) (family 0, t the exposure) or y successes of t trials at
success probability sigmoid(f) (family 1).  Against the posterior BEFORE the batch -- mu_i = w_i . u, v_i = max(pvar_i, 0) --

    Z = int l(f) N(f; mu, v) df,   alpha = d log Z / d mu,   beta = -d^2 log Z / d mu^2,
    tau = beta / (1 - v beta),   ytilde = mu + alpha / beta,   omega = sigma2 noise tau,

and the point enters the statistics as the target ytilde at noise noise_i / omega_i (effective noise variance 1 / tau).  v = 0 is the
Laplace site at mu.  A point is skipped (omega = 0, ytilde = mu, nothing enters) when omega < OMEGA_MIN, when beta is not positive and
finite, or when the input is invalid (y < 0, t <= 0, y > t for the binomial, a NaN: log Z = NaN).  A point outside the grid is dropped,
counted in err and reports (0, 0, 0).

Two evaluations live here.  ``sites`` is the reference: a composite trapezoid of 6001 nodes between the points where the log integrand
has fallen by 60 from its maximum, found by bisection -- plain numpy, nothing shared with the kernel but the definitions; it is pinned
to 50-digit mpmath.quad in tests/test_count_host.py.  ``rule_sites`` restates the KERNEL's rule (scatter_count.h: sectioning to the
mode, a ladder to the bracket, 64 Gauss-Legendre nodes on either side of the mode, two per lane) so that its accuracy on the specified
box can be asserted without a GPU.
"""
import math

import numpy as np
import torch

import interp_reference as ir
import regrid_reference as rr
from interval_reference import Grid, inside  # noqa: F401

OMEGA_MIN = 1e-12
POISSON, BINOMIAL = 0, 1
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


# ------------------------------------------------------------------------------------------------------------------ the families
def _softplus(f):
    return np.maximum(f, 0.0) + np.log1p(np.exp(-np.abs(f)))


def _sigmoid(f):
    e = np.exp(-np.abs(f))
    return np.where(f >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def log_lik(family, y, t, f):
    """g(f) = log l(f), with its constant."""
    with np.errstate(over="ignore"):
        if family == POISSON:
            return y * (f + math.log(t)) - t * np.exp(f) - math.lgamma(y + 1.0)
        return y * f - t * _softplus(f) + math.lgamma(t + 1.0) - math.lgamma(y + 1.0) - math.lgamma(t - y + 1.0)


def d_log_lik(family, y, t, f):
    with np.errstate(over="ignore"):
        return y - t * np.exp(f) if family == POISSON else y - t * _sigmoid(f)


def d2_log_lik(family, y, t, f):
    with np.errstate(over="ignore"):
        if family == POISSON:
            return -t * np.exp(f)
        s = _sigmoid(f)
        return -t * s * (1.0 - s)


def valid(family, y, t):
    if not (y == y and t == t) or y < 0 or t <= 0 or math.isinf(y) or math.isinf(t):
        return False
    return family == POISSON or y <= t


def _finish(mu, v, tau, alpha, beta, log_z, sigma2):
    """(ytilde, omega, log_z, alpha, beta, tau) with the skip rule applied."""
    if not (beta > 0.0 and math.isfinite(beta)):
        return mu, 0.0, log_z, alpha, beta, 0.0
    omega = sigma2 * tau
    if not (omega >= OMEGA_MIN and math.isfinite(omega)):
        return mu, 0.0, log_z, alpha, beta, 0.0
    return mu + alpha / beta, omega, log_z, alpha, beta, tau


def _mode(family, y, t, mu, v):
    """The tilted mode by bisection of h' on [mu, mu + v g'(mu)] (g' decreases: the mode lies between) and Newton steps."""
    d0 = float(d_log_lik(family, y, t, mu))
    a, b = (mu, mu + v * d0) if d0 >= 0 else (mu + v * d0, mu)
    dh = lambda f: float(d_log_lik(family, y, t, f)) - (f - mu) / v
    for _ in range(200):
        c = 0.5 * (a + b)
        if dh(c) > 0:
            a = c
        else:
            b = c
    return 0.5 * (a + b)


# ---------------------------------------------------------------------------------------------------------------- the reference
NREF, DROP_REF = 6001, 60.0


def _site_ref(family, y, t, mu, v, sigma2):
    nan = float("nan")
    if not valid(family, y, t) or not (mu == mu and v == v):
        return mu, 0.0, nan, nan, nan, 0.0
    v = max(v, 0.0)
    if v == 0.0:
        g0, g1, g2 = (float(fn(family, y, t, mu)) for fn in (log_lik, d_log_lik, d2_log_lik))
        return _finish(mu, v, -g2, g1, -g2, g0, sigma2)
    h = lambda f: log_lik(family, y, t, f) - (f - mu) ** 2 / (2.0 * v)
    c = _mode(family, y, t, mu, v)
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
    f = np.linspace(L, R, NREF)
    w = np.exp(h(f) - hc)
    w[0] *= 0.5
    w[-1] *= 0.5
    S0 = w.sum()
    x = f - c
    m1 = (w * x).sum() / S0
    V = (w * (x - m1) ** 2).sum() / S0
    g1c = float(d_log_lik(family, y, t, c))
    dg = d_log_lik(family, y, t, f) - g1c
    Eg = (w * dg).sum() / S0
    Vg = (w * (dg - Eg) ** 2).sum() / S0
    beta_w = -(w * d2_log_lik(family, y, t, f)).sum() / S0 - Vg
    log_z = hc + math.log(S0 * (R - L) / (NREF - 1)) - 0.5 * math.log(v) - HALF_LOG_2PI
    if v * beta_w < 0.25:                                                # a weak site: 1 / V - 1 / v would cancel
        beta, alpha = beta_w, g1c + Eg
        tau = beta / (1.0 - v * beta)
    else:                                                                # a sharp one: -E g'' - Var g' would
        tau = 1.0 / V - 1.0 / v
        beta, alpha = (v - V) / (v * v), (c + m1 - mu) / v
    return _finish(mu, v, tau, alpha, beta, log_z, sigma2)


def _table(fn, y, t, family, mean, pvar, sigma2):
    y, t, mean, pvar, sigma2 = np.broadcast_arrays(*(np.asarray(a, dtype=np.float64) for a in (y, t, mean, pvar, sigma2)))
    out = np.array([fn(family, *(float(a) for a in row)) for row in zip(y.ravel(), t.ravel(), mean.ravel(), pvar.ravel(), sigma2.ravel())]).reshape(-1, 6)
    r = {k: out[:, i].reshape(y.shape) for i, k in enumerate(("ytilde", "omega", "log_z", "alpha", "beta", "tau"))}
    r["skipped"] = r["omega"] == 0.0
    return r


def sites(y, t, family, mean, pvar, sigma2):
    """The reference sites of counts y at exposure / trials t against predictive means `mean` and posterior variances `pvar` (all [n],
    or scalars broadcast): dict of ytilde, omega, log_z, alpha, beta, tau [n] and skipped (bool [n]: omega == 0)."""
    return _table(_site_ref, y, t, family, mean, pvar, sigma2)


def moments(st, mean, pvar):
    """(mhat, Vhat): what the posterior receives from a site -- Vhat = 1 / (1 / v + tau), mhat = Vhat (mu / v + tau ytilde)."""
    mean, pvar = np.asarray(mean, dtype=np.float64), np.maximum(np.asarray(pvar, dtype=np.float64), 0.0)
    tau, yt = st["tau"], st["ytilde"]
    V = pvar / (1.0 + pvar * tau)
    return V * tau * (yt - mean) + mean, V


# ------------------------------------------------------------------------------------------------- the kernel's rule, restated
NPASS, NNEWTON, DROP, LADDER = 4, 2, 40.0, 1.3
GL_X, GL_W = (a[32:] for a in np.polynomial.legendre.leggauss(64))      # the positive half of the symmetric rule


def _site_rule(family, y, t, mu, v, sigma2):
    nan = float("nan")
    if not valid(family, y, t) or not (mu == mu and v == v):
        return mu, 0.0, nan, nan, nan, 0.0
    v = max(v, 0.0)
    g1 = lambda f: d_log_lik(family, y, t, f)
    g2 = lambda f: d2_log_lik(family, y, t, f)
    if v == 0.0:
        return _finish(mu, v, -float(g2(mu)), float(g1(mu)), -float(g2(mu)), float(log_lik(family, y, t, mu)), sigma2)
    lane = np.arange(64)
    h = lambda f: log_lik(family, y, t, f) - (f - mu) ** 2 / (2.0 * v)
    # the mode: it lies between mu and mu + v g'(mu); each pass puts 64 lanes on the bracket and keeps the sixty-fourth that holds it
    d0 = float(g1(mu))
    a, W = mu, v * d0
    up = d0 >= 0.0
    for _ in range(NPASS):
        x = a + W * (lane + 1) / 64.0
        dh = g1(x) - (x - mu) / v
        k = int(((dh > 0.0) if up else (dh < 0.0)).sum())
        a, W = a + W * k / 64.0, W / 64.0
    c = a + 0.5 * W
    for _ in range(NNEWTON):
        c = c - (float(g1(c)) - (c - mu) / v) / (float(g2(c)) - 1.0 / v)
    hc = float(h(c))
    # the bracket: lanes 0..31 look left, 32..63 right; a geometric ladder down from sqrt(2 DROP v), then 32 even steps
    side = np.where(lane < 32, -1.0, 1.0)
    k = lane & 31
    D = math.sqrt(2.0 * DROP * v)
    d = D * LADDER ** (-k.astype(np.float64))
    ok = hc - h(c + side * d) >= DROP
    e = np.empty(2)
    for s, sl in enumerate((slice(0, 32), slice(32, 64))):
        n_ok = int(ok[sl].sum())
        outer = D * LADDER ** (-float(max(n_ok - 1, 0)))
        inner = outer / LADDER if n_ok > 0 else outer
        step = inner + (outer - inner) * (k[sl] + 1) / 32.0
        short = hc - h(c + side[sl] * step) < DROP
        e[s] = inner + (outer - inner) * (min(int(short.sum()), 31) + 1) / 32.0
    # the nodes: each lane takes the pair -+ xi_k of the 64-point rule on its side (arrays [2, 64] below)
    half = 0.5 * np.where(lane < 32, e[0], e[1])
    x = half * np.stack([1.0 - GL_X[k], 1.0 + GL_X[k]])                    # distance from c
    f = c + side * x
    w = half * GL_W[k] * np.exp(h(f) - hc)
    g1c = float(g1(c))
    dg = g1(f) - g1c
    S0 = w.sum()
    S1, S2 = (w * side * x).sum() / S0, (w * x * x).sum() / S0
    G1, G2, H2 = (w * dg).sum() / S0, (w * dg * dg).sum() / S0, (w * g2(f)).sum() / S0
    V = S2 - S1 * S1
    beta_w = -H2 - (G2 - G1 * G1)
    log_z = hc + math.log(S0) - 0.5 * math.log(v) - HALF_LOG_2PI
    if v * beta_w < 0.5:
        beta, alpha = beta_w, g1c + G1
        tau = beta / (1.0 - v * beta)
    else:
        tau = 1.0 / V - 1.0 / v
        beta, alpha = (v - V) / (v * v), (c + S1 - mu) / v
    return _finish(mu, v, tau, alpha, beta, log_z, sigma2)


def rule_sites(y, t, family, mean, pvar, sigma2):
    """``sites`` by the kernel's rule (scatter_count.h), lane for lane."""
    return _table(_site_rule, y, t, family, mean, pvar, sigma2)


# --------------------------------------------------------------------------------------------------------------- the box
def box_cases(family, n, seed, vmax=9.0):
    """(y, t, mu, v) [n] on the specified box: mu in [-3, 3], v in [0, vmax] (every 20th exactly 0), t log-uniform in [1e-2, 1e2]
    (Poisson) or an integer in 1..200 (binomial); y in turn drawn from the model, 0, and adversarial up to 2000 (capped at t for the
    binomial, which makes most of them y = t: every success)."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-3.0, 3.0, n)
    v = rng.uniform(0.0, vmax, n)
    v[::20] = 0.0
    f = mu + np.sqrt(v) * rng.standard_normal(n)
    kind = np.arange(n) % 3
    if family == POISSON:
        t = np.exp(rng.uniform(math.log(1e-2), math.log(1e2), n))
        drawn = rng.poisson(np.minimum(t * np.exp(f), 1e6)).astype(np.float64)
        adv = rng.integers(1, 2001, n).astype(np.float64)
    else:
        t = rng.integers(1, 201, n).astype(np.float64)
        drawn = rng.binomial(t.astype(np.int64), _sigmoid(f)).astype(np.float64)
        adv = np.minimum(rng.integers(0, 2001, n).astype(np.float64), t)
    y = np.where(kind == 0, drawn, np.where(kind == 1, 0.0, adv))
    return y, t, mu, v


def deviation(got, ref, mean, pvar):
    """The deviations of sites `got` from `ref` in what the posterior receives: dict of m (|mhat - mhat_ref| / sqrt Vhat_ref, v > 0),
    V (relative, v > 0), log_z (relative), tau (relative, where v tau <= 1 or v = 0); the largest over the entering sites."""
    pvar = np.maximum(np.asarray(pvar, dtype=np.float64), 0.0)
    ent = ~ref["skipped"]
    pos = ent & (pvar > 0)
    mg, Vg = moments(got, mean, pvar)
    mr, Vr = moments(ref, mean, pvar)
    weak = ent & (pvar * ref["tau"] <= 1.0)
    mx = lambda a: float(a.max()) if a.size else 0.0
    return dict(m=mx(np.abs(mg - mr)[pos] / np.sqrt(Vr[pos])), V=mx(np.abs(Vg - Vr)[pos] / Vr[pos]),
                log_z=mx(np.abs(got["log_z"] - ref["log_z"])[ent] / np.abs(ref["log_z"][ent])),
                tau=mx(np.abs(got["tau"] - ref["tau"])[weak] / ref["tau"][weak]))


# ------------------------------------------------------------------------------------------------------------- the dense absorb
def dense_absorb(grid, X, y, t, family, wa, wb, noise, pvar, sigma2, u):
    """What one count absorb launch adds, densely: dict of ytilde, omega, log_z, skipped, mean_out [n], A [m, m], A_half (flat), b, cnt,
    res [m], stats [2] and err (bit 0 | 2 x dropped points).  omega = sigma2 noise tau."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, grid.d)
    W = ir.dense_rows(grid, torch.as_tensor(X)).numpy()                  # rows of a point outside the grid are zero
    y, t, wa, wb, noise, pvar, u = (np.asarray(a, dtype=np.float64) for a in (y, t, wa, wb, noise, pvar, u))
    ok = inside(grid, X)
    mean = W @ u
    st = sites(y, t, family, mean, pvar, sigma2 * noise)
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
