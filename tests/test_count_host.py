"""No GPU: the site of a count observation and the identity behind its absorb, in numpy fp64.

The reference sites of tests/count_reference.py (a 6001-node trapezoid) are pinned to 50-digit mpmath.quad on the specified box, per
family -- mu in [-3, 3], v in [0, 9], t log-uniform in [1e-2, 1e2] (Poisson) or an integer in 1..200 (binomial); a third of the counts
drawn from the model, a third zero, a third adversarial up to 2000 -- in the quantities the posterior receives: |mhat - mhat_ref| /
sqrt(Vhat_ref) and |Vhat - Vhat_ref| / Vhat_ref with Vhat = 1 / (1 / v + tau), mhat = Vhat (mu / v + tau ytilde); log Z relative; tau
relative where v tau <= 1 and at v = 0.  REF_BOUND = 1e-9 is what the reference has to keep, three orders below the 1e-6 the kernel's
rule is held to; the rule itself, restated in numpy lane for lane (count_reference.rule_sites), is held to RULE_BOUND = 1e-6 against
the same 50-digit values, the condition DESIGN.md 3.23 sets before any GPU run.  alpha and beta are the first and (minus the) second
derivative of log Z in the mean, checked against central differences formed at 50 digits.  A batch absorbed with the reference's
sites gives the posterior mean, covariance and marginal likelihood of the data-space GP (oracle/dataspace.py) fitted at (ytilde_i,
1 / tau_i).  Independent of the kernel and of the model."""
import ctypes
import os

import mpmath as mp
import numpy as np
import pytest

import count_reference as cref
import sample_paths_reference as ref
from oracle import dataspace, spec
from test_forgetting_host import ELL, G, GB, OSC, S2, _close, _from_stats, _stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCASE = 60                                                             # per family; the GPU sweep takes 400 against the pinned reference
REF_BOUND, RULE_BOUND = 1e-9, 1e-6
FAMILIES = [("poisson", cref.POISSON, 11), ("binomial", cref.BINOMIAL, 12)]


def _mp_g(family, y, t):
    """(g, g', g'') of the family at 50 digits."""
    y, t = mp.mpf(y), mp.mpf(t)
    if family == cref.POISSON:
        c = y * mp.log(t) - mp.loggamma(y + 1)
        return (lambda f: y * f - t * mp.exp(f) + c), (lambda f: y - t * mp.exp(f)), (lambda f: -t * mp.exp(f))
    c = mp.loggamma(t + 1) - mp.loggamma(y + 1) - mp.loggamma(t - y + 1)
    sig = lambda f: 1 / (1 + mp.exp(-f))
    return (lambda f: y * f - t * mp.log(1 + mp.exp(f)) + c), (lambda f: y - t * sig(f)), (lambda f: -t * sig(f) * (1 - sig(f)))


def _mp_points(family, y, t, mu, v):
    c = mp.mpf(cref._mode(family, y, t, mu, v))
    kappa = 1 / mp.mpf(v) - mp.mpf(float(cref.d2_log_lik(family, y, t, float(c))))
    sd, far = 1 / mp.sqrt(kappa), 16 * mp.sqrt(mp.mpf(v))
    return c, sorted({c - far, c - min(8 * sd, far / 2), c - min(3 * sd, far / 4), c, c + min(3 * sd, far / 4), c + min(8 * sd, far / 2), c + far})


def _mp_logz(family, y, t, mu, v, pts, c):
    g = _mp_g(family, y, t)[0]
    mu, v = mp.mpf(mu), mp.mpf(v)
    h = lambda f: g(f) - (f - mu) ** 2 / (2 * v)
    hc = h(c)
    return hc + mp.log(mp.quad(lambda f: mp.exp(h(f) - hc), pts)) - mp.log(2 * mp.pi * v) / 2


def _mp_site(family, y, t, mu, v):
    """dict of ytilde, tau, log_z, alpha, beta at 50 digits from the definitions: alpha = E g', beta = -E g'' - Var g' under the tilted
    density (the derivatives of log Z in mu, by differentiating under the integral)."""
    g, g1, g2 = _mp_g(family, y, t)
    if v == 0.0:
        m = mp.mpf(mu)
        return dict(ytilde=m + g1(m) / -g2(m), tau=-g2(m), log_z=g(m), alpha=g1(m), beta=-g2(m))
    c, pts = _mp_points(family, y, t, mu, v)
    mu_, v_ = mp.mpf(mu), mp.mpf(v)
    h = lambda f: g(f) - (f - mu_) ** 2 / (2 * v_)
    hc = h(c)
    w = lambda f: mp.exp(h(f) - hc)
    Z = mp.quad(w, pts)
    a = mp.quad(lambda f: w(f) * g1(f), pts) / Z
    q = mp.quad(lambda f: w(f) * (g1(f) - a) ** 2, pts) / Z
    e2 = mp.quad(lambda f: w(f) * g2(f), pts) / Z
    beta = -e2 - q
    return dict(ytilde=mu_ + a / beta, tau=beta / (1 - v_ * beta), log_z=hc + mp.log(Z) - mp.log(2 * mp.pi * v_) / 2, alpha=a, beta=beta)


_pinned = {}


def mp_sites(family, seed, n=NCASE):
    """The 50-digit sites of the box cases, rounded to fp64 and shaped like count_reference.sites; computed once."""
    key = (family, seed, n)
    if key not in _pinned:
        mp.mp.dps = 50
        y, t, mu, v = cref.box_cases(family, n, seed)
        rows = [_mp_site(family, *(float(a) for a in row)) for row in zip(y, t, mu, v)]
        r = {k: np.array([float(row[k]) for row in rows]) for k in ("ytilde", "tau", "log_z", "alpha", "beta")}
        r["omega"], r["skipped"] = r["tau"].copy(), np.zeros(n, dtype=bool)
        _pinned[key] = (y, t, mu, v, r)
    return _pinned[key]


@pytest.mark.parametrize("name,family,seed", FAMILIES)
def test_reference_sites_match_a_50_digit_quadrature_on_the_box(name, family, seed):
    y, t, mu, v, want = mp_sites(family, seed)
    got = cref.sites(y, t, family, mu, v, 1.0)
    assert not got["skipped"].any() and int((v == 0).sum()) >= 3 and int((y == 0).sum()) >= NCASE // 3 and y.max() > (1000 if family == cref.POISSON else 150)
    dev = cref.deviation(got, want, mu, v)
    print(f"{name} reference against 50 digits: " + "  ".join(f"{k} {e:.2e}" for k, e in dev.items()) + f"  (bound {REF_BOUND:.0e})")
    assert max(dev.values()) <= REF_BOUND, dev


@pytest.mark.parametrize("name,family,seed", FAMILIES)
def test_the_kernels_rule_restated_in_numpy_keeps_1e_6_on_the_box(name, family, seed):
    y, t, mu, v, want = mp_sites(family, seed)
    got = cref.rule_sites(y, t, family, mu, v, 1.0)
    dev = cref.deviation(got, want, mu, v)
    print(f"{name} rule (64 + 64 Gauss-Legendre nodes) against 50 digits: " + "  ".join(f"{k} {e:.2e}" for k, e in dev.items()) + f"  (bound {RULE_BOUND:.0e})")
    assert not got["skipped"].any() and max(dev.values()) <= RULE_BOUND, dev


@pytest.mark.parametrize("name,family,seed", FAMILIES)
def test_alpha_and_beta_are_the_derivatives_of_log_z(name, family, seed):
    """Central differences of the 50-digit log Z with step 1e-12 sqrt v (truncation ~1e-24): the reference's alpha and beta keep 1e-8
    of max(|alpha|, 1 / sqrt v) and of 1 / v, beta's natural scale (v beta < 1)."""
    mp.mp.dps = 50
    y, t, mu, v = (a[:18] for a in cref.box_cases(family, NCASE, seed + 10))
    r = cref.sites(y, t, family, mu, v, 1.0)
    for i in np.nonzero(v > 0)[0]:
        c, pts = _mp_points(family, float(y[i]), float(t[i]), float(mu[i]), float(v[i]))
        s = mp.sqrt(mp.mpf(float(v[i])))
        h = s * mp.mpf("1e-12")
        f0, fp, fm = (_mp_logz(family, float(y[i]), float(t[i]), mp.mpf(float(mu[i])) + d, float(v[i]), pts, c) for d in (0, h, -h))
        alpha, beta = (fp - fm) / (2 * h), -(fp - 2 * f0 + fm) / (h * h)
        assert abs(float(mp.mpf(r["alpha"][i]) - alpha)) <= 1e-8 * max(abs(float(alpha)), float(1 / s)), (name, i)
        assert abs(float(mp.mpf(r["beta"][i]) - beta)) <= 1e-8 * float(1 / s ** 2), (name, i)
        assert 0.0 < r["beta"][i] < float(1 / s ** 2)


def test_v_zero_is_the_laplace_site_at_the_mean():
    r = cref.sites([3.0, 0.0], [2.0, 0.5], cref.POISSON, [0.4, -1.0], 0.0, 1.0)
    lam = np.array([2.0 * np.exp(0.4), 0.5 * np.exp(-1.0)])
    assert np.allclose(r["tau"], lam, rtol=1e-15) and np.allclose(r["ytilde"], np.array([0.4, -1.0]) + (np.array([3.0, 0.0]) - lam) / lam, rtol=1e-15)
    r = cref.sites([3.0], [10.0], cref.BINOMIAL, [0.0], [-0.5], 1.0)       # (a negative variance is zero)
    assert np.allclose(r["tau"], 2.5) and np.allclose(r["ytilde"], (3.0 - 5.0) / 2.5) and np.allclose(r["log_z"], np.log(120.0) - 10 * np.log(2.0))


def test_the_skip_rule():
    nan = float("nan")
    y = np.array([-1.0, 1.0, 1.0, nan, 1.0, 5.0])
    t = np.array([1.0, 0.0, -2.0, 1.0, nan, 4.0])
    for fam in (cref.POISSON, cref.BINOMIAL):
        r = cref.sites(y, t, fam, 0.3, 0.8, 1.0)
        bad = np.ones(6, dtype=bool) if fam == cref.BINOMIAL else np.arange(6) < 5
        assert np.array_equal(r["skipped"], bad) and (r["ytilde"][bad] == 0.3).all() and np.isnan(r["log_z"][bad]).all()
        for rule in (cref.rule_sites(y, t, fam, 0.3, 0.8, 1.0),):
            assert np.array_equal(rule["skipped"], bad)
    # a weak site is skipped by the threshold on omega = sigma2 noise tau, not on tau: y = 0 at a tiny rate
    r = cref.sites(0.0, 1e-2, cref.POISSON, -3.0, 1.0, [1.0, 1e-9])
    assert list(r["skipped"]) == [False, True] and 1e-4 < r["omega"][0] < 1e-3 and np.isfinite(r["log_z"]).all()


def _problem(n0=30, q=24, seed=9):
    rng = np.random.default_rng(seed)
    n = n0 + q
    X = rng.uniform(-1.05, 1.05, (n, 2))
    noise = rng.uniform(0.3, 2.5, n)
    y = np.sin(2.5 * X.sum(1)) + 0.3 * rng.standard_normal(n)
    return X, y, noise, rng.uniform(-1.0, 1.0, (9, 2)), n0


@pytest.mark.parametrize("name,family,seed", FAMILIES)
def test_count_absorbed_statistics_are_the_gp_of_the_pseudo_observations(name, family, seed):
    X, y, noise, Xs, n0 = _problem()
    n = X.shape[0]
    g0, h, g = spec.make_grid(GB, G)
    O = dataspace.DataSpaceGP(GB, G, "rbf", ELL, OSC, S2)
    W, Ws, Kuu = ref.dense_w(g0, h, g, X), ref.dense_w(g0, h, g, Xs), ref.kuu_dense(O.cols)
    grid = cref.Grid(g0, h, g)
    A, b, c, ld = _stats(W[:n0], y[:n0], noise[:n0])
    Kt = Kuu / S2
    u = Kt @ np.linalg.solve(np.eye(36) + A @ Kt, b)
    sl = slice(n0, n)
    q = n - n0
    mean0, var0 = O.fit(X[:n0], y[:n0], noise[:n0]).predict(X[sl])
    rng = np.random.default_rng(seed)
    t = np.exp(rng.uniform(-1.0, 2.0, q)) if family == cref.POISSON else rng.integers(1, 30, q).astype(np.float64)
    cnt = rng.poisson(t * np.exp(y[sl])).astype(np.float64) if family == cref.POISSON else rng.binomial(t.astype(np.int64), cref._sigmoid(y[sl])).astype(np.float64)
    cnt[0], cnt[1], t[2], cnt[3] = 0.0, -1.0, 0.0, np.nan                 # a zero count enters; three invalid inputs do not
    one = np.ones(q)
    r = cref.dense_absorb(grid, X[sl], cnt, t, family, one, one, one, var0, S2, u)
    om, yt = r["omega"], r["ytilde"]
    assert list(np.nonzero(r["skipped"])[0]) == [1, 2, 3] and r["err"] == 0 and om[0] > 0
    ent = ~r["skipped"]
    assert _close(r["mean_out"], mean0)                                 # w . u IS the predictive mean
    keep = np.concatenate([np.ones(n0, dtype=bool), ent])
    nk = int(keep.sum())
    mean, cov, mll = _from_stats(Kuu, A + r["A"], b + r["b"], c + r["stats"][0], ld + r["stats"][1], nk, Ws)
    O.fit(X[keep], np.concatenate([y[:n0], yt[ent]]), np.concatenate([noise[:n0], 1.0 / om[ent]]))      # noise / omega at noise = 1
    assert _close(S2 / om[ent], 1.0 / cref.sites(cnt, t, family, mean0, var0, 1.0)["tau"][ent])          # ... is the variance 1 / tau
    mo, co = O.predict(Xs, full_cov=True)
    assert _close(mean, mo) and _close(cov, co) and _close(mll, O.mll())
    # and it is NOT the GP fed log(y + 1/2) (the check above can tell the two apart)
    O.fit(X[keep], np.concatenate([y[:n0], np.log(np.where(ent, cnt, 0.0) + 0.5)[ent]]), np.concatenate([noise[:n0], 1.0 / om[ent]]))
    assert not _close(mean, O.predict(Xs)[0], 1e-2)
    Z = np.linalg.solve(Kt, u)
    R = b - Z - A @ u
    assert _close(R + r["res"], (b + r["b"]) - Z - (A + r["A"]) @ u, 1e-12)
    assert _close(r["cnt"], r["A"].sum(1), 1e-12)


def test_a_point_outside_the_grid_is_dropped_and_counted():
    g0, h, g = spec.make_grid(GB, G)
    grid = cref.Grid(g0, h, g)
    X = np.array([[0.1, 0.2], [5.0, 0.0], [-0.3, 0.4]])
    r = cref.dense_absorb(grid, X, [1.0, 2.0, 0.0], np.ones(3), cref.POISSON, np.ones(3), np.ones(3), np.ones(3), np.full(3, 0.2), 0.5, np.linspace(-1, 1, 36))
    assert r["err"] == 3 and r["omega"][1] == 0.0 and r["ytilde"][1] == 0.0 and r["log_z"][1] == 0.0 and not r["skipped"][1]
    assert r["omega"][0] > 0 and r["omega"][2] > 0


def test_kernel_is_declared_and_listed_for_the_build():
    from online_gp_amd import _hip, grid_ops

    hdr = open(os.path.join(ROOT, "include", "wiski.h")).read()
    for name in ("wiski_absorb_count", "wiski_count_sites"):
        assert name + "_f32" in hdr and name + "_f64" in hdr
    assert "scatter_count.h" in _hip._HEADERS and os.path.exists(os.path.join(ROOT, "online_gp_amd", "csrc", "scatter_count.h"))
    assert '#include "scatter_count.h"' in open(os.path.join(ROOT, "online_gp_amd", "csrc", "scatter_stats.hip")).read()
    assert callable(grid_ops.scatter_stats_count) and callable(grid_ops.count_sites)
    # the Gauss-Legendre table of the kernel is the positive half of the 64-point rule
    src = open(os.path.join(ROOT, "online_gp_amd", "csrc", "scatter_count.h")).read()
    for x in list(cref.GL_X[:3]) + list(cref.GL_W[-3:]):
        assert f"{x:.17g}" in src
    # the public argument record has not grown: callers built against the previous header keep working
    assert ctypes.sizeof(_hip.wiski_absorb_args) == 224
