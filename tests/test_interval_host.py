"""No GPU: the site of an interval observation and the identity behind its absorb, in numpy fp64.

The sites of tests/interval_reference.py are pinned to a 50-digit mpmath evaluation of the same definitions on the tested domain --
bounds within 8 standard deviations of the predictive mean, two-sided widths 0.05 s .. 4 s, 400 random cases per kind -- at 1e-10
relative on ytilde and omega and 1e-12 on log Z; alpha and beta are the first and (minus the) second derivative of log Z in the
mean, checked against central differences formed at 50 digits.  A batch absorbed with those sites -- A and b, c = y^T D^-1 y and
log|D| as the kernel is specified to build them -- gives the posterior mean, the posterior covariance and the marginal likelihood of
the data-space GP (oracle/dataspace.py, which never forms a statistic) fitted at (ytilde_i, noise_i / omega_i) with the skipped
points left out.  Independent of the kernel and of the model."""
import ctypes
import os

import mpmath as mp
import numpy as np

import interval_reference as iref
import sample_paths_reference as ref
from oracle import dataspace, spec
from test_forgetting_host import ELL, G, GB, OSC, S2, _close, _from_stats, _stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NCASE = 400


def _cases(kind, seed):
    """(lo, hi, mu, v, dn) [NCASE] each: bounds within +-8 s of mu; two-sided widths 0.05 s .. 4 s (log-uniform)."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-3.0, 3.0, NCASE)
    v = rng.uniform(0.0, 2.0, NCASE)
    dn = rng.uniform(0.02, 1.5, NCASE)
    s = np.sqrt(v + dn)
    if kind == "lower":
        return mu + s * rng.uniform(-8.0, 8.0, NCASE), np.full(NCASE, INF), mu, v, dn
    if kind == "upper":
        return np.full(NCASE, -INF), mu + s * rng.uniform(-8.0, 8.0, NCASE), mu, v, dn
    width = np.exp(rng.uniform(np.log(0.05), np.log(4.0), NCASE))
    a = rng.uniform(-8.0, 8.0 - width)
    return mu + s * a, mu + s * (a + width), mu, v, dn


def _mp_logz(lo, hi, mu, s):
    a = mp.mpf("-inf") if lo == -INF else (mp.mpf(lo) - mu) / s
    b = mp.mpf("inf") if hi == INF else (mp.mpf(hi) - mu) / s
    return mp.log(mp.ncdf(b) - mp.ncdf(a))


def _mp_site(lo, hi, mu, v, dn):
    """(ytilde, omega, log Z, alpha, beta) at 50 digits from the definitions."""
    mu, v, dn = mp.mpf(mu), mp.mpf(v), mp.mpf(dn)
    s = mp.sqrt(v + dn)
    a = mp.mpf("-inf") if lo == -INF else (mp.mpf(lo) - mu) / s
    b = mp.mpf("inf") if hi == INF else (mp.mpf(hi) - mu) / s
    Z = mp.ncdf(b) - mp.ncdf(a)
    pa, pb = mp.npdf(a), mp.npdf(b)
    apa = 0 if lo == -INF else a * pa
    bpb = 0 if hi == INF else b * pb
    alpha = (pa - pb) / (s * Z)
    beta = alpha ** 2 + (bpb - apa) / (s * s * Z)
    return mu + alpha / beta, dn * beta / (1 - v * beta), mp.log(Z), alpha, beta


def test_sites_match_a_50_digit_evaluation():
    mp.mp.dps = 50
    for kind, seed in (("lower", 1), ("upper", 2), ("two-sided", 3)):
        lo, hi, mu, v, dn = _cases(kind, seed)
        r = iref.sites(lo, hi, mu, v, dn)
        worst = dict(ytilde=0.0, omega=0.0, log_z=0.0)
        nskip = 0
        for i in range(NCASE):
            yt, om, lz, _, _ = _mp_site(lo[i], hi[i], mu[i], v[i], dn[i])
            assert abs(float(mp.mpf(r["log_z"][i]) - lz)) <= 1e-12 * abs(float(lz)), (kind, i)
            worst["log_z"] = max(worst["log_z"], abs(float((mp.mpf(r["log_z"][i]) - lz) / lz)))
            if om < iref.OMEGA_MIN * 1e4:                              # at or near the skip threshold: which side is a matter of rounding
                assert r["omega"][i] < iref.OMEGA_MIN * 1e5
                nskip += 1
                continue
            assert not r["skipped"][i] and 0.0 < r["omega"][i] <= 1.0
            for key, want in (("ytilde", yt), ("omega", om)):
                e = abs(float((mp.mpf(r[key][i]) - want) / want))
                worst[key] = max(worst[key], e)
                assert e <= 1e-10, (kind, i, key, e)
        print(f"{kind}: worst relative deviation ytilde {worst['ytilde']:.2e}  omega {worst['omega']:.2e}  log Z {worst['log_z']:.2e}  "
              f"({nskip} of {NCASE} at the skip threshold)")
        assert nskip <= NCASE // 4


def test_alpha_and_beta_are_the_derivatives_of_log_z():
    """Central differences of the 50-digit log Z with step 1e-12 s: truncation ~1e-24, so the bound is that of the sites, 1e-9 of the
    natural scales 1 / s and 1 / s^2 (alpha of a centred interval is zero)."""
    mp.mp.dps = 50
    for kind, seed in (("lower", 4), ("upper", 5), ("two-sided", 6)):
        lo, hi, mu, v, dn = (t[:60] for t in _cases(kind, seed))
        r = iref.sites(lo, hi, mu, v, dn)
        for i in range(60):
            s = mp.sqrt(mp.mpf(v[i]) + mp.mpf(dn[i]))
            h = s * mp.mpf("1e-12")
            f0, fp, fm = (_mp_logz(lo[i], hi[i], mp.mpf(mu[i]) + t, s) for t in (0, h, -h))
            alpha, beta = (fp - fm) / (2 * h), -(fp - 2 * f0 + fm) / (h * h)
            assert abs(float(mp.mpf(r["alpha"][i]) - alpha)) <= 1e-9 * max(abs(float(alpha)), float(1 / s)), (kind, i)
            assert abs(float(mp.mpf(r["beta"][i]) - beta)) <= 1e-9 * float(1 / s ** 2), (kind, i)
            assert 0.0 < r["beta"][i] <= float(1 / s ** 2) * (1 + 1e-12)


def test_an_exact_value_is_itself_at_weight_one():
    lo = np.array([-2.5, 0.0, 0.3, 7.0])
    r = iref.sites(lo, lo, [0.1, 0.2, 0.3, -0.4], [0.5, 0.0, 1.0, 2.0], [0.3, 0.1, 1.0, 0.05])
    assert (r["omega"] == 1.0).all() and (r["ytilde"] == lo).all() and not r["skipped"].any()
    s = np.sqrt(np.array([0.8, 0.1, 2.0, 2.05]))
    z = (lo - np.array([0.1, 0.2, 0.3, -0.4])) / s
    assert np.allclose(r["log_z"], -0.5 * z * z - np.log(s) - 0.5 * np.log(2 * np.pi), rtol=1e-15, atol=0)


def test_the_skip_rule():
    mu, v, dn = 0.4, 0.7, 0.3                                          # s = 1
    lo = np.array([-INF, mu - 12.0, 1.0, np.nan, 0.0, -INF, INF])
    hi = np.array([INF, INF, 0.5, 1.0, np.nan, mu + 12.0, INF])
    r = iref.sites(lo, hi, mu, v, dn)
    assert r["skipped"].all() and (r["omega"] == 0.0).all() and (r["ytilde"] == mu).all()
    assert r["log_z"][0] == 0.0 and abs(r["log_z"][1]) < 1e-30 and r["log_z"][2] == -INF and np.isnan(r["log_z"][3:5]).all()
    assert abs(r["log_z"][5]) < 1e-30 and r["log_z"][6] == -INF
    # a bound satisfied by 6 s is informative still (omega ~ 1e-8), and a violated one always is
    r = iref.sites([mu - 6.0, mu + 8.0], [INF, INF], mu, v, dn)
    assert not r["skipped"].any() and 1e-9 < r["omega"][0] < 1e-7 and 0.2 < r["omega"][1] <= 1.0


def _problem(n0=30, q=24, seed=9):
    rng = np.random.default_rng(seed)
    n = n0 + q
    X = rng.uniform(-1.05, 1.05, (n, 2))
    noise = rng.uniform(0.3, 2.5, n)
    y = np.sin(2.5 * X.sum(1)) + 0.3 * rng.standard_normal(n)
    return X, y, noise, rng.uniform(-1.0, 1.0, (9, 2)), n0


def test_interval_absorbed_statistics_are_the_gp_of_the_pseudo_observations():
    X, y, noise, Xs, n0 = _problem()
    n = X.shape[0]
    g0, h, g = spec.make_grid(GB, G)
    O = dataspace.DataSpaceGP(GB, G, "rbf", ELL, OSC, S2)
    W, Ws, Kuu = ref.dense_w(g0, h, g, X), ref.dense_w(g0, h, g, Xs), ref.kuu_dense(O.cols)
    grid = iref.Grid(g0, h, g)
    # the posterior before the batch, from the statistics of the first n0 points
    A, b, c, ld = _stats(W[:n0], y[:n0], noise[:n0])
    Kt = Kuu / S2
    u = Kt @ np.linalg.solve(np.eye(36) + A @ Kt, b)
    sl = slice(n0, n)
    mean0, var0 = O.fit(X[:n0], y[:n0], noise[:n0]).predict(X[sl])
    # the batch: censored above 0.3, binned to width 0.5, two exact values, and four points that say nothing
    yb = y[sl]
    lo, hi = np.floor(yb / 0.5) * 0.5, np.floor(yb / 0.5) * 0.5 + 0.5
    cens = yb > 0.3
    lo[cens], hi[cens] = 0.3, INF
    lo[:2] = hi[:2] = yb[:2]
    lo[2], hi[2] = -INF, INF
    lo[3], hi[3] = -INF, mean0[3] + 12.0 * np.sqrt(var0[3] + S2 * noise[n0 + 3])
    lo[4], hi[4] = 1.0, 0.0
    lo[5] = np.nan
    r = iref.dense_absorb(grid, X[sl], lo, hi, 1.0 / noise[sl], 1.0 / noise[sl], noise[sl], var0, S2, u)
    om, yt = r["omega"], r["ytilde"]
    assert list(np.nonzero(r["skipped"])[0]) == [2, 3, 4, 5] and r["err"] == 0 and (om[:2] == 1.0).all() and (yt[:2] == yb[:2]).all()
    ent = ~r["skipped"]
    assert ((om[ent] > 0) & (om[ent] <= 1)).all() and int(cens[6:].sum()) >= 3 and int((~cens[6:]).sum()) >= 3
    assert _close(r["mean_out"], mean0)                                 # w . u IS the predictive mean
    keep = np.concatenate([np.ones(n0, dtype=bool), ent])
    nk = int(keep.sum())
    mean, cov, mll = _from_stats(Kuu, A + r["A"], b + r["b"], c + r["stats"][0], ld + r["stats"][1], nk, Ws)
    O.fit(X[keep], np.concatenate([y[:n0], yt[ent]]), np.concatenate([noise[:n0], noise[sl][ent] / om[ent]]))
    mo, co = O.predict(Xs, full_cov=True)
    assert _close(mean, mo) and _close(cov, co) and _close(mll, O.mll())
    # and it is NOT the GP fed the interval's finite end as a value (the check above can tell the two apart)
    O.fit(X[keep], np.concatenate([y[:n0], np.where(np.isfinite(lo), lo, hi)[ent]]), np.concatenate([noise[:n0], noise[sl][ent]]))
    assert not _close(mean, O.predict(Xs)[0], 1e-2)
    # the carried residual: R = b - Z - A U stays exact under the increment the sites define
    Z = np.linalg.solve(Kt, u)
    R = b - Z - A @ u
    assert _close(R + r["res"], (b + r["b"]) - Z - (A + r["A"]) @ u, 1e-12)
    # cnt is the row sums of the increment (rows of W sum to one)
    assert _close(r["cnt"], r["A"].sum(1), 1e-12)


def test_a_point_outside_the_grid_is_dropped_and_counted():
    g0, h, g = spec.make_grid(GB, G)
    grid = iref.Grid(g0, h, g)
    X = np.array([[0.1, 0.2], [5.0, 0.0], [-0.3, 0.4]])
    r = iref.dense_absorb(grid, X, [0.0, 0.0, 0.5], [INF, INF, 0.5], np.ones(3), np.ones(3), np.ones(3), np.full(3, 0.2), 0.5, np.linspace(-1, 1, 36))
    assert r["err"] == 3 and r["omega"][1] == 0.0 and r["ytilde"][1] == 0.0 and r["log_z"][1] == 0.0 and not r["skipped"][1]
    assert r["omega"][2] == 1.0 and 0 < r["omega"][0] < 1


def test_kernel_is_declared_and_listed_for_the_build():
    from online_gp_amd import _hip, grid_ops

    hdr = open(os.path.join(ROOT, "include", "wiski.h")).read()
    for name in ("wiski_absorb_interval_f32", "wiski_absorb_interval_f64"):
        assert name in hdr
    assert "scatter_interval.h" in _hip._HEADERS and os.path.exists(os.path.join(ROOT, "online_gp_amd", "csrc", "scatter_interval.h"))
    assert '#include "scatter_interval.h"' in open(os.path.join(ROOT, "online_gp_amd", "csrc", "scatter_stats.hip")).read()
    assert callable(grid_ops.scatter_stats_interval)
    # the public argument record has not grown: callers built against the previous header keep working
    assert ctypes.sizeof(_hip.wiski_absorb_args) == 224
