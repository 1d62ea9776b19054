"""No GPU: the noise site of the heteroscedastic absorb and the estimator as a dense stream, in numpy fp64.

The reference sites of tests/hetero_reference.py (a 6001-node trapezoid) are pinned to 50-digit mpmath.quad on the specified box --
mu_g in [-8, 8], v_g in {0} and [1e-4, 9], nu in {1, 4}, zeta = rho exp(-mu_g) in [1e-6, 400] -- in the quantities the posterior
receives, as the count form's are (count_reference.deviation): REF_BOUND = 1e-9, three orders below the 1e-6 the kernel is held to.
v_g = 0 is the Laplace site, rho = 0 is skipped and nothing else on the box is.  The property test runs the estimator as a dense
stream and asserts what the feature is for: predictive density close to the model that knows the noise, calibrated intervals in
the quiet and in the noisy half of the domain, no skipped site."""
import mpmath as mp
import numpy as np

import hetero_reference as href

NCASE = 60                                                             # the GPU sweep takes 400 against the pinned reference
REF_BOUND = 1e-9
BOX_SEED = 31
STREAM_SEED = 3                                                         # chosen so that the reference alone meets (a)-(c); the bands stay


def _mp_site(rho, nu, mu, v):
    """dict of ytilde, tau, log_z at 50 digits from the definitions: alpha = E l', beta = -E l'' - Var l' under the tilted density."""
    rho_, nu_, mu_, v_ = mp.mpf(rho), mp.mpf(nu), mp.mpf(mu), mp.mpf(v)
    l0 = lambda g: -nu_ * mp.log(2 * mp.pi) / 2 - (nu_ * g + rho_ * mp.exp(-g)) / 2
    l1 = lambda g: (rho_ * mp.exp(-g) - nu_) / 2
    l2 = lambda g: -rho_ * mp.exp(-g) / 2
    if v == 0.0:
        return dict(ytilde=mu_ + l1(mu_) / -l2(mu_), tau=-l2(mu_), log_z=l0(mu_))
    c = mp.mpf(href.mode(rho, nu, mu, v))
    kappa = 1 / v_ - l2(c)
    sd, far = 1 / mp.sqrt(kappa), 16 * mp.sqrt(v_)
    pts = sorted({c - far, c - min(8 * sd, far / 2), c - min(3 * sd, far / 4), c, c + min(3 * sd, far / 4), c + min(8 * sd, far / 2), c + far})
    h = lambda g: l0(g) - (g - mu_) ** 2 / (2 * v_)
    hc = h(c)
    w = lambda g: mp.exp(h(g) - hc)
    Z = mp.quad(w, pts)
    a = mp.quad(lambda g: w(g) * l1(g), pts) / Z
    q = mp.quad(lambda g: w(g) * (l1(g) - a) ** 2, pts) / Z
    e2 = mp.quad(lambda g: w(g) * l2(g), pts) / Z
    beta = -e2 - q
    return dict(ytilde=mu_ + a / beta, tau=beta / (1 - v_ * beta), log_z=hc + mp.log(Z) - mp.log(2 * mp.pi * v_) / 2)


_pinned = {}


def mp_sites(seed=BOX_SEED, n=NCASE):
    """The 50-digit sites of the box cases, rounded to fp64 and shaped like hetero_reference.sites; computed once."""
    if (seed, n) not in _pinned:
        mp.mp.dps = 50
        rho, nu, mu, v = href.box_cases(n, seed)
        rows = [_mp_site(*(float(a) for a in row)) for row in zip(rho, nu, mu, v)]
        r = {k: np.array([float(row[k]) for row in rows]) for k in ("ytilde", "tau", "log_z")}
        r["omega"], r["skipped"] = r["tau"].copy(), np.zeros(n, dtype=bool)
        _pinned[seed, n] = (rho, nu, mu, v, r)
    return _pinned[seed, n]


def test_reference_sites_match_a_50_digit_quadrature_on_the_box():
    rho, nu, mu, v, want = mp_sites()
    got = href.sites(rho, nu, mu, v)
    zeta = rho * np.exp(-mu)
    assert int((v == 0).sum()) >= 3 and zeta.min() < 1e-5 and zeta.max() > 100 and set(nu) == {1.0, 4.0} and mu.min() < -7 and mu.max() > 7
    assert not got["skipped"].any()                                    # the reference skips nothing on the box
    dev = href.deviation(got, want, mu, v)
    print("log-variance reference against 50 digits: " + "  ".join(f"{k} {e:.2e}" for k, e in dev.items()) + f"  (bound {REF_BOUND:.0e})")
    assert max(dev.values()) <= REF_BOUND, dev


def test_v_zero_is_the_laplace_site_at_the_mean():
    rho, nu, mu = np.array([3.0, 0.5, 7.0]), np.array([1.0, 4.0, 1.0]), np.array([0.4, -1.0, 2.0])
    for v in (0.0, -0.5):                                              # (a negative variance is zero)
        r = href.sites(rho, nu, mu, v)
        tau = 0.5 * rho * np.exp(-mu)
        assert np.allclose(r["tau"], tau, rtol=1e-15) and np.allclose(r["ytilde"], mu + (tau - 0.5 * nu) / tau, rtol=1e-15)
        assert np.allclose(r["log_z"], -0.5 * nu * np.log(2 * np.pi) - 0.5 * nu * mu - tau, rtol=1e-15)


def test_the_skip_rule():
    nan = float("nan")
    r = href.sites([0.0, 0.0, -1.0, nan, 1.0, np.inf, 1.0], [1.0, 1.0, 1.0, 1.0, 0.0, 1.0, nan], [0.3, -2.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    assert r["skipped"].all() and (r["tau"] == 0).all() and np.array_equal(r["ytilde"], [0.3, -2.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    assert np.isfinite(r["log_z"][:2]).all() and np.isnan(r["log_z"][2:]).all()   # rho = 0 is a valid datum that says nothing about g
    # rho = 0 under v > 0: log Z = -mu / 2 + v / 8 - log(2 pi) / 2 exactly, the Gaussian integral
    assert abs(r["log_z"][1] - (1.0 + 0.25 - 0.5 * np.log(2 * np.pi))) < 1e-12


def test_the_point_rule_and_the_deflated_residual():
    """e, omega_f, log Z_y and rho from their definitions; the deflation is what keeps rho's likelihood that of a residual of variance
    sigma2 noise e^g alone; a NaN target enters nothing."""
    y, mu_f, v_f, wug, v_g, noise, s2, g0 = np.array([1.0, 0.2, np.nan]), np.array([0.5, 0.2, 0.0]), np.array([0.3, 0.0, 0.1]), np.array([0.1, -0.4, 0.0]), \
        np.array([0.2, 0.0, 0.3]), np.array([1.0, 2.0, 1.0]), 0.25, 0.7
    ps = href.point_sites(y, mu_f, v_f, wug, v_g, noise, s2, g0)
    e = np.exp(g0 + wug + 0.5 * v_g)
    dn = s2 * noise * e
    assert np.allclose(ps["e"], e, rtol=1e-15) and np.allclose(ps["omega_f"][:2], 1 / e[:2], rtol=1e-15)
    assert np.isclose(ps["rho"][0], 0.25 / 0.25 * dn[0] / (dn[0] + 0.3), rtol=1e-15) and ps["rho"][1] == 0.0
    assert np.isclose(ps["log_zy"][0], -0.5 * np.log(2 * np.pi * (0.3 + dn[0])) - 0.5 * 0.25 / (0.3 + dn[0]), rtol=1e-14)
    assert list(ps["enters"]) == [True, True, False] and list(ps["skipped"]) == [False, True, False] and ps["tau"][0] > 0 and ps["tau"][2] == 0
    assert np.isnan(ps["log_zy"][2]) and np.isnan(ps["log_z"][2]) and ps["omega_f"][2] == 0


def test_the_dense_stream_learns_the_noise_field():
    """1-D grid of 40, sigma(x) = 0.05 + 0.45 x^2, f = sin 6x, 20 batches of 32 each taken against the posterior before it, 4 000 held-out
    points.  (a) the predictive density closes three quarters of the gap between the best constant noise and the true noise, (b) 90 %
    intervals cover 0.86 .. 0.94 in each half of the domain (binomial sd at 2 000 points: 0.7 %), (c) no site is skipped."""
    X, Y, _, _ = href.stream_data(STREAM_SEED)
    S = href.STREAM
    grid = href.Grid.from_bounds(S["grid_bounds"], S["grid_size"])
    het = href.DenseStream(grid, S["sigma2"], S["ell_f"], S["os_f"], S["ell_g"], S["os_g"], S["g0"])
    for xb, yb in zip(X, Y):
        het.absorb(xb, yb)
    r = href.stream_report(het.predictive, STREAM_SEED)
    Xg = np.linspace(0.05, 0.95, 19)
    _, mu_g, _ = het.posterior_g(het.rows(Xg))
    err = np.abs(0.5 * (mu_g + np.log(S["sigma2"])) - np.log(href.sigma_true(Xg)))
    print("dense stream: " + "  ".join(f"{k} {v:.4f}" for k, v in r.items()) + f"  skipped {het.skipped}  mean |log sigma error| {err.mean():.3f}")
    a, b = href.stream_conditions(r)
    assert a, r
    assert b, r
    assert het.skipped == 0
