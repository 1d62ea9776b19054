"""No GPU: the fp64 reference of the categorical-observation absorb (tests/label_reference.py) -- pinned to 50-digit
mpmath, held to the closed form of two classes, to sum_k P_k = 1, to central differences of log Z and to v beta < 1; the kernel's rule,
restated in numpy, held to the reference on the evaluator's box; the stored results of the box sweeps held to the code; and the margin of
the reference stream of tests/test_label_gpu.py over a model that learned nothing."""
import functools
import math

import mpmath as mp
import numpy as np
import pytest
from scipy import special as sp

import label_reference as lref

PIN = 1e-9


def _cases(n, seed, cmax=6):
    """n random cases: C in 2 .. cmax, mu ~ N(0, 2^2), v in [0, 4], s in [0.05, 2], a uniform label"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        C = int(rng.integers(2, cmax + 1))
        out.append((int(rng.integers(0, C)), 2.0 * rng.standard_normal(C), rng.uniform(0.0, 4.0, C), rng.uniform(0.05, 2.0, C)))
    return out


def test_reference_is_pinned_to_mpmath():
    """log Z, alpha and beta of every class on a dozen cases against 50-digit quadrature of the defining integrals (mpmath's own ncdf
    and npdf, split at the label's mean), to 1e-9 -- relative for log Z and beta, absolute over max(1, |alpha|) for alpha."""
    mp.mp.dps = 50
    worst = dict(log_z=0.0, alpha=0.0, beta=0.0)
    for y, mu, v, s in _cases(12, 7, cmax=4):
        C = len(mu)
        a = [mp.mpf(float(v[c])) + mp.mpf(float(s[c])) for c in range(C)]
        m = [mp.mpf(float(x)) for x in mu]
        # (tanh-sinh visits the same nodes for every integrand on the same intervals: the factors are evaluated once per node)
        z = lambda c, t: (t - m[c]) / mp.sqrt(a[c])
        cdf, pdf = functools.lru_cache(None)(lambda c, t: mp.ncdf(z(c, t))), functools.lru_cache(None)(lambda c, t: mp.npdf(z(c, t)))
        dens = functools.lru_cache(None)(lambda t: mp.npdf(t, m[y], mp.sqrt(a[y])) * mp.fprod(cdf(c, t) for c in range(C) if c != y))
        r = lambda c, t: pdf(c, t) / cdf(c, t)
        span = 14 * mp.sqrt(max(a))
        pts = [min(m) - span, m[y], max(m) + span]
        Z = mp.quad(dens, pts)
        E = lambda f: mp.quad(lambda t: f(t) * dens(t), pts) / Z
        st = lref._site_ref(float(y), mu, v, s)
        worst["log_z"] = max(worst["log_z"], abs(float(mp.log(Z)) - st["log_z"]) / abs(float(mp.log(Z))))
        for c in range(C):
            if c == y:
                Et = E(lambda t: t)
                al, be = (Et - m[y]) / a[y], 1 / a[y] - (E(lambda t: t * t) - Et * Et) / a[y] ** 2
            else:
                Er = E(lambda t: r(c, t))                          # (E[r (r + z)] - Var r = E[z r] + (E r)^2: one integral less, and 50 digits do not mind the cancellation)
                al = -Er / mp.sqrt(a[c])
                be = (E(lambda t: z(c, t) * r(c, t)) + Er * Er) / a[c]
            worst["alpha"] = max(worst["alpha"], abs(float(al) - st["alpha"][c]) / max(1.0, abs(float(al))))
            worst["beta"] = max(worst["beta"], abs(float(be) - st["beta"][c]) / abs(float(be)))
    print("reference against mpmath: " + "  ".join(f"{k} {e:.3e}" for k, e in worst.items()))
    assert max(worst.values()) <= PIN


def test_two_classes_have_a_closed_form_and_probabilities_sum_to_one():
    rng = np.random.default_rng(3)
    n = 40
    mu, v, s = 2.0 * rng.standard_normal((2, n)), rng.uniform(0.0, 4.0, (2, n)), rng.uniform(0.05, 2.0, (2, n))
    lab = rng.integers(0, 2, n).astype(np.float64)
    st = lref.sites(lab, mu, v, s)
    y, i = lab.astype(int), np.arange(n)
    closed = sp.log_ndtr((mu[y, i] - mu[1 - y, i]) / np.sqrt((v + s).sum(0)))
    e_c = np.abs(st["log_z"] - closed).max()
    worst = 0.0
    for C in (2, 3, 6):
        mu, v, s = 2.0 * rng.standard_normal((C, 10)), rng.uniform(0.0, 4.0, (C, 10)), rng.uniform(0.05, 2.0, (C, 10))
        worst = max(worst, np.abs(lref.proba(mu, v, s).sum(1) - 1.0).max())
    print(f"C = 2 closed form {e_c:.3e}   |sum_k P_k - 1| {worst:.3e}")
    assert e_c <= 1e-12 and worst <= 1e-12
    # two classes: the sites mirror each other
    assert np.abs(st["alpha"][0] + st["alpha"][1]).max() <= 1e-12 and np.abs(st["beta"][0] - st["beta"][1]).max() <= 1e-12 * st["beta"].max()


def test_alpha_and_beta_are_the_derivatives_of_log_z():
    """Central differences of log Z in every class mean, h = 1e-3: the difference error is h^2 |log Z''''| / 12 ~ 1e-7."""
    worst_a = worst_b = 0.0
    vb = 0.0
    for y, mu, v, s in _cases(12, 11):
        st = lref._site_ref(float(y), mu, v, s)
        vb = max(vb, float((v * st["beta"]).max()))
        assert (st["beta"] > 0).all() and (v * st["beta"] < 1.0).all()
        for c in range(len(mu)):
            h = 1e-3
            e = np.zeros(len(mu))
            e[c] = h
            lp, lm = lref.log_evidence(y, mu + e, v, s), lref.log_evidence(y, mu - e, v, s)
            worst_a = max(worst_a, abs((lp - lm) / (2 * h) - st["alpha"][c]))
            worst_b = max(worst_b, abs(-(lp - 2 * st["log_z"] + lm) / (h * h) - st["beta"][c]))
    print(f"central differences: alpha {worst_a:.3e}  beta {worst_b:.3e}   largest v beta {vb:.4f}")
    assert worst_a <= 2e-6 and worst_b <= 2e-6


@pytest.mark.parametrize("C", lref.SWEEP_CLASSES)
def test_the_kernels_rule_meets_the_reference_on_the_box(C):
    """On the evaluator's box -- |mu| <= 3, v in [0, 9] with a twentieth exactly 0, s in [0.05, 4] -- the kernel's rule in numpy against
    the reference's stored results, all 400 cases, in the quantities the posterior receives: 1e-9, and who is skipped agrees away from
    the threshold.  A sample of the stored columns is recomputed by the code as it stands.  v beta < 1 throughout.

    The reference DOES skip sites on this box: with s = 0.05 and v = 0 a class 6 below the label's is 19 joint standard deviations
    away, and its omega is below 1e-12 by hundreds of orders -- the skip rule at work, not a failure (every skipped site has a
    positive, finite beta).  The box that is MEASURED stays the specified one, skips included; "nothing is skipped" holds on another
    box, the same 400 cases with the noise variance drawn from [1, 4], and is asserted there: on all 400 by the rule, on the first 40
    by the reference."""
    sample = np.arange(0, lref.NSWEEP, 50)
    lab, mu, v, s, stored, P = lref.box_sweep(C)
    _, _, _, _, fresh, Pf = lref.box_sweep(C, recompute=sample)
    # (1e-10: the stored columns were computed by another build of numpy / scipy than the one that recomputes them)
    for k in ("ytilde", "tau", "log_z", "beta"):
        a, b = stored[k][..., sample], fresh[k][..., sample]
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.allclose(np.nan_to_num(a), np.nan_to_num(b), rtol=1e-10, atol=1e-300), k
    assert np.allclose(P, Pf, rtol=1e-10, atol=0.0) and np.array_equal(stored["skipped"], fresh["skipped"])
    rule = lref.rule_sites(lab, mu, v, s, unit=True)
    clear = ~((stored["omega_raw"] > lref.OMEGA_MIN / 1e3) & (stored["omega_raw"] < lref.OMEGA_MIN * 1e3))
    assert np.array_equal(rule["skipped"][clear], stored["skipped"][clear])
    dev = lref.deviation(rule, dict(stored, skipped=stored["skipped"] | ~clear), mu, v)
    print(f"C = {C}: the rule against the reference: " + "  ".join(f"{k} {e:.3e}" for k, e in dev.items()) + f"   {int(stored['skipped'].sum())} sites skipped")
    assert max(dev.values()) <= 1e-9
    sk = stored["skipped"]
    assert (stored["beta"][sk] > 0).all() and np.isfinite(stored["beta"][sk]).all() and (stored["omega_raw"][sk] < lref.OMEGA_MIN).all()
    assert (v * stored["beta"] < 1.0).all()
    # the other box: the evaluator's 400 cases with s drawn from [1, 4] instead -- by the rule on all of them, by the reference on 40
    lab, mu, v, s = lref.box_cases(C, lref.NSWEEP, 50 + C, s_min=1.0)
    by_rule = lref.rule_sites(lab, mu, v, s, unit=True)
    first = slice(0, 40)
    st = lref.sites(lab[first], mu[:, first], v[:, first], s[:, first], unit=True)
    print(f"C = {C}, s in [1, 4]: smallest omega {by_rule['omega_raw'].min():.3e} (rule, 400 cases)  {st['omega_raw'].min():.3e} (reference, 40 cases)")
    assert not by_rule["skipped"].any() and not st["skipped"].any() and s.min() >= 1.0
    assert np.abs(by_rule["tau"][:, first] / st["tau"] - 1.0).max() <= 1e-9


def test_the_reference_stream_learns():
    """The margin of the reference stream of test_label_gpu.py::test_a_stream_of_labels_pays over log(1 / 3): recorded 0.5548
    (held-out mean log-probability -0.5438 against -1.0986; accuracy 0.860 with a tenth of the labels flipped)."""
    ref = lref.sector_stream()
    margin = ref["log_prob"] - math.log(1.0 / 3.0)
    print(f"held-out mean log-probability {ref['log_prob']:.4f}  log(1/3) {math.log(1 / 3):.4f}  margin {margin:.4f}  accuracy {ref['accuracy']:.3f}")
    assert margin >= 0.5 and ref["accuracy"] >= 0.85
