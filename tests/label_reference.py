"""TEST INFRASTRUCTURE -- fp64 reference of the categorical-observation absorb, shared by tests/test_label_host.py
(no GPU) and tests/test_label_gpu.py.

A point carries a label y in {0 .. C - 1} over C independent outputs: y = argmax_c (f_c + eps_c), eps_c ~ N(0, s_c).  Against the
posterior BEFORE the batch -- f_c ~ N(mu_c, v_c), a_c = v_c + s_c, z_c(t) = (t - mu_c) / sqrt a_c, r = phi / Phi --

    Z = int N(t; mu_y, a_y) prod_{c != y} Phi(z_c(t)) dt,          E[.] under the normalised integrand
    c = y:   alpha = (E t - mu_y) / a_y,       beta = 1 / a_y - Var t / a_y^2
    c != y:  alpha = -E r(z_c) / sqrt a_c,     beta = E[r (r + z_c)] / a_c - Var r / a_c
    tau_c = beta_c / (1 - v_c beta_c),   ytilde_c = mu_c + alpha_c / beta_c,   omega_c = s_c tau_c

A site is skipped for its output (omega = 0, ytilde = mu) when beta is not positive and finite or omega < OMEGA_MIN; an invalid label
(not an integer in [0, C), NaN) skips the point for every output (log Z = NaN).

Two evaluations live here.  ``sites`` is the reference: a composite trapezoid of 6001 nodes between the points where the log
integrand has fallen by 60 from its maximum, found by bisection -- numpy / scipy, nothing shared with the kernel but the definitions;
tests/test_label_host.py pins it to 50-digit mpmath.  ``rule_sites`` restates the KERNEL's rule (scatter_label.h) so that its accuracy
on the specified box can be asserted without a GPU.
"""
import math
import os

import numpy as np
import torch
from scipy import special as sp

import interp_reference as ir
import regrid_reference as rr
from interval_reference import Grid, inside  # noqa: F401

OMEGA_MIN = 1e-12
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)


def log_phi(z):
    """log Phi(z)"""
    return sp.log_ndtr(z)


def ratio(z):
    """r(z) = phi(z) / Phi(z), to rounding for z -> -inf"""
    z = np.asarray(z, dtype=np.float64)
    neg = math.sqrt(2.0 / math.pi) / sp.erfcx(-np.minimum(z, 0.0) / math.sqrt(2.0))
    with np.errstate(under="ignore"):
        pos = np.exp(-0.5 * np.maximum(z, 0.0) ** 2) / math.sqrt(2.0 * math.pi) / sp.ndtr(np.maximum(z, 0.0))
    return np.where(z < 0, neg, pos)


def label_class(lab, C):
    return int(lab) if (lab == lab and 0 <= lab < C and lab == math.floor(lab)) else -1


def _g(y, mu, a, t):
    """g(t) = sum_{c != y} log Phi(z_c(t)), g', g'' at the nodes t [k]"""
    t = np.asarray(t, dtype=np.float64)
    g, g1, g2 = np.zeros_like(t), np.zeros_like(t), np.zeros_like(t)
    for c in range(len(mu)):
        if c == y:
            continue
        z = (t - mu[c]) / math.sqrt(a[c])
        r = ratio(z)
        g, g1, g2 = g + log_phi(z), g1 + r / math.sqrt(a[c]), g2 - r * (r + z) / a[c]
    return g, g1, g2


def _finish(y, mu, v, s, alpha, beta, log_z, unit=False):
    """The sites of all classes with the skip rule applied; omega = s tau, or tau itself with ``unit`` (wiski_label_sites).  omega_raw
    is omega before the threshold (NaN where beta is not positive and finite)."""
    C = len(mu)
    yt, om, tau, raw = mu.copy(), np.zeros(C), np.zeros(C), np.full(C, np.nan)
    for c in range(C):
        if not (beta[c] > 0.0 and math.isfinite(beta[c])):
            continue
        t_c = beta[c] / (1.0 - v[c] * beta[c])
        o_c = t_c if unit else s[c] * t_c
        raw[c] = o_c
        if not (o_c >= OMEGA_MIN and math.isfinite(o_c)):
            continue
        yt[c], om[c], tau[c] = mu[c] + alpha[c] / beta[c], o_c, t_c
    return dict(ytilde=yt, omega=om, tau=tau, alpha=alpha, beta=beta, log_z=log_z, omega_raw=raw)


def _invalid(mu):
    C = len(mu)
    nan = np.full(C, np.nan)
    return dict(ytilde=np.array(mu, dtype=np.float64), omega=np.zeros(C), tau=np.zeros(C), alpha=nan, beta=nan.copy(), log_z=float("nan"), omega_raw=nan.copy())


# ---------------------------------------------------------------------------------------------------------------- the reference
NREF, DROP_REF = 6001, 60.0


def _nodes_ref(y, mu, a):
    """(t, w, c, hc, step): trapezoid nodes, weights exp(h - hc) (ends halved), the mode, h there and the node spacing"""
    h = lambda t: _g(y, mu, a, t)[0] - (t - mu[y]) ** 2 / (2.0 * a[y])
    dh = lambda t: float(_g(y, mu, a, t)[1]) - (t - mu[y]) / a[y]
    lo, hi = mu[y], mu[y] + a[y] * float(_g(y, mu, a, mu[y])[1])
    for _ in range(200):
        c = 0.5 * (lo + hi)
        if dh(c) > 0:
            lo = c
        else:
            hi = c
    c = 0.5 * (lo + hi)
    hc = float(h(c))

    def edge(sign):
        lo, hi = 0.0, math.sqrt(2.0 * DROP_REF * a[y]) * 1.001                # -h'' >= 1 / a_y: the drop is reached within this
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            if hc - float(h(c + sign * mid)) < DROP_REF:
                lo = mid
            else:
                hi = mid
        return c + sign * hi

    L, R = edge(-1.0), edge(1.0)
    t = np.linspace(L, R, NREF)
    w = np.exp(h(t) - hc)
    w[0] *= 0.5
    w[-1] *= 0.5
    return t, w, c, hc, (R - L) / (NREF - 1)


def log_evidence(y, mu, v, s):
    """log P(y) alone"""
    mu, v, s = (np.asarray(x, dtype=np.float64) for x in (mu, v, s))
    a = np.maximum(v, 0.0) + s
    t, w, c, hc, step = _nodes_ref(y, mu, a)
    return hc + math.log(w.sum() * step) - 0.5 * math.log(a[y]) - HALF_LOG_2PI


def _site_ref(lab, mu, v, s, unit=False):
    mu, v, s = (np.asarray(x, dtype=np.float64) for x in (mu, v, s))
    C = len(mu)
    y = label_class(lab, C)
    v = np.maximum(v, 0.0)
    a = v + s
    if y < 0 or not (np.isfinite(mu).all() and np.isfinite(a).all() and (a > 0).all()):
        return _invalid(mu)
    t, w, c, hc, step = _nodes_ref(y, mu, a)
    S0 = w.sum()
    E = lambda q: float((w * q).sum() / S0)
    log_z = hc + math.log(S0 * step) - 0.5 * math.log(a[y]) - HALF_LOG_2PI
    alpha, beta = np.zeros(C), np.zeros(C)
    for k in range(C):
        if k == y:
            _, g1, g2 = _g(y, mu, a, t)
            Eg = E(g1)
            beta_w = -E(g2) - E((g1 - Eg) ** 2)
            if a[y] * beta_w < 0.25:                                          # a weak site: 1 / a - Var t / a^2 would cancel
                alpha[k], beta[k] = Eg, beta_w
            else:
                Et = E(t - c)
                alpha[k], beta[k] = (c + Et - mu[y]) / a[y], 1.0 / a[y] - E((t - c - Et) ** 2) / a[y] ** 2
        else:
            z = (t - mu[k]) / math.sqrt(a[k])
            r = ratio(z)
            Er = E(r)
            alpha[k], beta[k] = -Er / math.sqrt(a[k]), (E(r * (r + z)) - E((r - Er) ** 2)) / a[k]
    return _finish(y, mu, v, s, alpha, beta, log_z, unit)


def _table(fn, labels, mu, v, s, unit=False):
    """mu, v, s [C, n], labels [n] -> dict of ytilde, omega, tau, alpha, beta [C, n], log_z [n], skipped [C, n]"""
    mu, v, s = (np.asarray(x, dtype=np.float64) for x in (mu, v, s))
    mu, v, s = np.broadcast_arrays(mu, v, s)
    rows = [fn(float(labels[i]), mu[:, i], v[:, i], s[:, i], unit) for i in range(mu.shape[1])]
    out = {k: np.stack([r[k] for r in rows], axis=1) for k in ("ytilde", "omega", "tau", "alpha", "beta", "omega_raw")}
    out["log_z"] = np.array([r["log_z"] for r in rows])
    out["skipped"] = out["omega"] == 0.0
    return out


def sites(labels, mu, v, s, unit=False):
    """The reference sites of labels [n] against class means mu, latent variances v and noise variances s, all [C, n]; omega = s tau,
    with ``unit`` omega = tau (the skip threshold is on omega)."""
    return _table(_site_ref, labels, mu, v, s, unit)


def proba(mu, v, s):
    """P(y = k) [n, C], every class by its own integral (NOT normalised)."""
    mu, v, s = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (mu, v, s)))
    C, n = mu.shape
    return np.array([[math.exp(log_evidence(k, mu[:, i], v[:, i], s[:, i])) for k in range(C)] for i in range(n)])


def moments(st, mu, v):
    """(mhat, Vhat) [C, n]: what the posterior of each output receives from its site."""
    mu, v = np.asarray(mu, dtype=np.float64), np.maximum(np.asarray(v, dtype=np.float64), 0.0)
    V = v / (1.0 + v * st["tau"])
    return V * st["tau"] * (st["ytilde"] - mu) + mu, V


def deviation(got, ref, mu, v):
    """The deviations of sites `got` (ytilde, tau [C, n], log_z [n]) from `ref` in what the posterior receives, as
    count_reference.deviation: m (|mhat - mhat_ref| / sqrt Vhat_ref, v > 0), V (relative, v > 0), log_z (relative), tau (relative, where
    v tau <= 1 or v = 0); the largest over the entering sites."""
    v = np.maximum(np.asarray(v, dtype=np.float64), 0.0) * np.ones_like(ref["tau"])
    ent = ~ref["skipped"]
    pos = ent & (v > 0)
    mg, Vg = moments(got, mu, v)
    mr, Vr = moments(ref, mu, v)
    weak = ent & (v * ref["tau"] <= 1.0)
    fin = np.isfinite(ref["log_z"])
    mx = lambda x: float(x.max()) if x.size else 0.0
    return dict(m=mx(np.abs(mg - mr)[pos] / np.sqrt(Vr[pos])), V=mx(np.abs(Vg - Vr)[pos] / Vr[pos]),
                log_z=mx(np.abs(got["log_z"] - ref["log_z"])[fin] / np.maximum(np.abs(ref["log_z"][fin]), 1e-3)),
                tau=mx(np.abs(got["tau"] - ref["tau"])[weak] / ref["tau"][weak]))


# ------------------------------------------------------------------------------------------------- the kernel's rule, restated
NPASS, NNEWTON, DROP, LADDER = 4, 2, 40.0, 1.3
GL_X, GL_W = (x[32:] for x in np.polynomial.legendre.leggauss(64))       # the positive half of the symmetric rule


def _rule_nodes(y, mu, a):
    """(t [2, 64], w [2, 64], side, x, c, hc, g1c): the kernel's nodes and weights exp(h - hc) times the Gauss-Legendre weights"""
    lane = np.arange(64)
    my, ay = mu[y], a[y]
    h = lambda t: _g(y, mu, a, t)[0] - (t - my) ** 2 / (2.0 * ay)
    lo, W = my, ay * float(_g(y, mu, a, my)[1])
    for _ in range(NPASS):
        x = lo + W * (lane + 1) / 64.0
        dh = _g(y, mu, a, x)[1] - (x - my) / ay
        lo, W = lo + W * int((dh > 0.0).sum()) / 64.0, W / 64.0
    c = lo + 0.5 * W
    for _ in range(NNEWTON):
        _, g1, g2 = _g(y, mu, a, c)
        c = c - (float(g1) - (c - my) / ay) / (float(g2) - 1.0 / ay)
    hc, g1c = float(h(c)), float(_g(y, mu, a, c)[1])
    side = np.where(lane < 32, -1.0, 1.0)
    k = lane & 31
    D = math.sqrt(2.0 * DROP * ay)
    ok = hc - h(c + side * D * LADDER ** (-k.astype(np.float64))) >= DROP
    e = np.empty(2)
    for i, sl in enumerate((slice(0, 32), slice(32, 64))):
        n_ok = int(ok[sl].sum())
        outer = D * LADDER ** (-float(max(n_ok - 1, 0)))
        inner = outer / LADDER if n_ok > 0 else outer
        step = inner + (outer - inner) * (k[sl] + 1) / 32.0
        short = hc - h(c + side[sl] * step) < DROP
        e[i] = inner + (outer - inner) * (min(int(short.sum()), 31) + 1) / 32.0
    half = 0.5 * np.where(lane < 32, e[0], e[1])
    x = half * np.stack([1.0 - GL_X[k], 1.0 + GL_X[k]])
    t = c + side * x
    w = half * GL_W[k] * np.exp(h(t) - hc)
    return t, w, side, x, c, hc, g1c


def _site_rule(lab, mu, v, s, unit=False):
    mu, v, s = (np.asarray(q, dtype=np.float64) for q in (mu, v, s))
    C = len(mu)
    y = label_class(lab, C)
    v = np.maximum(v, 0.0)
    a = v + s
    if y < 0 or not (np.isfinite(mu).all() and np.isfinite(a).all() and (a > 0).all()):
        return _invalid(mu)
    t, w, side, x, c, hc, g1c = _rule_nodes(y, mu, a)
    S0 = w.sum()
    E = lambda q: float((w * q).sum() / S0)
    log_z = hc + math.log(S0) - 0.5 * math.log(a[y]) - HALF_LOG_2PI
    alpha, beta = np.zeros(C), np.zeros(C)
    for k in range(C):
        if k == y:
            _, g1, g2 = _g(y, mu, a, t)
            dg = g1 - g1c
            G1, G2, H2 = E(dg), E(dg * dg), E(g2)
            beta_w = -H2 - (G2 - G1 * G1)
            if a[y] * beta_w < 0.5:
                alpha[k], beta[k] = g1c + G1, beta_w
            else:
                S1, S2 = E(side * x), E(x * x)
                alpha[k], beta[k] = (c + S1 - mu[y]) / a[y], (a[y] - (S2 - S1 * S1)) / a[y] ** 2
        else:
            ic = 1.0 / math.sqrt(a[k])
            r0 = float(ratio((c - mu[k]) * ic))
            z = (t - mu[k]) * ic
            r = ratio(z)
            dr = r - r0
            P1, P2 = E(dr), E(r * (r + z) - dr * dr)
            alpha[k], beta[k] = -(r0 + P1) * ic, (P2 + P1 * P1) * ic * ic
    return _finish(y, mu, v, s, alpha, beta, log_z, unit)


def rule_sites(labels, mu, v, s, unit=False):
    """``sites`` by the kernel's rule (scatter_label.h), lane for lane."""
    return _table(_site_rule, labels, mu, v, s, unit)


def rule_proba(mu, v, s):
    mu, v, s = np.broadcast_arrays(*(np.asarray(x, dtype=np.float64) for x in (mu, v, s)))
    C, n = mu.shape
    out = np.empty((n, C))
    for i in range(n):
        a = np.maximum(v[:, i], 0.0) + s[:, i]
        for k in range(C):
            t, w, side, x, c, hc, g1c = _rule_nodes(k, mu[:, i], a)
            out[i, k] = math.exp(hc + math.log(w.sum()) - 0.5 * math.log(a[k]) - HALF_LOG_2PI)
    return out


# --------------------------------------------------------------------------------------------------------------- the box
def box_cases(C, n, seed, s_min=0.05):
    """(labels [n], mu, v, s [C, n]) on the specified box: |mu| <= 3, v in [0, 9] with every 20th column exactly 0, s in [s_min, 4],
    all rounded to fp32 (so that both precisions are handed the same numbers); the labels in turn drawn from the model, the class of
    the largest mean, and uniform."""
    rng = np.random.default_rng(seed)
    mu = rng.uniform(-3.0, 3.0, (C, n))
    v = rng.uniform(0.0, 9.0, (C, n))
    v[:, ::20] = 0.0
    s = np.exp(rng.uniform(math.log(s_min), math.log(4.0), (C, n)))
    mu, v, s = (x.astype(np.float32).astype(np.float64) for x in (mu, v, s))
    s = np.clip(s, np.float64(np.float32(s_min)) if np.float32(s_min) >= s_min else np.nextafter(np.float32(s_min), np.float32(9)).astype(np.float64), 4.0)
    drawn = np.argmax(mu + np.sqrt(v + s) * rng.standard_normal((C, n)), axis=0)
    kind = np.arange(n) % 3
    labels = np.where(kind == 0, drawn, np.where(kind == 1, np.argmax(mu, axis=0), rng.integers(0, C, n))).astype(np.float64)
    return labels, mu, v, s


NSWEEP, SWEEP_CLASSES = 400, (2, 3, 5, 16)
_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label_box_C%d.npz")
_SWEEP_KEYS = ("ytilde", "tau", "beta", "omega_raw", "log_z")       # what the files hold; omega = tau and skipped = (tau == 0) follow


def box_sweep(C, recompute=None):
    """The evaluator sweep of C classes: box_cases(C, NSWEEP, 50 + C) with its reference sites (omega = tau) and class probabilities --
    (labels, mu, v, s, sites, P).  The reference takes minutes for the four sweeps, so its results are kept under tests/golden/
    (written by running this file with the repository root on PYTHONPATH; their ``source`` tag says "oracle" as every fixture of this
    repository's own making does: they come from ``sites`` and ``proba`` above).  The inputs are always drawn afresh and must equal
    the stored ones, and ``recompute`` (indices) are evaluated again and returned in place of the stored columns:
    tests/test_label_host.py holds the files to the code that way."""
    lab, mu, v, s = box_cases(C, NSWEEP, 50 + C)
    z = np.load(_GOLDEN % C)
    assert all(np.array_equal(z[k], q) for k, q in (("labels", lab), ("mu", mu), ("v", v), ("s", s)))
    ref, P = {k: z[k].copy() for k in _SWEEP_KEYS}, z["P"].copy()
    ref["omega"], ref["skipped"] = ref["tau"].copy(), ref["tau"] == 0.0
    if recompute is not None:
        idx = np.asarray(recompute)
        fresh = sites(lab[idx], mu[:, idx], v[:, idx], s[:, idx], unit=True)
        for k in _SWEEP_KEYS + ("omega", "skipped"):
            ref[k][..., idx] = fresh[k]
        P[idx] = proba(mu[:, idx], v[:, idx], s[:, idx])
    return lab, mu, v, s, ref, P


def _write_golden():
    """(the inputs are exact in fp32 and are stored so; box_sweep draws them afresh and compares)"""
    os.makedirs(os.path.dirname(_GOLDEN), exist_ok=True)
    for C in SWEEP_CLASSES:
        lab, mu, v, s = box_cases(C, NSWEEP, 50 + C)
        ref = sites(lab, mu, v, s, unit=True)
        np.savez_compressed(_GOLDEN % C, labels=lab.astype(np.int8), mu=mu.astype(np.float32), v=v.astype(np.float32), s=s.astype(np.float32),
                            P=proba(mu, v, s), source="oracle", **{k: ref[k] for k in _SWEEP_KEYS})
        print(f"C = {C}: {int(ref['skipped'].sum())} of {ref['skipped'].size} sites skipped", flush=True)


# ------------------------------------------------------------------------------------------------------------- the dense absorb
def dense_absorb(grid, X, labels, wa, wb, noise, pvar, sigma2, U):
    """What one label absorb launch adds, densely, per output: dict of ytilde, omega [C, n], log_z [n], skipped, mean_out [C, n],
    A [C, m, m], A_half [C, flat], b, cnt, res [C, m], stats [C, 2] and err (bit 0 | 2 x dropped points).  wa, wb, noise, pvar
    [C, n]; sigma2 [C]; U [C, m]."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, grid.d)
    W = ir.dense_rows(grid, torch.as_tensor(X)).numpy()                  # rows of a point outside the grid are zero
    wa, wb, noise, pvar, U, sigma2 = (np.asarray(q, dtype=np.float64) for q in (wa, wb, noise, pvar, U, sigma2))
    C, n = pvar.shape
    ok = inside(grid, X)
    mean = U @ W.T
    st = sites(labels, mean, pvar, sigma2[:, None] * noise)
    omega = np.where(ok[None], st["omega"], 0.0)
    yt = np.where(ok[None], st["ytilde"], 0.0)
    log_z = np.where(ok, st["log_z"], 0.0)
    out = {"ytilde": yt, "omega": omega, "log_z": log_z, "skipped": ok[None] & (omega == 0.0), "mean_out": mean,
           "err": int((~ok).any()) + 2 * int((~ok).sum())}
    A, Ah, b, cnt, res, stats = [], [], [], [], [], []
    for c in range(C):
        ent = omega[c] > 0.0
        wae, wbe = wa[c] * omega[c], wb[c] * omega[c]
        Ac = W.T @ (W * wae[:, None])
        Ac = np.triu(Ac) + np.triu(Ac, 1).T
        A.append(Ac)
        Ah.append(rr.pack_half(torch.as_tensor(Ac), grid.g).numpy())
        b.append(W.T @ (wbe * yt[c]))
        cnt.append(W.T @ wae)
        res.append(W.T @ (wbe * yt[c] - wae * mean[c]))
        stats.append([(wbe * yt[c] * yt[c])[ent].sum(), (np.log(noise[c][ent]) - np.log(omega[c][ent])).sum()])
    out.update(A=np.stack(A), A_half=np.stack(Ah), b=np.stack(b), cnt=np.stack(cnt), res=np.stack(res), stats=np.array(stats))
    return out


# --------------------------------------------------------------------------------------------------------------- the ADF stream
def adf_stream(make_oracle, sigma2, X, labels, batches, Xs, init, noise=None, site_fn=None):
    """Assumed-density filtering in data space: one exact GP per class (``make_oracle(c)`` -> an oracle.dataspace.DataSpaceGP), fitted
    at the pseudo-observations so far (ytilde_c at noise variance 1 / tau_c, i.e. noise / omega_c in the oracle's units of sigma2_c).
    Before batch k every class predicts the batch, the sites follow, and each class appends the points whose site entered.
    ``init`` = (X0 [n0, d], Y0 [C, n0], noise0 [n0]): the values every class holds before the first batch (a model is created from
    points, so there always are some).  ``site_fn``: ``sites`` (the default) or ``rule_sites``.  Returns per batch dict(sites,
    mean [C, ns], var [C, ns], n [C]: points held per class, batch_mean / batch_var [C, q]: what the sites were matched against)."""
    site_fn = site_fn or sites
    C = len(sigma2)
    O = [make_oracle(c) for c in range(C)]
    noise = np.ones(len(X)) if noise is None else np.asarray(noise, dtype=np.float64)
    held = [dict(X=np.asarray(init[0], dtype=np.float64), y=np.asarray(init[1][c], dtype=np.float64), eff=np.asarray(init[2], dtype=np.float64))
            for c in range(C)]
    steps = []

    def predict(c, Xq):
        O[c].fit(held[c]["X"], held[c]["y"], held[c]["eff"])
        return O[c].predict(Xq)

    for sl in batches:
        mv = [predict(c, X[sl]) for c in range(C)]
        mean, var = np.stack([m for m, _ in mv]), np.stack([q for _, q in mv])
        st = site_fn(labels[sl], mean, var, np.asarray(sigma2)[:, None] * noise[sl][None])
        for c in range(C):
            ent = st["omega"][c] > 0.0
            held[c] = dict(X=np.concatenate([held[c]["X"], X[sl][ent]]), y=np.concatenate([held[c]["y"], st["ytilde"][c][ent]]),
                           eff=np.concatenate([held[c]["eff"], noise[sl][ent] / st["omega"][c][ent]]))
        mo = [predict(c, Xs) for c in range(C)]
        steps.append(dict(sites=st, mean=np.stack([m for m, _ in mo]), var=np.stack([q for _, q in mo]), n=[h["y"].size for h in held],
                          batch_mean=mean, batch_var=var))
    return steps


# ------------------------------------------------------------------------------------------------------------ the sector stream
STREAM_GB, STREAM_GS, STREAM_VOID_NOISE = [[-1.0, 1.0], [-1.0, 1.0]], [12, 12], 1e6
_sector_stream = {}


def sector_data(seed=17, n=600, n_held=300, q=50, flip=0.1):
    """Three classes in 2-D, separable by sectors, with a tenth of the labels flipped: dict of X [600, 2], labels, X_held [300, 2],
    y_held, X0 (four corner points that say nothing: a model is created from points) and the batches of 50.  The data alone: cheap."""
    rng = np.random.default_rng(seed)
    C = 3
    sector = lambda X: np.floor((np.arctan2(X[:, 1], X[:, 0]) + np.pi) / (2 * np.pi / C)).clip(0, C - 1)
    X, Xh = rng.uniform(-0.95, 0.95, (n, 2)), rng.uniform(-0.95, 0.95, (n_held, 2))
    labels, yh = sector(X), sector(Xh)
    for lab in (labels, yh):
        f = rng.uniform(size=len(lab)) < flip
        lab[f] = (lab[f] + rng.integers(1, C, int(f.sum()))) % C
    X0 = np.array([[-0.9, -0.9], [-0.9, 0.9], [0.9, -0.9], [0.9, 0.9]])
    return dict(X=X, labels=labels, X_held=Xh, y_held=yh, X0=X0, batches=[slice(k, k + q) for k in range(0, n, q)])


def sector_stream(hyp=None):
    """``sector_data`` through the ADF stream on a 12 x 12 grid (rbf; ``hyp``: per class (lengthscales, outputscale, sigma2), None:
    softplus(0) throughout), both sides starting from the four corner points at zero targets and a noise of 1e6.  The sites of the
    stream are taken by ``rule_sites`` -- the kernel's rule restated in numpy -- and NOT by the independent trapezoid ``sites``: 600
    reference sites, 300 held-out ones and 900 integrals would take minutes.  What this reference adds to the kernel's own rule is
    therefore the exact GP per class and the bookkeeping of the stream; the rule itself is held to ``sites`` on the box by
    tests/test_label_host.py, and the model tests of tests/test_label_gpu.py use ``sites``.  Returns the data with the stream's
    held-out mean log-probability and accuracy; once per ``hyp``."""
    from oracle import dataspace, spec

    if hyp in _sector_stream:
        return _sector_stream[hyp]
    C = 3
    hy = hyp or ((spec.SOFTPLUS0, spec.SOFTPLUS0, spec.SOFTPLUS0),) * C
    d = sector_data()
    X0, Xh, yh = d["X0"], d["X_held"], d["y_held"]
    sigma2 = [h[2] for h in hy]
    make = lambda c: dataspace.DataSpaceGP(STREAM_GB, STREAM_GS, "rbf", *hy[c])
    steps = adf_stream(make, sigma2, d["X"], d["labels"], d["batches"], Xh, (X0, np.zeros((C, len(X0))), np.full(len(X0), STREAM_VOID_NOISE)),
                       site_fn=rule_sites)
    mean, var = steps[-1]["mean"], steps[-1]["var"]
    s = np.array(sigma2)[:, None] * np.ones((1, len(Xh)))
    lz = rule_sites(yh, mean, var, s)["log_z"]
    P = rule_proba(mean, var, s)
    out = dict(d, log_prob=float(lz.mean()), accuracy=float((P.argmax(1) == yh).mean()), steps=steps)
    _sector_stream[hyp] = out
    return out


if __name__ == "__main__":
    _write_golden()
