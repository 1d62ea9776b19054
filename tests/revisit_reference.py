"""TEST INFRASTRUCTURE -- fp64 reference of the site revisit, shared by tests/test_site_revisit_host.py (no GPU) and
tests/test_site_revisit_gpu.py.

A stored point carries its location, two data numbers (d0, d1) -- (lo, hi) of an interval, (count, exposure) or (count, trials) of a
count --, a form code, noise, wa, wb and its current site (ytilde, omega); omega = 0: nothing of it is in the statistics.  With
dn = sigma2 noise, tau = omega / dn, nu = tau ytilde and (mu, v) the marginal of f at the point under the CURRENT posterior,

    cavity:  p = 1 / v - tau,   v_ = 1 / p,   mu_ = v_ (mu / v - nu)
    fresh:   (ytilde', omega', log Z') = interval_reference.sites / count_reference.sites at (mu_, v_, dn)
    damped:  tau_new = (1 - delta) tau + delta omega' / dn,   nu_new = (1 - delta) nu + delta (omega' / dn) ytilde',
             omega_new = dn tau_new,   ytilde_new = nu_new / tau_new

and the slot enters the statistics with the difference of its site.  A slot is left as it is when it is empty, of another form, outside
the grid, an exact value (lo == hi), when v is not positive and finite, when p <= CAVITY_MIN / v, or when delta = 0.  An omega_new below
OMEGA_MIN becomes exactly 0 (ytilde_new = mu).  Dense numpy, independent of the kernel and of the model; the site functions are the
references of the two forms, the half-stencil layout is ``regrid_reference.pack_half``.
"""
import numpy as np
import torch

import count_reference as cref
import interp_reference as ir
import interval_reference as iref
import regrid_reference as rr
from interval_reference import Grid, inside  # noqa: F401

CAVITY_MIN = 1e-4
OMEGA_MIN = 1e-12
EMPTY, INTERVAL, POISSON, BINOMIAL = 0, 1, 2, 3
FORM_NAMES = {INTERVAL: "interval", POISSON: "poisson", BINOMIAL: "binomial"}
RING_KEYS = ("x", "d0", "d1", "noise", "wa", "wb", "ytilde", "omega", "form")


def fresh_sites(form, d0, d1, mean, pvar, dn):
    """The form's own reference sites at the given marginals: dict with ytilde, omega, log_z [n]."""
    if form == INTERVAL:
        return iref.sites(d0, d1, mean, pvar, dn)
    return cref.sites(d0, d1, cref.POISSON if form == POISSON else cref.BINOMIAL, mean, pvar, dn)


def revisit(form, ring, mean, pvar, sigma2, damping, ok=None):
    """One parallel sweep over the slots of `form`, on the sites alone: dict of the new ytilde, omega [cap], log_z (NaN where the slot
    was left alone), change, touched (bool: re-matched), entered / left (bool) and the cavity precision relative to 1 / v (rel_p)."""
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    d0, d1, noise, yt, om, mean, pvar = (f64(a) for a in (ring["d0"], ring["d1"], ring["noise"], ring["ytilde"], ring["omega"], mean, pvar))
    cap = d0.shape[0]
    ok = np.ones(cap, dtype=bool) if ok is None else np.asarray(ok, dtype=bool)
    dn = sigma2 * noise
    tau, v = om / dn, pvar
    nu = tau * yt
    with np.errstate(divide="ignore", invalid="ignore"):
        p = 1.0 / v - tau
        rel_p = p * v
        touched = (np.asarray(ring["form"]) == form) & ok & (damping != 0.0) & (v > 0.0) & np.isfinite(v) & (p > CAVITY_MIN / v)
    if form == INTERVAL:
        touched &= ~(d0 == d1)
    yn, on, log_z = yt.copy(), om.copy(), np.full(cap, np.nan)
    idx = np.nonzero(touched)[0]
    if idx.size:
        vc = 1.0 / p[idx]
        muc = vc * (mean[idx] / v[idx] - nu[idx])
        st = fresh_sites(form, d0[idx], d1[idx], muc, vc, dn[idx])
        tf = st["omega"] / dn[idx]
        tau_new = (1.0 - damping) * tau[idx] + damping * tf
        nu_new = (1.0 - damping) * nu[idx] + damping * tf * st["ytilde"]
        o = dn[idx] * tau_new
        keep = (o >= OMEGA_MIN) & np.isfinite(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            on[idx] = np.where(keep, o, 0.0)
            yn[idx] = np.where(keep, nu_new / tau_new, mean[idx])
        log_z[idx] = st["log_z"]
    big = np.maximum(on, om)
    with np.errstate(divide="ignore", invalid="ignore"):
        change = np.where(touched & (big > 0.0), np.abs(on - om) / big, 0.0)
    return dict(ytilde=yn, omega=on, log_z=log_z, change=change, touched=touched, entered=(om == 0.0) & (on > 0.0), left=(om > 0.0) & (on == 0.0),
                rel_p=rel_p)


def dense_revisit(grid, ring, form, pvar, sigma2, u, damping):
    """What one revisit launch adds, densely: dict of A [m, m], A_half (flat), b, cnt, res [m], stats [2], ring (the new one; only
    ytilde / omega differ), log_z, change [cap] and the flags of ``revisit``.  ``ring``: dict of RING_KEYS, arrays of cap slots."""
    X = np.asarray(ring["x"], dtype=np.float64).reshape(-1, grid.d)
    W = ir.dense_rows(grid, torch.as_tensor(X)).numpy()                  # rows of a point outside the grid are zero
    u = np.asarray(u, dtype=np.float64)
    mean = W @ u
    r = revisit(form, ring, mean, pvar, sigma2, damping, ok=inside(grid, X))
    wa, wb, noise, yo, oo = (np.asarray(ring[k], dtype=np.float64) for k in ("wa", "wb", "noise", "ytilde", "omega"))
    yn, on = r["ytilde"], r["omega"]
    dwa, dwb = wa * (on - oo), wb * (on * yn - oo * yo)
    A = W.T @ (W * dwa[:, None])
    A = np.triu(A) + np.triu(A, 1).T
    with np.errstate(divide="ignore"):
        ld = np.where(on > 0.0, np.log(noise / np.where(on > 0.0, on, 1.0)), 0.0) - np.where(oo > 0.0, np.log(noise / np.where(oo > 0.0, oo, 1.0)), 0.0)
    t = r["touched"]
    new_ring = dict(ring, ytilde=yn, omega=on)
    return dict(r, A=A, A_half=rr.pack_half(torch.as_tensor(A), grid.g).numpy(), b=W.T @ dwb, cnt=W.T @ dwa, res=W.T @ (dwb - dwa * mean),
                stats=np.array([(wb * (on * yn * yn - oo * yo * yo))[t].sum(), ld[t].sum()]), ring=new_ring, mean=mean)


# ------------------------------------------------------------------------------------------------------------ the data-space driver
def _posterior(O, X, y, eff, Xq):
    """Mean and variance of f at Xq under the exact SKI GP (oracle.dataspace.DataSpaceGP) of the pseudo-data (y at noise eff); the
    prior where there is none."""
    if len(y) == 0:
        _, WK = O._WK(Xq)
        Wq, _ = O._WK(Xq)
        prior = np.ones(np.asarray(Xq).reshape(-1, O.d).shape[0])
        for i in range(O.d):
            prior *= np.einsum("ij,ij->i", WK[i], Wq[i])
        return np.zeros_like(prior), prior
    O.fit(X, y, eff)
    return O.predict(Xq)


class EPStream:
    """State of ``ep_stream``: `frozen`, the pseudo-data nothing revisits any more (the Gaussian base points and the sites of evicted
    slots) and `ring`, the stored points, oldest first (dict of arrays: x, d0, d1, noise, ytilde, omega, form)."""

    def __init__(self, O, cap):
        self.O, self.cap, self.d = O, int(cap), O.d
        self.fX, self.fy, self.feff = np.zeros((0, O.d)), np.zeros(0), np.zeros(0)
        self.ring = {k: np.zeros((0, O.d) if k == "x" else 0, dtype=np.int64 if k == "form" else np.float64) for k in RING_KEYS if k not in ("wa", "wb")}
        self.changes, self.last = [], None

    def pseudo(self):
        """(X, y, eff): everything that is in the posterior -- the frozen data and the ring's sites with omega > 0."""
        r = self.ring
        ent = r["omega"] > 0.0
        return (np.concatenate([self.fX, r["x"][ent]]), np.concatenate([self.fy, r["ytilde"][ent]]),
                np.concatenate([self.feff, r["noise"][ent] / r["omega"][ent]]))

    @property
    def num_data(self):
        return self.fy.shape[0] + int((self.ring["omega"] > 0.0).sum())

    def marginals(self, Xq):
        return _posterior(self.O, *self.pseudo(), Xq)

    def add_values(self, X, y, noise):
        self.fX, self.fy, self.feff = np.concatenate([self.fX, np.reshape(X, (-1, self.d))]), np.concatenate([self.fy, y]), np.concatenate([self.feff, noise])

    def add_batch(self, form, X, d0, d1, noise=None):
        """ADF: the batch is matched against the posterior before it, enters, and is stored (its last `cap` points; what the ring
        pushes out keeps its site, frozen)."""
        X = np.asarray(X, dtype=np.float64).reshape(-1, self.d)
        n = X.shape[0]
        noise = np.ones(n) if noise is None else np.asarray(noise, dtype=np.float64)
        mean, var = self.marginals(X)
        st = fresh_sites(form, d0, d1, mean, var, self.O.sigma2 * noise)
        new = dict(x=X, d0=np.asarray(d0, dtype=np.float64), d1=np.asarray(d1, dtype=np.float64), noise=noise, ytilde=st["ytilde"], omega=st["omega"],
                   form=np.full(n, form, dtype=np.int64))
        allp = {k: np.concatenate([self.ring[k], new[k]]) for k in new}
        out = max(0, allp["omega"].shape[0] - self.cap)
        ev = {k: v[:out] for k, v in allp.items()}
        ent = ev["omega"] > 0.0
        self.add_values(ev["x"][ent], ev["ytilde"][ent], ev["noise"][ent] / ev["omega"][ent])
        self.ring = {k: v[out:] for k, v in allp.items()}
        return st

    def sweep(self, damping=1.0):
        """One parallel EP sweep over the ring: every form against the same marginals.  Returns max(change)."""
        r = self.ring
        if r["omega"].shape[0] == 0:
            self.changes.append(0.0)
            return 0.0
        mean, var = self.marginals(r["x"])
        n = r["omega"].shape[0]
        yn, on, lz, ch = r["ytilde"].copy(), r["omega"].copy(), np.full(n, np.nan), np.zeros(n)
        for form in FORM_NAMES:
            if (r["form"] == form).any():
                o = revisit(form, r, mean, var, self.O.sigma2, damping)
                m = r["form"] == form
                yn[m], on[m], lz[m], ch[m] = o["ytilde"][m], o["omega"][m], o["log_z"][m], o["change"][m]
        self.ring = dict(r, ytilde=yn, omega=on)
        self.last = dict(ytilde=yn, omega=on, log_z=lz, change=ch, mean=mean, var=var)
        self.changes.append(float(ch.max()))
        return self.changes[-1]


def ep_stream(O, batches, cap, sweeps, damping=1.0, sweeps_per_batch=0, base=None):
    """Streams `batches` -- tuples (form, X, d0, d1[, noise]) -- through the exact SKI GP `O` in data space: each is matched against the
    posterior before it (ADF) and stored in a ring of `cap` points; `sweeps_per_batch` sweeps follow every batch and `sweeps` the last.
    `base`: (X, y, noise) of Gaussian points that enter first.  Returns the EPStream."""
    S = EPStream(O, cap)
    if base is not None:
        S.add_values(*base)
    for bt in batches:
        S.add_batch(*bt)
        for _ in range(sweeps_per_batch):
            S.sweep(damping)
    for _ in range(sweeps):
        S.sweep(damping)
    return S
