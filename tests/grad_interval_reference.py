"""TEST INFRASTRUCTURE -- fp64 reference of interval sites on values and partial derivatives, shared by
tests/test_grad_interval_host.py (no GPU) and tests/test_grad_interval_gpu.py.

A point carries C = d + 1 channels as in tests/grad_obs_reference.py (0: f(x), 1 + q: df/dx_q (x)); every present channel says
lo_c <= row_c . u + eps_c <= hi_c and is moment-matched as tests/interval_reference.py matches a value, against its own predictive
mean row_c . u and its own posterior variance, independently of the point's other channels.  It then enters the statistics as the
pseudo-target ytilde_c at noise noise_c / omega_c, which is ``grad_obs_reference.dense_absorb`` at those targets and weights.  Dense
numpy, independent of the kernel and of the model; nothing here is new arithmetic -- the sites are ``interval_reference.sites``, the
rows ``grad_obs_reference.stacked_rows``.

:class:`DenseStream` is the streamed model in statistics space: (A, b, c, log|D|, N) with the posterior u = (I + Kt A)^-1 Kt b,
cov u = (I + Kt A)^-1 Kuu, whose jet moments at a batch give the batch's sites -- condition, sites, absorb, batch after batch.
"""
import numpy as np
import scipy.linalg as sla

import grad_obs_reference as gr
import interval_reference as iref
from grad_obs_reference import Grid, inside  # noqa: F401

INF = float("inf")
N = 37                                                            # three blocks of 16; the last pass of the last block holds one point
KS2 = 0.7                                                         # sigma2 of the kernel cases
KGRIDS = {"d1": [8], "d2": [8, 8], "d3": [8, 8, 8], "d4": [6, 6, 6, 6]}
# what the points of a kernel case are for (the kinds of the bounds go round the channels, see kernel_case)
P_OUTSIDE, P_ABSENT, P_VALUE_ONLY, P_GRAD_ONLY = 10, 22, 23, 24


def sites(lo, hi, mean, pvar, dn, present):
    """``interval_reference.sites`` per channel, all [n, C]: dict of ytilde, omega, log_z and the bool masks skipped (present,
    omega = 0) and zero (not present: an absent channel, a point outside the grid -- the caller folds that into `present` -- which
    reports (0, 0, 0))."""
    present = np.asarray(present, dtype=bool)
    st = iref.sites(lo, hi, mean, pvar, dn)
    out = {k: np.where(present, st[k], 0.0) for k in ("ytilde", "omega", "log_z")}
    out["skipped"] = present & (out["omega"] == 0.0)
    out["zero"] = ~present
    return out


def dense_absorb(grid, X, lo, hi, wa, wb, noise, pvar, sigma2, u):
    """What one launch adds, densely.  All per-point inputs [n, C] as the kernel takes them (an absent channel: wa = wb = 0,
    noise = 1).  dict of A, A_half, b, cnt, res [m], stats [2], err, mean_out [n, C] and the sites (ytilde, omega, log_z, skipped,
    zero [n, C])."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, grid.d)
    lo, hi, wa, wb, noise, pvar, u = (np.asarray(t, dtype=np.float64) for t in (lo, hi, wa, wb, noise, pvar, u))
    mean = gr.stacked_rows(grid, X) @ u                               # rows of a point outside the grid are zero
    present = (wa != 0.0) & inside(grid, X)[:, None]
    st = sites(lo, hi, mean, pvar, sigma2 * noise, present)
    om = st["omega"]
    ent = om > 0.0
    out = gr.dense_absorb(grid, X, np.where(ent, st["ytilde"], 0.0), wa * om, wb * om, np.where(ent, noise / np.where(ent, om, 1.0), 1.0), u)
    out.update(st)
    return out


_cases = {}


def kernel_case(name):
    """Grid, 37 points (fp64 values that are exact in fp32) with [37, C] channel tensors, and the dense reference; built once.
    Points: 10 outside the grid, 22 every channel absent, 23 value only, 24 gradient only, 4 + q / 16 + q in the first / last
    (boundary) cell of dim q, 12 .. 15 in one interior cell (colliding atomics).  The kind of the bounds of channel c of point i is
    slot (i + 5 c) mod 37 of one list, so that every channel meets every kind and the channels of a point differ:
      0, 1 exact   2 (-inf, inf)   3 a lower bound satisfied by 12 s (skipped)   4 lo > hi   5 .. 36 in turn lower-only, upper-only
      (from violated by 8 s to satisfied by 6 s, evenly) and two-sided (width 0.05 s .. 4 s, anywhere within 8 s)
    placed around the reference's own predictive mean of the channel in units of s = sqrt(max(pvar, 0) + sigma2 noise).  pvar in
    [0, 2], exactly 0 in slot 7 and negative (treated as 0) in slot 8."""
    if name in _cases:
        return _cases[name]
    g = KGRIDS[name]
    d, C = len(g), len(g) + 1
    rng = np.random.default_rng(300 + d)
    grid = Grid.from_bounds([[-1.0, 1.0 + 0.25 * q] for q in range(d)], g)
    cell = np.stack([rng.integers(1, gq - 2, N) for gq in g], 1).astype(np.float64)     # interior cells
    frac = 0.5 + rng.choice([-1.0, 1.0], (N, d)) * rng.uniform(0.05, 0.45, (N, d))      # away from nodes and cell midpoints
    for q in range(d):
        cell[4 + q, q] = 0                                          # first (boundary) cell of dim q
        cell[16 + q, q] = g[q] - 2                                  # last (boundary) cell of dim q
    cell[12:16] = 1
    X = np.array(grid.g0) + np.array(grid.h) * (cell + frac)
    X[P_OUTSIDE, 0] = grid.g0[0] - 1.0
    f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
    X = f32(X)
    present = np.ones((N, C), dtype=bool)
    present[P_ABSENT] = False
    present[P_VALUE_ONLY, 1:] = False
    present[P_GRAD_ONLY, 0] = False
    slot = (np.arange(N)[:, None] + 5 * np.arange(C)[None, :]) % N
    noise = np.where(present, f32(rng.uniform(0.5, 2.0, (N, C))), 1.0)
    wa = np.where(present, f32(1.0 / noise), 0.0)
    pvar = f32(rng.uniform(0.0, 2.0, (N, C)))
    pvar[slot == 7] = 0.0
    pvar[slot == 8] = -0.25
    u = f32(rng.standard_normal(grid.m))
    mean = gr.stacked_rows(grid, X) @ u
    s = np.sqrt(np.maximum(pvar, 0.0) + KS2 * noise)
    nrest = N - 5
    one_sided = np.linspace(-8.0, 6.0, 2 * ((nrest + 2) // 3))        # > 0: satisfied by t s, < 0: violated
    rng.shuffle(one_sided)
    lo, hi = np.full((N, C), -INF), np.full((N, C), INF)
    kind = np.empty((N, C), dtype=object)
    for c in range(C):
        for i in range(N):
            k, mu, sc = slot[i, c], mean[i, c], s[i, c]
            if k in (0, 1):
                lo[i, c] = hi[i, c] = mu + sc * rng.uniform(-2.0, 2.0)
                kind[i, c] = "exact"
            elif k == 2:
                kind[i, c] = "open"
            elif k == 3:
                lo[i, c] = mu - 12.0 * sc
                kind[i, c] = "far"
            elif k == 4:
                lo[i, c], hi[i, c] = mu + 0.5 * sc, mu - 0.5 * sc
                kind[i, c] = "empty"
            else:
                j = k - 5
                kk = ("lower", "upper", "two")[j % 3]
                kind[i, c] = kk
                if kk == "two":
                    width = np.exp(rng.uniform(np.log(0.05), np.log(4.0)))
                    a = rng.uniform(-8.0, 8.0 - width)
                    lo[i, c], hi[i, c] = mu + sc * a, mu + sc * (a + width)
                else:
                    t = one_sided[2 * (j // 3) + (j % 3)]
                    if kk == "lower":
                        lo[i, c] = mu - t * sc
                    else:
                        hi[i, c] = mu + t * sc
    lo, hi = np.where(present, f32(lo), 0.0), np.where(present, f32(hi), 0.0)
    ref = dense_absorb(grid, X, lo, hi, wa, wa, noise, pvar, KS2, u)
    _cases[name] = dict(grid=grid, g=g, X=X, lo=lo, hi=hi, wa=wa, noise=noise, pvar=pvar, u=u, ref=ref, ok=inside(grid, X), present=present,
                        kind=kind, slot=slot, s=s)
    return _cases[name]


# ------------------------------------------------------------------------------------------------------- the streamed model
def channels(n, d, Y=None, lower=None, upper=None, noise=None, grad_lower=None, grad_upper=None, grad_noise=None, grad_mask=None):
    """The [n, d + 1] channel tensors (lo, hi, noise, present) of one condition_on_observations call with grad_lower / grad_upper:
    the value channel is Y (equal bounds), lower / upper, or absent; a missing side is -inf / +inf; grad_noise None: the value's
    noise (unit noise without one)."""
    lo, hi = np.full((n, d + 1), -INF), np.full((n, d + 1), INF)
    nz = np.ones((n, d + 1))
    present = np.ones((n, d + 1), dtype=bool)
    if grad_lower is not None:
        lo[:, 1:] = np.broadcast_to(np.asarray(grad_lower, dtype=np.float64), (n, d))
    if grad_upper is not None:
        hi[:, 1:] = np.broadcast_to(np.asarray(grad_upper, dtype=np.float64), (n, d))
    if Y is not None:
        lo[:, 0] = hi[:, 0] = np.asarray(Y, dtype=np.float64).reshape(n)
    elif lower is not None or upper is not None:
        if lower is not None:
            lo[:, 0] = np.asarray(lower, dtype=np.float64).reshape(n)
        if upper is not None:
            hi[:, 0] = np.asarray(upper, dtype=np.float64).reshape(n)
    else:
        present[:, 0] = False
    if noise is not None:
        nz[:, 0] = np.asarray(noise, dtype=np.float64).reshape(n)
    if grad_noise is None:
        nz[:, 1:] = nz[:, :1]
    else:
        gn = np.asarray(grad_noise, dtype=np.float64)
        nz[:, 1:] = gn[:, None] if gn.ndim == 1 else gn
    if grad_mask is not None:
        present[:, 1:] = np.asarray(grad_mask, dtype=bool)
    return lo, hi, nz, present


class DenseStream:
    """The model in statistics space, dense fp64: A = Phi^T D^-1 Phi, b = Phi^T D^-1 y, c = y^T D^-1 y, ld = log|D| over the N scalar
    observations absorbed so far, with Kt = Kuu / sigma2:  u = (I + Kt A)^-1 Kt b,  cov u = (I + Kt A)^-1 Kuu."""

    def __init__(self, grid, Kuu, sigma2):
        self.grid, self.K, self.sigma2 = grid, Kuu, float(sigma2)
        m = grid.m
        self.A, self.b, self.c, self.ld, self.n = np.zeros((m, m)), np.zeros(m), 0.0, 0.0, 0
        self._post = None

    def posterior(self):
        if self._post is None:
            Kt = self.K / self.sigma2
            lu = sla.lu_factor(np.eye(self.grid.m) + Kt @ self.A)
            self._post = (sla.lu_solve(lu, Kt @ self.b), sla.lu_solve(lu, self.K), float(np.sum(np.log(np.abs(np.diag(lu[0]))))))
        return self._post

    def jet(self, X):
        """(mean [n, C], variance [n, C]) of f and its partial derivatives at X."""
        u, cov, _ = self.posterior()
        Phi = gr.stacked_rows(self.grid, X)
        return Phi @ u, np.einsum("pca,ab,pcb->pc", Phi, cov, Phi)

    def add(self, X, y, wa, wb, noise, ent):
        """Absorb the entering channels (ent bool [n, C]) of [n, C] targets at the given weights and noise."""
        Phi = gr.stacked_rows(self.grid, X)
        wa, wb = np.where(ent, wa, 0.0), np.where(ent, wb, 0.0)
        y = np.where(ent, y, 0.0)
        self.A += np.einsum("pca,pc,pcb->ab", Phi, wa, Phi)
        self.b += np.einsum("pca,pc->a", Phi, wb * y)
        self.c += float((wb * y * y).sum())
        self.ld += float(np.log(noise[ent]).sum())
        self.n += int(ent.sum())
        self._post = None

    def add_values(self, X, y, noise):
        """The initial data: values at their noise."""
        n, C = np.asarray(X).reshape(-1, self.grid.d).shape[0], self.grid.d + 1
        Y, nz, ent = np.zeros((n, C)), np.ones((n, C)), np.zeros((n, C), dtype=bool)
        Y[:, 0], nz[:, 0], ent[:, 0] = y, noise, True
        self.add(X, Y, 1.0 / nz, 1.0 / nz, nz, ent)
        return self

    def decay(self, gamma):
        self.A *= gamma
        self.b *= gamma
        self.c *= gamma
        self.ld -= self.n * np.log(gamma)
        self._post = None

    def condition(self, X, lo, hi, noise, present, gamma=None):
        """One update: decay, match every present channel against the current posterior, absorb.  Returns the sites."""
        if gamma is not None:
            self.decay(gamma)
        X = np.asarray(X, dtype=np.float64).reshape(-1, self.grid.d)
        mean, var = self.jet(X)
        pres = np.asarray(present, dtype=bool) & inside(self.grid, X)[:, None]
        st = sites(np.where(pres, lo, 0.0), np.where(pres, hi, 0.0), mean, var, self.sigma2 * noise, pres)
        om = st["omega"]
        ent = om > 0.0
        oms = np.where(ent, om, 1.0)
        self.add(X, st["ytilde"], oms / np.maximum(noise, 1e-7), oms / noise, noise / oms, ent)      # (the weight floor of every update)
        return st

    def predict(self, Xs):
        """(mean [ns], variance [ns], gradient of the mean [ns, d]) at Xs."""
        mean, var = self.jet(Xs)
        return mean[:, 0], var[:, 0], mean[:, 1:]

    def mll(self):
        u, _, logdet = self.posterior()
        n = self.n
        return -0.5 * ((self.c - self.b @ u) / self.sigma2 + logdet + self.ld + n * np.log(self.sigma2) + n * np.log(2.0 * np.pi)) / n


# ------------------------------------------------------------------------------------------------------------------ the toy
TB, TG, TELL, TOSC, TS2 = [[-0.15, 1.15]], [32], 0.1, 1.0, 0.05
TNB, TQ = 4, 6                                                    # batches, points per batch
TNU = 1e-4                                                        # grad_noise of the sign constraint
TSEEDS = (0, 1, 2, 3, 4)


def toy_f(x):
    return np.tanh(4.0 * x - 2.0) + x


def toy(seed):
    """tanh(4x - 2) + x on [0, 1], noise variance 0.05: 4 batches of 6 points, 50 queries.  (RBF lengthscale 0.1 and 24 points, not
    0.25 and 48: DESIGN.md 3.25 says why.)"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (TNB * TQ, 1))
    y = toy_f(X[:, 0]) + np.sqrt(TS2) * rng.standard_normal(TNB * TQ)
    return X, y, np.linspace(0.02, 0.98, 50)[:, None]


def toy_figures(mean, slope, Xs):
    """(RMSE of the posterior mean to the truth, share of the queries where the posterior mean's slope is negative)."""
    return float(np.sqrt(np.mean((mean - toy_f(Xs[:, 0])) ** 2))), float(np.mean(slope < 0.0))


_toys = {}


def toy_reference(seed, constrained):
    """The toy through DenseStream, started from one point that says nothing (noise 1e6): its two figures."""
    key = (seed, constrained)
    if key not in _toys:
        X, y, Xs = toy(seed)
        grid = Grid.from_bounds(TB, TG)
        S = DenseStream(grid, gr.dense_kuu(grid, "rbf", TELL, TOSC), TS2).add_values(np.array([[0.5]]), np.array([0.0]), np.array([1e6]))
        for a in range(0, TNB * TQ, TQ):
            kw = dict(grad_lower=0.0, grad_noise=np.full((TQ, 1), TNU)) if constrained else dict(grad_mask=np.zeros((TQ, 1), dtype=bool))
            S.condition(X[a:a + TQ], *channels(TQ, 1, Y=y[a:a + TQ], **kw))
        mean, _, grad = S.predict(Xs)
        _toys[key] = toy_figures(mean, grad[:, 0], Xs)
    return _toys[key]
