"""TEST INFRASTRUCTURE -- host reference of the polynomial trend with marginalised coefficients, numpy fp64 on the
CPU, shared by tests/test_trend_host.py (checks of this reference, no GPU) and tests/test_trend_gpu.py (the kernels and the model
against it).  Independent of every kernel and of grid_ops' wrappers; it imports ``oracle/`` read-only.

* :func:`basis`: the monomials of total degree <= deg in t = (x - center) / scale, graded lexicographic;
* :func:`stencil`: taps and weights of points as include/wiski.h defines them for ``wiski_scatter_trend`` -- the inside / outside
  verdict in the working precision, the weights in fp64, one rounding per operation in the kernel's order;
* :func:`scatter`: C, G, g with, per element of C, the number of non-zero addends and the sum of their absolute values (what the
  kernel test derives its bound from); :func:`rows`: R* = H* - W* S with the magnitude its bound needs;
* :func:`posterior` / :func:`evidence`: the GP in DATA space with the kernel W Kuu W^T + tau2 H H^T + sigma2 D (flat prior: GPML
  eq. 2.42), W Kuu W^T from ``oracle/dataspace.py`` -- they never form A, b, C, G, g or M;
* :func:`statspace`: the block-elimination formulas of DESIGN.md 3.22 on dense matrices -- what the model computes.
"""
import numpy as np
import scipy.linalg as sla

from oracle import dataspace, spec


def size(d, deg):
    return {0: 1, 1: d + 1, 2: (d + 1) * (d + 2) // 2}[deg]


def frame(g0, h, g):
    """(center, scale) of the basis: centre and half-extent of the grid."""
    g0, h, g = np.asarray(g0, np.float64), np.asarray(h, np.float64), np.asarray(g)
    half = 0.5 * h * (g - 1)
    return g0 + half, half


def basis(X, deg, center, scale):
    """H [n, p]: 1, t_1 .. t_d, t_1^2, t_1 t_2, .., t_1 t_d, t_2^2, ..  with t_k = (x_k - c_k) / s_k."""
    X = np.asarray(X, dtype=np.float64)
    X = X.reshape(-1, len(center))
    t = (X - np.asarray(center, np.float64)) / np.asarray(scale, np.float64)
    d = t.shape[1]
    cols = [np.ones(X.shape[0])]
    if deg >= 1:
        cols += [t[:, k] for k in range(d)]
    if deg >= 2:
        cols += [t[:, a] * t[:, b] for a in range(d) for b in range(a, d)]
    return np.stack(cols, axis=1)


def _dim_stencil(x, g0, h, g):
    """wiski_interp's rule for one dim in fp64: (j0 [n], w [n, 4]); boundary cells collapse to a one-hot on the nearest node."""
    u = (x - g0) / h
    fl = np.floor(u)
    t = u - fl
    j0 = fl.astype(np.int64) - 1
    w = np.stack([spec.keys_cubic(t + 1.0), spec.keys_cubic(t), spec.keys_cubic(t - 1.0), spec.keys_cubic(t - 2.0)], axis=1)
    edge = (j0 < 0) | (j0 > g - 4)
    base = np.where(j0 < 0, 0, g - 4)
    dist = np.abs(g0 + h * (base[:, None] + np.arange(4)[None, :]).astype(np.float64) - x[:, None])
    hot = np.eye(4)[np.argmin(dist, axis=1)]
    w = np.where(edge[:, None], hot, w)
    j0 = np.where(edge, base, j0)
    return j0, w


def stencil(g0, h, g, X, dtype=np.float64):
    """(ok [n], idx [n, T], w [n, T]) of the points X [n, d], given in `dtype`: flat node indices (dim 0 slowest) and weights
    ((w_0 w_1) w_2) w_3 of the 4^d taps, tap index = base-4 digits with dim 0 first.  ok: inside the grid as the working precision
    sees it (g0 and the last node rounded to `dtype`, the last node computed in it); accepted points are moved onto the fp64 grid."""
    d = len(g)
    Xr = np.asarray(X, dtype=dtype).reshape(-1, d)
    n = Xr.shape[0]
    ok = np.ones(n, dtype=bool)
    idx = np.zeros((n, 1), dtype=np.int64)
    w = np.ones((n, 1))
    stride = [int(np.prod(g[q + 1:])) for q in range(d)]
    for q in range(d):
        g0r, hr = dtype(g0[q]), dtype(h[q])
        hir = dtype(g0r + dtype(hr * dtype(int(g[q]) - 1)))
        xr = Xr[:, q]
        ok &= (xr >= g0r) & (xr <= hir)
        hi = float(g0[q]) + float(h[q]) * float(int(g[q]) - 1)
        xd = np.clip(xr.astype(np.float64), float(g0[q]), hi)
        xd = np.where(np.isfinite(xd), xd, float(g0[q]))          # (a NaN coordinate: outside; any stencil will do)
        j0, wq = _dim_stencil(xd, float(g0[q]), float(h[q]), int(g[q]))
        idx = (idx[:, :, None] + ((j0[:, None] + np.arange(4)[None, :]) * stride[q])[:, None, :]).reshape(n, -1)
        w = (w[:, :, None] * wq[:, None, :]).reshape(n, -1)
    return ok, idx, w


def scatter(g0, h, g, X, wa, wby, deg, center, scale, dtype=np.float64):
    """The trend statistics of the points X (in `dtype`; wa None: unit weights): a dict with C [m, p], G [p, p] (symmetric), g [p],
    and for the kernel's bounds k [m, p] (non-zero addends per element of C), abs_C [m, p], abs_G [p, p], abs_g [p] (sums of the
    absolute values of the addends), n_in (points inside).  Addends in fp64 as the kernel forms them, (wa w) h_j, summed in extended
    precision."""
    d = len(g)
    Xr = np.asarray(X, dtype=dtype).reshape(-1, d)
    n = Xr.shape[0]
    m, p = int(np.prod(g)), size(d, deg)
    ok, idx, w = stencil(g0, h, g, Xr, dtype)
    H = basis(Xr.astype(np.float64), deg, center, scale)
    wa = np.ones(n) if wa is None else np.asarray(wa, dtype=dtype).astype(np.float64)
    wby = np.asarray(wby, dtype=dtype).astype(np.float64)
    wa, wby = np.where(ok, wa, 0.0), np.where(ok, wby, 0.0)
    add = (wa[:, None] * w)[:, :, None] * H[:, None, :]                   # [n, T, p]
    add[~ok] = 0.0
    C = np.zeros((m, p), dtype=np.longdouble)
    absC = np.zeros((m, p), dtype=np.longdouble)
    k = np.zeros((m, p), dtype=np.int64)
    flat = idx.reshape(-1)
    np.add.at(C, flat, add.reshape(-1, p).astype(np.longdouble))
    np.add.at(absC, flat, np.abs(add).reshape(-1, p).astype(np.longdouble))
    np.add.at(k, flat, (add != 0.0).reshape(-1, p).astype(np.int64))
    tG = (wa[:, None] * H)[:, :, None] * H[:, None, :]                    # (wa h_a) h_b
    tg = wby[:, None] * H
    return {"C": C.astype(np.float64), "G": tG.astype(np.longdouble).sum(0).astype(np.float64), "g": tg.astype(np.longdouble).sum(0).astype(np.float64),
            "k": k, "abs_C": absC.astype(np.float64), "abs_G": np.abs(tG).sum(0), "abs_g": np.abs(tg).sum(0), "n_in": int(ok.sum()), "ok": ok}


def rows(g0, h, g, X, deg, center, scale, S, dtype=np.float64):
    """(R* [n, p], H* [n, p], mag [n, p], ok [n]): R* = h(x*) - sum_t w_t S[idx_t] for points inside (h(x*) outside), and
    mag = |h| + sum_t |w_t S[idx_t]|.  S [m, p] or None (R* = H*)."""
    d = len(g)
    Xr = np.asarray(X, dtype=dtype).reshape(-1, d)
    ok, idx, w = stencil(g0, h, g, Xr, dtype)
    H = basis(Xr.astype(np.float64), deg, center, scale)
    if S is None:
        return H.copy(), H, np.abs(H), ok
    S = np.asarray(S, dtype=np.float64)
    terms = w[:, :, None] * S[idx]                                        # [n, T, p]
    terms[~ok] = 0.0
    return H - terms.sum(1), H, np.abs(H) + np.abs(terms).sum(1), ok


# ------------------------------------------------------------------ data space --
def _gp(grid_bounds, grid_size, ell, osc, sigma2):
    return dataspace.DataSpaceGP(grid_bounds, grid_size, "rbf", ell, osc, sigma2)


def posterior(grid_bounds, grid_size, ell, osc, sigma2, X, y, noise, Xs, deg, center, scale, tau2):
    """(mean [q], cov [q, q], beta [p], cov_beta [p, p]) of f + h^T beta at Xs in data space.  tau2 a float: the GP with the kernel
    W Kuu W^T + tau2 H H^T + sigma2 D, literally; tau2 None: the flat prior, GPML eq. 2.42."""
    O = _gp(grid_bounds, grid_size, ell, osc, sigma2)
    X = np.asarray(X, np.float64).reshape(-1, O.d)
    Xs = np.asarray(Xs, np.float64).reshape(-1, O.d)
    y, noise = np.asarray(y, np.float64).reshape(-1), np.asarray(noise, np.float64).reshape(-1)
    H, Hs = basis(X, deg, center, scale), basis(Xs, deg, center, scale)
    K, Ks, Kss = O.cross(X, X), O.cross(Xs, X), O.cross(Xs, Xs)
    Ky = K + np.diag(sigma2 * noise)
    p = H.shape[1]
    if tau2 is not None:
        Kt = Ky + tau2 * H @ H.T
        cf = sla.cho_factor(Kt, lower=True)
        Kst = Ks + tau2 * Hs @ H.T
        mean = Kst @ sla.cho_solve(cf, y)
        cov = Kss + tau2 * Hs @ Hs.T - Kst @ sla.cho_solve(cf, Kst.T)
        # the coefficients given the data: prior N(0, tau2 I), observed through H
        beta = tau2 * H.T @ sla.cho_solve(cf, y)
        cov_beta = tau2 * np.eye(p) - tau2 * H.T @ sla.cho_solve(cf, H) * tau2
        return mean, cov, beta, cov_beta
    cf = sla.cho_factor(Ky, lower=True)
    KiH, Kiy = sla.cho_solve(cf, H), sla.cho_solve(cf, y)
    A = H.T @ KiH
    beta = np.linalg.solve(A, H.T @ Kiy)
    R = Hs - Ks @ KiH
    mean = Ks @ Kiy + R @ beta
    cov = Kss - Ks @ sla.cho_solve(cf, Ks.T) + R @ np.linalg.solve(A, R.T)
    return mean, cov, beta, np.linalg.inv(A)


def evidence(grid_bounds, grid_size, ell, osc, sigma2, X, y, noise, deg, center, scale, tau2):
    """log N(y; 0, W Kuu W^T + tau2 H H^T + sigma2 D) - log N(y; 0, W Kuu W^T + sigma2 D)."""
    O = _gp(grid_bounds, grid_size, ell, osc, sigma2)
    X = np.asarray(X, np.float64).reshape(-1, O.d)
    y, noise = np.asarray(y, np.float64).reshape(-1), np.asarray(noise, np.float64).reshape(-1)
    H = basis(X, deg, center, scale)
    Ky = O.cross(X, X) + np.diag(sigma2 * noise)

    def logp(Kmat):
        L = np.linalg.cholesky(Kmat)
        a = sla.solve_triangular(L, y, lower=True)
        return -0.5 * float(a @ a) - float(np.log(np.diag(L)).sum())

    return logp(Ky + tau2 * H @ H.T) - logp(Ky)


# ----------------------------------------------------------------- statistics space --
def dense_w(g0, h, g, X):
    ok, idx, w = stencil(g0, h, g, X)
    assert ok.all()
    W = np.zeros((idx.shape[0], int(np.prod(g))))
    np.add.at(W, (np.arange(idx.shape[0])[:, None], idx), w)
    return W


def statspace(grid_bounds, grid_size, ell, osc, sigma2, X, y, noise, Xs, deg, center, scale, tau2):
    """The formulas of DESIGN.md 3.22 on dense matrices: (mean, cov, beta, cov_beta, evidence or None)."""
    g0, h, g = spec.make_grid(grid_bounds, grid_size)
    d = len(g)
    X, Xs = np.asarray(X, np.float64).reshape(-1, d), np.asarray(Xs, np.float64).reshape(-1, d)
    y, noise = np.asarray(y, np.float64).reshape(-1), np.asarray(noise, np.float64).reshape(-1)
    Kuu = np.ones((1, 1))
    for c in spec.toeplitz_columns("rbf", h, g, ell, osc):
        Kuu = np.kron(Kuu, sla.toeplitz(c))
    W, Ws = dense_w(g0, h, g, X), dense_w(g0, h, g, Xs)
    H, Hs = basis(X, deg, center, scale), basis(Xs, deg, center, scale)
    wa = 1.0 / noise
    A, b = W.T @ (wa[:, None] * W), W.T @ (wa * y)
    C, G, gv = W.T @ (wa[:, None] * H), H.T @ (wa[:, None] * H), H.T @ (wa * y)
    Kt = Kuu / sigma2
    M = Kt @ np.linalg.inv(np.eye(Kuu.shape[0]) + A @ Kt)                 # (Kt^-1 + A)^-1 without Kuu^-1
    M = 0.5 * (M + M.T)
    mu0, S = M @ b, M @ C
    lam0 = G - C.T @ S
    p = G.shape[0]
    lam = lam0 + (0.0 if tau2 is None else sigma2 / tau2) * np.eye(p)
    v = gv - S.T @ b
    beta = np.linalg.solve(lam, v)
    Rs = Hs - Ws @ S
    mean = Ws @ mu0 + Rs @ beta
    cov = sigma2 * (Ws @ M @ Ws.T + Rs @ np.linalg.solve(lam, Rs.T))
    ev = None
    if tau2 is not None:
        ev = -0.5 * np.linalg.slogdet(np.eye(p) + (tau2 / sigma2) * lam0)[1] + 0.5 * float(v @ np.linalg.solve(lam, v)) / sigma2
    return mean, cov, beta, sigma2 * np.linalg.inv(lam), ev
