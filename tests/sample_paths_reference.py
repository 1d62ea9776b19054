"""TEST INFRASTRUCTURE -- host reference of the posterior sample paths, numpy fp64 on the CPU, shared by
tests/test_sample_paths_host.py (checks of this reference, no GPU) and tests/test_sample_paths_gpu.py (the kernel and the model
against it).  Independent of every kernel and of grid_ops' wrappers; it imports ``oracle/`` read-only.

* :func:`philox4x32_10` and :func:`normals`: the generator of include/wiski.h (``wiski_scatter_probes``), word for word;
* :func:`dense_w`: interpolation rows from ``oracle/spec.py``'s per-dim weights (dim 0 slowest in the flat index);
* :func:`probes`: ``P[:, s] = W^T (sqrt(wa) * eps[:, s])`` with, per node, the number of contributions and the sum of their
  absolute values (what the kernel test derives its tolerance from);
* :func:`path_statspace`: ``u = eta + M (b - A eta - sigma P)``, ``M = (Kt^-1 + A)^-1`` -- what the model computes;
* :func:`path_dataspace`: ``eta + Kuu W^T (W Kuu W^T + sigma^2 D)^-1 (y - W eta - sigma D^(1/2) eps)``, ``D = diag(1 / wa)`` --
  Matheron's rule in data space, which never forms A, b, P or M.
"""
import numpy as np
import scipy.linalg as sla

from oracle import spec

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (broadcastable), unsigned 32-bit words -> [..., 4] output words (uint64 arrays holding 32-bit values)."""
    c = np.asarray(counter, dtype=np.uint64) & MASK
    k = np.asarray(key, dtype=np.uint64) & MASK
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = k[..., 0].copy(), k[..., 1].copy()
    for _ in range(10):
        p0 = np.uint64(M0) * c0                      # < 2^64: exact
        p1 = np.uint64(M1) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n1 = p1 & MASK
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        n3 = p0 & MASK
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1)


def normals(seed, indices, S):
    """eps [n, S] (fp64): the standard normals of the points with global indices `indices` (S even)."""
    assert S % 2 == 0
    idx = np.asarray(indices, dtype=np.uint64).reshape(-1)
    n = idx.shape[0]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.zeros((n, S // 2, 4), dtype=np.uint64)
    ctr[..., 0] = (idx & MASK)[:, None]
    ctr[..., 1] = (idx >> np.uint64(32))[:, None]
    ctr[..., 2] = np.arange(S // 2, dtype=np.uint64)[None, :]
    key = np.array([seed & MASK, seed >> 32], dtype=np.uint64)
    w = philox4x32_10(ctr, key)
    u0 = ((w[..., 0] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (w[..., 1] >> np.uint64(6)).astype(np.float64) + 1.0) * (1.0 / 9007199254740992.0)
    u1 = ((w[..., 2] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (w[..., 3] >> np.uint64(6)).astype(np.float64) + 1.0) * (1.0 / 9007199254740992.0)
    r = np.sqrt(-2.0 * np.log(u0))
    th = 6.283185307179586 * u1
    out = np.empty((n, S), dtype=np.float64)
    out[:, 0::2] = r * np.cos(th)
    out[:, 1::2] = r * np.sin(th)
    return out


def dense_w(g0, h, g, X):
    """Dense interpolation rows [n, m] of the points X [n, d] (oracle/spec.py's per-dim weights, one-hot boundary rule included)."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, len(g))
    W = np.ones((X.shape[0], 1))
    for q in range(len(g)):
        Wq = spec.interp_1d_dense(X[:, q], float(g0[q]), float(h[q]), int(g[q]))
        W = (W[:, :, None] * Wq[:, None, :]).reshape(X.shape[0], -1)
    return W


def probes(g0, h, g, X, wa, first_index, seed, S, with_bounds=False):
    """P [m, S] of the points X [n, d] with weights wa [n] (None: unit) and global indices first_index .. first_index + n - 1.
    with_bounds: also (count [m], abs_sum [m, S]) -- contributions per node and the sum of their absolute values."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, len(g))
    n = X.shape[0]
    W = dense_w(g0, h, g, X)
    eps = normals(seed, first_index + np.arange(n), S)
    sw = np.ones(n) if wa is None else np.sqrt(np.asarray(wa, dtype=np.float64).reshape(-1))
    sc = sw[:, None] * eps
    P = W.T @ sc
    if not with_bounds:
        return P
    return P, (W != 0).sum(0), np.abs(W).T @ np.abs(sc)


def kuu_dense(cols):
    K = np.ones((1, 1))
    for c in cols:
        K = np.kron(K, sla.toeplitz(np.asarray(c, dtype=np.float64)))
    return K


def sym_sqrt(K):
    lam, V = np.linalg.eigh(K)
    return (V * np.sqrt(np.clip(lam, 0.0, None))) @ V.T


def path_statspace(Kuu, W, wa, y, sigma2, eta, P):
    """u [S, m] = eta_s + M (b - A eta_s - sigma P_s) with M = (Kt^-1 + A)^-1 = Kt (I + A Kt)^-1 ... written without Kuu^-1:
    (Kt^-1 + A)^-1 r = Kt (I + A Kt)^-1 r.  eta [S, m], P [m, S]."""
    wa = np.asarray(wa, dtype=np.float64)
    A = W.T @ (wa[:, None] * W)
    b = W.T @ (wa * y)
    Kt = Kuu / sigma2
    rhs = b[:, None] - A @ eta.T - np.sqrt(sigma2) * P
    return (eta.T + Kt @ np.linalg.solve(np.eye(Kuu.shape[0]) + A @ Kt, rhs)).T


def statspace_map(Kuu, W, wa, sigma2):
    """The linear map (z, eps) -> u - E u of :func:`path_statspace` as two matrices (Lz [m, m], Le [m, n]): u - E u = Lz z + Le eps."""
    wa = np.asarray(wa, dtype=np.float64)
    A = W.T @ (wa[:, None] * W)
    Kt = Kuu / sigma2
    Mop = Kt @ np.linalg.inv(np.eye(Kuu.shape[0]) + A @ Kt)
    R = sym_sqrt(Kuu)
    Lz = R - Mop @ A @ R
    Le = -np.sqrt(sigma2) * Mop @ (W.T * np.sqrt(wa)[None, :])
    return Lz, Le, Mop


def path_dataspace(Kuu, W, wa, y, sigma2, eta, eps):
    """u [S, m] = eta_s + Kuu W^T (W Kuu W^T + sigma^2 D)^-1 (y - W eta_s - sigma D^(1/2) eps_s), D = diag(1 / wa); eps [n, S]."""
    wa = np.asarray(wa, dtype=np.float64)
    D = 1.0 / wa
    KW = Kuu @ W.T
    C = W @ KW
    C[np.diag_indices_from(C)] += sigma2 * D
    resid = y[:, None] - W @ eta.T - np.sqrt(sigma2) * np.sqrt(D)[:, None] * eps
    return (eta.T + KW @ sla.cho_solve(sla.cho_factor(C, lower=True), resid)).T
