"""No GPU: the identity behind exponential forgetting, in numpy fp64 on a 6 x 6 grid.  The streamed statistics
A = W^T D^-1 W, b = W^T D^-1 y, c = y^T D^-1 y, log|D| scaled by gamma (log|D| moved by -n log gamma) give the posterior mean, the
posterior covariance and the marginal likelihood of the data-space GP (oracle/dataspace.py, which never forms a statistic) at the
noise d / gamma -- and, decayed once per batch, at d_i gamma^-(batches since i).  Independent of the kernel and of the model."""
import os

import numpy as np

import sample_paths_reference as ref
from oracle import dataspace, spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GB, G = [[-1.1, 1.1]] * 2, [6, 6]
ELL, OSC, S2 = [0.45, 0.6], 1.3, 0.37


def _problem(n=50, seed=5):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.05, 1.05, (n, 2))
    y = np.sin(2.5 * X.sum(1)) + 0.3 * rng.standard_normal(n)
    noise = rng.uniform(0.3, 2.5, n)
    Xs = rng.uniform(-1.0, 1.0, (9, 2))
    return X, y, noise, Xs


def _stats(W, y, noise):
    return W.T @ (W / noise[:, None]), W.T @ (y / noise), float(y @ (y / noise)), float(np.log(noise).sum())


def _from_stats(Kuu, A, b, c, ld, n, Ws):
    """(mean, covariance at the rows Ws, MLL / n) of y ~ N(0, W Kuu W^T + s2 D) from the statistics alone (Woodbury)."""
    m = Kuu.shape[0]
    Kt = Kuu / S2
    B = np.eye(m) + A @ Kt
    M = Kt @ np.linalg.inv(B)                                         # (Kt^-1 + A)^-1 without Kuu^-1
    mean = Ws @ (M @ b)
    cov = S2 * Ws @ M @ Ws.T
    quad = (c - b @ M @ b) / S2
    logdet = np.linalg.slogdet(B)[1] + ld + n * np.log(S2)
    return mean, cov, -0.5 * (quad + logdet + n * np.log(2.0 * np.pi)) / n


def _close(a, b, tol=1e-10):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= tol * max(1.0, np.abs(np.asarray(b)).max())


def _setup(X, Xs):
    g0, h, g = spec.make_grid(GB, G)
    O = dataspace.DataSpaceGP(GB, G, "rbf", ELL, OSC, S2)
    return ref.dense_w(g0, h, g, X), ref.dense_w(g0, h, g, Xs), ref.kuu_dense(O.cols), O


def test_scaled_statistics_are_the_gp_at_inflated_noise():
    X, y, noise, Xs = _problem()
    n = X.shape[0]
    W, Ws, Kuu, O = _setup(X, Xs)
    A, b, c, ld = _stats(W, y, noise)
    for gamma in (1.0, 0.9, 2.0 ** -10):
        mean, cov, mll = _from_stats(Kuu, gamma * A, gamma * b, gamma * c, ld - n * np.log(gamma), n, Ws)
        O.fit(X, y, noise / gamma)
        mo, co = O.predict(Xs, full_cov=True)
        assert _close(mean, mo) and _close(cov, co) and _close(mll, O.mll()), gamma
    # and it is NOT the undecayed GP (the check above can tell the two apart)
    O.fit(X, y, noise)
    assert not _close(mean, O.predict(Xs)[0], 1e-3)


def test_one_decay_per_batch_ages_every_point_by_its_batches():
    X, y, noise, Xs = _problem(n=60, seed=6)
    W, Ws, Kuu, O = _setup(X, Xs)
    gamma, batch = 0.8, 20
    A = np.zeros((36, 36)); b = np.zeros(36); c = ld = 0.0
    for k, lo in enumerate(range(0, 60, batch)):
        if k:                                                          # an update decays what is there, then absorbs
            A, b, c, ld = gamma * A, gamma * b, gamma * c, ld - lo * np.log(gamma)
        dA, db, dc, dl = _stats(W[lo:lo + batch], y[lo:lo + batch], noise[lo:lo + batch])
        A, b, c, ld = A + dA, b + db, c + dc, ld + dl
    age = 2 - np.arange(60) // batch
    O.fit(X, y, noise * gamma ** -age)
    mean, cov, mll = _from_stats(Kuu, A, b, c, ld, 60, Ws)
    mo, co = O.predict(Xs, full_cov=True)
    assert _close(mean, mo) and _close(cov, co) and _close(mll, O.mll())


def test_residual_follows_in_closed_form():
    """R = b - Z - A U with Z = Kt^-1 U: after the decay the same (U, Z) has the residual gamma R - (1 - gamma) Z."""
    X, y, noise, Xs = _problem()
    W, _, Kuu, _ = _setup(X, Xs)
    A, b, _, _ = _stats(W, y, noise)
    rng = np.random.default_rng(1)
    Z = rng.standard_normal(36)
    U = (Kuu / S2) @ Z
    R = b - Z - A @ U
    gamma = 0.7
    assert _close(gamma * R - (1 - gamma) * Z, gamma * b - Z - gamma * A @ U, 1e-13)


def test_kernel_is_declared_and_listed_for_the_build():
    from online_gp_amd import _hip

    hdr = open(os.path.join(ROOT, "include", "wiski.h")).read()
    assert "wiski_decay_stats_f32" in hdr and "wiski_decay_stats_f64" in hdr and "wiski_decay_plan" in hdr
    assert "decay_stats.hip" in _hip._SOURCES
    assert os.path.exists(os.path.join(ROOT, "online_gp_amd", "csrc", "decay_stats.hip"))
    assert ctypes_plan_matches_header(_hip)


def ctypes_plan_matches_header(_hip):
    import ctypes

    n = _hip.DECAY_MAX_REGIONS
    return ctypes.sizeof(_hip.wiski_decay_plan) == n * (8 + 8 + 8) + 8 and _hip.DECAY_MAX_OUTPUTS == 8
