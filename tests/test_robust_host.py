"""No GPU: the identity behind the outlier-robust absorb, in numpy fp64 on a 6 x 6 grid.  A batch absorbed with the
Huber weights omega of tests/robust_reference.py -- A and b, c = y^T D^-1 y and log|D| as the kernel is specified to build them --
gives the posterior mean, the posterior covariance and the marginal likelihood of the data-space GP (oracle/dataspace.py, which
never forms a statistic) at the noise d_i / omega_i.  Bound: that of tests/test_forgetting_host.py.  Independent of the kernel and
of the model."""
import ctypes
import os

import numpy as np

import robust_reference as rref
import sample_paths_reference as ref
from oracle import dataspace, spec
from test_forgetting_host import ELL, G, GB, OSC, S2, _close, _from_stats, _stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C = 1.5


def _problem(n0=30, q=20, seed=9):
    rng = np.random.default_rng(seed)
    n = n0 + q
    X = rng.uniform(-1.05, 1.05, (n, 2))
    noise = rng.uniform(0.3, 2.5, n)
    y = np.sin(2.5 * X.sum(1)) + 0.3 * rng.standard_normal(n)
    bad = n0 + np.arange(0, q, 3)                                     # every third point of the batch is a gross outlier
    y[bad] += rng.choice([-1.0, 1.0], bad.size) * rng.uniform(8.0, 40.0, bad.size) * np.sqrt(S2 * noise[bad])
    return X, y, noise, rng.uniform(-1.0, 1.0, (9, 2)), n0


def test_robustly_absorbed_statistics_are_the_gp_at_noise_over_omega():
    X, y, noise, Xs, n0 = _problem()
    n = X.shape[0]
    g0, h, g = spec.make_grid(GB, G)
    O = dataspace.DataSpaceGP(GB, G, "rbf", ELL, OSC, S2)
    W, Ws, Kuu = ref.dense_w(g0, h, g, X), ref.dense_w(g0, h, g, Xs), ref.kuu_dense(O.cols)
    grid = rref.Grid(g0, h, g)
    # the posterior before the batch, from the statistics of the first n0 points
    A, b, c, ld = _stats(W[:n0], y[:n0], noise[:n0])
    Kt = Kuu / S2
    u = Kt @ np.linalg.solve(np.eye(36) + A @ Kt, b)
    sl = slice(n0, n)
    inv_scale = 1.0 / np.sqrt(S2 * noise[sl])
    r = rref.dense_absorb(grid, X[sl], y[sl], 1.0 / noise[sl], 1.0 / noise[sl], noise[sl], inv_scale, C, u)
    om = r["omega"]
    assert int((om < 1).sum()) >= 7 and float(om.min()) < 0.2 and int((om == 1).sum()) >= 8 and r["err"] == 0
    assert _close(r["mean_out"], O.fit(X[:n0], y[:n0], noise[:n0]).predict(X[sl])[0])     # w . u IS the predictive mean
    mean, cov, mll = _from_stats(Kuu, A + r["A"], b + r["b"], c + r["stats"][0], ld + r["stats"][1], n, Ws)
    O.fit(X, y, np.concatenate([noise[:n0], noise[sl] / om]))
    mo, co = O.predict(Xs, full_cov=True)
    assert _close(mean, mo) and _close(cov, co) and _close(mll, O.mll())
    # and it is NOT the plainly absorbed GP (the check above can tell the two apart)
    O.fit(X, y, noise)
    assert not _close(mean, O.predict(Xs)[0], 1e-2)
    # the carried residual: R = b - Z - A U stays exact under the increment the weights define
    Z = np.linalg.solve(Kt, u)
    R = b - Z - A @ u
    assert _close(R + r["res"], (b + r["b"]) - Z - (A + r["A"]) @ u, 1e-12)
    # cnt is the row sums of the increment (rows of W sum to one)
    assert _close(r["cnt"], r["A"].sum(1), 1e-12)


def test_zero_inverse_scale_exempts_a_point_and_the_weight_is_continuous():
    om, z = rref.huber_weights([5.0, 5.0, 1.0, -3.0], [0.0, 0.0, 0.0, 0.0], [0.0, 1.0, 1.0, 1.0], 2.0)
    assert list(om) == [1.0, 0.4, 1.0, 2.0 / 3.0] and list(z) == [0.0, 5.0, 1.0, -3.0]
    eps = 1e-12
    lo, hi = rref.huber_weights([2.0 - eps, 2.0 + eps], [0.0, 0.0], [1.0, 1.0], 2.0)[0]
    assert lo == 1.0 and 0.0 <= 1.0 - hi < 1e-11


def test_kernel_is_declared_and_listed_for_the_build():
    from online_gp_amd import _hip

    hdr = open(os.path.join(ROOT, "include", "wiski.h")).read()
    for name in ("wiski_absorb_robust_f32", "wiski_absorb_robust_f64"):
        assert name in hdr
    assert "scatter_robust.h" in _hip._HEADERS and os.path.exists(os.path.join(ROOT, "online_gp_amd", "csrc", "scatter_robust.h"))
    assert '#include "scatter_robust.h"' in open(os.path.join(ROOT, "online_gp_amd", "csrc", "scatter_stats.hip")).read()
    # the public argument record has not grown: callers built against the previous header keep working
    assert ctypes.sizeof(_hip.wiski_absorb_args) == 224
