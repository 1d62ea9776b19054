"""No GPU: the identities behind the polynomial trend with marginalised coefficients, in numpy fp64.  The
block-elimination formulas the model computes from the statistics A, b, C, G, g (tests/trend_reference.py: statspace) are the
posterior and the evidence of the data-space GP with the kernel W Kuu W^T + tau2 H H^T + sigma2 D (flat prior: GPML eq. 2.42), which
never forms a statistic.  Plus the basis' order and size, the ABI's declarations, and the constructor's checks that need no device."""
import os
import re

import numpy as np
import pytest
import torch

import trend_reference as tref
from oracle import spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELL, OSC, S2 = 0.6, 1.3, 0.7


def _problem(d, seed=5):
    rng = np.random.default_rng(seed + d)
    gb = [[-1.0, 1.0]] * d
    gs = [9] if d == 1 else [7, 6]
    n = 40
    X = rng.uniform(-0.95, 0.95, (n, d))
    noise = rng.uniform(0.05, 0.6, n)
    y = 5.0 + 2.0 * X[:, 0] - (X[:, 1] if d > 1 else 0.0) + np.sin(3.0 * X.sum(1)) + np.sqrt(S2 * noise) * rng.standard_normal(n)
    Xs = rng.uniform(-0.95, 0.95, (11, d))
    return gb, gs, X, y, noise, Xs


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("tau2", [100.0, None])
@pytest.mark.parametrize("deg", [0, 1, 2])
@pytest.mark.parametrize("d", [1, 2])
def test_block_elimination_is_the_dataspace_gp(d, deg, tau2):
    gb, gs, X, y, noise, Xs = _problem(d)
    g0, h, g = spec.make_grid(gb, gs)
    center, scale = tref.frame(g0, h, g)
    args = (gb, gs, ELL, OSC, S2, X, y, noise)
    mean, cov, beta, cov_beta, ev = tref.statspace(*args, Xs, deg, center, scale, tau2)
    mean_o, cov_o, beta_o, cov_beta_o = tref.posterior(*args, Xs, deg, center, scale, tau2)
    assert _rel(mean, mean_o) < 1e-10
    assert _rel(cov, cov_o) < 1e-10
    assert _rel(beta, beta_o) < 1e-10
    assert _rel(cov_beta, cov_beta_o) < 1e-10
    if tau2 is not None:
        ev_o = tref.evidence(*args, deg, center, scale, tau2)
        assert abs(ev - ev_o) < 1e-10 * max(1.0, abs(ev_o))
        assert ev_o > 0.0                                # a level of 5 under a zero-mean prior: the trend explains the data better


def test_basis_order_and_size():
    assert [tref.size(d, deg) for d in (1, 2, 3, 4) for deg in (0, 1, 2)] == [1, 2, 3, 1, 3, 6, 1, 4, 10, 1, 5, 15]
    x = np.array([[2.0, 9.0, 16.0]])                                    # t = (0.5, 2, 3): distinct products
    H = tref.basis(x, 2, np.array([1.0, 1.0, 1.0]), np.array([2.0, 4.0, 5.0]))
    t1, t2, t3 = 0.5, 2.0, 3.0
    assert H.tolist() == [[1.0, t1, t2, t3, t1 * t1, t1 * t2, t1 * t3, t2 * t2, t2 * t3, t3 * t3]]
    assert tref.basis(x, 1, np.ones(3), np.array([2.0, 4.0, 5.0])).tolist() == [[1.0, t1, t2, t3]]
    assert tref.basis(x, 0, np.ones(3), np.ones(3)).tolist() == [[1.0]]
    from online_gp_amd import grid_ops

    assert all(grid_ops.trend_size(d, deg) == tref.size(d, deg) for d in (1, 2, 3, 4) for deg in (0, 1, 2))
    assert grid_ops.TREND_DEGREES == {"constant": 0, "linear": 1, "quadratic": 2}
    with pytest.raises(ValueError):
        grid_ops.trend_size(2, 3)


def test_reference_stencil_is_the_oracles_interpolation():
    rng = np.random.default_rng(3)
    gb, gs = [[-1.0, 1.0], [0.0, 2.0]], [6, 5]
    g0, h, g = spec.make_grid(gb, gs)
    hi = g0 + h * (g - 1)
    X = np.concatenate([rng.uniform(g0, hi, (50, 2)), [g0, hi]])            # boundary cells, the first and the last node
    W = tref.dense_w(g0, h, g, X)
    Wo = np.einsum("ni,nj->nij", spec.interp_1d_dense(X[:, 0], g0[0], h[0], 6), spec.interp_1d_dense(X[:, 1], g0[1], h[1], 5)).reshape(len(X), -1)
    assert np.array_equal(W, Wo)
    ok, _, _ = tref.stencil(g0, h, g, np.array([[hi[0] + 1e-3, 0.5], [0.0, np.nan]]))
    assert not ok.any()


def test_scatter_reference_is_the_dense_products():
    rng = np.random.default_rng(4)
    gb, gs = [[-1.0, 1.0], [0.0, 2.0]], [6, 5]
    g0, h, g = spec.make_grid(gb, gs)
    center, scale = tref.frame(g0, h, g)
    X = rng.uniform([-1.0, 0.0], [1.0, 2.0], (30, 2))
    wa, y = rng.uniform(0.5, 2.0, 30), rng.standard_normal(30)
    r = tref.scatter(g0, h, g, X, wa, wa * y, 2, center, scale)
    W, H = tref.dense_w(g0, h, g, X), tref.basis(X, 2, center, scale)
    assert np.allclose(r["C"], W.T @ (wa[:, None] * H), rtol=0, atol=1e-13)
    assert np.allclose(r["G"], H.T @ (wa[:, None] * H), rtol=0, atol=1e-12) and np.allclose(r["g"], H.T @ (wa * y), rtol=0, atol=1e-12)
    assert (r["k"] <= 30).all() and (r["abs_C"] >= np.abs(r["C"]) - 1e-15).all()
    S = rng.standard_normal((30, 6))
    R, Hs, mag, ok = tref.rows(g0, h, g, X, 2, center, scale, S)
    assert ok.all() and np.allclose(R, H - W @ S, rtol=0, atol=1e-13) and (mag >= np.abs(R) - 1e-15).all()


def test_abi_declares_both_entry_points():
    header = open(os.path.join(ROOT, "include", "wiski.h")).read()
    for name in ("wiski_scatter_trend", "wiski_trend_rows"):
        for suf in ("_f32", "_f64"):
            assert re.search(r"\bint " + name + suf + r"\(const wiski_grid\* grid,", header), name + suf
    from online_gp_amd import _hip

    assert "trend.hip" in _hip._SOURCES
    assert os.path.exists(os.path.join(ROOT, "online_gp_amd", "csrc", "trend.hip"))
    for name in ("scatter_trend", "trend_rows"):
        from online_gp_amd import grid_ops

        assert callable(getattr(grid_ops, name))


def _data(out=1):
    X = torch.linspace(-0.5, 0.5, 12, dtype=torch.float64)[:, None]
    return X, torch.ones(12, out, dtype=torch.float64), torch.ones(12, out, dtype=torch.float64)


@pytest.mark.parametrize("kwargs, exc, word", [
    (dict(trend="cubic"), ValueError, "trend must be"),
    (dict(trend="linear", trend_prior_var=0.0), ValueError, "trend_prior_var"),
    (dict(trend="linear", trend_prior_var=float("inf")), ValueError, "trend_prior_var"),
    (dict(trend_prior_var=10.0), ValueError, "needs trend"),
    (dict(trend="linear", robust_c=1.5), NotImplementedError, "robust_c"),
    (dict(trend="linear", window=8), NotImplementedError, "window"),
    (dict(trend="constant", num_path_probes=4), NotImplementedError, "path probes"),
])
def test_constructor_validates_and_refuses_before_it_needs_a_device(kwargs, exc, word):
    """These checks come before the model touches the device: CPU tensors suffice."""
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    X, Y, N = _data()
    with pytest.raises(exc, match=word):
        FixedNoiseOnlineSKIGP(X, Y, N, grid_bounds=torch.tensor([[-3.0, 3.0]]), grid_size=16, **kwargs)


def test_constructor_refuses_several_outputs_and_mismatched_caches():
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    X, Y, N = _data(out=2)
    with pytest.raises(NotImplementedError, match="single output"):
        FixedNoiseOnlineSKIGP(X, Y, N, grid_bounds=torch.tensor([[-3.0, 3.0]]), grid_size=16, trend="linear")
    ic = torch.zeros(1, 16, 1, dtype=torch.float64)
    with pytest.raises(ValueError, match="carries no trend statistics"):
        FixedNoiseOnlineSKIGP(kernel_cache={"interpolation_cache": ic}, trend="linear", num_data=0)
    with pytest.raises(ValueError, match="degree"):
        FixedNoiseOnlineSKIGP(kernel_cache={"interpolation_cache": ic, "trend_C": torch.zeros(16, 1, dtype=torch.float64), "trend_deg": 0},
                              trend="quadratic", num_data=0)
