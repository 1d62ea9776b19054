"""CPU: checks of the derivative-observation reference itself (tests/grad_obs_reference.py) -- no GPU, no kernel."""
import numpy as np

import grad_obs_reference as gr
from oracle import dataspace

GB, GS = [[-1.0, 1.0], [-0.5, 1.5]], [9, 8]


def _case(seed=0, n=25):
    rng = np.random.default_rng(seed)
    grid = gr.Grid.from_bounds(GB, GS)
    lo, hi = np.array(GB)[:, 0], np.array(GB)[:, 1]
    X = rng.uniform(lo, hi, (n, 2))
    f = np.sin(2 * X[:, 0]) * X[:, 1]
    G = np.stack([2 * np.cos(2 * X[:, 0]) * X[:, 1], np.sin(2 * X[:, 0])], 1)
    Y = np.concatenate([f[:, None], G], 1) + 0.05 * rng.standard_normal((n, 3))
    noise = rng.uniform(0.5, 2.0, (n, 3))
    return rng, grid, X, Y, noise


def test_data_space_and_statistics_space_posteriors_agree():
    rng, grid, X, Y, noise = _case()
    present = rng.uniform(size=Y.shape) < 0.7
    gp = gr.GradObsGP(grid, gr.dense_kuu(grid), sigma2=0.6).fit(X, Y, noise, present)
    Xs = rng.uniform(-0.4, 0.9, (30, 2))
    mean, var, grad = gp.predict(Xs)
    mean2, var2, grad2, mll2 = gp.stats_space(Xs)
    for a, b in ((mean, mean2), (var, var2), (grad, grad2)):
        assert np.abs(a - b).max() <= 1e-9 * np.abs(a).max()
    assert abs(gp.mll() - mll2) <= 1e-9 * abs(gp.mll())


def test_every_derivative_channel_masked_is_the_value_only_oracle():
    rng, grid, X, Y, noise = _case(1)
    present = np.zeros(Y.shape, dtype=bool)
    present[:, 0] = True
    gp = gr.GradObsGP(grid, gr.dense_kuu(grid), sigma2=0.8).fit(X, Y, noise, present)
    O = dataspace.DataSpaceGP(GB, GS, sigma2=0.8).fit(X, Y[:, 0], noise[:, 0])
    Xs = rng.uniform(-0.4, 0.9, (20, 2))
    mean, var, _ = gp.predict(Xs)
    mo, vo = O.predict(Xs)
    assert np.abs(mean - mo).max() <= 1e-9 * np.abs(mo).max() and np.abs(var - vo).max() <= 1e-9 * np.abs(vo).max()
    assert abs(gp.mll() - O.mll()) <= 1e-9 * abs(O.mll())


def test_boundary_cell_derivative_channel_moves_the_mll_but_not_the_mean():
    """In a one-hot boundary cell of dim q the value row does not depend on x_q, so the derivative row is zero: the observation is
    pure noise for the model -- it enters c, log|D| and N, never A or b."""
    rng, grid, X, Y, noise = _case(2)
    X[0, 0] = grid.g0[0] + 0.3 * grid.h[0]                               # first cell of dim 0
    present = np.ones(Y.shape, dtype=bool)
    K = gr.dense_kuu(grid)
    with_it = gr.GradObsGP(grid, K).fit(X, Y, noise, present)
    present2 = present.copy()
    present2[0, 1] = False
    without = gr.GradObsGP(grid, K).fit(X, Y, noise, present2)
    assert np.abs(gr.stacked_rows(grid, X[:1])[0, 1]).max() == 0.0 and np.abs(gr.stacked_rows(grid, X[:1])[0, 2]).max() > 0.0
    Xs = rng.uniform(-0.4, 0.9, (20, 2))
    for a, b in zip(with_it.predict(Xs), without.predict(Xs)):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    assert with_it.N == without.N + 1 and abs(with_it.mll() - without.mll()) > 1e-4


def test_dense_absorb_is_the_statistics_of_the_stacked_rows():
    rng, grid, X, Y, noise = _case(3)
    X[3] = [5.0, 0.0]                                                    # outside the grid: dropped, counted
    wa = 1.0 / noise
    u = rng.standard_normal(grid.m)
    ref = gr.dense_absorb(grid, X, Y, wa, wa, noise, u)
    Phi = gr.stacked_rows(grid, X).reshape(-1, grid.m)
    w = wa.reshape(-1)
    assert np.abs(ref["A"] - Phi.T @ (Phi * w[:, None])).max() <= 1e-12 * np.abs(ref["A"]).max()
    assert np.abs(ref["res"] - (ref["b"] - ref["A"] @ u)).max() <= 1e-11 * np.abs(ref["res"]).max()
    assert ref["err"] == 3 and ref["A_half"].shape == ((7 ** 2 + 1) // 2 * grid.m,)
    keep = np.arange(len(X)) != 3
    assert abs(ref["stats"][1] - np.log(noise[keep]).sum()) < 1e-12
