"""No GPU: checks of the jet-posterior reference itself (tests/jet_reference.py)."""
import numpy as np
import pytest
import torch

import grad_obs_reference as gr
import interp_reference as ir
import jet_reference as jr

GB, GS = [[-1.0, 1.0], [-1.0, 1.0]], [12, 10]


@pytest.fixture(scope="module")
def fitted():
    grid = gr.Grid.from_bounds(GB, GS)
    D = jr.model_data(grid)
    gp = gr.GradObsGP(grid, gr.dense_kuu(grid), 0.7).fit(D["X"], D["Y"], D["noise"], D["present"])
    return grid, D, gp, jr.JetGP(gp)


def test_data_space_and_statistics_space_agree(fitted):
    grid, D, gp, J = fitted
    m1, c1 = J.jet(D["Xs"], "data")
    m2, c2 = J.jet(D["Xs"], "stats")
    e_m, e_c = np.abs(m1 - m2).max() / np.abs(m1).max(), np.abs(c1 - c2).max() / np.abs(c1).max()
    print(f"data vs statistics space: mean {e_m:.3e}  covariance {e_c:.3e}  (bound 1e-9)")
    assert e_m <= 1e-9 and e_c <= 1e-9


def test_gradient_covariance_is_the_mixed_second_difference_of_the_posterior_covariance(fitted):
    """cov(d_q f(x), d_r f(x)) = d/dx_q d/dx'_r k_post(x, x') at x' = x, by central differences at interior points.

    k_post(x, x') = w(x)^T S w(x') is bilinear in the two rows, so the mixed difference equals (D_q w)^T S (D_r w) with
    D_q w = (w(x + s e_q) - w(x - s e_q)) / 2 s, and its error is first order in the error of each D w.  Per cell w is a cubic in
    every dim with |k'''| <= 9 in units of the spacing hg, so with r = s / hg the truncation of D_q w is r^2 / 6 * 9 = 1.5 r^2
    relative to 1 / hg; the rounding is the error of two weights -- eps times the size of the polynomial's terms, at most 8 per
    weight -- over 2 s: 8 eps / r relative to 1 / hg.  Balanced at r^3 = 8 eps / 1.5, r = 1.06e-5.  With two factors per entry
    and the usual factor 8: tol = 8 * 2 * (1.5 r^2 + 8 eps / r) of the entry's scale |d_q w|^T |S| |d_r w| (the difference rows
    have the size of the derivative rows)."""
    grid, D, gp, J = fitted
    r = (8 * ir.EPS64 / 1.5) ** (1.0 / 3.0)
    tol = 8 * 2 * (1.5 * r * r + 8 * ir.EPS64 / r)
    print(f"step {r:.3e} of the grid spacing, tolerance {tol:.3e} of |d_q w|^T |S| |d_r w|")
    rng = np.random.default_rng(5)
    hg = np.array(grid.h)
    cells = np.stack([rng.integers(1, g - 2, 12) for g in grid.g], 1)          # interior cells, points away from the cell faces
    X = np.array(grid.g0) + hg * (cells + rng.uniform(0.1, 0.9, cells.shape))
    n, d = X.shape
    _, cov = J.jet(X)
    got = jr.blocks_of(cov, n, d + 1)[:, 1:, 1:]
    S, _ = J.data_space()
    Ja = np.abs(gr.stacked_rows(grid, X))[:, 1:]
    scale = np.einsum("pqa,ab,prb->pqr", Ja, np.abs(S), Ja)
    # the four-point difference, taken on the rows before the product with S (k_post is bilinear in them): differencing the four
    # rounded values of k_post instead would divide THEIR rounding, eps |w|^T |S| |w|, by 4 s^2
    rows = lambda dx: ir.dense_rows(grid, torch.as_tensor(X + dx)).numpy()
    Dw = [(rows(np.eye(d)[q] * r * hg[q]) - rows(-np.eye(d)[q] * r * hg[q])) / (2 * r * hg[q]) for q in range(d)]
    worst = 0.0
    for q in range(d):
        for s_ in range(d):
            fd = np.einsum("pa,ab,pb->p", Dw[q], S, Dw[s_])
            worst = max(worst, float((np.abs(fd - got[:, q, s_]) / scale[:, q, s_]).max()))
    print(f"largest deviation {worst:.3e}")
    assert worst <= tol


def test_value_variance_and_gradient_mean_equal_the_grad_obs_reference(fitted):
    grid, D, gp, J = fitted
    mean, cov = J.jet(D["Xs"])
    n, C = mean.shape
    mo, vo, go = gp.predict(D["Xs"])
    B = jr.blocks_of(cov, n, C)
    e = [np.abs(mean[:, 0] - mo).max() / np.abs(mo).max(), np.abs(B[:, 0, 0] - vo).max() / np.abs(vo).max(), np.abs(mean[:, 1:] - go).max() / np.abs(go).max()]
    print("value mean %.3e  value variance %.3e  gradient mean %.3e  (bound 1e-9)" % tuple(e))
    assert max(e) <= 1e-9


def test_boundary_cell_zeroes_that_dims_row_and_column(fitted):
    grid, D, gp, J = fitted
    mean, cov = J.jet(D["Xs"])
    n, C = mean.shape
    B = jr.blocks_of(cov, n, C)
    assert np.all(B[-1, 1, :] == 0.0) and np.all(B[-1, :, 1] == 0.0) and mean[-1, 1] == 0.0      # last query: boundary cell of dim 0
    assert B[-1, 0, 0] > 0 and B[-1, 2, 2] > 0
    assert np.all(np.abs(B[:-1, np.arange(C), np.arange(C)]) > 0)
    # the kernel-case rows: a boundary-cell dim has an identically zero derivative row, and so has its first-order term
    g = ir.make_grid("d3g20x5x11")
    x = ir.make_points(g, 37, np.random.default_rng(1), torch.float64)
    Jr, S1 = jr.jet_rows(g, x), jr.rows_first_order(g, x)
    assert bool((S1[Jr.abs().sum(-1) == 0].abs().sum(-1) == 0).all()) and bool((S1 >= 0).all())
