"""Host: checks of the analytic interpolation reference (tests/interp_reference.py) that tests/test_interp_derivatives_gpu.py holds
the derivative kernels to, and of that module's inputs.  No GPU: value rows against oracle/spec.py, the closed-form derivative
against central differences and against autograd of the value rows, continuity across interior nodes, zero gradient in boundary
cells; then every listed case is built once to see that its input is sound (S_abs > 0, no fp32 point on the wrong side of a
discontinuity)."""
import numpy as np
import pytest
import torch

import interp_reference as ir
from oracle import spec


def _interior(grid, n, rng, margin):
    """Random points with every coordinate in the cubic (non-boundary) cells and at least `margin` h away from every node."""
    x = np.empty((n, grid.d))
    for q in range(grid.d):
        cell = rng.integers(1, grid.g[q] - 2, n)
        x[:, q] = grid.g0[q] + grid.h[q] * (cell + rng.uniform(margin, 1.0 - margin, n))
    return torch.as_tensor(x)


@pytest.mark.parametrize("gname", list(ir.ALL_GRIDS))
def test_value_rows_are_the_products_of_the_oracle_rows(gname):
    grid = ir.make_grid(gname)
    g0, h, g = spec.make_grid(grid.grid_bounds, grid.g)
    assert np.array_equal(g0, np.array(grid.g0)) and np.array_equal(h, np.array(grid.h))
    rng = np.random.default_rng(1)
    x = ir.make_points(grid, 140, rng, torch.float64)
    x = torch.cat([x, _interior(grid, 60, rng, 0.0)])
    per = [torch.as_tensor(spec.interp_1d_dense(x[:, q].numpy(), g0[q], h[q], int(g[q]))) for q in range(grid.d)]
    W = ir.dense_rows(grid, x)
    assert W.shape == (200, grid.m)
    assert float((W - ir._kron_rows(per)).abs().max()) <= 1e-14
    assert float((W.sum(1) - 1).abs().max()) <= 1e-13          # the cubic and the one-hot rule both reproduce constants
    # dim 0 is the slowest: the row of a point on a node in every dim is the one-hot of that node's flat index
    j = [min(2, gi - 2) for gi in grid.g]
    xn = torch.tensor([[float(grid.grid_points()[q][j[q]]) for q in range(grid.d)]], dtype=torch.float64)
    flat = 0
    for q in range(grid.d):
        flat = flat * grid.g[q] + j[q]
    Wn = ir.dense_rows(grid, xn)[0]
    assert abs(float(Wn[flat]) - 1.0) <= 1e-13 and float(Wn.abs().sum()) <= 1 + 1e-12


def test_points_outside_the_grid_have_zero_rows_and_gradients():
    grid = ir.make_grid("d3g20x5x11")
    x = ir.make_points(grid, 40, np.random.default_rng(2), torch.float64, outside=True)
    W, dW = ir.dense_both(grid, x)
    out = torch.arange(40) % 3 == 1
    assert float(W[out].abs().max()) == 0 and float(dW[out].abs().max()) == 0
    assert bool((W[~out].sum(1) > 0.99).all())
    with pytest.raises(RuntimeError):
        spec.interp_1d_dense(x[out][:1, 0].numpy(), grid.g0[0], grid.h[0], grid.g[0])


@pytest.mark.parametrize("gname", list(ir.GRIDS))
def test_row_gradients_match_central_differences_of_the_rows(gname):
    """eps = 1e-5 h, points at least 1e-3 h away from every cell edge: truncation eps^2 k''' / 6 = 1.5e-10 and rounding
    eps64 / 1e-5 = 2e-11 relative to k' / h, so 1e-8 relative holds with room."""
    grid = ir.make_grid(gname)
    x = _interior(grid, 300, np.random.default_rng(3), 1e-3)
    dW = ir.dense_row_grads(grid, x)
    for q in range(grid.d):
        e = 1e-5 * grid.h[q]
        xp, xm = x.clone(), x.clone()
        xp[:, q] += e
        xm[:, q] -= e
        cd = (ir.dense_rows(grid, xp) - ir.dense_rows(grid, xm)) / (xp[:, q] - xm[:, q])[:, None]
        assert float((dW[:, q] - cd).abs().max()) <= 1e-8 * float(dW[:, q].abs().max())


@pytest.mark.parametrize("gname", ["d1g37", "d2g9x31"])
def test_row_gradients_match_autograd_of_the_rows_on_interior_points(gname):
    """10^4 random interior points: autograd through dense_rows (floor has a zero derivative, so the graph is the cubic of the
    point's own cell) agrees with the hand-written derivative to 1e-13 relative to 1 / h."""
    grid = ir.make_grid(gname)
    x = _interior(grid, 10000, np.random.default_rng(4), 0.0).requires_grad_(True)
    W = ir.dense_rows(grid, x)
    dW = ir.dense_row_grads(grid, x.detach())
    worst = 0.0
    for c in range(grid.m):
        (gc,) = torch.autograd.grad(W[:, c].sum(), x, retain_graph=True)
        worst = max(worst, float(((gc - dW[:, :, c]) * torch.tensor(grid.h, dtype=torch.float64)).abs().max()))
    assert worst <= 1e-13


@pytest.mark.parametrize("gname", list(ir.GRIDS))
def test_row_gradients_are_continuous_across_interior_nodes(gname):
    """The Keys cubic is C1: one-sided evaluations at node -+ 1e-9 h differ by less than 1e-7 / h (k'' <= 9: 1.8e-8 / h), and the
    evaluation exactly on the node (which belongs to the right-hand cell) lies within the same distance of both."""
    grid = ir.make_grid(gname)
    rng = np.random.default_rng(5)
    for q in range(grid.d):
        if grid.g[q] < 5:
            continue
        x = _interior(grid, grid.g[q] - 4, rng, 0.05)
        node = grid.grid_points()[q][2:grid.g[q] - 2]
        xs = []
        for off in (-1e-9, 0.0, 1e-9):
            xx = x.clone()
            xx[:, q] = node + off * grid.h[q]
            xs.append(xx)
        lo, at, hi = (ir.dense_row_grads(grid, xx) for xx in xs)
        hh = torch.tensor(grid.h, dtype=torch.float64)[None, :, None]
        for a, b in ((lo, hi), (lo, at), (at, hi)):
            assert float(((a - b) * hh).abs().max()) < 1e-7
        Wl, Wa, Wh = (ir.dense_rows(grid, xx) for xx in xs)
        assert float((Wl - Wh).abs().max()) < 1e-8 and float((Wa - Wh).abs().max()) < 1e-8


@pytest.mark.parametrize("gname", list(ir.GRIDS))
def test_row_gradients_are_zero_in_boundary_cell_dims_only(gname):
    grid = ir.make_grid(gname)
    rng = np.random.default_rng(6)
    for q in range(grid.d):
        x = _interior(grid, 20, rng, 0.05)
        x[:, q] = torch.tensor([grid.g0[q] + grid.h[q] * ir._boundary_u(rng, grid.g[q]) for _ in range(20)], dtype=torch.float64)
        dW = ir.dense_row_grads(grid, x)
        assert float(dW[:, q].abs().max()) == 0
        for o in range(grid.d):
            if o != q:
                assert bool((dW[:, o].abs().amax(1) > 0).all())
    # the switch nodes: node 1 opens the first cubic cell, node g - 2 the last (one-hot) cell
    for q in range(grid.d):
        x = _interior(grid, 2, rng, 0.05)
        x[0, q], x[1, q] = grid.grid_points()[q][1], grid.grid_points()[q][grid.g[q] - 2]
        u = (x[:, q] - grid.g0[q]) / grid.h[q]
        dW = ir.dense_row_grads(grid, x)
        for i in range(2):
            cubic = 1 <= float(torch.floor(u[i])) <= grid.g[q] - 3
            assert (float(dW[i, q].abs().max()) > 0) == cubic


def test_weight_roundings_are_relative_to_the_polynomial_terms_not_to_the_weight():
    """Why the two forwards' fp64 bound carries the first-order term S_1.  Against exact rational arithmetic, the reference's own
    fp64 weights are within 4 eps64 keys_terms(s) (Horner: three multiply-adds and one add) everywhere -- which is what S_1 allows,
    one weight at a time -- but not within 8 eps64 of their own value: the outer taps (|s| > 1) are at most 0.07 with terms up to
    24, and next to a node they vanish by cancellation.  No fp64 evaluation of the cubic, in whatever order, can be held to a bound
    relative to the weight where an outer tap carries the result."""
    from fractions import Fraction as Fr

    def exact(s):
        a = abs(Fr(s))
        if a <= 1:
            return ((Fr(3, 2) * a - Fr(5, 2)) * a) * a + 1
        return ((Fr(-1, 2) * a + Fr(5, 2)) * a - 4) * a + 2 if a < 2 else Fr(0)

    rng = np.random.default_rng(8)
    t = np.concatenate([rng.uniform(0, 1, 1500), 10.0 ** rng.uniform(-12, -6, 250), 1 - 10.0 ** rng.uniform(-12, -6, 250)])
    worst_terms, worst_generic, worst_node = 0.0, 0.0, 0.0
    for c in range(4):
        s64 = (t + 1.0) - c
        w = ir.keys(torch.as_tensor(s64)).numpy()
        terms = ir.keys_terms(torch.as_tensor(s64)).numpy()
        for i in range(len(t)):
            err = abs(float(Fr(float(w[i])) - exact(float(s64[i]))))
            worst_terms = max(worst_terms, err / terms[i])
            if w[i] != 0 and c in (0, 3):
                rel = err / abs(w[i])
                if i < 1500:
                    worst_generic = max(worst_generic, rel)
                else:
                    worst_node = max(worst_node, rel)
    assert worst_terms <= 4 * ir.EPS64
    assert worst_generic > 8 * ir.EPS64 and worst_node > 800 * ir.EPS64


# ------------------------------------------------------------------------------------------------- the GPU module's inputs
def _sound(R, grid, label):
    """S_abs is not identically zero, and an fp32 case's own restatement deviates from fp64 by no more than rounding of u explains:
    derivative weights times h differ by up to about 5 eps32 g per dim (measured on 1-D restatements), so 8 d eps32 max(g) of
    max S_abs bounds a sound input, while a point that fp32 puts on the other side of a discontinuity costs O(1) of it."""
    assert float(R.sabs.max()) > 0 and bool(torch.isfinite(R.ref).all()), label
    if R.ref32 is not None:
        assert R.dev32() <= R.tol32() / ir.C_ROUND, label                        # margin 1 of its own bound
        assert R.dev32() <= 8 * grid.d * ir.EPS32 * max(grid.g) * float(R.sabs.max()), (label, R.dev32(), float(R.sabs.max()))


@pytest.mark.parametrize("dname", list(ir.DTYPES))
@pytest.mark.parametrize("gname", list(ir.GRIDS))
def test_inputs_of_the_gather_cases_are_sound(gname, dname):
    for n in ir.GATHER_GRAD_N:
        for diag in (False, True):
            _sound(ir.gather_grad_case(gname, dname, n, diag)["R"], ir.make_grid(gname), f"gather_grad n={n} diag={diag}")
    for n in ir.ROWS_VJP_N:
        for ncols in ir.ROWS_VJP_NCOLS:
            _sound(ir.gather_rows_vjp_case(gname, dname, n, ncols)["R"], ir.make_grid(gname), f"gather_rows_vjp n={n} ncols={ncols}")


@pytest.mark.parametrize("dname", list(ir.DTYPES))
@pytest.mark.parametrize("gname", list(ir.ALL_GRIDS))
def test_inputs_of_the_bilinear_cases_are_sound(gname, dname):
    for qL, qR, nb, sym in ir.bilinear_shapes(gname):
        c = ir.bilinear_case(gname, dname, qL, qR, nb, sym)
        for k in ("fwd", "gL", "gR"):
            if k in c:
                _sound(c[k], c["grid"], f"bilinear {k} qL={qL} qR={qR} nb={nb} sym={sym}")


@pytest.mark.parametrize("dname", list(ir.DTYPES))
@pytest.mark.parametrize("gname", list(ir.GRIDS))
def test_inputs_of_the_basis_cases_are_sound(gname, dname):
    for (n, r, kmax, sc, cs, pr) in ir.basis_shapes(gname):
        c = ir.basis_case(gname, dname, n, r, kmax, sc, cs, pr)
        for k in ("F", "prior", "gx"):
            _sound(c[k], c["grid"], f"basis {k} n={n} r={r} kmax={kmax}")


def test_bilinear_cases_reach_every_form_combination_that_exists():
    """(forward, left VJP) forms over the case list.  The VJP's row form needs d rows in LDS where the forward needs one, and both
    compare the same number of other points with m, so (pair, row) cannot occur; the other three must all be present."""
    seen = set()
    for gname in ir.ALL_GRIDS:
        for dname, dtype in ir.DTYPES.items():
            for qL, qR, nb, sym in ir.bilinear_shapes(gname):
                f = ir.bilinear_forms(gname, dtype, qL, qR)
                seen.add((f[0], f[1]))
    assert seen == {("pair", "pair"), ("row", "row"), ("row", "pair")}
