"""No GPU: checks of the box-integral reference itself (tests/quadrature_reference.py).

Bounds, from eps64 and the size of the terms (none taken from a run):

* closed form against Gauss-Legendre, per entry: eps64 (16 T + 8 Q + 4 h g).  T is the entry with every term of its closed form
  replaced by its absolute value (``terms=True``): an entry is a sum of differences of two quartics of about eight operations each,
  every operation rounding by at most eps64 / 2 of a partial result no larger than the terms, once for each end.  Q is the quadrature
  of ``rows_1d(terms=True)`` with the same weights: the other side's own roundings (``interp_reference.C_ROUND`` = 8 per weight).
  4 h g: u = (x - g0) / h carries a relative rounding, at most eps64 g in cell units, at both ends of the box and on both sides; the
  integrand is at most 1, and a cell is h wide.
* row sums against the clipped width: eps64 (16 sum_j T_j + 4 h g).
* data space against statistics space: 1e-9 of the largest entry, the bound of tests/test_jet_host.py for the same two solves.
* data space against brute-force tensor quadrature of ``DataSpaceGP.predict``: the quadrature sums N points of magnitude at most
  max |f| with weights that sum to the volume, 8 N eps64 vol max|mean| for the mean and the same with both volumes for the covariance,
  plus eps64 cond for the solve the two sides share in different order -- taken as 1e-10 of the largest entry; the issue's own
  figures (2.5e-15 and 1.4e-16) show the reference far inside."""
import numpy as np
import pytest
import torch

import interp_reference as ir
import quadrature_reference as qr
from oracle import dataspace

EPS = ir.EPS64
GS = (4, 5, 9, 31)


def _boxes_1d(g, rng, n=40):
    """n intervals in units of the nodes: the full span, one cell, entirely outside, partly outside, and random ones."""
    last = g - 1
    fixed = [(0.0, float(last)), (1.0, 2.0), (0.0, 1.0), (last - 1.0, float(last)), (-3.0, -1.0), (last + 0.5, last + 2.0),
             (-0.7, 1.3), (last - 1.4, last + 0.8), (-1.0, last + 1.0), (0.2, 0.4), (0.3, 0.8), (last - 0.9, last - 0.2)]
    out = list(fixed)
    while len(out) < n:
        a, c = sorted(rng.uniform(-0.5, last + 0.5, 2))
        if c - a > 1e-3:
            out.append((a, c))
    return np.array(out)


@pytest.mark.parametrize("g", GS)
def test_closed_form_against_gauss_legendre_and_row_sums(g):
    rng = np.random.default_rng(100 + g)
    g0, h = -0.37, 0.23
    U = _boxes_1d(g, rng)
    lo, hi = g0 + h * U[:, 0], g0 + h * U[:, 1]
    rows, width, flag, rngs = qr.box_rows_1d(g0, h, g, lo, hi)
    T = qr.box_rows_1d(g0, h, g, lo, hi, terms=True)[0]
    worst = wsum = 0.0
    for b in range(len(lo)):
        x, w = qr.gl_pieces_1d(g0, h, g, lo[b], hi[b])
        if len(x):
            xt = torch.as_tensor(x)
            Q = (torch.as_tensor(w)[:, None] * ir.rows_1d(g0, h, g, xt)[0]).sum(0).numpy()
            Qt = (torch.as_tensor(w)[:, None] * ir.rows_1d(g0, h, g, xt, terms=True)[0]).sum(0).numpy()
        else:
            Q = Qt = np.zeros(g)
        bound = EPS * (16 * T[b] + 8 * Qt + 4 * h * g)
        worst = max(worst, float((np.abs(rows[b] - Q) / bound).max()))
        wsum = max(wsum, abs(rows[b].sum() - width[b]) / (EPS * (16 * T[b].sum() + 4 * h * g)))
        clipped = max(0.0, min(hi[b], g0 + h * (g - 1)) - max(lo[b], g0))
        assert abs(width[b] - clipped) <= 4 * EPS * h * g
        assert flag[b] == (lo[b] < g0 or hi[b] > g0 + h * (g - 1))
        nz = np.flatnonzero(rows[b])
        assert len(nz) == 0 or (rngs[b, 0] <= nz[0] and nz[-1] < rngs[b, 1] <= g)
    print(f"g = {g}: closed form vs Gauss-Legendre err/bound {worst:.3f}; row sum vs clipped width err/bound {wsum:.3f}")
    assert worst <= 1.0 and wsum <= 1.0


def test_a_whole_interior_cell_is_h_times_minus1_13_13_minus1_over_24():
    g0, h, g = 0.5, 0.125, 9
    rows = qr.box_rows_1d(g0, h, g, [g0 + 3 * h], [g0 + 4 * h])[0][0]
    want = np.zeros(g)
    want[2:6] = h * np.array([-1.0, 13.0, 13.0, -1.0]) / 24.0
    assert np.abs(rows - want).max() <= 16 * EPS * h * 8


@pytest.mark.parametrize("dname", ["f64", "f32"])
@pytest.mark.parametrize("g", GS)
def test_a_degenerate_dim_is_the_point_row_bit_for_bit(g, dname):
    dt = ir.DTYPES[dname]
    g0, h = -0.37, 0.23
    u = np.concatenate([np.random.default_rng(g).uniform(0.0, g - 1.0, 20), [0.0, g - 1.0, -0.5, g - 0.5]])
    x = torch.as_tensor(g0 + h * u).to(dt)
    rows, width, flag, _ = qr.box_rows_1d(g0, h, g, x.double().numpy(), x.double().numpy(), dtype=dt)
    W, _, inside = ir.rows_1d(g0, h, g, x)
    assert np.array_equal(rows, torch.where(inside[:, None], W, torch.zeros_like(W)).double().numpy())
    assert np.array_equal(width, inside.double().numpy()) and np.array_equal(flag, ~inside.numpy())


def test_invalid_bounds_give_a_zero_row_and_the_flag():
    rows, width, flag, rng = qr.box_rows_1d(0.0, 1.0, 6, [2.0, np.nan, 1.0], [1.0, 3.0, np.nan])
    assert not rows.any() and not width.any() and flag.all() and not rng.any()


# ------------------------------------------------------------------------------------------------------------ the posterior
GB, GSZ = [[-1.0, 1.0], [-1.0, 1.0]], [6, 5]


@pytest.fixture(scope="module")
def fitted():
    rng = np.random.default_rng(5)
    X = rng.uniform(-0.95, 0.95, (30, 2))
    y = np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.05 * rng.standard_normal(30)
    gp = dataspace.DataSpaceGP(GB, GSZ, "rbf", 0.6, 0.9, 0.7).fit(X, y, rng.uniform(0.5, 2.0, 30))
    B = qr.BoxGP(gp)
    g = B.grid
    node = lambda q, u: g.g0[q] + g.h[q] * u
    lo = np.array([[node(0, 0.0), node(1, 0.0)], [node(0, 1.2), node(1, 0.3)], [node(0, 0.6), node(1, 1.5)], [node(0, 2.3), node(1, 2.2)]])
    hi = np.array([[node(0, 5.0), node(1, 4.0)], [node(0, 3.7), node(1, 0.9)], [node(0, 4.4), node(1, 1.5)], [node(0, 2.3), node(1, 2.2)]])
    return gp, B, lo, hi                                      # the domain, a box, a line (dim 1 degenerate), a point


def test_data_space_and_statistics_space_agree(fitted):
    gp, B, lo, hi = fitted
    mean, cov, vol = B.integral(lo, hi)
    S, u = B.stats_space()
    C, vol2 = qr.box_rows(B.grid, lo, hi)
    m2, c2 = C @ u, C @ S @ C.T
    e_m, e_c = np.abs(mean - m2).max() / np.abs(mean).max(), np.abs(cov - c2).max() / np.abs(cov).max()
    print(f"data vs statistics space: mean {e_m:.3e}  covariance {e_c:.3e}  (bound 1e-9)")
    assert e_m <= 1e-9 and e_c <= 1e-9 and np.array_equal(vol, vol2)


def test_data_space_against_brute_force_quadrature_of_predict(fitted):
    gp, B, lo, hi = fitted
    mean, cov, vol = B.integral(lo, hi)
    pts = [qr.gl_box(B.grid, lo[b], hi[b]) for b in range(len(lo))]
    X = np.concatenate([p[0] for p in pts])
    mu, K = gp.predict(X, full_cov=True)
    ends = np.cumsum([0] + [len(p[1]) for p in pts])
    Wm = np.zeros((len(pts), len(X)))
    for b, p in enumerate(pts):
        Wm[b, ends[b]:ends[b + 1]] = p[1]
    m2, c2 = Wm @ mu, Wm @ K @ Wm.T
    e_m, e_c = np.abs(mean - m2).max() / np.abs(mean).max(), np.abs(cov - c2).max() / np.abs(cov).max()
    print(f"closed-form functionals vs tensor quadrature of predict ({len(X)} points): mean {e_m:.3e}  covariance {e_c:.3e}  (bound 1e-10)")
    assert e_m <= 1e-10 and e_c <= 1e-10
    assert abs(vol[0] - np.prod([B.grid.h[q] * (B.grid.g[q] - 1) for q in range(2)])) <= 1e-14 and vol[3] == 1.0
    # the point box is predict at that point; the average of the domain box is its integral over its volume
    mp, vp = gp.predict(lo[3:4])
    assert abs(mean[3] - mp[0]) <= 1e-12 and abs(cov[3, 3] - vp[0]) <= 1e-12
    ma, ca, _ = B.integral(lo, hi, average=True)
    assert np.allclose(ma, mean / vol, rtol=1e-14, atol=0) and np.allclose(ca, cov / np.outer(vol, vol), rtol=1e-14, atol=0)
