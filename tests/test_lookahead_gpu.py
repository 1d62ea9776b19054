"""GPU: look-ahead acquisitions in the dense regime.  The interpolated bilinear-form kernels
(wiski_interp_bilinear and its VJP) against dense interpolation rows and central differences; differentiable fantasies on the
30^2 Matern-1/2 geometry; collapsed qNIPV against the fantasy path; one-shot qKG against a brute force through fantasize; the
active-learning and BO loops with the gradient optimiser."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GB = [[-1.1, 1.1]]


def _grid(d, g):
    from online_gp_amd import grid_ops

    return grid_ops.GridSpec(torch.tensor(GB * d), g)


def _points(rng, grid, nb, q, boundary=0, dtype=torch.float64):
    """[nb, q, d] interior points; the first `boundary` points of every batch sit in the one-hot boundary cells (inside the grid)."""
    x = rng.uniform(-0.9, 0.9, (nb, q, grid.d))
    for j in range(boundary):
        for k in range(grid.d):
            x[:, j, k] = grid.g0[k] + (0.3 + 0.4 * rng.uniform()) * grid.h[k] if (j + k) % 2 == 0 else grid.g0[k] + (grid.g[k] - 1.7) * grid.h[k]
    return torch.as_tensor(x, device=DEV, dtype=dtype)


def _sym(rng, m):
    A = rng.standard_normal((m, m))
    return torch.as_tensor(A + A.T, device=DEV)


def _dense_ref(grid, A, xL, xR):
    from online_gp_amd import grid_ops

    err = grid_ops.new_err_flag(DEV)
    WL = grid_ops.wt_columns(grid, xL.reshape(-1, grid.d).double(), err).reshape(xL.shape[0], xL.shape[1], grid.m)
    WR = grid_ops.wt_columns(grid, xR.reshape(-1, grid.d).double(), err).reshape(xR.shape[0], xR.shape[1], grid.m)
    return WL @ A.double() @ WR.transpose(-1, -2)


# --------------------------------------------------------------------------------------------------------------- kernels
# (d, g, qL, qR): qR * 4^d below and above m, so both the pair form and the row form run
CASES = [(1, 20, 3, 2), (1, 20, 4, 9), (2, 12, 5, 3), (2, 12, 3, 13), (3, 9, 4, 5), (3, 9, 2, 20)]


@pytest.mark.parametrize("d,g,qL,qR", CASES)
def test_interp_bilinear_matches_dense_rows_fp64(d, g, qL, qR):
    from online_gp_amd import grid_ops

    rng = np.random.default_rng(10 * d + qR)
    grid = _grid(d, g)
    A = _sym(rng, grid.m)
    xL, xR = _points(rng, grid, 3, qL, boundary=1), _points(rng, grid, 3, qR, boundary=2)
    err = grid_ops.new_err_flag(DEV)
    out = grid_ops.interp_bilinear(grid, A, xL, xR, err)
    ref = _dense_ref(grid, A, xL, xR)
    assert out.shape == (3, qL, qR)
    assert float((out - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    # symmetric mode: one triangle mirrored, exactly symmetric
    for xs in (xL, xR):
        s = grid_ops.interp_bilinear(grid, A, xs, None, err)
        rs = _dense_ref(grid, A, xs, xs)
        assert float((s - rs).abs().max()) <= 1e-12 * float(rs.abs().max())
        assert torch.equal(s, s.transpose(-1, -2))
    assert grid_ops.read_flag(err) == 0
    # n = 0 and an empty side are no-ops
    assert grid_ops.interp_bilinear(grid, A, xL[:0], xR[:0], err).shape == (0, qL, qR)
    assert grid_ops.interp_bilinear(grid, A, xL, xR[:, :0], err).shape == (3, qL, 0)


@pytest.mark.parametrize("d,g,qL,qR", [CASES[1], CASES[2], CASES[5]])
def test_interp_bilinear_fp32(d, g, qL, qR):
    from online_gp_amd import grid_ops

    rng = np.random.default_rng(7 + d)
    grid = _grid(d, g)
    A = _sym(rng, grid.m)
    xL, xR = _points(rng, grid, 2, qL, boundary=1), _points(rng, grid, 2, qR)
    ref = _dense_ref(grid, A, xL, xR)
    out = grid_ops.interp_bilinear(grid, A.float(), xL.float(), xR.float())
    dev = float((out.double() - ref).abs().max()) / float(ref.abs().max())
    print(f"fp32 interp_bilinear d={d} rel deviation {dev:.3e}")
    assert dev <= 3 * 8.5e-7                                  # 3x the largest measured deviation (d = 1)


def test_interp_bilinear_flags_points_outside_the_grid():
    from online_gp_amd import grid_ops

    rng = np.random.default_rng(3)
    grid = _grid(2, 10)
    A = _sym(rng, grid.m)
    xL = _points(rng, grid, 1, 3)
    xR = xL.clone()
    xR[0, 1, 0] = 5.0
    err = grid_ops.new_err_flag(DEV)
    grid_ops.interp_bilinear(grid, A, xL, None, err)
    assert grid_ops.read_flag(err) == 0
    out = grid_ops.interp_bilinear(grid, A, xL, xR, err)
    assert grid_ops.read_flag(err) != 0
    assert float(out[0, :, 1].abs().max()) == 0.0


def _cd_points(f, x, eps=1e-6):
    out = torch.empty_like(x)
    flat, of = x.reshape(-1), out.reshape(-1)
    for i in range(flat.numel()):
        xp, xm = flat.clone(), flat.clone()
        xp[i] += eps
        xm[i] -= eps
        of[i] = (f(xp.reshape(x.shape)) - f(xm.reshape(x.shape))) / (2 * eps)
    return out


@pytest.mark.parametrize("d,g,qL,qR", [CASES[0], CASES[1], CASES[2], CASES[3], CASES[4], CASES[5]])
def test_interp_bilinear_vjp_against_central_differences(d, g, qL, qR):
    from online_gp_amd import grid_ops

    rng = np.random.default_rng(100 + 10 * d + qR)
    grid = _grid(d, g)
    A = _sym(rng, grid.m)
    nb = 2
    xL, xR = _points(rng, grid, nb, qL), _points(rng, grid, nb, qR)
    G = torch.as_tensor(rng.standard_normal((nb, qL, qR)), device=DEV)
    err = grid_ops.new_err_flag(DEV)
    gL, gR = grid_ops.interp_bilinear_vjp(grid, A, xL, xR, G)
    rL = _cd_points(lambda x: float((grid_ops.interp_bilinear_raw(grid, A, x, xR, err) * G).sum()), xL)
    rR = _cd_points(lambda x: float((grid_ops.interp_bilinear_raw(grid, A, xL, x, err) * G).sum()), xR)
    scale = max(1.0, float(rL.abs().max()), float(rR.abs().max()))
    assert float((gL - rL).abs().max()) < 1e-6 * scale and float((gR - rR).abs().max()) < 1e-6 * scale
    # symmetric mode: the whole gradient in one output
    Gs = torch.as_tensor(rng.standard_normal((nb, qL, qL)), device=DEV)
    gS, none = grid_ops.interp_bilinear_vjp(grid, A, xL, None, Gs)
    assert none is None
    rS = _cd_points(lambda x: float((grid_ops.interp_bilinear_raw(grid, A, x, None, err) * Gs).sum()), xL)
    assert float((gS - rS).abs().max()) < 1e-6 * max(1.0, float(rS.abs().max()))
    # deterministic, and the autograd Function runs the same kernels
    assert torch.equal(grid_ops.interp_bilinear_vjp(grid, A, xL, xR, G)[0], gL)
    xa, xb = xL.clone().requires_grad_(True), xR.clone().requires_grad_(True)
    (grid_ops.interp_bilinear(grid, A, xa, xb) * G).sum().backward()
    assert torch.equal(xa.grad, gL) and torch.equal(xb.grad, gR)


@pytest.mark.parametrize("q", [4, 9])
def test_points_outside_the_grid_contribute_nothing_in_both_forms(q):
    """q * 16 against m = 100: q = 4 runs the pair form, q = 9 the row form (forward and both VJP sides)."""
    from online_gp_amd import grid_ops

    rng = np.random.default_rng(40 + q)
    grid = _grid(2, 10)
    A = _sym(rng, grid.m)
    xL, xR = _points(rng, grid, 2, q), _points(rng, grid, 2, q + 1)
    xL[1, 2, 0] = 5.0
    xR[0, 3, 1] = -4.0
    G = torch.as_tensor(rng.standard_normal((2, q, q + 1)), device=DEV)
    err = grid_ops.new_err_flag(DEV)
    out = grid_ops.interp_bilinear_raw(grid, A, xL, xR, err)
    assert grid_ops.read_flag(err) != 0
    assert float(out[1, 2].abs().max()) == 0.0 and float(out[0, :, 3].abs().max()) == 0.0
    inside = _dense_ref(grid, A, xL.clamp(-1, 1), xR.clamp(-1, 1))
    mask = torch.ones_like(out, dtype=torch.bool)
    mask[1, 2] = False
    mask[0, :, 3] = False
    assert float((out - inside)[mask].abs().max()) <= 1e-12 * float(inside.abs().max())
    gL, gR = grid_ops.interp_bilinear_vjp(grid, A, xL, xR, G)
    assert float(gL[1, 2].abs().max()) == 0.0 and float(gR[0, 3].abs().max()) == 0.0
    # every other gradient is what the same call gives with the outside point's pairs taken out of G
    G0 = G.clone()
    G0[1, 2] = 0.0
    G0[0, :, 3] = 0.0
    xLc, xRc = xL.clone(), xR.clone()
    xLc[1, 2, 0] = 0.0
    xRc[0, 3, 1] = 0.0
    hL, hR = grid_ops.interp_bilinear_vjp(grid, A, xLc, xRc, G0)
    hL[1, 2] = 0.0
    hR[0, 3] = 0.0
    scale = max(float(hL.abs().max()), float(hR.abs().max()))
    assert float((gL - hL).abs().max()) <= 1e-12 * scale and float((gR - hR).abs().max()) <= 1e-12 * scale


def test_a_right_side_that_aliases_the_left_is_a_second_input():
    """The symmetric mode is asked for by leaving xR out, never inferred from shared storage: x against x.detach() differentiates
    the left side only, x against itself sums both sides, and prefix views of one tensor are two point sets."""
    from online_gp_amd import grid_ops

    rng = np.random.default_rng(21)
    grid = _grid(2, 12)
    A = _sym(rng, grid.m)
    x = _points(rng, grid, 2, 5)
    G = torch.as_tensor(rng.standard_normal((2, 5, 5)), device=DEV)
    err = grid_ops.new_err_flag(DEV)
    xg = x.clone().requires_grad_(True)
    out = grid_ops.interp_bilinear(grid, A, xg, xg.detach())
    assert float((out.detach() - _dense_ref(grid, A, x, x)).abs().max()) <= 1e-12 * float(out.detach().abs().max())
    (out * G).sum().backward()
    ref = _cd_points(lambda y: float((grid_ops.interp_bilinear_raw(grid, A, y, x, err) * G).sum()), x)
    assert float((xg.grad - ref).abs().max()) < 1e-6 * max(1.0, float(ref.abs().max()))
    xs = x.clone().requires_grad_(True)
    (grid_ops.interp_bilinear(grid, A, xs, xs) * G).sum().backward()
    gS, _ = grid_ops.interp_bilinear_vjp(grid, A, x, None, G)
    assert float((xs.grad - gS).abs().max()) <= 1e-12 * float(gS.abs().max())
    one = x[:1].clone().requires_grad_(True)
    pre = grid_ops.interp_bilinear(grid, A, one[:, :2], one[:, :4])
    assert pre.shape == (1, 2, 4)
    assert float((pre.detach() - _dense_ref(grid, A, x[:1, :2], x[:1, :4])).abs().max()) <= 1e-12 * float(pre.detach().abs().max())
    pre.sum().backward()
    assert bool(torch.isfinite(one.grad).all())


def test_interp_bilinear_vjp_is_zero_in_one_hot_cells_and_checks_arguments():
    from online_gp_amd import _hip, grid_ops

    rng = np.random.default_rng(5)
    grid = _grid(2, 12)
    A = _sym(rng, grid.m)
    xL, xR = _points(rng, grid, 2, 3, boundary=3), _points(rng, grid, 2, 4)
    G = torch.as_tensor(rng.standard_normal((2, 3, 4)), device=DEV)
    gL, gR = grid_ops.interp_bilinear_vjp(grid, A, xL, xR, G)
    assert float(gL.abs().max()) == 0.0 and float(gR.abs().max()) > 0
    gS, _ = grid_ops.interp_bilinear_vjp(grid, A, xL, None, torch.ones((2, 3, 3), device=DEV, dtype=torch.float64))
    assert float(gS.abs().max()) == 0.0
    f = _hip.fn("wiski_interp_bilinear_vjp", torch.float64)
    gx = torch.empty_like(xL)
    s = _hip.stream_ptr(xL.device)
    args = lambda lda, xr, qr, gxr: (grid.ref, _hip.dptr(A), ctypes.c_int64(lda), _hip.dptr(xL), ctypes.c_int32(3), xr, ctypes.c_int32(qr), ctypes.c_int64(2),
                                     _hip.dptr(G), _hip.dptr(gx), gxr, s)
    assert f(*args(grid.m - 1, _hip.dptr(xR), 4, None)) != 0                                  # lda < m
    assert f(*args(grid.m, None, 3, _hip.dptr(torch.empty_like(xL)))) != 0                     # symmetric mode with a right gradient
    assert f(*args(grid.m, _hip.dptr(xR), -1, None)) != 0                                      # negative size
    fb = _hip.fn("wiski_interp_bilinear", torch.float64)
    assert fb(grid.ref, None, ctypes.c_int64(grid.m), _hip.dptr(xL), ctypes.c_int32(3), None, ctypes.c_int32(3), ctypes.c_int64(2), _hip.dptr(G),
              _hip.dptr(grid_ops.new_err_flag(DEV)), s) != 0                                  # no table
    with pytest.raises(ValueError):
        grid_ops.interp_bilinear(grid, A[:, :5], xL, xR)
    with pytest.raises(ValueError):
        grid_ops.interp_bilinear(grid, A, xL, xR[:1])


# ------------------------------------------------------------------------------------------------------------- fantasies
def _model(g=30, n=40, dense=True, d=2, outputs=1):
    from online_gp_amd import settings
    from online_gp_amd.kernels import GridInterpolationKernel, MaternKernel, ScaleKernel
    from online_gp_amd.models import OnlineSKIBotorchModel

    rng = np.random.default_rng(0)
    X = rng.uniform(0, 1, (n, d)); y = np.sin(4 * X[:, 0]) * np.cos(3 * X[:, -1]) + 0.05 * rng.standard_normal(n)
    nz = rng.uniform(0.3, 0.8, n)
    Y = np.stack([y + 0.1 * o for o in range(outputs)], -1)
    gb = torch.tensor([[0.0, 1.0]] * d, dtype=torch.float64)
    bs = torch.Size([outputs]) if outputs > 1 else torch.Size([])
    cov = GridInterpolationKernel(ScaleKernel(MaternKernel(nu=0.5, ard_num_dims=d, batch_shape=bs), batch_shape=bs), grid_size=g, num_dims=d, grid_bounds=gb)
    with settings.dense_small_grids(dense):
        m = OnlineSKIBotorchModel(torch.as_tensor(X, device=DEV), torch.as_tensor(Y, device=DEV), torch.as_tensor(np.repeat(nz[:, None], outputs, 1), device=DEV),
                                  covar_module=cov, learn_additional_noise=True)
    m.eval()
    return m


class _FixedSampler:
    def __init__(self, z):
        self.z = z
        self.sample_shape = torch.Size([z.shape[0]])

    def __call__(self, posterior):
        return posterior.rsample(self.sample_shape, base_samples=self.z)


def _fantasy_fn(m, Xq, Gm, Gv):
    def f(X, Y, Xqq):
        fm = m.condition_on_observations(X=X, Y=Y, noise=torch.full_like(Y, 0.4))
        post = fm.posterior(Xqq)
        return (post.mean[..., 0] * Gm).sum() + (post.variance[..., 0] * Gv).sum()

    return f


def test_fantasy_values_with_grad_equal_the_values_without():
    m = _model()
    rng = np.random.default_rng(1)
    b, q, F = 3, 2, 4
    X = torch.as_tensor(rng.uniform(0.1, 0.9, (b, q, 2)), device=DEV)
    z = torch.as_tensor(rng.standard_normal((F, b, q)), device=DEV)
    Xq = torch.as_tensor(rng.uniform(0.05, 0.95, (5, 2)), device=DEV)
    Xqb = torch.as_tensor(rng.uniform(0.05, 0.95, (b, 4, 2)), device=DEV)
    with torch.no_grad():
        fm0 = m.fantasize(X, _FixedSampler(z))
        p0, pb0 = fm0.posterior(Xq), fm0.posterior(Xqb)
    Xg = X.clone().requires_grad_(True)
    fm1 = m.fantasize(Xg, _FixedSampler(z))
    assert fm1.train_targets.requires_grad                                      # reparameterised end to end
    for Q, P0 in ((Xq, p0), (Xqb, pb0)):
        P1 = fm1.posterior(Q.clone().requires_grad_(True))
        for a, r in ((P1.mean, P0.mean), (P1.variance, P0.variance), (P1.mvn.covariance_matrix, P0.mvn.covariance_matrix)):
            assert a.shape == r.shape
            assert float((a.detach() - r).abs().max()) <= 1e-12 * max(1.0, float(r.abs().max()))
    # a model built without grad, queried with grad, takes the same values
    P2 = fm0.posterior(Xq.clone().requires_grad_(True))
    assert float((P2.mean.detach() - p0.mean).abs().max()) <= 1e-12 * max(1.0, float(p0.mean.abs().max()))


def test_fantasy_gradients_match_central_differences():
    m = _model()
    rng = np.random.default_rng(2)
    b, q, F = 2, 3, 2
    X = torch.as_tensor(rng.uniform(0.1, 0.9, (b, q, 2)), device=DEV)
    Y = torch.as_tensor(rng.standard_normal((F, b, q, 1)), device=DEV)
    Xq = torch.as_tensor(rng.uniform(0.05, 0.95, (b, 4, 2)), device=DEV)
    Gm = torch.as_tensor(rng.standard_normal((F, b, 4)), device=DEV)
    Gv = torch.as_tensor(rng.standard_normal((F, b, 4)), device=DEV)
    f = _fantasy_fn(m, Xq, Gm, Gv)
    Xg, Yg, Qg = X.clone().requires_grad_(True), Y.clone().requires_grad_(True), Xq.clone().requires_grad_(True)
    gX, gY, gQ = torch.autograd.grad(f(Xg, Yg, Qg), (Xg, Yg, Qg))
    with torch.no_grad():
        rX = _cd_points(lambda x: float(f(x, Y, Xq)), X)
        rY = _cd_points(lambda y: float(f(X, y, Xq)), Y)
        rQ = _cd_points(lambda x: float(f(X, Y, x)), Xq)
    for g_, r_ in ((gX, rX), (gY, rY), (gQ, rQ)):
        assert float((g_ - r_).abs().max()) < 1e-6 * max(1.0, float(r_.abs().max())), (g_, r_)
    # shared queries [q', d]: the expand's gradient sums over the candidate sets
    Xs = Xq[0]
    Gs = torch.as_tensor(rng.standard_normal((F, b, 4)), device=DEV)
    fs = _fantasy_fn(m, Xs, Gs, Gs)
    Qs = Xs.clone().requires_grad_(True)
    (gs,) = torch.autograd.grad(fs(X, Y, Qs), (Qs,))
    with torch.no_grad():
        rs = _cd_points(lambda x: float(fs(X, Y, x)), Xs)
    assert float((gs - rs).abs().max()) < 1e-6 * max(1.0, float(rs.abs().max()))


@pytest.mark.parametrize("b", [1, 3])
def test_fantasy_posterior_at_its_own_inputs_is_differentiable(b):
    """fantasize(X) queried at X itself (queries and fantasy inputs are views of one tensor), and with one candidate set at X[0]."""
    m = _model()
    rng = np.random.default_rng(30 + b)
    q, F = 3, 2
    X = torch.as_tensor(rng.uniform(0.1, 0.9, (b, q, 2)), device=DEV)
    z = torch.as_tensor(rng.standard_normal((F, b, q)), device=DEV)
    Gm = torch.as_tensor(rng.standard_normal((F, b, q)), device=DEV)
    Gv = torch.as_tensor(rng.standard_normal((F, b, q)), device=DEV)

    def f(Xc, shared):
        fm = m.fantasize(Xc, _FixedSampler(z))
        post = fm.posterior(Xc[0] if shared else Xc)
        return (post.mean[..., 0] * Gm).sum() + (post.variance[..., 0] * Gv).sum()

    for shared in ((False, True) if b == 1 else (False,)):
        Xg = X.clone().requires_grad_(True)
        (gx,) = torch.autograd.grad(f(Xg, shared), (Xg,))
        with torch.no_grad():
            r = _cd_points(lambda x: float(f(x, shared)), X)
        assert float((gx - r).abs().max()) < 1e-6 * max(1.0, float(r.abs().max())), (shared, gx, r)


def test_fantasy_gradients_outside_the_dense_regime_raise():
    from online_gp_amd import settings

    rng = np.random.default_rng(4)
    X = torch.as_tensor(rng.uniform(0.1, 0.9, (2, 2, 2)), device=DEV)
    Y = torch.zeros((2, 2), device=DEV, dtype=torch.float64)
    with settings.dense_small_grids(False), settings.cg_tolerance(1e-10):
        m = _model(g=8, dense=False)
        with torch.no_grad():
            fm = m.condition_on_observations(X=X, Y=Y)                         # values without grad work as before
            v0 = fm.posterior(X[0]).variance
        assert bool(torch.isfinite(v0).all())
        with pytest.raises(NotImplementedError, match="dense regime"):
            m.condition_on_observations(X=X.clone().requires_grad_(True), Y=Y)
        with pytest.raises(NotImplementedError, match="dense regime"):
            fm.posterior(X[0].clone().requires_grad_(True))
    mo = _model(g=8, outputs=2)
    with pytest.raises(NotImplementedError, match="dense regime"):
        mo.condition_on_observations(X=X.clone().requires_grad_(True), Y=torch.zeros((2, 2, 2), device=DEV, dtype=torch.float64))


# ----------------------------------------------------------------------------------------------------------------- qNIPV
def test_collapsed_qnipv_equals_the_fantasy_path_and_its_gradient():
    from online_gp_amd import harness

    m = _model()
    rng = np.random.default_rng(6)
    mc = torch.as_tensor(rng.uniform(0, 1, (500, 2)), device=DEV)
    X = torch.as_tensor(rng.uniform(0.02, 0.98, (5, 6, 2)), device=DEV)

    class _S:
        sample_shape = torch.Size([2])

        def __call__(self, post):
            return post.rsample(self.sample_shape)

    ref = harness.qnipv_select(m, X, mc, _S())
    val = harness.acqf_values(m, X, "qnipv", mc_points=mc)
    assert float(((val - ref) / ref).abs().max()) <= 1e-10
    cache = harness.qnipv_cache(m, mc)
    assert harness.qnipv_cache(m, mc) is cache                                   # built once per (model, MC set)
    Xg = X.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(harness.acqf_values(m, Xg, "qnipv", mc_points=mc).sum(), (Xg,))
    with torch.no_grad():
        r = _cd_points(lambda x: float(harness.acqf_values(m, x, "qnipv", mc_points=mc).sum()), X)
    assert float((gx - r).abs().max()) < 1e-6 * max(1e-3, float(r.abs().max()))
    with pytest.raises(ValueError):
        harness.acqf_values(m, X, "qnipv")


def test_qnipv_cache_follows_in_place_updates_and_checks_the_grid():
    from online_gp_amd import harness

    m = _model()
    rng = np.random.default_rng(12)
    mc = torch.as_tensor(rng.uniform(0, 1, (300, 2)), device=DEV)
    X = torch.as_tensor(rng.uniform(0.02, 0.98, (4, 6, 2)), device=DEV)
    v0 = harness.acqf_values(m, X, "qnipv", mc_points=mc)
    xn = torch.as_tensor(rng.uniform(0, 1, (8, 2)), device=DEV)
    m.condition_on_observations(X=xn, Y=torch.sin(3 * xn[:, :1]), noise=torch.full((8, 1), 0.5, device=DEV, dtype=torch.float64), inplace=True)
    v1 = harness.acqf_values(m, X, "qnipv", mc_points=mc)
    assert not torch.equal(v0, v1)
    assert torch.equal(v1, harness.QNIPVCache(m, mc).values(X))

    class _S:
        sample_shape = torch.Size([1])

        def __call__(self, post):
            return post.rsample(self.sample_shape)

    ref = harness.qnipv_select(m, X, mc, _S())
    assert float(((v1 - ref) / ref).abs().max()) <= 1e-10
    Xo = X.clone()
    Xo[1, 2, 0] = 3.0
    with pytest.raises(RuntimeError, match="out of bounds"):
        harness.acqf_values(m, Xo, "qnipv", mc_points=mc)
    assert torch.equal(harness.acqf_values(m, X, "qnipv", mc_points=mc), v1)          # the flag does not leak into later calls


# ------------------------------------------------------------------------------------------------------------------- qKG
def _kg_brute(m, X, Xp, z, cv):
    """fantasize at X [q, d] with the normals z [J, q], posterior mean of fantasy j at x'_j, averaged, minus cv."""
    with torch.no_grad():
        fm = m.fantasize(X[None], _FixedSampler(z[:, None, :]))
        mean = fm.posterior(Xp[None]).mean[:, 0, :, 0]                         # [J, J]: fantasy j at every x'
        return float(mean.diagonal().mean()) - cv


def test_kg_equals_brute_force_fantasies_and_its_gradient():
    from online_gp_amd import harness

    m = _model()
    rng = np.random.default_rng(8)
    b, q, J = 3, 2, 16
    X = torch.as_tensor(rng.uniform(0.05, 0.95, (b, q + J, 2)), device=DEV)
    z = torch.as_tensor(rng.standard_normal((J, q)), device=DEV)
    cv = 0.3
    val = harness.acqf_values(m, X, "kg", base_samples=z, best_f=cv)
    for i in range(b):
        ref = _kg_brute(m, X[i, :q], X[i, q:], z, cv)
        assert abs(float(val[i]) - ref) <= 1e-10 * max(1.0, abs(ref + cv))
    assert torch.equal(harness.acqf_values(m, X, "kg", base_samples=z, current_value=cv), val)
    Xg = X.clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(harness.acqf_values(m, Xg, "kg", base_samples=z, best_f=cv).sum(), (Xg,))
    with torch.no_grad():
        r = _cd_points(lambda x: float(harness.acqf_values(m, x, "kg", base_samples=z, best_f=cv).sum()), X)
    assert float((gx - r).abs().max()) < 1e-6 * max(1.0, float(r.abs().max()))
    with pytest.raises(ValueError):
        harness.acqf_values(m, X, "kg", base_samples=z)                         # no current value
    with pytest.raises(ValueError):
        harness.acqf_values(m, X[:, :5], "kg", base_samples=z, best_f=cv)      # not q + J points


def test_optimize_acqf_kg_returns_an_in_box_batch_no_worse_than_the_raw_starts():
    from online_gp_amd import harness

    m = _model()
    bounds = torch.tensor([[0.1, 0.2], [0.9, 0.8]], dtype=torch.float64)
    q, J, raw, seed = 2, 32, 16, 5
    Xb, v = harness.optimize_acqf(m, "kg", bounds, q, num_restarts=2, raw_samples=raw, maxiter=20, seed=seed, best_f=0.0, num_fantasies=J)
    assert Xb.shape == (q, 2)
    assert bool((Xb >= bounds[0].to(Xb)).all()) and bool((Xb <= bounds[1].to(Xb)).all())
    g = torch.Generator(device="cpu").manual_seed(seed)
    starts = bounds[0] + (bounds[1] - bounds[0]) * torch.rand((raw, q + J, 2), generator=g, dtype=torch.float64)
    z = torch.randn((J, q), generator=g, dtype=torch.float64)
    with torch.no_grad():
        v0 = harness.acqf_values(m, starts.to(DEV), "kg", base_samples=z.to(DEV), best_f=0.0)
    assert float(v) >= float(v0.max()) - 1e-12


# ----------------------------------------------------------------------------------------------------------------- loops
def test_gradient_qnipv_active_learning_on_the_config5_geometry():
    from online_gp_amd import harness
    from online_gp_amd.kernels import GridInterpolationKernel, MaternKernel, ScaleKernel
    from online_gp_amd.models import OnlineSKIBotorchModel
    from online_gp_amd.priors import GammaPrior

    rng = np.random.default_rng(3)
    f = lambda X: torch.sin(5 * X[:, 0]) * torch.cos(4 * X[:, 1]) + 0.5 * X[:, 0]
    pool = torch.as_tensor(rng.uniform(0, 1, (3600, 2)), device=DEV)
    mc = torch.as_tensor(rng.uniform(0, 1, (500, 2)), device=DEV)
    nvar = lambda X: (1e-6 + 0.05 * (0.5 + 0.5 * torch.sin(17 * X.sum(-1)))).clamp(1e-6, 0.05)
    x0 = torch.as_tensor(rng.uniform(0, 1, (10, 2)), device=DEV)
    gb = torch.tensor([[0.0, 1.0]] * 2, dtype=torch.float64)
    cov = GridInterpolationKernel(ScaleKernel(MaternKernel(nu=0.5, ard_num_dims=2, lengthscale_prior=GammaPrior(3.0, 6.0)),
                                              outputscale_prior=GammaPrior(2.0, 0.15)), grid_size=30, num_dims=2, grid_bounds=gb)
    gen = torch.Generator(device="cpu").manual_seed(1)
    obs = lambda X: f(X) + nvar(X).sqrt() * torch.randn(X.shape[0], generator=gen, dtype=torch.float64).to(X)
    y0 = obs(x0)
    model = OnlineSKIBotorchModel(x0, y0.reshape(-1, 1), nvar(x0).reshape(-1, 1), covar_module=cov, learn_additional_noise=True)
    model.eval()
    ipv0 = float(model.posterior(mc).variance.mean())
    seen, models = {}, [model]

    def on_step(s, m):
        seen[s] = m.num_data
        models.append(m)

    rows, model, chosen = harness.qnipv_active_learning(model, pool, obs, mc, batch_size=6, num_steps=20, noise_fn=nvar, selector="gradient",
                                                        on_step=on_step)
    ipv = [ipv0] + [r["integrated_posterior_variance"] for r in rows]
    assert all(b < a for a, b in zip(ipv, ipv[1:]))
    assert chosen.numel() == 120 and chosen.unique().numel() == 120
    assert seen == {s: 10 + 6 * (s + 1) for s in range(20)} and [r["num_data"] for r in rows] == [10 + 6 * (s + 1) for s in range(20)]
    assert all(np.isfinite(r["qnipv_best"]) and r["qnipv_best"] < 0 for r in rows)
    for s in (0, 7, 19):                                # qnipv_best is the score of the snapped pool points under the model of that step
        v = harness.acqf_values(models[s], pool[chosen[6 * s:6 * s + 6].to(DEV)][None], "qnipv", mc_points=mc)
        assert abs(float(v[0]) - rows[s]["qnipv_best"]) <= 1e-12 * abs(rows[s]["qnipv_best"])
    with pytest.raises(ValueError):
        harness.qnipv_active_learning(model, pool, obs, mc, num_steps=1, selector="best")


def test_bayesopt_with_one_shot_kg():
    from online_gp_amd import harness
    from online_gp_amd.models import OnlineSKIBotorchModel

    d = 2
    bounds = torch.tensor([[-2.0, 2.0]] * d, dtype=torch.float64)
    gen = torch.Generator().manual_seed(0)
    init_x = torch.rand(8, d, generator=gen, dtype=torch.float64).to(DEV)
    fn = lambda Xr: -((Xr - 0.5) ** 2).sum(-1) + torch.cos(3 * Xr).sum(-1)
    init_y = fn(bounds[:, 0].to(DEV) + (bounds[:, 1] - bounds[:, 0]).to(DEV) * init_x).reshape(-1, 1)

    def make_model(train_x, train_y, old):
        if old is None:
            return OnlineSKIBotorchModel(train_x, train_y, None, grid_bounds=bounds, grid_size=16, learn_additional_noise=True)
        return OnlineSKIBotorchModel(covar_module=old.covar_module, kernel_cache=old._kernel_cache, learn_additional_noise=True,
                                     likelihood=old.likelihood, num_data=old.num_data)

    rows, tx, ty, _ = harness.bayesopt(fn, bounds, make_model, init_x, init_y, num_steps=10, batch_size=2, fit_iters=3, num_candidates=32,
                                       acqf_optimizer="gradient", acqf="kg", num_restarts=2, maxiter=15, num_fantasies=32)
    assert len(rows) == 10 and tx.shape == (28, d)
    assert bool((tx >= 0).all()) and bool((tx <= 1).all()) and bool(torch.isfinite(ty).all())
    best = [r["max_achieved"] for r in rows]
    assert all(np.isfinite(best)) and all(b >= a for a, b in zip(best, best[1:]))
