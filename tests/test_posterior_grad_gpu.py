"""GPU: gradients of the posterior w.r.t. its query points.  The two VJP kernels (wiski_gather_rows_vjp, wiski_basis_project_vjp)
against central differences of their forwards; the posterior's mean / variance / q-block covariance / root / fixed-sample rsample
gradients in each regime (dense factor, spectral factor, PCG) against central differences of the same posterior and of the
data-space oracle; the BoTorch adaptor's base_samples; harness.optimize_acqf on a fitted model."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import dataspace

pytestmark = pytest.mark.gpu
DEV = "cuda"
GB = [[-1.1, 1.1]]


def _grid(d, g):
    from online_gp_amd import grid_ops

    return grid_ops.GridSpec(torch.tensor(GB * d), g)


def _interior(rng, n, d, lo=-0.9, hi=0.9):
    return torch.as_tensor(rng.uniform(lo, hi, (n, d)), device=DEV, dtype=torch.float64)


def _cd(f, x, eps):
    """Central differences of the scalar-per-point function f(x) -> [n] w.r.t. every coordinate (the points are independent)."""
    out = torch.empty_like(x)
    for q in range(x.shape[1]):
        xp, xm = x.clone(), x.clone()
        xp[:, q] += eps
        xm[:, q] -= eps
        out[:, q] = (f(xp) - f(xm)) / (2 * eps)
    return out


# --------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("d,g,ncols", [(2, 12, 5), (3, 9, 70), (2, 10, 300), (1, 20, 3)])
def test_gather_rows_vjp_against_central_differences(d, g, ncols):
    from online_gp_amd import grid_ops

    rng = np.random.default_rng(d * 100 + ncols)
    grid = _grid(d, g)
    x = _interior(rng, 97, d)
    Vr = torch.as_tensor(rng.standard_normal((grid.m, ncols)), device=DEV)
    G = torch.as_tensor(rng.standard_normal((97, ncols)), device=DEV)
    err = grid_ops.new_err_flag(DEV)
    gx = grid_ops.gather_rows_vjp(grid, x, Vr, G)
    ref = _cd(lambda xx: (grid_ops.gather_rows(grid, xx, Vr, err) * G).sum(1), x, 1e-6)
    assert (gx - ref).abs().max() < 1e-7 * max(1.0, float(ref.abs().max()))
    # the autograd Function runs the same kernel
    xg = x.clone().requires_grad_(True)
    (grid_ops.GatherRows.apply(grid, xg, Vr, err) * G).sum().backward()
    assert torch.equal(xg.grad, gx)


def test_gather_rows_vjp_with_one_column_is_the_gather_gradient():
    from online_gp_amd import grid_ops

    rng = np.random.default_rng(5)
    grid = _grid(3, 10)
    x = _interior(rng, 200, 3)
    v = torch.as_tensor(rng.standard_normal(grid.m), device=DEV)
    g = torch.as_tensor(rng.standard_normal(200), device=DEV)
    a = grid_ops.gather_rows_vjp(grid, x, v[:, None], g[:, None])
    b = grid_ops.gather_grad(grid, x, v) * g[:, None]
    assert (a - b).abs().max() < 1e-12 * float(b.abs().max())


def _basis_case(rng, d, g, kmax, r):
    from oracle import spec

    grid = _grid(d, g)
    cols = spec.toeplitz_columns("rbf", np.array(grid.h), np.array(grid.g), 0.5, 0.8)
    Vs = []
    for c in cols:
        idx = np.abs(np.arange(len(c))[:, None] - np.arange(len(c))[None, :])
        _, V = np.linalg.eigh(c[idx])
        Vs.append(V[:, ::-1][:, :kmax].copy())
    Vtab = torch.as_tensor(np.concatenate([V.reshape(-1) for V in Vs]), device=DEV)
    S = torch.as_tensor(rng.integers(0, kmax, (d, r)).astype(np.int32), device=DEV)
    tcol = torch.as_tensor(np.concatenate(cols), device=DEV)
    cs = torch.as_tensor(rng.uniform(0.5, 2, r), device=DEV)
    return grid, Vtab, S, tcol, cs


@pytest.mark.parametrize("d,n", [(2, 16), (3, 16), (2, 300), (3, 300)])
def test_basis_project_vjp_against_central_differences(d, n):
    """n = 16, r = 200: the few-points launch (four waves share a point); n = 300: one wave per point."""
    from online_gp_amd import grid_ops

    rng = np.random.default_rng(d * 7 + n)
    kmax, r = 8, 200
    grid, Vtab, S, tcol, cs = _basis_case(rng, d, 12, kmax, r)
    x = _interior(rng, n, d)
    GF = torch.as_tensor(rng.standard_normal((n, r)), device=DEV)
    Gp = torch.as_tensor(rng.standard_normal(n), device=DEV)
    gx = grid_ops.basis_project_vjp(grid, x, Vtab, kmax, S, GF, Gp, colscale=cs, tcol=tcol)

    def f(xx):
        F, pr = grid_ops.basis_project(grid, xx, Vtab, kmax, S, colscale=cs, tcol=tcol, want_prior=True)
        return (F * GF).sum(1) + pr * Gp

    ref = _cd(f, x, 1e-6)
    assert (gx - ref).abs().max() < 1e-7 * max(1.0, float(ref.abs().max()))
    # deterministic: the same bits twice
    assert torch.equal(gx, grid_ops.basis_project_vjp(grid, x, Vtab, kmax, S, GF, Gp, colscale=cs, tcol=tcol))
    # F alone (no prior gradient), and the autograd Function
    gxF = grid_ops.basis_project_vjp(grid, x, Vtab, kmax, S, GF, None, colscale=cs, tcol=tcol)
    refF = _cd(lambda xx: (grid_ops.basis_project(grid, xx, Vtab, kmax, S, colscale=cs) * GF).sum(1), x, 1e-6)
    assert (gxF - refF).abs().max() < 1e-7 * max(1.0, float(refF.abs().max()))
    xg = x.clone().requires_grad_(True)
    F, pr = grid_ops.BasisProject.apply(grid, xg, Vtab, kmax, S, cs, tcol, None)
    ((F * GF).sum() + (pr * Gp).sum()).backward()
    assert torch.equal(xg.grad, gx)


def test_vjps_are_zero_in_one_hot_boundary_cells():
    from online_gp_amd import grid_ops

    rng = np.random.default_rng(3)
    grid, Vtab, S, tcol, cs = _basis_case(rng, 2, 12, 6, 40)
    x = _interior(rng, 8, 2)
    x[:4, 0] = grid.g0[0] + 0.5 * grid.h[0]                   # first cell of dim 0: one-hot stencil
    x[4:, 1] = grid.g0[1] + grid.h[1] * (grid.g[1] - 1.5)     # last cell of dim 1
    Vr = torch.as_tensor(rng.standard_normal((grid.m, 7)), device=DEV)
    G = torch.as_tensor(rng.standard_normal((8, 7)), device=DEV)
    a = grid_ops.gather_rows_vjp(grid, x, Vr, G)
    GF = torch.as_tensor(rng.standard_normal((8, 40)), device=DEV)
    b = grid_ops.basis_project_vjp(grid, x, Vtab, 6, S, GF, torch.ones(8, device=DEV, dtype=torch.float64), colscale=cs, tcol=tcol)
    for t in (a, b):
        assert bool((t[:4, 0] == 0).all()) and bool((t[4:, 1] == 0).all())
        assert bool((t[:4, 1] != 0).all()) and bool((t[4:, 0] != 0).all())


def test_vjp_entry_points_take_n_zero_and_refuse_bad_arguments():
    from online_gp_amd import _hip, grid_ops

    grid = _grid(2, 10)
    x0 = torch.empty((0, 2), device=DEV, dtype=torch.float64)
    Vr = torch.zeros((grid.m, 3), device=DEV, dtype=torch.float64)
    assert grid_ops.gather_rows_vjp(grid, x0, Vr, torch.empty((0, 3), device=DEV, dtype=torch.float64)).shape == (0, 2)
    rng = np.random.default_rng(0)
    _, Vtab, S, tcol, cs = _basis_case(rng, 2, 10, 4, 9)
    assert grid_ops.basis_project_vjp(grid, x0, Vtab, 4, S, torch.empty((0, 9), device=DEV, dtype=torch.float64)).shape == (0, 2)
    lib, s = _hip.lib(), _hip.stream_ptr(torch.device(DEV))
    x = torch.zeros((4, 2), device=DEV, dtype=torch.float64)
    gx = torch.empty((4, 2), device=DEV, dtype=torch.float64)
    G = torch.zeros((4, 3), device=DEV, dtype=torch.float64)
    bad = -1
    f = lib.wiski_gather_rows_vjp_f64
    assert f(grid.ref, _hip.dptr(x), ctypes.c_int64(4), None, ctypes.c_int32(3), _hip.dptr(G), _hip.dptr(gx), s) == bad
    assert f(grid.ref, _hip.dptr(x), ctypes.c_int64(4), _hip.dptr(Vr), ctypes.c_int32(0), _hip.dptr(G), _hip.dptr(gx), s) == bad
    assert f(None, _hip.dptr(x), ctypes.c_int64(4), _hip.dptr(Vr), ctypes.c_int32(3), _hip.dptr(G), _hip.dptr(gx), s) == bad
    GF = torch.zeros((4, 9), device=DEV, dtype=torch.float64)
    Gp = torch.zeros(4, device=DEV, dtype=torch.float64)
    h = lib.wiski_basis_project_vjp_f64
    args = lambda kmax, ldg, gp, tc, gf: (grid.ref, _hip.dptr(x), ctypes.c_int64(4), _hip.dptr(Vtab), ctypes.c_int32(kmax), _hip.dptr(S), ctypes.c_int32(9),
                                          None, _hip.dptr(cs), tc, gf, ctypes.c_int64(ldg), gp, _hip.dptr(gx), s)
    assert h(*args(4, 9, _hip.dptr(Gp), None, _hip.dptr(GF))) == bad           # a prior gradient needs the Toeplitz columns
    assert h(*args(4, 8, None, None, _hip.dptr(GF))) == bad                     # ldg < r
    assert h(*args(33, 9, None, None, _hip.dptr(GF))) == bad                    # kmax > 32
    assert h(*args(4, 9, None, None, None)) == bad
    assert h(*args(4, 9, _hip.dptr(Gp), _hip.dptr(tcol), _hip.dptr(GF))) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------- model
def _fit_data(rng, n, d, out=1):
    X = rng.uniform(-1, 1, (n, d))
    y = np.sin(2 * X.sum(1, keepdims=True)) + np.cos(3 * X[:, :1]) * np.arange(1, out + 1)[None, :] / out + 0.05 * rng.standard_normal((n, out))
    nz = rng.uniform(0.5, 1.5, (n, out))
    return X, y, nz


def _model(X, y, nz, g, dtype=torch.float64, kind="rbf", ell=0.5):
    from online_gp_amd.kernels import GridInterpolationKernel, MaternKernel, RBFKernel, ScaleKernel
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    d = X.shape[1]
    t = lambda a: torch.as_tensor(a, device=DEV, dtype=dtype)
    if y.shape[1] > 1:
        m = FixedNoiseOnlineSKIGP(t(X), t(y), t(nz), grid_bounds=torch.tensor(GB * d), grid_size=g, learn_additional_noise=True)
    else:
        base = RBFKernel(ard_num_dims=d) if kind == "rbf" else MaternKernel(nu=0.5, ard_num_dims=d)
        cov = GridInterpolationKernel(ScaleKernel(base), grid_size=g, num_dims=d, grid_bounds=torch.tensor(GB * d))
        cov.base_kernel.base_kernel.lengthscale = torch.full((d,), float(ell))
        m = FixedNoiseOnlineSKIGP(t(X), t(y), t(nz), covar_module=cov, learn_additional_noise=True)
    m.likelihood.second_noise = 0.05
    return m.eval()


def _moments(m, X, q, A, B, C, Z):
    """A scalar of every moment the acquisition functions read: weighted mean and variance of the flat points, a q-block
    covariance of X [b, q, d] and fixed-sample draws."""
    flat = X.reshape(-1, X.shape[-1])
    mvn = m(flat)
    val = (mvn.mean * A).sum() + (mvn.variance * B).sum()
    mb = m(X.reshape(-1, q, X.shape[-1]))
    val = val + (mb.covariance_matrix * C).sum()
    val = val + (mb.rsample(torch.Size([Z.shape[0]]), base_samples=Z) * Z).sum()
    return val


def _grad_and_cd(m, X, q, eps=1e-5, seed=0):
    rng = np.random.default_rng(seed)
    mvn = m(X)
    t = lambda s: torch.as_tensor(rng.standard_normal(s), device=DEV, dtype=torch.float64)
    A, B = t(tuple(mvn.mean.shape)), t(tuple(mvn.mean.shape))
    nb = X.shape[0] // q
    lead = (nb, q) if m.num_outputs == 1 else (m.num_outputs, nb, q)
    C, Z = t(lead + (q,)), t((3,) + lead)
    A, B, C, Z = (v.to(X.dtype) for v in (A, B, C, Z))
    Xg = X.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(_moments(m, Xg, q, A, B, C, Z), Xg)
    cd = torch.empty_like(X, dtype=torch.float64)
    with torch.no_grad():
        for i in range(X.shape[0]):
            for k in range(X.shape[1]):
                xp, xm = X.clone(), X.clone()
                xp[i, k] += eps
                xm[i, k] -= eps
                cd[i, k] = (_moments(m, xp, q, A, B, C, Z) - _moments(m, xm, q, A, B, C, Z)).double() / (2 * eps)
    return g.double(), cd, (A, B, C, Z)


def _oracle_cd(m, X, y, nz, Xq, q, A, B, C, kind, g, eps=1e-5):
    """The mean / variance / q-block parts of _moments from the data-space oracle at the model's hyper-parameters."""
    k = m.covar_module.base_kernel
    ell = k.base_kernel.lengthscale.detach().cpu().numpy().reshape(-1)
    O = dataspace.DataSpaceGP(GB * X.shape[1], g, kind, ell, float(k.outputscale), float(m.likelihood.second_noise)).fit(X, y[:, 0], nz[:, 0])
    a, b, c = A.cpu().numpy(), B.cpu().numpy(), C.cpu().numpy()

    def f(x):
        mo, co = O.predict(x, full_cov=True)
        v = (a * mo).sum() + (b * np.diag(co)).sum()
        for bi in range(x.shape[0] // q):
            v += (c[bi] * co[bi * q:(bi + 1) * q, bi * q:(bi + 1) * q]).sum()
        return v

    x0 = Xq.cpu().numpy()
    out = np.empty_like(x0)
    for i in range(x0.shape[0]):
        for kk in range(x0.shape[1]):
            xp, xm = x0.copy(), x0.copy()
            xp[i, kk] += eps
            xm[i, kk] -= eps
            out[i, kk] = (f(xp) - f(xm)) / (2 * eps)
    return out


def _grad_no_draws(m, Xq, q, A, B, C):
    Xg = Xq.clone().requires_grad_(True)
    mvn = m(Xg)
    val = (mvn.mean * A).sum() + (mvn.variance * B).sum() + (m(Xg.reshape(-1, q, Xg.shape[-1])).covariance_matrix * C).sum()
    (gx,) = torch.autograd.grad(val, Xg)
    return gx.double().cpu().numpy()


@pytest.mark.parametrize("g", [16, 30])
def test_dense_regime_gradients(g):
    from online_gp_amd import settings

    rng = np.random.default_rng(g)
    X, y, nz = _fit_data(rng, 300, 2)
    m = _model(X, y, nz, g)
    Xq = _interior(rng, 8, 2)
    gx, cd, (A, B, C, Z) = _grad_and_cd(m, Xq, 4)
    assert hasattr(m.prediction_cache["pred_cov"], "dense")
    err = float((gx - cd).abs().max() / cd.abs().max())
    print(f"MEASURED dense {g}^2 model-vs-fd {err:.2e}")
    assert err < 1e-6
    oc = _oracle_cd(m, X, y, nz, Xq, 4, A, B, C, "rbf", g)
    ge = _grad_no_draws(m, Xq, 4, A, B, C)
    oerr = np.abs(ge - oc).max() / np.abs(oc).max()
    print(f"MEASURED dense {g}^2 model-vs-oracle {oerr:.2e}")
    assert oerr < 1e-5
    # the root of fast_pred_samples: R = s W* L_M
    with settings.fast_pred_samples(True):
        Xg = Xq.clone().requires_grad_(True)
        R = m(Xg).lazy_covariance_matrix.root                 # (fast_pred_samples: the model hands out the root form)
        W = torch.as_tensor(rng.standard_normal(tuple(R.shape)), device=DEV)
        (gr,) = torch.autograd.grad((R * W).sum(), Xg)
        with torch.no_grad():
            fr = lambda xx: (m(xx).lazy_covariance_matrix.root * W).sum()
            cdr = torch.empty_like(Xq)
            for i in range(Xq.shape[0]):
                for k in range(2):
                    xp, xm = Xq.clone(), Xq.clone()
                    xp[i, k] += 1e-6
                    xm[i, k] -= 1e-6
                    cdr[i, k] = (fr(xp) - fr(xm)) / 2e-6
        assert float((gr - cdr).abs().max() / cdr.abs().max()) < 1e-6


def test_spectral_regime_gradients_at_50pow3():
    from online_gp_amd import settings

    rng = np.random.default_rng(50)
    X, y, nz = _fit_data(rng, 400, 3)
    m = _model(X, y, nz, 50, ell=0.6)
    Xq = _interior(rng, 6, 3)
    gx, cd, (A, B, C, Z) = _grad_and_cd(m, Xq, 3)
    fac = m._spectral[0]
    assert fac.cur is not None
    err = float((gx - cd).abs().max() / cd.abs().max())
    print(f"MEASURED spectral 50^3 model-vs-fd {err:.2e} (rel bound {fac.rel_bound():.1e})")
    assert err < 1e-5
    oc = _oracle_cd(m, X, y, nz, Xq, 3, A, B, C, "rbf", 50)
    ge = _grad_no_draws(m, Xq, 3, A, B, C)
    oerr = np.abs(ge - oc).max() / np.abs(oc).max()
    print(f"MEASURED spectral 50^3 model-vs-oracle {oerr:.2e}")
    assert oerr < max(1e-4, 1e3 * fac.rel_bound())
    # the root the spectral factor hands to fast_pred_samples, and its diagonal term
    with settings.fast_pred_samples(True):
        Xg = Xq.clone().requires_grad_(True)
        rt = m(Xg).lazy_covariance_matrix.root_decomposition()
        W = torch.as_tensor(rng.standard_normal(tuple(rt.root.shape)), device=DEV)
        (gr,) = torch.autograd.grad((rt.root * W).sum() + rt.extra.sum(), Xg)
        with torch.no_grad():
            def fr(xx):
                r2 = m(xx).lazy_covariance_matrix.root_decomposition()
                return (r2.root * W).sum() + r2.extra.sum()
            cdr = torch.empty_like(Xq)
            for i in range(Xq.shape[0]):
                for k in range(3):
                    xp, xm = Xq.clone(), Xq.clone()
                    xp[i, k] += 1e-6
                    xm[i, k] -= 1e-6
                    cdr[i, k] = (fr(xp) - fr(xm)) / 2e-6
        assert float((gr - cdr).abs().max() / cdr.abs().max()) < 1e-5


def test_pcg_regime_gradients():
    from online_gp_amd import settings

    rng = np.random.default_rng(14)
    X, y, nz = _fit_data(rng, 300, 3)
    with settings.spectral_factor(False), settings.cg_tolerance(1e-11), settings.variance_cg_tolerance(None):
        m = _model(X, y, nz, 14, kind="matern12", ell=0.8)
        assert m._grid.m > settings.max_cholesky_size.value()
        Xq = _interior(rng, 6, 3)
        gx, cd, (A, B, C, Z) = _grad_and_cd(m, Xq, 3, eps=1e-5)
        err = float((gx - cd).abs().max() / cd.abs().max())
        print(f"MEASURED pcg 14^3 model-vs-fd {err:.2e}")
        assert err < 1e-5
        oc = _oracle_cd(m, X, y, nz, Xq, 3, A, B, C, "matern12", 14)
        ge = _grad_no_draws(m, Xq, 3, A, B, C)
        oerr = np.abs(ge - oc).max() / np.abs(oc).max()
        print(f"MEASURED pcg 14^3 model-vs-oracle {oerr:.2e}")
        assert oerr < 1e-4
        # over the memory cap the backward solves again: the same gradient
        from online_gp_amd.lazy.operators import PredictiveCovariance

        keep = PredictiveCovariance.grad_keep_bytes
        PredictiveCovariance.grad_keep_bytes = 0
        try:
            ge2 = _grad_no_draws(m, Xq, 3, A, B, C)
        finally:
            PredictiveCovariance.grad_keep_bytes = keep
        assert np.abs(ge2 - ge).max() < 1e-8 * np.abs(ge).max()


def test_two_outputs_and_fp32():
    rng = np.random.default_rng(2)
    X, y, nz = _fit_data(rng, 250, 2, out=2)
    m = _model(X, y, nz, 16)
    Xq = _interior(rng, 6, 2)
    gx, cd, _ = _grad_and_cd(m, Xq, 3)
    assert float((gx - cd).abs().max() / cd.abs().max()) < 1e-6
    # fp32 model against the fp64 gradient of the same data
    X1, y1, nz1 = _fit_data(rng, 250, 2)
    m64, m32 = _model(X1, y1, nz1, 16), _model(X1, y1, nz1, 16, dtype=torch.float32)
    Xq = _interior(rng, 6, 2)
    r = np.random.default_rng(9)
    A = torch.as_tensor(r.standard_normal(6), device=DEV)
    B = torch.as_tensor(r.standard_normal(6), device=DEV)
    C = torch.as_tensor(r.standard_normal((2, 3, 3)), device=DEV)
    g64 = _grad_no_draws(m64, Xq, 3, A, B, C)
    g32 = _grad_no_draws(m32, Xq.float(), 3, A.float(), B.float(), C.float())
    dev = np.abs(g32 - g64).max() / np.abs(g64).max()
    print(f"MEASURED fp32-vs-fp64 gradient {dev:.2e}")
    assert dev < 6e-6                                         # ~3x the measured 1.1e-6 .. 1.8e-6 (run to run)


def test_values_without_gradients_are_bitwise_the_same_and_detach_interp_coeff():
    from online_gp_amd import settings

    rng = np.random.default_rng(4)
    X, y, nz = _fit_data(rng, 200, 2)
    for g, kw in ((16, {}), (50, {})):
        m = _model(X, y, nz, g)
        Xq = _interior(rng, 12, 2)
        Xb = Xq.reshape(4, 3, 2)
        plain = m(Xq)
        with torch.no_grad():
            ng = m(Xq)
        Xg = Xq.clone().requires_grad_(True)
        gr = m(Xg)
        assert gr.mean.grad_fn is not None and gr.variance.grad_fn is not None
        for a in (plain, ng):
            assert torch.equal(a.mean, gr.mean.detach()) and torch.equal(a.variance, gr.variance.detach())
        cb = m(Xb).covariance_matrix
        cbg = m(Xb.clone().requires_grad_(True)).covariance_matrix
        assert torch.equal(cb, cbg.detach())
        with settings.detach_interp_coeff(True):
            Xg = Xq.clone().requires_grad_(True)
            mv = m(Xg)
            assert mv.variance.grad_fn is None
            (gm,) = torch.autograd.grad(mv.mean.sum() + mv.variance.sum(), Xg)
            (gm2,) = torch.autograd.grad(m(Xg).mean.sum(), Xg)
            assert torch.equal(gm, gm2) and float(gm.abs().sum()) > 0


def test_botorch_rsample_with_base_samples_is_deterministic_and_differentiable():
    from online_gp_amd.models import OnlineSKIBotorchModel

    rng = np.random.default_rng(6)
    X, y, _ = _fit_data(rng, 200, 2)
    m = OnlineSKIBotorchModel(torch.as_tensor(X, device=DEV), torch.as_tensor(y, device=DEV), None, grid_bounds=torch.tensor(GB * 2), grid_size=16,
                              learn_additional_noise=True)
    m.eval()
    Xq = _interior(rng, 8, 2).reshape(4, 2, 2).requires_grad_(True)
    z = torch.randn((5, 4, 2, 1), generator=torch.Generator().manual_seed(0), dtype=torch.float64).to(DEV)
    s1 = m.posterior(Xq).rsample(torch.Size([5]), base_samples=z)
    s2 = m.posterior(Xq).rsample(torch.Size([5]), base_samples=z)
    assert s1.shape == (5, 4, 2, 1) and torch.equal(s1, s2)
    (gx,) = torch.autograd.grad(s1.sum(), Xq)
    assert bool(torch.isfinite(gx).all()) and float(gx.abs().sum()) > 0
    s3 = m.posterior(Xq).rsample(torch.Size([5]), base_samples=2 * z)
    assert not torch.equal(s1, s3)


def _bo_model(rng):
    from online_gp_amd.models import OnlineSKIBotorchModel
    from online_gp_amd import harness

    X = rng.uniform(0, 1, (40, 2))
    y = -((X - 0.6) ** 2).sum(1, keepdims=True) * 4 + 0.05 * rng.standard_normal((40, 1))
    m = OnlineSKIBotorchModel(torch.as_tensor(X, device=DEV), torch.as_tensor(y, device=DEV), None, grid_bounds=torch.tensor([[-0.2, 1.2]] * 2),
                              grid_size=20, learn_additional_noise=True)
    harness.fit_mll(m, 10)
    return m, y


@pytest.mark.parametrize("acqf,q", [("ucb", 1), ("qei", 3)])
def test_optimize_acqf_on_a_fitted_model(acqf, q):
    from online_gp_amd import harness

    rng = np.random.default_rng(8)
    m, y = _bo_model(rng)
    bounds = torch.tensor([[0.0, 0.0], [1.0, 1.0]], dtype=torch.float64)
    best_f = float(y.max())
    X, v = harness.optimize_acqf(m, acqf, bounds, q, num_restarts=4, raw_samples=64, maxiter=200, seed=3, best_f=best_f, num_mc_samples=64)
    assert X.shape == (q, 2) and bool((X >= 0).all()) and bool((X <= 1).all())
    g = torch.Generator().manual_seed(3)
    raw = torch.rand((64, q, 2), generator=g, dtype=torch.float64).to(DEV)
    base = torch.randn((64, q), generator=g, dtype=torch.float64).to(DEV)
    with torch.no_grad():
        best_raw = harness.acqf_values(m, raw, acqf, best_f=best_f, base_samples=base).max()
    assert float(v) >= float(best_raw)
    # projected gradient at the returned point: ~0 in the interior coordinates
    Xg = X[None].clone().requires_grad_(True)
    (gx,) = torch.autograd.grad(harness.acqf_values(m, Xg, acqf, best_f=best_f, base_samples=base).sum(), Xg)
    inner = (Xg.detach() > 1e-3) & (Xg.detach() < 1 - 1e-3)
    gmax = float(gx[inner].abs().max()) if bool(inner.any()) else 0.0
    print(f"MEASURED optimize_acqf {acqf} q={q}: value {float(v):.4e}, interior |grad| {gmax:.2e}")
    assert gmax < 1e-2 * (1.0 + abs(float(v)))


def test_bayesopt_with_the_gradient_optimizer():
    from online_gp_amd import harness
    from online_gp_amd.models import OnlineSKIBotorchModel

    d = 3
    bounds = torch.tensor([[-32.768, 32.768]] * d, dtype=torch.float64)
    gen = torch.Generator().manual_seed(0)
    init_x = torch.rand(10, d, generator=gen, dtype=torch.float64).to(DEV)

    def fn(Xr):
        a = -20 * torch.exp(-0.2 * torch.sqrt((Xr ** 2).mean(-1))) - torch.exp(torch.cos(2 * np.pi * Xr).mean(-1)) + 20 + np.e
        return -a

    init_y = fn(bounds[:, 0].to(DEV) + (bounds[:, 1] - bounds[:, 0]).to(DEV) * init_x).reshape(-1, 1)

    def make_model(train_x, train_y, old):
        if old is None:
            return OnlineSKIBotorchModel(train_x, train_y, None, grid_bounds=bounds, grid_size=10, learn_additional_noise=True)
        return OnlineSKIBotorchModel(covar_module=old.covar_module, kernel_cache=old._kernel_cache, learn_additional_noise=True,
                                     likelihood=old.likelihood, num_data=old.num_data)

    rows, tx, ty, _ = harness.bayesopt(fn, bounds, make_model, init_x, init_y, num_steps=3, batch_size=3, fit_iters=3, num_candidates=64,
                                       acqf_optimizer="gradient", num_restarts=3, maxiter=10)
    assert len(rows) == 3 and tx.shape == (19, d)
    assert bool((tx >= 0).all()) and bool((tx <= 1).all())
    for r in rows:
        assert set(r) == {"step", "fit_time", "acqf_time", "condition_time", "total", "max_achieved"}
