"""Host: the periodic, rational-quadratic, product and separable kernels (online_gp_amd/kernels.py) on the CPU op graph
against the closed forms of tests/kernel_family_reference.py, and that reference against its own mpmath form at 40 digits.

Bounds.  numpy against mpmath: 1e-13 relative to max(1, max |ref|), on cases with (g - 1) h / p <= 10 and ell >= 0.3 (the argument of the
sine is at most 10 pi, the exponent at most 2 / 0.09: a few hundred ulp of 1.1e-16 at the worst).  The op graph against numpy, fp64:
1e-12 for values and 1e-10 for gradients, the fp64 bounds of the existing fused-columns test."""
import numpy as np
import pytest
import torch

import kernel_family_reference as kr
from online_gp_amd import kernels as K

CASES = kr.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_numpy_reference_agrees_with_mpmath(case):
    _, bounds, g, terms, theta, S = case
    h = kr.grid_steps(bounds, g)
    assert all(ell >= 0.3 for ell in (theta[t[2]] for t in terms))
    assert all((g[t[0]] - 1) * h[t[0]] / theta[t[3]] <= 10 for t in terms if t[1] == 4)
    got, want = kr.columns(g, h, terms, theta, S), kr.columns_mp(g, h, terms, theta, S)
    for a, b, what in zip(got, want, ("values", "d theta", "d S")):
        e = kr.err(a, b)
        print(case[0], what, e)
        assert e < 1e-13, (what, e)


def test_rq_with_large_alpha_is_the_rbf_column():
    """alpha = 1e4: |RQ - RBF| <= x^2 / (2 alpha) e^-x-ish < 2 / alpha for every lag."""
    _, bounds, g, terms, theta, S = next(c for c in CASES if c[0] == "rq_large_alpha")
    h = kr.grid_steps(bounds, g)
    rq = kr.columns(g, h, terms, theta, S)[0]
    rbf = kr.columns(g, h, [(0, 0, 0, -1)], theta[:1], S)[0]
    assert np.abs(rq - rbf).max() < 2.0 / theta[1]


def _randomise(kernel, seed):
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in kernel.parameters():
            p.add_(torch.randn(p.shape, generator=gen, dtype=p.dtype) * 0.3)


def _configs():
    """name -> (kernel, bounds, g, terms, slots): terms over theta, slots[i] = (raw parameter, flat element) behind theta[i]."""
    b4, g4 = [[-1.0, 1.0 + 0.3 * q] for q in range(4)], [9, 12, 7, 6]
    out = {}
    per, rbf, rq, mat = K.PeriodicKernel(), K.RBFKernel(), K.RQKernel(), K.MaternKernel(nu=2.5)
    sep = K.SeparableKernel([K.ProductKernel(per, rbf), rq, mat])
    out["scale_separable"] = (K.ScaleKernel(sep), b4[:3], g4[:3], [(0, 4, 0, 1), (0, 0, 2, -1), (1, 5, 3, 4), (2, 3, 5, -1)],
                              [(per.raw_lengthscale, 0), (per.raw_period_length, 0), (rbf.raw_lengthscale, 0), (rq.raw_lengthscale, 0), (rq.raw_alpha, 0),
                               (mat.raw_lengthscale, 0)])
    per = K.PeriodicKernel(ard_num_dims=2)
    out["periodic_ard"] = (per, b4[:2], g4[:2], [(0, 4, 0, 2), (1, 4, 1, 3)],
                           [(per.raw_lengthscale, 0), (per.raw_lengthscale, 1), (per.raw_period_length, 0), (per.raw_period_length, 1)])
    rq = K.RQKernel(ard_num_dims=2)
    out["scale_rq_ard"] = (K.ScaleKernel(K.ScaleKernel(rq)), b4[:2], g4[:2], [(0, 5, 0, 2), (1, 5, 1, 2)],
                           [(rq.raw_lengthscale, 0), (rq.raw_lengthscale, 1), (rq.raw_alpha, 0)])
    per, rbf = K.PeriodicKernel(), K.RBFKernel(ard_num_dims=2)
    out["locally_periodic"] = (K.ProductKernel(per, rbf), b4[:2], g4[:2], [(0, 4, 0, 1), (0, 0, 2, -1), (1, 4, 0, 1), (1, 0, 3, -1)],
                               [(per.raw_lengthscale, 0), (per.raw_period_length, 0), (rbf.raw_lengthscale, 0), (rbf.raw_lengthscale, 1)])
    return out


CONFIGS = _configs()


def _scales(kernel):
    out = []
    while isinstance(kernel, K.ScaleKernel):
        out.append(kernel.raw_outputscale)
        kernel = kernel.base_kernel
    return out


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_op_graph_columns_and_gradients_equal_the_reference(name):
    kernel, bounds, g, terms, slots = CONFIGS[name]
    kernel = kernel.double()
    _randomise(kernel, len(name))
    gk = K.GridInterpolationKernel(kernel, grid_size=g, num_dims=len(g), grid_bounds=bounds)
    h = gk.grid_spec.h
    assert h == kr.grid_steps(bounds, g)
    theta = [float(kr.softplus(raw.detach().reshape(-1)[i].item())) for raw, i in slots]
    scales = _scales(kernel)
    S = float(np.prod([kr.softplus(s.item()) for s in scales])) if scales else 1.0
    ref, dth, dS = kr.columns(g, h, terms, theta, S)
    # lag_column per dimension, lag_columns_cat through the grid wrapper
    per_dim = torch.cat([kernel.lag_column(q, h[q] * torch.arange(g[q], dtype=torch.float64)) for q in range(len(g))])
    for p in gk.parameters():
        p.grad = None
    cols = gk.toeplitz_columns()
    assert cols.dtype == torch.float64 and cols.shape == (sum(g),)
    for got in (per_dim, cols):
        assert kr.err(got.detach().numpy(), ref) < 1e-12
    w = torch.randn(sum(g), dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    (cols * w).sum().backward()
    wn = w.numpy()
    want = {}
    for (raw, i), row in zip(slots, dth):
        want.setdefault(id(raw), np.zeros(raw.numel()))[i] += (wn @ row) * kr.softplus_grad(raw.detach().reshape(-1)[i].item())
    for s in scales:
        want[id(s)] = np.array([(wn @ dS) * S / kr.softplus(s.item()) * kr.softplus_grad(s.item())])
    seen = 0
    for p in gk.parameters():
        assert id(p) in want, "a parameter the reference does not know"
        assert kr.err(p.grad.reshape(-1).numpy(), want[id(p)]) < 1e-10
        seen += 1
    assert seen == len(want)


def test_the_mutant_references_are_told_apart_by_the_bounds():
    """ell in place of ell^2 in the periodic profile, and the alpha-derivative of RQ without its log1p term: each misses the bound
    that the true forms keep, against mpmath and against the classes."""
    for name, mutant, part in (("one_periodic", "ell_not_squared", 0), ("rq_small_alpha", "alpha_no_log1p", 1)):
        _, bounds, g, terms, theta, S = next(c for c in CASES if c[0] == name)
        h = kr.grid_steps(bounds, g)
        good, bad, mp = kr.columns(g, h, terms, theta, S), kr.columns(g, h, terms, theta, S, mutant=mutant), kr.columns_mp(g, h, terms, theta, S)
        assert kr.err(good[part], mp[part]) < 1e-13
        assert kr.err(bad[part], mp[part]) > 1e-3
    per = K.PeriodicKernel().double()
    lags = 0.2 * torch.arange(6, dtype=torch.float64)
    ell, p = float(per.lengthscale), float(per.period_length)
    bad = kr.columns([6], [0.2], [(0, 4, 0, 1)], [ell, p], mutant="ell_not_squared")[0]
    assert kr.err(per.lag_column(0, lags).detach().numpy(), bad) > 1e-3


@pytest.mark.parametrize("d", [1, 3])
def test_separable_of_tied_rbf_factors_is_the_rbf_kernel(d):
    g, bounds = [9, 12, 7][:d], [[-1.0, 1.0 + 0.3 * q] for q in range(d)]
    one, plain = K.RBFKernel(), K.RBFKernel()
    with torch.no_grad():
        one.raw_lengthscale.fill_(0.37)
        plain.raw_lengthscale.fill_(0.37)
    a = K.GridInterpolationKernel(K.SeparableKernel([one] * d), grid_size=g, num_dims=d, grid_bounds=bounds).toeplitz_columns()
    b = K.GridInterpolationKernel(plain, grid_size=g, num_dims=d, grid_bounds=bounds).toeplitz_columns()
    assert torch.equal(a, b)
    assert len(list(K.SeparableKernel([one] * d).parameters())) == 1


def test_batch_index_selects_the_hyper_parameters_of_one_output():
    per = K.PeriodicKernel(batch_shape=torch.Size([2])).double()
    rq = K.RQKernel(batch_shape=torch.Size([2])).double()
    _randomise(per, 1)
    _randomise(rq, 2)
    lags = 0.3 * torch.arange(5, dtype=torch.float64)
    for o in range(2):
        ell, p = per.lengthscale[o].item(), per.period_length[o].item()
        assert kr.err(per.lag_column(0, lags, o).detach().numpy(), kr.columns([5], [0.3], [(0, 4, 0, 1)], [ell, p])[0]) < 1e-12
        ell, a = rq.lengthscale[o].item(), rq.alpha[o].item()
        assert kr.err(rq.lag_column(0, lags, o).detach().numpy(), kr.columns([5], [0.3], [(0, 5, 0, 1)], [ell, a])[0]) < 1e-12


def test_constructor_errors_and_setters():
    with pytest.raises(TypeError):
        K.PeriodicKernel(active_dims=[0])
    with pytest.raises(TypeError):
        K.RQKernel(nu=2.5)
    with pytest.raises(TypeError):
        K.ProductKernel(K.RBFKernel(), eps=1.0)
    with pytest.raises(TypeError):
        K.SeparableKernel([K.RBFKernel(ard_num_dims=2)])
    with pytest.raises(TypeError):
        K.SeparableKernel([K.SpectralMixtureKernel(num_mixtures=2)])
    with pytest.raises(ValueError):
        K.GridInterpolationKernel(K.ScaleKernel(K.SeparableKernel([K.RBFKernel()] * 3)), grid_size=8, num_dims=2, grid_bounds=[[-1.0, 1.0]] * 2)
    with pytest.raises(ValueError):                   # (also where the SeparableKernel stands inside a ProductKernel)
        K.GridInterpolationKernel(K.ProductKernel(K.SeparableKernel([K.RBFKernel()] * 3), K.RBFKernel()), grid_size=8, num_dims=2, grid_bounds=[[-1.0, 1.0]] * 2)
    per, rq = K.PeriodicKernel(ard_num_dims=2), K.RQKernel()
    assert per.raw_period_length.shape == (1, 2) and rq.raw_alpha.shape == (1,)
    assert float(per.period_length[0, 0]) == pytest.approx(np.log(2.0)) and float(rq.alpha) == pytest.approx(np.log(2.0))
    per.period_length = 0.25
    rq.alpha = 3.0
    rq.lengthscale = 0.5
    assert torch.allclose(per.period_length, torch.full((1, 2), 0.25)) and float(rq.alpha) == pytest.approx(3.0) and float(rq.lengthscale) == pytest.approx(0.5)
