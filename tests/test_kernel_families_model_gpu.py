"""GPU: models under the periodic / rational-quadratic / product / separable kernels, checked against the data-space
oracle (oracle.dataspace.DataSpaceGP) fed with the columns of tests/kernel_family_reference.py at the model's hyper-parameters.

Tolerances are those of the existing comparisons against that oracle in the same regime and dtype: dense regime fp64 1e-6
(tests/test_model_gpu.py), beyond it 1e-4 in fp64 and 1e-2 in fp32 (tests/test_spectral_gpu.py), the MLL value 1e-8 (ibid.).

There is no test of a captured hyper-parameter step with these kernels: GraphedHyperStep declines them; the op-by-op
step that runs instead is tested below."""
import contextlib

import numpy as np
import pytest
import torch

import kernel_family_reference as kr
from oracle import dataspace

pytestmark = pytest.mark.gpu
DEV = "cuda"
GB2, G2 = [[-1.0, 1.0]] * 2, [12, 10]
H2 = kr.grid_steps(GB2, G2)
P_STAR = 1.0                                          # period of the 1-D stream
GB1, G1 = [[-1.6, 1.6]], [64]


def _f(v):
    return float(v.detach().double().reshape(-1)[0])


def _cov2(period, product=True, dtype=torch.float64):
    """Scale(Separable([Product(Periodic, RBF) | Periodic, Matern-5/2])) with hyper-parameters in `dtype`."""
    from online_gp_amd import kernels as K

    per, rbf, mat = K.PeriodicKernel(), K.RBFKernel(), K.MaternKernel(nu=2.5)
    cov = K.ScaleKernel(K.SeparableKernel([K.ProductKernel(per, rbf) if product else per, mat])).to(dtype)
    per.period_length = period
    per.lengthscale = 1.3
    rbf.lengthscale = 0.9
    mat.lengthscale = 0.8
    cov.outputscale = 1.2
    return cov, (per, rbf, mat)


def _ref_cols2(cov, parts, product, g=G2, h=H2):
    per, rbf, mat = parts
    theta = [_f(per.lengthscale), _f(per.period_length), _f(rbf.lengthscale), _f(mat.lengthscale)]
    terms = [(0, 4, 0, 1)] + ([(0, 0, 2, -1)] if product else []) + [(1, 3, 3, -1)]
    out = kr.columns(g, h, terms, theta, _f(cov.outputscale))[0]
    return [out[:g[0]], out[g[0]:]]


def _data2(seed, n):
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.95, 0.95, (n, 2))
    y = np.sin(2 * np.pi * X[:, 0] / 0.96) * np.cos(X[:, 1]) + 0.05 * rng.standard_normal(n)
    return X, y, rng.uniform(-0.9, 0.9, (16, 2))


def _stream_model(cov, X, y, dtype, first):
    """A model on the first `first` points; the rest arrives in three condition_on_observations calls."""
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    Xt, yt = torch.as_tensor(X, device=DEV, dtype=dtype), torch.as_tensor(y, device=DEV, dtype=dtype)[:, None]
    m = FixedNoiseOnlineSKIGP(Xt[:first], yt[:first], None, covar_module=cov, grid_bounds=torch.tensor(GB2), grid_size=G2, learn_additional_noise=True)
    cuts = np.linspace(first, len(X), 4).astype(int)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        m.condition_on_observations(Xt[lo:hi], yt[lo:hi], torch.ones_like(yt[lo:hi]), inplace=True)
    return m, Xt, yt


@pytest.mark.parametrize("case", ["2.5_periods", "p_is_3h_product", "p_is_3h_rank_deficient"])
def test_dense_regime_matches_the_oracle(case):
    """Grid 12 x 10, 40 points, fp64: mean and variance at 16 queries and the MLL.  The grid of dimension 0 spans 11 h = 2.4: p = 0.96 is 2.5
    periods.  With p = 3 h exactly the periodic column repeats every three nodes, so a purely periodic factor has rank 3 of 12; under the product
    with an RBF profile the factor is positive definite again (a Hadamard product with a positive definite matrix), so both are run."""
    from online_gp_amd.mlls import BatchedWoodburyMarginalLogLikelihood

    product = case != "p_is_3h_rank_deficient"
    cov, parts = _cov2(0.96 if case == "2.5_periods" else 3.0 * H2[0], product)
    X, y, Xs = _data2(1, 40)
    m, Xt, yt = _stream_model(cov, X, y, torch.float64, 4)
    assert m._use_dense() and m.num_data == 40
    m.eval()
    mvn = m(torch.as_tensor(Xs, device=DEV))
    s2 = _f(m.likelihood.second_noise)
    cols = _ref_cols2(cov, parts, product)
    if not product:
        assert np.linalg.matrix_rank(dataspace.sla.toeplitz(cols[0])) == 3
    O = dataspace.DataSpaceGP(GB2, G2, sigma2=s2, cols=cols).fit(X, y, np.ones(40))
    mo, vo = O.predict(Xs)
    em = np.abs(mvn.mean.cpu().numpy() - mo).max() / np.abs(mo).max()
    ev = np.abs(mvn.variance.cpu().numpy() - vo).max() / np.abs(vo).max()
    mll = BatchedWoodburyMarginalLogLikelihood(m.likelihood, m)
    m.train()
    v = float(mll(m(Xt), yt[:, 0]).detach())
    print(case, "mean", em, "variance", ev, "mll", v, O.mll())
    assert em < 1e-6 and ev < 1e-6
    assert abs(v - O.mll()) < 1e-8 * abs(O.mll())


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-4), (torch.float32, 1e-2)], ids=["f64", "f32"])
@pytest.mark.parametrize("spectral", [True, False], ids=["spectral", "pcg"])
def test_beyond_the_dense_regime_matches_the_oracle(spectral, dtype, tol):
    """The same model with max_cholesky_size(64) (m = 120: matrix-free), served by the spectral factor and by PCG at cg_tolerance(1e-10)."""
    from online_gp_amd import settings

    cov, parts = _cov2(0.96, True, dtype)
    X, y, Xs = _data2(2, 40)
    with settings.max_cholesky_size(64), settings.spectral_factor(spectral), settings.cg_tolerance(1e-10):
        m, Xt, yt = _stream_model(cov, X, y, dtype, 4)
        assert not m._use_dense()
        m.eval()
        mvn = m(torch.as_tensor(Xs, device=DEV, dtype=dtype))
        mean, var = mvn.mean.double().cpu().numpy(), mvn.variance.double().cpu().numpy()
        assert (m._spectral_state(0) is not None) == spectral
    O = dataspace.DataSpaceGP(GB2, G2, sigma2=_f(m.likelihood.second_noise), cols=_ref_cols2(cov, parts, True)).fit(X, y, np.ones(40))
    mo, vo = O.predict(Xs)
    em, ev = np.abs(mean - mo).max() / np.abs(mo).max(), np.max(np.abs(var - vo) / vo)
    print("spectral" if spectral else "pcg", dtype, "mean", em, "variance", ev)
    assert em < tol and ev < tol


def _stream1(seed=0, noise=0.1, n=60, ns=30):
    """y = sin(2 pi t / p*) + eps on two periods [-1.5, 0.5], held out on the third (0.5, 1.5]."""
    rng = np.random.default_rng(seed)
    t, ts = np.sort(rng.uniform(-1.5, 0.5, n)), np.sort(rng.uniform(0.5, 1.5, ns))
    f = lambda x: np.sin(2 * np.pi * x / P_STAR)          # noqa: E731
    return t, f(t) + noise * rng.standard_normal(n), ts, f(ts) + noise * rng.standard_normal(ns)


def _nll(mean, var, s2, ys):
    v = var + s2
    return float(np.mean(0.5 * ((ys - mean) ** 2 / v + np.log(v) + np.log(2 * np.pi))))


def test_a_periodic_kernel_extrapolates_where_rbf_does_not():
    """Held-out Gaussian NLL on the third period, equal noise 0.1^2: periodic (p = p*, ell = 1) against RBF (ell = 0.3).  On the CPU oracle
    (seed 0, noise 0.1) the two are -0.83 and +0.89; the model's predictions are held to the oracle's at the dense-regime tolerance."""
    from online_gp_amd import kernels as K
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    t, y, ts, ys = _stream1()
    h = kr.grid_steps(GB1, G1)
    Xt, yt = torch.as_tensor(t, device=DEV)[:, None], torch.as_tensor(y, device=DEV)[:, None]
    got = {}
    for name in ("periodic", "rbf"):
        base = K.PeriodicKernel() if name == "periodic" else K.RBFKernel()
        cov = K.ScaleKernel(base).double()
        cov.outputscale = 1.0
        base.lengthscale = 1.0 if name == "periodic" else 0.3
        if name == "periodic":
            base.period_length = P_STAR
        m = FixedNoiseOnlineSKIGP(Xt, yt, None, covar_module=cov, grid_bounds=torch.tensor(GB1, dtype=torch.float64), grid_size=G1, learn_additional_noise=True)
        m.likelihood.second_noise = 0.01
        m._dump_caches()
        m.eval()
        mvn = m(torch.as_tensor(ts, device=DEV)[:, None])
        s2 = _f(m.likelihood.second_noise)
        terms, theta = ([(0, 4, 0, 1)], [_f(base.lengthscale), _f(base.period_length)]) if name == "periodic" else ([(0, 0, 0, -1)], [_f(base.lengthscale)])
        O = dataspace.DataSpaceGP(GB1, G1, sigma2=s2, cols=[kr.columns(G1, h, terms, theta, _f(cov.outputscale))[0]]).fit(t[:, None], y, np.ones(len(t)))
        mo, vo = O.predict(ts[:, None])
        mean, var = mvn.mean.cpu().numpy(), mvn.variance.cpu().numpy()
        assert np.abs(mean - mo).max() < 1e-6 * np.abs(mo).max() and np.abs(var - vo).max() < 1e-6 * np.abs(vo).max()
        got[name] = (_nll(mean, var, s2, ys), _nll(mo, vo, s2, ys))
    print("held-out NLL (model, oracle):", got)
    assert got["periodic"][0] < got["rbf"][0] and got["periodic"][1] < got["rbf"][1]


@pytest.mark.parametrize("case", ["nodal_periodic_rq", "spectral_rq_product"])
def test_mll_gradient_against_central_differences_of_the_oracle(case):
    """BatchedWoodburyMarginalLogLikelihood backward w.r.t. raw_period_length, raw_alpha and every lengthscale against central differences
    of the oracle's MLL (1e-5 of max(|fd|, 1e-3), the bound of test_mll_value_and_gradients_from_the_spectral_factor; relative step 1e-5:
    truncation ~1e-10, rounding ~1e-16 |mll| / 1e-5 ~ 1e-9, both far inside).  nodal_periodic_rq: Scale(Separable([Product(Periodic, RBF),
    RQ])) in the dense regime.  spectral_rq_product: Scale(Separable([Product(RQ, RBF), RQ])) beyond it (max_cholesky_size(64)), served by
    the spectral factor with the un-truncated basis that the existing test of that path uses."""
    from online_gp_amd import kernels as K
    from online_gp_amd import settings
    from online_gp_amd.mlls import BatchedWoodburyMarginalLogLikelihood
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    spectral = case == "spectral_rq_product"
    first, rbf, rq = (K.RQKernel() if spectral else K.PeriodicKernel()), K.RBFKernel(), K.RQKernel()
    cov = K.ScaleKernel(K.SeparableKernel([K.ProductKernel(first, rbf), rq])).double()
    first.lengthscale, rbf.lengthscale, rq.lengthscale, rq.alpha, cov.outputscale = 1.3, 0.9, 0.8, 1.7, 1.2
    if spectral:
        first.alpha = 0.6
    else:
        first.period_length = 0.96
    aux = first.raw_alpha if spectral else first.raw_period_length
    # theta = [ell_first, aux_first, ell_rbf, ell_rq, alpha_rq]
    terms = [(0, 5 if spectral else 4, 0, 1), (0, 0, 2, -1), (1, 5, 3, 4)]
    raws = [first.raw_lengthscale, aux, rbf.raw_lengthscale, rq.raw_lengthscale, rq.raw_alpha]
    X, y, _ = _data2(3, 40)
    Xt, yt = torch.as_tensor(X, device=DEV), torch.as_tensor(y, device=DEV)[:, None]
    with contextlib.ExitStack() as stack:
        if spectral:
            for ctx in (settings.max_cholesky_size(64), settings.spectral_factor(True), settings.spectral_tail(1e-12), settings.spectral_max_rank(2048)):
                stack.enter_context(ctx)
        m = FixedNoiseOnlineSKIGP(Xt, yt, None, covar_module=cov, grid_bounds=torch.tensor(GB2), grid_size=G2, learn_additional_noise=True)
        assert m._use_dense() != spectral
        mll = BatchedWoodburyMarginalLogLikelihood(m.likelihood, m)
        m.train()
        v = mll(m(Xt), yt[:, 0]).sum()
        v.backward()
        assert (m.__dict__.get("_spectral", {}).get(0) is not None and m._spectral[0].cur is not None) == spectral
    theta = np.array([_f(first.lengthscale), _f(first.alpha if spectral else first.period_length), _f(rbf.lengthscale), _f(rq.lengthscale), _f(rq.alpha)])
    S, s2 = _f(cov.outputscale), _f(m.likelihood.second_noise)

    def ref(th):
        out = kr.columns(G2, H2, terms, list(th), S)[0]
        return dataspace.DataSpaceGP(GB2, G2, sigma2=s2, cols=[out[:G2[0]], out[G2[0]:]]).fit(X, y, np.ones(40)).mll()

    assert abs(float(v.detach()) - ref(theta)) < 1e-8 * abs(ref(theta))
    for i, raw in enumerate(raws):
        got = _f(raw.grad) / _f(torch.sigmoid(raw))               # (softplus: d theta / d raw = sigmoid(raw))
        e = np.zeros(5)
        e[i] = 1e-5 * theta[i]
        fd = (ref(theta + e) - ref(theta - e)) / (2 * e[i])
        print(case, "theta", i, "autograd", got, "oracle central difference", fd)
        assert abs(got - fd) < 1e-5 * max(abs(fd), 1e-3), (i, got, fd)


def test_period_gradient_beyond_the_dense_regime_comes_from_the_pcg_terms():
    """The 12 x 10 model beyond the dense regime (max_cholesky_size(64)) with spectral_factor ON: predictions may use the factor, but the
    MLL terms of a kernel with a periodic member and their gradient come from the PCG path (model._mll_spectral_state is None), through both
    doors of the MLL (the value's autograd function and the Woodbury terms).  The gradient w.r.t. (ell_per, p, ell_rbf, ell_matern) is held
    against central differences of the oracle with the bound that test_mll_feature_gradient_matrix_free_regime (tests/test_mll_gpu.py) sets for the Hutchinson
    trace of that path at 4000 probes: 0.1 in norm.  At these hyper-parameters (p = 1.15 against 0.96 in the data, sigma2 = 0.05) the
    oracle's period component alone is 0.27 of the norm, so a gradient with the period's part missing or of the wrong sign -- what the
    truncated factor gave, DESIGN.md 3.29 -- misses the bound; that is asserted from the oracle's figures first."""
    from online_gp_amd import settings
    from online_gp_amd.mlls import BatchedWoodburyMarginalLogLikelihood
    from online_gp_amd.mlls.batched_woodbury_marginal_log_likelihood import _WoodburyTerms, num_trace_samples
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    cov, (per, rbf, mat) = _cov2(1.15, True)
    X, y, _ = _data2(2, 40)
    Xt, yt = torch.as_tensor(X, device=DEV), torch.as_tensor(y, device=DEV)[:, None]
    with settings.max_cholesky_size(64), settings.spectral_factor(True), settings.cg_tolerance(1e-10), num_trace_samples(4000):
        m = FixedNoiseOnlineSKIGP(Xt, yt, None, covar_module=cov, grid_bounds=torch.tensor(GB2), grid_size=G2, learn_additional_noise=True)
        m.likelihood.second_noise = 0.05
        m._dump_caches()
        assert not m._use_dense() and m._spectral_allowed()
        assert m._spectral_state(0) is not None and m._mll_spectral_state(0) is None
        mll = BatchedWoodburyMarginalLogLikelihood(m.likelihood, m)
        m.train()
        v = mll(m(Xt), yt[:, 0]).sum()
        v.backward()
        # both doors: no factor state in the Woodbury terms either
        kappa = torch.ones((), dtype=torch.float64, device=DEV, requires_grad=True)
        tcol = m.covar_module.toeplitz_columns().double()
        bMb, _ = _WoodburyTerms.apply(tcol, kappa, m, 0, False)
        assert bMb.grad_fn is not None and getattr(bMb.grad_fn, "spectral", 0) is None
    theta = np.array([_f(per.lengthscale), _f(per.period_length), _f(rbf.lengthscale), _f(mat.lengthscale)])
    S, s2 = _f(cov.outputscale), _f(m.likelihood.second_noise)
    terms = [(0, 4, 0, 1), (0, 0, 2, -1), (1, 3, 3, -1)]

    def ref(th):
        out = kr.columns(G2, H2, terms, list(th), S)[0]
        return dataspace.DataSpaceGP(GB2, G2, sigma2=s2, cols=[out[:G2[0]], out[G2[0]:]]).fit(X, y, np.ones(40)).mll()

    fd, got = np.zeros(4), np.zeros(4)
    for i, raw in enumerate([per.raw_lengthscale, per.raw_period_length, rbf.raw_lengthscale, mat.raw_lengthscale]):
        e = np.zeros(4)
        e[i] = 1e-5 * theta[i]
        fd[i] = (ref(theta + e) - ref(theta - e)) / (2 * e[i])
        got[i] = _f(raw.grad) / _f(torch.sigmoid(raw))
    print("autograd", got, "oracle central differences", fd, "relative error in norm", np.linalg.norm(got - fd) / np.linalg.norm(fd))
    assert abs(fd[1]) > 0.2 * np.linalg.norm(fd)                  # (the period's part is twice what the bound lets through)
    assert np.linalg.norm(got - fd) < 0.1 * np.linalg.norm(fd)


def test_the_streaming_wrapper_declines_the_captured_step_for_these_kernels():
    """OnlineSKIRegression on a 16 x 16 grid with fused capturable Adam and Scale(Separable([Product(Periodic, RBF), Matern])): the
    hyper-parameter step of these kernels is declined by the captured step and runs op by op -- nothing captured, nothing
    disabled, finite losses, and the period receives updates (a gate test: that the step learns in the right direction is
    test_learning_moves_the_period_towards_the_truth's)."""
    from online_gp_amd.models import Identity, OnlineSKIRegression
    from online_gp_amd.models._graphed_step import WARMUP_STEPS

    steps, n0 = WARMUP_STEPS + 5, 300
    X, y, _ = _data2(4, n0 + 4 * steps)
    cov, parts = _cov2(0.96, True, torch.float32)
    Xt, yt = torch.as_tensor(X, device=DEV, dtype=torch.float32), torch.as_tensor(y, device=DEV, dtype=torch.float32)[:, None]
    reg = OnlineSKIRegression(Identity(2), Xt[:n0], yt[:n0], 1e-2, 16, 1.0, covar_module=cov)
    p0, losses = _f(parts[0].period_length), []
    for i in range(steps):
        lo = n0 + 4 * i
        losses.append(reg.update(Xt[lo:lo + 4], yt[lo:lo + 4])[1])
    gs = reg._graphed
    assert gs is not None and gs.disabled is None and gs.captures == 0 and gs.replays == 0
    assert np.isfinite(losses).all()
    assert abs(_f(parts[0].period_length) - p0) > 1e-3


def test_learning_moves_the_period_towards_the_truth():
    """The 1-D stream with the period started 20 % off (1.2 p*): 200 single-point updates later |p - p*| is smaller and the oracle's MLL of all
    the data at the learned hyper-parameters is higher than at the initial ones."""
    from online_gp_amd import kernels as K
    from online_gp_amd.models import Identity, OnlineSKIRegression

    t, y, _, _ = _stream1(n=220)
    order = np.random.default_rng(1).permutation(220)
    t, y = t[order], y[order]
    per = K.PeriodicKernel()
    cov = K.ScaleKernel(per)
    per.period_length = 1.2 * P_STAR
    per.lengthscale = 1.0
    cov.outputscale = 1.0
    Xt, yt = torch.as_tensor(t, device=DEV, dtype=torch.float64)[:, None], torch.as_tensor(y, device=DEV, dtype=torch.float64)[:, None]
    reg = OnlineSKIRegression(Identity(1), Xt[:20], yt[:20], 1e-2, 64, 1.5, covar_module=cov)
    gb, h = reg.gp._grid.grid_bounds, reg.gp._grid.h          # (the wrapper's own bounds: +-(1.5 + 0.1) as it rounds them)
    assert list(reg.gp._grid.g) == G1 and abs(gb[0][1] - 1.6) < 1e-6

    def oracle_mll():
        cols = [kr.columns(G1, h, [(0, 4, 0, 1)], [_f(per.lengthscale), _f(per.period_length)], _f(cov.outputscale))[0]]
        return dataspace.DataSpaceGP(gb, G1, sigma2=_f(reg.gp.likelihood.second_noise), cols=cols).fit(t[:, None], y, np.ones(220)).mll()

    # the wrapper's MLL gradient w.r.t. the raw period against central differences of the oracle (1e-5 of max(|fd|, 1e-3), the bound of
    # test_mll_value_and_gradients_from_the_spectral_factor).  Measured on an MI355X: taken from the truncated spectral factor this gradient
    # was +0.0119 against -0.1928, which is why a model with a periodic kernel keeps the nodal factor here
    def oracle_mll_at(p, n=20):
        cols = [kr.columns(G1, h, [(0, 4, 0, 1)], [_f(per.lengthscale), p], _f(cov.outputscale))[0]]
        return dataspace.DataSpaceGP(gb, G1, sigma2=_f(reg.gp.likelihood.second_noise), cols=cols).fit(t[:n, None], y[:n], np.ones(n)).mll()

    reg.gp.zero_grad()
    reg.mll(None, None).sum().backward()
    raw = per.raw_period_length
    g_p = _f(raw.grad) / _f(torch.sigmoid(raw))
    eps = 1e-5 * _f(per.period_length)
    fd = (oracle_mll_at(_f(per.period_length) + eps) - oracle_mll_at(_f(per.period_length) - eps)) / (2 * eps)
    reg.gp.zero_grad()
    print("d MLL / d period:", g_p, "oracle central difference:", fd)
    assert abs(g_p - fd) < 1e-5 * max(abs(fd), 1e-3)
    p0, mll0 = _f(per.period_length), oracle_mll()
    for i in range(200):
        reg.update(Xt[20 + i:21 + i], yt[20 + i:21 + i])
    p1, mll1 = _f(per.period_length), oracle_mll()
    print("period", p0, "->", p1, "oracle MLL", mll0, "->", mll1)
    assert abs(p1 - P_STAR) < abs(p0 - P_STAR)
    assert mll1 > mll0
