"""GPU: derivative observations -- values and gradients absorbed in one launch -- against the fp64 data-space
reference of tests/grad_obs_reference.py: the kernel through the C ABI, then the model surface.

Measured on one MI355X (relative to max |reference|; 12 x 10 grid, 40 points with values and gradients, 50 queries):

    regime       dtype  mean      variance  mean gradient  MLL (relative)
    dense        fp64   2.0e-15   1.3e-14   6.9e-15        4.4e-16   (bounds 1e-4, 1e-4, 1e-4, 1e-7)
    dense        fp32   1.4e-06   1.6e-06   3.3e-06        --        (bounds 1e-2)
    matrix-free  fp64   6.4e-14   1.4e-14   2.2e-13        7.7e-03   (bounds 1e-4, 1e-4, 1e-4, 5e-2)
    matrix-free  fp32   2.9e-06   2.7e-06   1.2e-06        --        (bounds 1e-2)

The MLL bounds are those of tests/test_mll_gpu.py (fp64 there as here); how the data's noise range follows from them: _data.
"""
import ctypes

import numpy as np
import pytest
import torch

import grad_obs_reference as gr

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [(torch.float64, 1e-11), (torch.float32, 2e-4)]          # the scatter tolerances of tests/test_hip_ops.py
RTOL = {torch.float64: 1e-4, torch.float32: 1e-2}                 # tests/test_model_gpu.py
MLL_DENSE, MLL_FREE = 1e-7, 0.05                                  # tests/test_mll_gpu.py: dense branch / stochastic branch, relative
KGRIDS = {"d1": [8], "d2": [5, 7], "d3": [6, 5, 4], "d4": [5, 4, 4, 4]}
N = 37                                                            # not a multiple of the 4 points per block


# ------------------------------------------------------------------------------------------------------------------ the kernel
_cases = {}


def _kernel_case(name):
    """Grid, the 37 points with their channel tensors (fp64 values that are exact in fp32) and the dense reference; built once."""
    if name in _cases:
        return _cases[name]
    from online_gp_amd import grid_ops

    g = KGRIDS[name]
    d, C = len(g), len(g) + 1
    rng = np.random.default_rng(100 + d)
    grid = grid_ops.GridSpec([[-1.0, 1.0 + 0.25 * q] for q in range(d)], g)
    cell = np.stack([rng.integers(0, gq - 1, N) for gq in g], 1).astype(np.float64)
    frac = 0.5 + rng.choice([-1.0, 1.0], (N, d)) * rng.uniform(0.05, 0.45, (N, d))      # away from nodes and cell midpoints
    for q in range(d):
        cell[q, q] = 0                                              # points 0 .. d-1: first (boundary) cell of dim q
        cell[d + q, q] = g[q] - 2                                   # points d .. 2d-1: last (boundary) cell of dim q
    cell[12:17] = 1                                                 # five points in one interior cell: colliding atomics
    U = cell + frac
    X = np.array(grid.g0) + np.array(grid.h) * U
    X[10, 0] = grid.g0[0] - 1.0                                      # two points outside the grid
    X[11, d - 1] = grid.g0[d - 1] + grid.h[d - 1] * (g[d - 1] - 1) + 1.0
    X = X.astype(np.float32).astype(np.float64)
    present = rng.uniform(size=(N, C)) < 0.7
    present[:2 * d] = True                                          # boundary-cell derivative channels that are present
    present[12:17] = True
    present[20] = [True] + [False] * d                              # value only
    present[21] = [False] + [True] * d                              # gradient only
    present[22] = False                                             # nothing at all
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    noise = np.where(present, f32(rng.uniform(0.5, 2.0, (N, C))), 1.0)
    wa = np.where(present, f32(1.0 / noise), 0.0)
    Y = np.where(present, f32(rng.standard_normal((N, C))), 0.0)
    u = f32(rng.standard_normal(grid.m))
    ref = gr.dense_absorb(grid, X, Y, wa, wa, noise, u)
    _cases[name] = dict(grid=grid, X=X, Y=Y, wa=wa, noise=noise, u=u, ref=ref, present=present)
    return _cases[name]


def _buffers(grid, tdt, init=None):
    H = (grid.R + 1) // 2
    z = lambda *s: torch.zeros(s, device=DEV, dtype=tdt)
    out = dict(b=z(grid.m), A=z(H * grid.m), cnt=z(grid.m), res=z(grid.m), stats=torch.zeros(2, device=DEV, dtype=torch.float64))
    if init is not None:
        for k, v in out.items():
            v.copy_(torch.as_tensor(init[k]).to(v))
    return out


def _compare(got, ref, tol, keys, label):
    for k in keys:
        r = np.asarray(ref[k], dtype=np.float64)
        e = float(np.abs(got[k].double().cpu().numpy() - r).max())
        bound = 10 * tol * float(np.abs(r).max())
        print(f"{label} {k}: max err {e:.3e}  bound {bound:.3e}")
        assert e <= bound, (label, k, e, bound)


@pytest.mark.parametrize("tdt,tol", DTYPES)
@pytest.mark.parametrize("name", list(KGRIDS))
def test_kernel_matches_the_dense_reference(name, tdt, tol):
    from online_gp_amd import grid_ops

    c = _kernel_case(name)
    grid, ref = c["grid"], c["ref"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    X, Y, wa, noise, u = (mk(c[k]) for k in ("X", "Y", "wa", "noise", "u"))
    keys = ("A", "b", "cnt", "stats", "res")
    rname = dict(ref, A=ref["A_half"])
    # from zero
    got, err = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    mean = torch.full((N, grid.d + 1), float("nan"), device=DEV, dtype=tdt)
    grid_ops.scatter_stats_grad(grid, X, Y, wa, wa, noise, got["b"], got["A"], got["cnt"], got["stats"], err, u=u, res=got["res"], mean_out=mean)
    _compare(dict(got, mean_out=mean), rname, tol, keys + ("mean_out",), f"{name} zero-init")
    assert int(err.item()) == ref["err"] == 1 + 2 * 2                # bit 0 | two points dropped, each counted once
    # on top of non-zero buffers: every statistic is added, none assigned
    rng = np.random.default_rng(5)
    init = {k: 0.5 * float(np.abs(rname[k]).max()) * rng.standard_normal(np.shape(rname[k])) for k in keys}
    got = _buffers(grid, tdt, init)
    start = {k: v.double().cpu().numpy().copy() for k, v in got.items()}
    err.zero_()
    grid_ops.scatter_stats_grad(grid, X, Y, wa, wa, noise, got["b"], got["A"], got["cnt"], got["stats"], err, u=u, res=got["res"])
    _compare(got, {k: start[k] + rname[k] for k in keys}, tol, keys, f"{name} on top")


@pytest.mark.parametrize("tdt,tol", DTYPES)
@pytest.mark.parametrize("name", list(KGRIDS))
def test_kernel_without_derivative_channels_is_the_value_absorb(name, tdt, tol):
    from online_gp_amd import grid_ops

    c = _kernel_case(name)
    grid = c["grid"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    only = np.zeros_like(c["present"])
    only[:, 0] = c["present"][:, 0]
    X, u = mk(c["X"]), mk(c["u"])
    Y, wa, noise = mk(np.where(only, c["Y"], 0.0)), mk(np.where(only, c["wa"], 0.0)), mk(np.where(only, c["noise"], 1.0))
    got, want = _buffers(grid, tdt), _buffers(grid, tdt)
    e1, e2 = grid_ops.new_err_flag(DEV), grid_ops.new_err_flag(DEV)
    grid_ops.scatter_stats_grad(grid, X, Y, wa, wa, noise, got["b"], got["A"], got["cnt"], got["stats"], e1, u=u, res=got["res"])
    y0, w0, n0 = Y[:, 0].contiguous(), wa[:, 0].contiguous(), noise[:, 0].contiguous()
    grid_ops.scatter_stats_cnt(grid, X, y0, w0, w0, n0, want["b"], want["A"], True, want["cnt"], want["stats"], e2, u=u, res=want["res"])
    _compare(got, {k: v.double().cpu().numpy() for k, v in want.items()}, tol, ("A", "b", "cnt", "stats", "res"), f"{name} value-only")
    assert int(e1.item()) == int(e2.item()) == 5


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64])
def test_absorb_refuses_channels_with_what_the_kernel_does_not_do(tdt):
    """Through the full argument record (wiski_absorb): channels with the full stencil, a guard, zero regions, a shard, nout > 1 or a
    channel count other than d + 1 is WISKI_E_BADARG before any launch -- every buffer untouched -- while the same record without
    the offending field runs and equals grid_ops.scatter_stats_grad."""
    from online_gp_amd import _hip, grid_ops

    c = _kernel_case("d3")
    grid = c["grid"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    X, Y, wa, noise, u = (mk(c[k]) for k in ("X", "Y", "wa", "noise", "u"))
    buf, err = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    mean = torch.full((N, 4), float("nan"), device=DEV, dtype=tdt)
    full = torch.zeros((grid.R, grid.m), device=DEV, dtype=tdt)
    guard = torch.tensor([7], device=DEV, dtype=torch.int64)
    z1 = torch.full((2,), 0x01010101, device=DEV, dtype=torch.int32)
    p = lambda t: t.data_ptr()
    stream = _hip.stream_ptr(torch.device("cuda", torch.cuda.current_device()))

    def call(**kw):
        a = _hip.wiski_absorb_args(d_x=p(X), d_y=p(Y), d_wa=p(wa), d_wb=p(wa), d_noise=p(noise), n=N, d_b=p(buf["b"]), d_A=p(buf["A"]), half=1,
                                   channels=4, d_cnt=p(buf["cnt"]), d_stats=p(buf["stats"]), d_err=p(err), d_u=p(u), d_res=p(buf["res"]),
                                   d_mean_out=p(mean), nout=1)
        for k, v in kw.items():
            setattr(a, k, v)
        return _hip.fn("wiski_absorb", tdt)(grid.ref, ctypes.byref(a), stream)

    refused = [("full stencil", call(half=0, d_A=p(full), d_u=None, d_res=None, d_mean_out=None)), ("guard", call(d_guard=p(guard), guard_expect=7)),
               ("zero region", call(z1=p(z1), n1_bytes=8)), ("shard", call(g_lo=0, g_hi=3)), ("nout = 2", call(nout=2, d_mean_out=None)),
               ("channels = 3", call(channels=3)), ("channels = 5", call(channels=5))]
    torch.cuda.synchronize()
    assert [(what, rc) for what, rc in refused if rc != -1] == []
    assert all(float(v.abs().max()) == 0.0 for v in buf.values()) and float(full.abs().max()) == 0.0 and int(err.item()) == 0
    assert bool(torch.isnan(mean).all()) and bool((z1 == 0x01010101).all())
    assert call() == 0
    want, e2 = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    grid_ops.scatter_stats_grad(grid, X, Y, wa, wa, noise, want["b"], want["A"], want["cnt"], want["stats"], e2, u=u, res=want["res"])
    tol = dict(DTYPES)[tdt]
    _compare(buf, {k: v.double().cpu().numpy() for k, v in want.items()}, tol, ("A", "b", "cnt", "stats", "res"), "record")
    assert int(err.item()) == int(e2.item()) == 5


# ------------------------------------------------------------------------------------------------------------------- the model
GB, GS = [[-1.0, 1.0], [-1.0, 1.0]], [12, 10]


def _f(X):
    return np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.5 * X[:, 1]


def _df(X):
    return np.stack([2 * np.cos(2 * X[:, 0]) * np.cos(X[:, 1]), -np.sin(2 * X[:, 0]) * np.sin(X[:, 1]) + 0.5], 1)


def _data(n=40, seed=0):
    """n points with values and gradients.  The noise range is fixed by what the MLL bounds mean: they are RELATIVE to |MLL|, and
    -2 MLL = quad / N + logdet / N + mean log(sigma2 noise) + log 2 pi >= log(2 pi sigma2 min noise), the first two terms being
    non-negative.  With sigma2 = log 2 (the model's default) and noise >= 0.5 that is >= 0.78, so |MLL| >= 0.39 per observation
    whatever the data, as in tests/test_mll_gpu.py (unit noise); below noise = 1 / (2 pi sigma2) = 0.23 the terms can cancel and a
    relative bound loses its meaning.  For the stochastic branch the reference gives the estimator's own spread: Hutchinson's
    variance 2 sum_{i != j} L_ij^2 / P of L = log(I + Kt^1/2 A Kt^1/2) with P = 64 Rademacher probes is a standard deviation of 1.3
    in logdet on this data, against the 12 that 5 % of |MLL| = 1.0 over 120 observations allows.  (A first version drew the noise
    from U(0.05, 0.2): MLL = -0.0408 by cancellation, the same 5 % allowed 0.49 in logdet against an estimator spread of 2.6, and
    the matrix-free fp64 case measured -0.0578, relative 0.42 -- 1.5 standard deviations of the estimator.  Mean, variance and
    gradient of that model agreed to 1e-12 and its dense MLL to 1.5e-13.)"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-0.95, 0.95, (n, 2))
    Y = np.concatenate([_f(X)[:, None], _df(X)], 1) + 0.05 * rng.standard_normal((n, 3))
    noise = rng.uniform(0.5, 2.0, (n, 3))
    return rng, X, Y, noise


def _t(a, dtype):
    return torch.as_tensor(a, device=DEV, dtype=dtype)


def _model(X, y, nz, dtype, **kw):
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    return FixedNoiseOnlineSKIGP(_t(X, dtype), _t(y, dtype)[:, None], _t(nz, dtype)[:, None], grid_bounds=torch.tensor(GB), grid_size=GS,
                                 learn_additional_noise=True, **kw)


def _reference(m, X, Y, noise, present, gb=GB, gs=GS):
    k = m.covar_module.base_kernel
    ell, s, s2 = k.base_kernel.lengthscale.detach().cpu().numpy().reshape(-1), float(k.outputscale), float(m.likelihood.second_noise)
    grid = gr.Grid.from_bounds(gb, gs)
    return gr.GradObsGP(grid, gr.dense_kuu(grid, "rbf", ell, s), s2).fit(X, Y, noise, present)


def _mll(m):
    from online_gp_amd.mlls import BatchedWoodburyMarginalLogLikelihood

    m.train()
    v = float(BatchedWoodburyMarginalLogLikelihood(m.likelihood, m)(m(None), None).detach())
    m.eval()
    return v


def _fit_all(dtype):
    """Values of the first 10 points at construction; values + gradients of the other 30 and the gradients of the first 10 in two
    in-place updates: the model of all 40 points with values and gradients."""
    rng, X, Y, noise = _data()
    m = _model(X[:10], Y[:10, 0], noise[:10, 0], dtype).eval()
    m.condition_on_observations(_t(X[10:], dtype), _t(Y[10:, 0], dtype), _t(noise[10:, 0], dtype), inplace=True,
                                grad_Y=_t(Y[10:, 1:], dtype), grad_noise=_t(noise[10:, 1:], dtype))
    m.condition_on_observations(_t(X[:10], dtype), None, inplace=True, grad_Y=_t(Y[:10, 1:], dtype), grad_noise=_t(noise[:10, 1:], dtype))
    assert m.num_data == 120
    return rng, X, Y, noise, m


def _check_regime(dtype, label, mll_bound):
    rng, X, Y, noise, m = _fit_all(dtype)
    ref = _reference(m, X, Y, noise, np.ones(Y.shape, dtype=bool))
    Xs = rng.uniform(-0.95, 0.95, (50, 2))
    mo, vo, go = ref.predict(Xs)
    mvn = m(_t(Xs, dtype))
    mean, var = mvn.mean.detach().double().cpu().numpy(), mvn.variance.detach().double().cpu().numpy()
    # the posterior mean's gradient at the observed points, by autograd through the posterior
    Xq = _t(X, dtype).requires_grad_(True)
    m(Xq).mean.sum().backward()
    _, _, gx = ref.predict(X)
    e_m, e_v = np.abs(mean - mo).max() / np.abs(mo).max(), np.abs(var - vo).max() / np.abs(vo).max()
    e_g = np.abs(Xq.grad.double().cpu().numpy() - gx).max() / np.abs(gx).max()
    print(f"{label} {dtype}: mean {e_m:.3e}  var {e_v:.3e}  grad {e_g:.3e}  (bound {RTOL[dtype]:.0e})")
    assert e_m <= RTOL[dtype] and e_v <= RTOL[dtype] and e_g <= RTOL[dtype]
    if dtype == torch.float64:
        v, r = _mll(m), ref.mll()
        print(f"{label}: mll {v:.10f}  reference {r:.10f}  rel {abs(v - r) / abs(r):.3e}  (bound {mll_bound:.0e})")
        assert abs(v - r) <= mll_bound * abs(r)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_dense_regime_matches_the_data_space_reference(dtype):
    """12 x 10 grid, 40 points with values and gradients (120 scalar observations), 50 queries; figures printed before the asserts."""
    _check_regime(dtype, "dense", MLL_DENSE)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_matrix_free_regime_matches_the_data_space_reference(dtype):
    from online_gp_amd import settings
    from online_gp_amd.mlls.batched_woodbury_marginal_log_likelihood import num_trace_samples

    with settings.dense_small_grids(False), settings.spectral_factor(False), num_trace_samples(64), \
            settings.cg_tolerance(1e-10 if dtype == torch.float64 else 1e-6):
        _check_regime(dtype, "matrix-free", MLL_FREE)


def test_three_in_place_updates_equal_one_fit_and_the_functional_form_leaves_the_parent_alone():
    dtype = torch.float64
    rng, X, Y, noise = _data(48, seed=1)
    mask = rng.uniform(size=(16, 2)) < 0.6
    m = _model(X[:12], Y[:12, 0], noise[:12, 0], dtype).eval()
    m.condition_on_observations(_t(X[12:24], dtype), _t(Y[12:24, 0], dtype), _t(noise[12:24, 0], dtype), inplace=True)          # values
    m.condition_on_observations(_t(X[24:32], dtype), None, inplace=True, grad_Y=_t(Y[24:32, 1:], dtype), grad_noise=_t(noise[24:32, 1], dtype))
    before = [t.clone() for t in m.stats_buffers()]
    args = (_t(X[32:], dtype), _t(Y[32:, 0], dtype), _t(noise[32:, 0], dtype))
    kw = dict(grad_Y=_t(Y[32:, 1:], dtype), grad_noise=_t(noise[32:, 1:], dtype), grad_mask=torch.as_tensor(mask, device=DEV))
    child = m.condition_on_observations(*args, **kw)
    assert all(torch.equal(a, b) for a, b in zip(before, m.stats_buffers())) and m.num_data == 24 + 16
    m.condition_on_observations(*args, inplace=True, **kw)
    present = np.zeros(Y.shape, dtype=bool)
    present[:, 0] = True
    present[24:32] = [False, True, True]
    present[32:, 1:] = mask
    nz = noise.copy()
    nz[24:32, 2] = nz[24:32, 1]                                      # grad_noise [n]: one noise for the d partials of a point
    ref = _reference(m, X, Y, nz, present)
    assert m.num_data == child.num_data == ref.N == 24 + 16 + 16 + int(mask.sum())
    Xs = rng.uniform(-0.95, 0.95, (50, 2))
    mo, vo, _ = ref.predict(Xs)
    for mod in (m, child.eval()):
        mvn = mod(_t(Xs, dtype))
        assert np.abs(mvn.mean.detach().cpu().numpy() - mo).max() <= RTOL[dtype] * np.abs(mo).max()
        assert np.abs(mvn.variance.detach().cpu().numpy() - vo).max() <= RTOL[dtype] * np.abs(vo).max()
        assert abs(_mll(mod) - ref.mll()) <= MLL_DENSE * abs(ref.mll())


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-9), (torch.float32, 2e-4)])
def test_carried_residual_follows_a_derivative_update(dtype, tol):
    """Matrix-free regime, mean state current: after the update R is b - Z - A U (bound: that of
    tests/test_model_gpu.py::test_residual_carry_over_tracks_true_residual), and the warm solve from it equals a cold one."""
    from online_gp_amd import grid_ops, settings

    rng, X, Y, noise = _data()
    with settings.dense_small_grids(False), settings.spectral_factor(False), settings.cg_tolerance(1e-10 if dtype == torch.float64 else 1e-6), torch.no_grad():
        m = _model(X[:20], Y[:20, 0], noise[:20, 0], dtype).eval()
        m.prediction_cache
        assert m._mean_state["R_ok"]
        m.condition_on_observations(_t(X[20:], dtype), _t(Y[20:, 0], dtype), _t(noise[20:, 0], dtype), inplace=True,
                                    grad_Y=_t(Y[20:, 1:], dtype), grad_noise=_t(noise[20:, 1:], dtype))
        ms, c = m._mean_state, m._kernel_cache
        assert ms["R_ok"]
        b = c["interpolation_cache"][0, :, 0]
        true_r = b - ms["Z"][0] - grid_ops.stencil_spmv(m._grid, c["WtW"].stencil, ms["U"][0:1])[0]
        e, bound = float((ms["R"][0] - true_r).abs().max()), tol * float(b.abs().max()) * 50
        print(f"carried residual {dtype}: {e:.3e}  bound {bound:.3e}")
        assert e <= bound
        warm = m.prediction_cache["pred_mean"][0, :, 0].clone()
        m._mean_state = None
        m._dump_caches()
        cold = m.prediction_cache["pred_mean"][0, :, 0]
        assert float((warm - cold).abs().max()) <= RTOL[dtype] * float(cold.abs().max())


def test_spectral_factor_is_rebuilt_after_a_derivative_update():
    """The set-up of tests/test_spectral_gpu.py (d = 3, g = 14: matrix-free, spectral factor in use): a derivative batch marks the
    factor stale, it rebuilds from the stencil, and the predictions match the reference."""
    from online_gp_amd import settings
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    dtype, d, g, n0, q = torch.float64, 3, 14, 300, 37
    rng = np.random.default_rng(11)
    gb = [[-1.1, 1.1]] * d
    X = rng.uniform(-1, 1, (n0 + q, d))
    s = X.sum(1)
    Y = np.concatenate([np.sin(2 * s)[:, None], np.repeat(2 * np.cos(2 * s)[:, None], d, 1)], 1) + 0.1 * rng.standard_normal((n0 + q, d + 1))
    nz = rng.uniform(0.5, 2.0, (n0 + q, d + 1))
    Xs = rng.uniform(-1, 1, (50, d))
    with settings.cg_tolerance(1e-10), settings.spectral_max_rank(1024):
        m = FixedNoiseOnlineSKIGP(_t(X[:n0], dtype), _t(Y[:n0, :1], dtype), _t(nz[:n0, :1], dtype), grid_bounds=torch.tensor(gb), grid_size=g,
                                  learn_additional_noise=True).eval()
        m(_t(Xs, dtype)).variance
        fac = m._spectral[0]
        assert fac.ref is not None and fac.rebuilds == 1 and not fac.stale
        m.condition_on_observations(_t(X[n0:], dtype), _t(Y[n0:, 0], dtype), _t(nz[n0:, 0], dtype), inplace=True,
                                    grad_Y=_t(Y[n0:, 1:], dtype), grad_noise=_t(nz[n0:, 1:], dtype))
        assert fac.stale
        mvn = m(_t(Xs, dtype))
        mean, var = mvn.mean.detach().cpu().numpy(), mvn.variance.detach().cpu().numpy()
        assert m._spectral[0].rebuilds == 2 and not m._spectral[0].stale
    present = np.ones(Y.shape, dtype=bool)
    present[:n0, 1:] = False
    mo, vo, _ = _reference(m, X, Y, nz, present, gb, g).predict(Xs)
    assert np.abs(mean - mo).max() <= RTOL[dtype] * np.abs(mo).max() and np.max(np.abs(var - vo) / vo) <= RTOL[dtype]


def test_forgetting_scales_the_noise_of_every_scalar_observation():
    """forgetting_factor = 0.9 over three updates: the reference with every noise scaled by gamma^-age (age = updates since)."""
    dtype, gam = torch.float64, 0.9
    rng, X, Y, noise = _data(40, seed=2)
    m = _model(X[:10], Y[:10, 0], noise[:10, 0], dtype, forgetting_factor=gam).eval()
    for i in range(3):
        sl = slice(10 + 10 * i, 20 + 10 * i)
        m.condition_on_observations(_t(X[sl], dtype), _t(Y[sl, 0], dtype), _t(noise[sl, 0], dtype), inplace=True,
                                    grad_Y=_t(Y[sl, 1:], dtype), grad_noise=_t(noise[sl, 1:], dtype))
    age = np.repeat([3, 2, 1, 0], 10)
    present = np.ones(Y.shape, dtype=bool)
    present[:10, 1:] = False
    ref = _reference(m, X, Y, noise * gam ** -age[:, None], present)
    Xs = rng.uniform(-0.95, 0.95, (50, 2))
    mo, vo, _ = ref.predict(Xs)
    mvn = m(_t(Xs, dtype))
    assert np.abs(mvn.mean.detach().cpu().numpy() - mo).max() <= RTOL[dtype] * np.abs(mo).max()
    assert np.abs(mvn.variance.detach().cpu().numpy() - vo).max() <= RTOL[dtype] * np.abs(vo).max()
    assert m.num_data == ref.N == 100 and abs(_mll(m) - ref.mll()) <= MLL_DENSE * abs(ref.mll())


def test_refusals():
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    dtype = torch.float64
    rng, X, Y, noise = _data(12)
    Xt, G = _t(X, dtype), _t(Y[:, 1:], dtype)
    m = _model(X, Y[:, 0], noise[:, 0], dtype)
    before = [t.clone() for t in m.stats_buffers()]
    with pytest.raises(NotImplementedError):                        # fantasies
        m.condition_on_observations(Xt[None], _t(Y[:, 0], dtype)[None], grad_Y=G)
    with pytest.raises(NotImplementedError):                        # the data-parallel statistics exchange
        m._absorb_grad(m._kernel_cache, Xt, _t(Y, dtype), _t(noise, dtype), torch.ones(12, 3, dtype=torch.bool, device=DEV),
                       half_delta=m._half_buffers())
    with pytest.raises(ValueError):
        m.condition_on_observations(Xt, _t(Y[:, 0], dtype), grad_noise=_t(noise[:, 1:], dtype))
    with pytest.raises(ValueError):
        m.condition_on_observations(Xt, _t(Y[:, 0], dtype), grad_Y=G[:, :1])
    two = FixedNoiseOnlineSKIGP(Xt, _t(Y[:, :2], dtype), None, grid_bounds=torch.tensor(GB), grid_size=GS)
    with pytest.raises(NotImplementedError):                        # several outputs
        two.condition_on_observations(Xt, _t(Y[:, :2], dtype), grad_Y=G)
    probes = FixedNoiseOnlineSKIGP(Xt, _t(Y[:, :1], dtype), None, grid_bounds=torch.tensor(GB), grid_size=GS, num_path_probes=2)
    with pytest.raises(NotImplementedError):                        # a cache with path probes
        probes.condition_on_observations(Xt, _t(Y[:, 0], dtype), grad_Y=G)
    assert all(torch.equal(a, b) for a, b in zip(before, m.stats_buffers())) and m.num_data == 12
