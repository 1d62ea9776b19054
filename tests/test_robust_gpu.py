"""GPU: the outlier-robust absorb -- every point Huber-weighted against the posterior before its batch, inside the
launch that absorbs it -- against the fp64 reference of tests/robust_reference.py and the data-space oracle at noise d_i / omega_i:
the kernel through the C ABI, the contract, then the model surface.

Bounds: those of tests/test_grad_obs_gpu.py (scatter 1e-11 / 2e-4, x 10, relative to max |reference|; model 1e-4 / 1e-2; MLL 1e-7
dense, 0.05 matrix-free).  The measured deviations are tabulated in DESIGN.md 3.16.
"""
import ctypes

import numpy as np
import pytest
import torch

import robust_reference as rref
import sample_paths_reference as spr
from oracle import dataspace, spec

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [(torch.float64, 1e-11), (torch.float32, 2e-4)]          # the scatter tolerances of tests/test_grad_obs_gpu.py
RTOL = {torch.float64: 1e-4, torch.float32: 1e-2}
MLL_DENSE, MLL_FREE = 1e-7, 0.05
KGRIDS = {"d1": [8], "d2": [5, 7], "d3": [6, 5, 4], "d4": [5, 4, 4, 4]}
N = 37                                                            # not a multiple of the 4 points per block
KC = 1.5                                                          # the Huber threshold of the kernel cases
KEYS = ("A", "b", "cnt", "stats", "res")


# ------------------------------------------------------------------------------------------------------------------ the kernel
_cases = {}


def _kernel_case(name):
    """Grid, the 37-point layout of tests/test_grad_obs_gpu.py (fp64 values that are exact in fp32) and the dense reference; built
    once.  The targets are placed around the reference's own predictive mean so that every third point is an outlier."""
    if name in _cases:
        return _cases[name]
    from online_gp_amd import grid_ops

    g = KGRIDS[name]
    d = len(g)
    rng = np.random.default_rng(100 + d)
    grid = grid_ops.GridSpec([[-1.0, 1.0 + 0.25 * q] for q in range(d)], g)
    cell = np.stack([rng.integers(0, gq - 1, N) for gq in g], 1).astype(np.float64)
    frac = 0.5 + rng.choice([-1.0, 1.0], (N, d)) * rng.uniform(0.05, 0.45, (N, d))      # away from nodes and cell midpoints
    for q in range(d):
        cell[q, q] = 0                                              # points 0 .. d-1: first (boundary) cell of dim q
        cell[d + q, q] = g[q] - 2                                   # points d .. 2d-1: last (boundary) cell of dim q
    cell[12:17] = 1                                                 # five points in one interior cell: colliding atomics
    X = np.array(grid.g0) + np.array(grid.h) * (cell + frac)
    X[10, 0] = grid.g0[0] - 1.0                                      # two points outside the grid
    X[11, d - 1] = grid.g0[d - 1] + grid.h[d - 1] * (g[d - 1] - 1) + 1.0
    f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
    X = f32(X)
    noise = f32(rng.uniform(0.5, 2.0, N))
    wa = f32(1.0 / noise)
    inv_scale = f32(1.0 / np.sqrt(noise))
    u = f32(rng.standard_normal(grid.m))
    # |z|: every third point beyond the threshold (four of them beyond 10 c), the others at most c - 0.1
    az = rng.uniform(0.0, KC - 0.1, N)
    out = np.arange(0, N, 3)
    az[out] = rng.uniform(KC + 0.5, 4.0 * KC, out.size)
    az[out[:4]] = rng.uniform(10.0 * KC + 1.0, 20.0 * KC, 4)
    az[14] = 3.0 * KC                                                # one of the five colliding points as well
    z = az * rng.choice([-1.0, 1.0], N)
    mean = rref.dense_absorb(grid, X, np.zeros(N), wa, wa, noise, inv_scale, KC, u)["mean_out"]
    Y = f32(mean + z / inv_scale)
    ref = rref.dense_absorb(grid, X, Y, wa, wa, noise, inv_scale, KC, u)
    _cases[name] = dict(grid=grid, X=X, Y=Y, wa=wa, noise=noise, inv_scale=inv_scale, u=u, ref=ref, ok=rref.inside(grid, X))
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


@pytest.mark.parametrize("name", list(KGRIDS))
def test_reference_split_of_the_kernel_case(name):
    """About a third of the points beyond the threshold, some beyond ten times it, the rest at least 0.05 inside it."""
    c = _kernel_case(name)
    az, ok = np.abs(c["ref"]["z"]), c["ok"]
    outl = ok & (az > KC)
    print(f"{name}: {int(outl.sum())} of {int(ok.sum())} beyond c, {int((ok & (az > 10 * KC)).sum())} beyond 10 c, "
          f"largest inlier |z| {az[ok & ~outl].max():.4f}")
    assert int(ok.sum()) == N - 2 and 10 <= int(outl.sum()) <= 14 and int((ok & (az > 10 * KC)).sum()) >= 3
    assert (az[ok & ~outl] <= KC - 0.05).all() and outl[12:17].any() and (~outl[12:17]).any()
    om = c["ref"]["omega"]
    assert (om[ok & ~outl] == 1.0).all() and (om[~ok] == 0.0).all() and (om[outl] < 1.0).all() and om[outl].min() < 0.1


@pytest.mark.parametrize("tdt,tol", DTYPES)
@pytest.mark.parametrize("name", list(KGRIDS))
def test_kernel_matches_the_dense_reference(name, tdt, tol):
    from online_gp_amd import grid_ops

    test_reference_split_of_the_kernel_case(name)                    # the split holds on the reference before the kernel is looked at
    c = _kernel_case(name)
    grid, ref, ok = c["grid"], c["ref"], c["ok"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    X, Y, wa, noise, isc, u = (mk(c[k]) for k in ("X", "Y", "wa", "noise", "inv_scale", "u"))
    rname = dict(ref, A=ref["A_half"])
    # from zero
    got, err = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    mean = torch.full((N,), float("nan"), device=DEV, dtype=tdt)
    omega = grid_ops.scatter_stats_robust(grid, X, Y, wa, wa, noise, isc, KC, got["b"], got["A"], got["cnt"], got["stats"], err, u,
                                          res=got["res"], mean_out=mean)
    _compare(dict(got, mean_out=mean, omega=omega), rname, tol, KEYS + ("mean_out", "omega"), f"{name} zero-init")
    om = omega.double().cpu().numpy()
    inl = ok & (np.abs(ref["z"]) <= KC)
    assert (om[inl] == 1.0).all() and (om[~ok] == 0.0).all()         # exactly
    assert int(err.item()) == ref["err"] == 1 + 2 * 2                # bit 0 | two points dropped, each counted once
    # on top of non-zero buffers: every statistic is added, none assigned; the weights do not depend on what the buffers hold
    rng = np.random.default_rng(5)
    init = {k: 0.5 * float(np.abs(rname[k]).max()) * rng.standard_normal(np.shape(rname[k])) for k in KEYS}
    got = _buffers(grid, tdt, init)
    start = {k: v.double().cpu().numpy().copy() for k, v in got.items()}
    err.zero_()
    omega2 = grid_ops.scatter_stats_robust(grid, X, Y, wa, wa, noise, isc, KC, got["b"], got["A"], got["cnt"], got["stats"], err, u, res=got["res"])
    _compare(got, {k: start[k] + rname[k] for k in KEYS}, tol, KEYS, f"{name} on top")
    assert torch.equal(omega2, omega)


@pytest.mark.parametrize("tdt,tol", DTYPES)
@pytest.mark.parametrize("name", list(KGRIDS))
def test_kernel_with_zero_inverse_scale_is_the_plain_absorb(name, tdt, tol):
    from online_gp_amd import grid_ops

    c = _kernel_case(name)
    grid = c["grid"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    X, Y, wa, noise, u = (mk(c[k]) for k in ("X", "Y", "wa", "noise", "u"))
    got, want = _buffers(grid, tdt), _buffers(grid, tdt)
    e1, e2 = grid_ops.new_err_flag(DEV), grid_ops.new_err_flag(DEV)
    omega = grid_ops.scatter_stats_robust(grid, X, Y, wa, wa, noise, torch.zeros_like(Y), KC, got["b"], got["A"], got["cnt"], got["stats"], e1, u,
                                          res=got["res"])
    grid_ops.scatter_stats_cnt(grid, X, Y, wa, wa, noise, want["b"], want["A"], True, want["cnt"], want["stats"], e2, u=u, res=want["res"])
    _compare(got, {k: v.double().cpu().numpy() for k, v in want.items()}, tol, KEYS, f"{name} exempt")
    assert int(e1.item()) == int(e2.item()) == 5
    assert np.array_equal(omega.double().cpu().numpy(), c["ok"].astype(np.float64))


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64])
def test_absorb_refuses_the_robust_group_with_what_the_kernel_does_not_do(tdt):
    """Through the full argument record plus the robust group (wiski_absorb_robust): every combination the contract refuses is
    WISKI_E_BADARG before any launch -- every buffer untouched -- while the record without the offending field runs and equals
    grid_ops.scatter_stats_robust; res and mean_out are optional."""
    from online_gp_amd import _hip, grid_ops

    c = _kernel_case("d3")
    grid = c["grid"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    X, Y, wa, noise, isc, u = (mk(c[k]) for k in ("X", "Y", "wa", "noise", "inv_scale", "u"))
    buf, err = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    mean = torch.full((N,), float("nan"), device=DEV, dtype=tdt)
    omega = torch.full((N,), float("nan"), device=DEV, dtype=tdt)
    full = torch.zeros((grid.R, grid.m), device=DEV, dtype=tdt)
    guard = torch.tensor([7], device=DEV, dtype=torch.int64)
    z1 = torch.full((2,), 0x01010101, device=DEV, dtype=torch.int32)
    bin_ws = torch.zeros(1 << 16, device=DEV, dtype=torch.uint8)
    p = lambda t: t.data_ptr()
    stream = _hip.stream_ptr(torch.device("cuda", torch.cuda.current_device()))
    real = _hip.creal(tdt)

    def call(huber_c=KC, inv_scale=isc, omega_out=omega, **kw):
        a = _hip.wiski_absorb_args(d_x=p(X), d_y=p(Y), d_wa=p(wa), d_wb=p(wa), d_noise=p(noise), n=N, d_b=p(buf["b"]), d_A=p(buf["A"]), half=1,
                                   channels=0, d_cnt=p(buf["cnt"]), d_stats=p(buf["stats"]), d_err=p(err), d_u=p(u), d_res=p(buf["res"]),
                                   d_mean_out=p(mean), nout=1)
        for k, v in kw.items():
            setattr(a, k, v)
        return _hip.fn("wiski_absorb_robust", tdt)(grid.ref, ctypes.byref(a), _hip.dptr(inv_scale), real(huber_c), _hip.dptr(omega_out), stream)

    refused = [("no u", call(d_u=None, d_res=None, d_mean_out=None)), ("full stencil", call(half=0, d_A=p(full))), ("no A", call(d_A=None)),
               ("no cnt", call(d_cnt=None)), ("nout = 2", call(nout=2, d_mean_out=None)), ("channels", call(channels=4)),
               ("guard", call(d_guard=p(guard), guard_expect=7)), ("zero region", call(z1=p(z1), n1_bytes=8)), ("shard", call(g_lo=0, g_hi=3)),
               ("owner workspace", call(d_bin=p(bin_ws), bin_bytes=bin_ws.numel())), ("c = 0", call(huber_c=0.0)), ("c < 0", call(huber_c=-1.0)),
               ("c = inf", call(huber_c=float("inf"))), ("c = nan", call(huber_c=float("nan"))), ("no omega_out", call(omega_out=None)),
               ("no inv_scale", call(inv_scale=None))]
    torch.cuda.synchronize()
    assert [(what, rc) for what, rc in refused if rc != -1] == []
    assert all(float(v.abs().max()) == 0.0 for v in buf.values()) and float(full.abs().max()) == 0.0 and int(err.item()) == 0
    assert bool(torch.isnan(mean).all()) and bool(torch.isnan(omega).all()) and bool((z1 == 0x01010101).all())
    assert call() == 0
    want, e2 = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    om = grid_ops.scatter_stats_robust(grid, X, Y, wa, wa, noise, isc, KC, want["b"], want["A"], want["cnt"], want["stats"], e2, u, res=want["res"])
    tol = dict(DTYPES)[tdt]
    _compare(buf, {k: v.double().cpu().numpy() for k, v in want.items()}, tol, KEYS, "record")
    assert torch.equal(om, omega) and int(err.item()) == int(e2.item()) == 5
    assert call(d_res=None, d_mean_out=None) == 0                    # u alone is a complete request: res and mean_out are optional
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- the model
GB, GS = [[-1.0, 1.0], [-1.0, 1.0]], [12, 10]
MC = 2.0                                                           # the models' robust_c
N0, Q, NB, NBAD = 40, 16, 3, 3
STREAM_SEED = 4


def _f(X):
    return np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.5 * X[:, 1]


def _stream(seed=STREAM_SEED):
    """40 clean points, then 3 batches of 16 with 3 gross outliers each, offset by 15 to 25 noise standard deviations
    sqrt(sigma2 noise_i) (sigma2 = log 2, the model's default).  The declared noise is drawn from U(0.5, 2) for the reason
    tests/test_grad_obs_gpu.py::_data gives: the MLL bounds are relative."""
    rng = np.random.default_rng(seed)
    n = N0 + NB * Q
    X = rng.uniform(-0.95, 0.95, (n, 2))
    noise = rng.uniform(0.5, 2.0, n)
    y = _f(X) + 0.05 * rng.standard_normal(n)
    bad = np.zeros(n, dtype=bool)
    for k in range(NB):
        bad[N0 + k * Q + rng.choice(Q, NBAD, replace=False)] = True
    y[bad] += rng.choice([-1.0, 1.0], int(bad.sum())) * rng.uniform(15.0, 25.0, int(bad.sum())) * np.sqrt(spec.SOFTPLUS0 * noise[bad])
    Xs = rng.uniform(-0.95, 0.95, (50, 2))
    return X, y, noise, bad, Xs


def _oracle(hyp=None):
    ell, s, s2 = hyp if hyp is not None else (spec.SOFTPLUS0, spec.SOFTPLUS0, spec.SOFTPLUS0)
    return dataspace.DataSpaceGP(GB, GS, "rbf", ell, s, s2)


_refs = {}


def _reference_stream(c=MC, scale="noise", gamma=None, nb=NB, seed=STREAM_SEED, hyp=None):
    """The stream through the fp64 oracle: before batch k the oracle holds every earlier point at its effective noise (d_i / omega_i,
    aged by 1 / gamma per batch under forgetting); its predictive mean (and variance, "predictive") at the batch gives the batch's
    weights (robust_reference.huber_weights).  c = None: the plain model.  Returns per batch (omega, effective noise of all points so
    far, mean and variance at the queries, MLL); computed once per setting."""
    key = (c, scale, gamma, nb, seed, hyp)
    if key in _refs:
        return _refs[key]
    X, y, noise, bad, Xs = _stream(seed)
    O = _oracle(hyp)
    eff = noise.copy()
    steps = []
    for k in range(nb):
        lo, hi = N0 + k * Q, N0 + (k + 1) * Q
        if gamma is not None:
            eff[:lo] /= gamma
        O.fit(X[:lo], y[:lo], eff[:lo])
        mean, var = O.predict(X[lo:hi])
        scale2 = O.sigma2 * noise[lo:hi] + (var if scale == "predictive" else 0.0)
        omega = np.ones(Q) if c is None else rref.huber_weights(y[lo:hi], mean, 1.0 / np.sqrt(scale2), c)[0]
        eff[lo:hi] = noise[lo:hi] / omega
        O.fit(X[:hi], y[:hi], eff[:hi])
        mo, vo = O.predict(Xs)
        steps.append(dict(omega=omega, eff=eff[:hi].copy(), mean=mo, var=vo, mll=O.mll()))
    _refs[key] = steps
    return steps


def _t(a, dtype):
    return torch.as_tensor(a, device=DEV, dtype=dtype)


def _model(X, y, nz, dtype, **kw):
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    return FixedNoiseOnlineSKIGP(_t(X, dtype), _t(y, dtype)[:, None], _t(nz, dtype)[:, None], grid_bounds=torch.tensor(GB), grid_size=GS,
                                 learn_additional_noise=True, **kw)


def _hyp(m):
    k = m.covar_module.base_kernel
    return (tuple(float(v) for v in k.base_kernel.lengthscale.detach().cpu().reshape(-1)), float(k.outputscale), float(m.likelihood.second_noise))


def _mll(m):
    from online_gp_amd.mlls import BatchedWoodburyMarginalLogLikelihood

    m.train()
    v = float(BatchedWoodburyMarginalLogLikelihood(m.likelihood, m)(m(None), None).detach())
    m.eval()
    return v


def _check_against(m, step, Xs, dtype, label, mll_bound, omega=True):
    if omega:
        om = m.last_robust_weights.double().cpu().numpy()
        e_o = np.abs(om - step["omega"]).max()
        print(f"{label} {dtype}: omega {e_o:.3e}  (bound {RTOL[dtype]:.0e}; {int((step['omega'] < 1).sum())} of {om.size} down-weighted, "
              f"smallest {step['omega'].min():.4f})")
        assert e_o <= RTOL[dtype]
    mvn = m(_t(Xs, dtype))
    mean, var = mvn.mean.detach().double().cpu().numpy(), mvn.variance.detach().double().cpu().numpy()
    e_m, e_v = np.abs(mean - step["mean"]).max() / np.abs(step["mean"]).max(), np.abs(var - step["var"]).max() / np.abs(step["var"]).max()
    print(f"{label} {dtype}: mean {e_m:.3e}  var {e_v:.3e}  (bound {RTOL[dtype]:.0e})")
    assert e_m <= RTOL[dtype] and e_v <= RTOL[dtype]
    if dtype == torch.float64 and mll_bound is not None:
        v, r = _mll(m), step["mll"]
        print(f"{label}: mll {v:.10f}  reference {r:.10f}  rel {abs(v - r) / abs(r):.3e}  (bound {mll_bound:.0e})")
        assert abs(v - r) <= mll_bound * abs(r)


def _check_regime(dtype, label, mll_bound, **kw):
    X, y, noise, bad, Xs = _stream()
    m = _model(X[:N0], y[:N0], noise[:N0], dtype, robust_c=MC, **kw).eval()
    assert m.last_robust_weights is None                             # the initial data is absorbed plainly
    steps = _reference_stream(MC, kw.get("robust_scale", "noise"), kw.get("forgetting_factor"), hyp=_hyp(m))
    for k, step in enumerate(steps):
        lo, hi = N0 + k * Q, N0 + (k + 1) * Q
        assert (step["omega"][bad[lo:hi]] < 0.2).all()               # the planted outliers are what the reference down-weights
        m.condition_on_observations(_t(X[lo:hi], dtype), _t(y[lo:hi], dtype), _t(noise[lo:hi], dtype), inplace=True)
        assert m.num_data == hi and m.last_robust_weights.shape == (Q,) and m.last_robust_weights.is_cuda
        _check_against(m, step, Xs, dtype, f"{label} batch {k}", mll_bound)
    return m


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_dense_regime_matches_the_oracle_at_noise_over_omega(dtype):
    """12 x 10 grid, 40 clean points, 3 robust batches of 16 with 3 outliers each, 50 queries; figures printed before the asserts."""
    _check_regime(dtype, "dense", MLL_DENSE)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_matrix_free_regime_matches_the_oracle_at_noise_over_omega(dtype):
    from online_gp_amd import settings
    from online_gp_amd.mlls.batched_woodbury_marginal_log_likelihood import num_trace_samples

    with settings.dense_small_grids(False), settings.spectral_factor(False), num_trace_samples(64), \
            settings.cg_tolerance(1e-10 if dtype == torch.float64 else 1e-6):
        m = _check_regime(dtype, "matrix-free", MLL_FREE)
        assert m._mean_state is not None


def test_predictive_scale_adds_the_posterior_variance():
    dtype = torch.float64
    X, y, noise, bad, Xs = _stream()
    m = _model(X[:N0], y[:N0], noise[:N0], dtype, robust_c=MC, robust_scale="predictive").eval()
    step = _reference_stream(MC, "predictive", None, nb=1, hyp=_hyp(m))[0]
    other = _reference_stream(MC, "noise", None, nb=1, hyp=_hyp(m))[0]
    assert np.abs(step["omega"] - other["omega"]).max() > 10 * RTOL[dtype]      # the two scalings can be told apart
    sl = slice(N0, N0 + Q)
    m.condition_on_observations(_t(X[sl], dtype), _t(y[sl], dtype), _t(noise[sl], dtype), inplace=True)
    _check_against(m, step, Xs, dtype, "predictive", MLL_DENSE)


def test_functional_form_leaves_the_parent_alone_and_sets_the_weights_on_the_child():
    dtype = torch.float64
    X, y, noise, bad, Xs = _stream()
    m = _model(X[:N0], y[:N0], noise[:N0], dtype, robust_c=MC).eval()
    step = _reference_stream(MC, "noise", None, nb=1, hyp=_hyp(m))[0]
    before = [t.clone() for t in m.stats_buffers()]
    sl = slice(N0, N0 + Q)
    child = m.condition_on_observations(_t(X[sl], dtype), _t(y[sl], dtype), _t(noise[sl], dtype))
    assert all(torch.equal(a, b) for a, b in zip(before, m.stats_buffers())) and m.num_data == N0 and m.last_robust_weights is None
    assert child.robust_c == MC and child.robust_scale == "noise" and child.num_data == N0 + Q
    _check_against(child.eval(), step, Xs, dtype, "functional", MLL_DENSE)
    m.condition_on_observations(_t(X[sl], dtype), _t(y[sl], dtype), _t(noise[sl], dtype), inplace=True)
    _check_against(m, step, Xs, dtype, "in place", MLL_DENSE)


def test_forgetting_ages_the_effective_noise():
    """forgetting_factor = 0.9 with robust_c over two batches: the oracle at d_i gamma^-k / omega_i, the weights of a batch taken against
    the decayed posterior; in place and, for the second batch, functional."""
    dtype, gam = torch.float64, 0.9
    X, y, noise, bad, Xs = _stream()
    m = _model(X[:N0], y[:N0], noise[:N0], dtype, robust_c=MC, forgetting_factor=gam).eval()
    steps = _reference_stream(MC, "noise", gam, nb=2, hyp=_hyp(m))
    assert np.abs(steps[1]["mean"] - _reference_stream(MC, "noise", None, nb=2, hyp=_hyp(m))[1]["mean"]).max() > 10 * RTOL[dtype] * np.abs(steps[1]["mean"]).max()
    sl = slice(N0, N0 + Q)
    m.condition_on_observations(_t(X[sl], dtype), _t(y[sl], dtype), _t(noise[sl], dtype), inplace=True)
    _check_against(m, steps[0], Xs, dtype, "forgetting batch 0", MLL_DENSE)
    sl = slice(N0 + Q, N0 + 2 * Q)
    child = m.condition_on_observations(_t(X[sl], dtype), _t(y[sl], dtype), _t(noise[sl], dtype))
    _check_against(child.eval(), steps[1], Xs, dtype, "forgetting batch 1, functional", MLL_DENSE)
    m.condition_on_observations(_t(X[sl], dtype), _t(y[sl], dtype), _t(noise[sl], dtype), inplace=True)
    _check_against(m, steps[1], Xs, dtype, "forgetting batch 1, in place", MLL_DENSE)


def test_path_probes_receive_the_effective_weights():
    """num_path_probes > 0, PCG route: after a robust batch the sample paths equal Matheron's rule in data space at the weights
    omega_i / d_i, path by path -- the probes entered with sqrt(wa omega), so cov(P) is still A.  Bound: that of
    tests/test_sample_paths_gpu.py, 3 x the deviation of the model's own posterior mean from the oracle."""
    from online_gp_amd import settings
    from online_gp_amd.kernels import GridInterpolationKernel, MaternKernel, ScaleKernel
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    dtype, S, seed, ell, osc, s2 = torch.float64, 8, 21, [0.35, 0.5], 1.2, 0.3
    X, y, noise, bad, Xs = _stream()
    n = N0 + Q
    with settings.dense_small_grids(False), settings.spectral_factor(False), settings.cg_tolerance(1e-10), torch.no_grad():
        k = GridInterpolationKernel(ScaleKernel(MaternKernel(nu=2.5, ard_num_dims=2)), grid_size=GS, num_dims=2, grid_bounds=torch.tensor(GB))
        k.base_kernel.outputscale = osc
        k.base_kernel.base_kernel.lengthscale = torch.as_tensor(ell)
        m = FixedNoiseOnlineSKIGP(_t(X[:N0], dtype), _t(y[:N0], dtype)[:, None], _t(noise[:N0], dtype)[:, None], covar_module=k,
                                  learn_additional_noise=True, num_path_probes=S, path_seed=seed, robust_c=MC)
        m.likelihood.second_noise = s2
        m.eval()
        m.condition_on_observations(_t(X[N0:n], dtype), _t(y[N0:n], dtype), _t(noise[N0:n], dtype), inplace=True)
        O = dataspace.DataSpaceGP(GB, GS, "matern52", ell, osc, s2).fit(X[:N0], y[:N0], noise[:N0])
        omega = rref.huber_weights(y[N0:n], O.predict(X[N0:n])[0], 1.0 / np.sqrt(s2 * noise[N0:n]), MC)[0]
        assert (omega[bad[N0:n]] < 0.2).all() and np.abs(m.last_robust_weights.cpu().numpy() - omega).max() <= RTOL[dtype]
        wts = np.concatenate([np.ones(N0), omega]) / noise[:n]
        O.fit(X[:n], y[:n], 1.0 / wts)
        g0, h, gg = spec.make_grid(GB, GS)
        W, Kuu = spr.dense_w(g0, h, gg, X[:n]), spr.kuu_dense(O.cols)
        u_mean = Kuu @ (W.T @ O.alpha)
        z = torch.randn((S, m._grid.m), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        paths = m.sample_paths(S, base_samples=z.to(DEV))
        assert paths.last_converged
        U = m.prediction_cache["pred_mean"][0, :, 0].cpu().numpy()
        dev_mean = np.abs(U - u_mean).max() / np.abs(u_mean).max()
        uo = spr.path_dataspace(Kuu, W, wts, y[:n], s2, (spr.sym_sqrt(Kuu) @ z.numpy().T).T, spr.normals(seed, np.arange(n), S))
        dev_path = np.abs(paths.values.cpu().numpy() - uo).max() / np.abs(uo).max()
        plain = spr.path_dataspace(Kuu, W, 1.0 / noise[:n], y[:n], s2, (spr.sym_sqrt(Kuu) @ z.numpy().T).T, spr.normals(seed, np.arange(n), S))
        print(f"robust paths: path deviation {dev_path:.3e}, mean deviation {dev_mean:.3e}, ratio {dev_path / dev_mean:.2f}; "
              f"distance to the plainly weighted paths {np.abs(plain - uo).max() / np.abs(uo).max():.3e}")
        assert dev_path <= 3.0 * dev_mean
        assert np.abs(plain - uo).max() / np.abs(uo).max() > 1e-2      # (the check can tell the effective weights from the plain ones)


def _rmse(mean, Xs):
    return float(np.sqrt(np.mean((mean - _f(Xs)) ** 2)))


def test_robust_model_is_closer_to_the_truth_than_the_plain_one():
    """Same stream, same hyper-parameters: RMSE to the noise-free truth at the queries.  The stream is one on which the two fp64
    references differ by at least a factor of 2 (asserted here first, on the CPU references)."""
    dtype = torch.float64
    X, y, noise, bad, Xs = _stream()
    r_rob, r_plain = _rmse(_reference_stream(MC)[-1]["mean"], Xs), _rmse(_reference_stream(None)[-1]["mean"], Xs)
    print(f"reference RMSE: robust {r_rob:.4f}  plain {r_plain:.4f}  ratio {r_plain / r_rob:.2f}")
    assert r_plain >= 2.0 * r_rob
    got = {}
    for name, kw in (("robust", dict(robust_c=MC)), ("plain", {})):
        m = _model(X[:N0], y[:N0], noise[:N0], dtype, **kw).eval()
        for lo in range(N0, N0 + NB * Q, Q):
            m.condition_on_observations(_t(X[lo:lo + Q], dtype), _t(y[lo:lo + Q], dtype), _t(noise[lo:lo + Q], dtype), inplace=True)
        got[name] = _rmse(m(_t(Xs, dtype)).mean.detach().cpu().numpy(), Xs)
    print(f"model RMSE: robust {got['robust']:.4f}  plain {got['plain']:.4f}")
    assert got["robust"] < got["plain"]


def test_default_model_never_enters_the_robust_path(monkeypatch):
    """Without robust_c the robust launch is never made (the binding is replaced by one that raises), and two plain models fed the
    stream hold the same statistics: the two scalars, which one block reduces in a fixed order, bit for bit; b, cnt and the half
    stencil, which are sums of floating-point atomics whose order the hardware does not fix, to within what reordering a sum can
    change -- |fl(sum) - sum| <= (n - 1) eps sum|terms| for any order (Higham, Accuracy and Stability, 4.2), so two orders differ by
    at most 2 n eps sum|terms|, with sum|terms| from the dense rows of the reference (largest entry of each buffer), n = 88 points.
    (Bit-equality of the atomic sums was asserted first and does not hold for the unchanged plain absorb: on one MI355X two plain
    models differed in last bits.)"""
    from online_gp_amd import grid_ops

    def forbidden(*a, **k):
        raise AssertionError("the robust absorb was launched by a model without robust_c")

    monkeypatch.setattr(grid_ops, "scatter_stats_robust", forbidden)
    dtype = torch.float64
    X, y, noise, bad, Xs = _stream()
    models = []
    for _ in range(2):
        m = _model(X[:N0], y[:N0], noise[:N0], dtype).eval()
        for lo in range(N0, N0 + NB * Q, Q):
            m.condition_on_observations(_t(X[lo:lo + Q], dtype), _t(y[lo:lo + Q], dtype), _t(noise[lo:lo + Q], dtype), inplace=True)
        assert m.robust_c is None and m.last_robust_weights is None
        models.append(m)
    g0, h, gg = spec.make_grid(GB, GS)
    Wa = np.abs(spr.dense_w(g0, h, gg, X))
    n, eps = X.shape[0], np.finfo(np.float64).eps
    asum = [float((Wa.T @ np.abs(y / noise)).max()), 0.0, float((Wa.T @ (1.0 / noise)).max()), float((Wa.T @ (Wa / noise[:, None])).max())]
    for name, a, b, s_abs in zip(("b", "stats", "cnt", "A"), models[0].stats_buffers(), models[1].stats_buffers(), asum):
        dev = float((a - b).abs().max())
        print(f"two plain models, {name}: max difference {dev:.3e}  bound {2 * n * eps * s_abs:.3e}  ({int((a != b).sum())} of {a.numel()} entries differ)")
        assert dev <= 2 * n * eps * s_abs
    assert torch.equal(models[0].stats_buffers()[1], models[1].stats_buffers()[1]) and models[0].num_data == models[1].num_data == n


def test_stream_step_takes_the_generic_path_and_weights_its_batch():
    from online_gp_amd import settings

    dtype = torch.float32
    X, y, noise, bad, Xs = _stream()
    with settings.dense_small_grids(False), settings.spectral_factor(False):
        m = _model(X[:N0], y[:N0], np.ones(N0), dtype, robust_c=MC).eval()
        m.prediction_cache
        sl = slice(N0, N0 + Q)
        assert m._stream_fast_state(_t(X[sl], dtype), _t(y[sl], dtype)) is None
        mean = m.stream_step(_t(X[sl], dtype), _t(y[sl], dtype))
        om = m.last_robust_weights.cpu().numpy()
        assert mean.shape == (Q,) and m.num_data == N0 + Q and (om[bad[sl]] < 0.2).all() and (om[~bad[sl]] == 1.0).all()


def test_refusals():
    from online_gp_amd.distributed import ShardedStatsUpdater
    from online_gp_amd.models import FixedNoiseOnlineSKIGP, OnlineSKIBotorchModel

    dtype = torch.float64
    X, y, noise, bad, Xs = _stream()
    Xt, yt, nt = _t(X[:12], dtype), _t(y[:12], dtype), _t(noise[:12], dtype)
    with pytest.raises(NotImplementedError):                        # several outputs, at construction
        FixedNoiseOnlineSKIGP(Xt, torch.stack([yt, yt], 1), None, grid_bounds=torch.tensor(GB), grid_size=GS, robust_c=MC)
    with pytest.raises(ValueError):
        _model(X[:12], y[:12], noise[:12], dtype, robust_c=0.0)
    with pytest.raises(ValueError):
        _model(X[:12], y[:12], noise[:12], dtype, robust_c=MC, robust_scale="variance")
    m = _model(X[:12], y[:12], noise[:12], dtype, robust_c=MC)
    before = [t.clone() for t in m.stats_buffers()]
    with pytest.raises(NotImplementedError):                        # derivative observations
        m.condition_on_observations(Xt, yt, nt, grad_Y=torch.zeros(12, 2, device=DEV, dtype=dtype))
    with pytest.raises(NotImplementedError):                        # the data-parallel statistics exchange
        m._absorb(m._kernel_cache, Xt, yt, nt[:, None], init=False, half_delta=m._half_buffers())
    with pytest.raises(NotImplementedError):
        ShardedStatsUpdater(m)
    assert all(torch.equal(a, b) for a, b in zip(before, m.stats_buffers())) and m.num_data == 12
    # a handed-over full-stencil cache
    cache = m._clone_cache(m._kernel_cache)
    op = cache["WtW"]
    full = torch.zeros((m._grid.R, m._grid.m), device=DEV, dtype=dtype)
    cache["WtW"] = type(op)(m._grid, full)
    h = FixedNoiseOnlineSKIGP(covar_module=m.covar_module, kernel_cache=cache, likelihood=m.likelihood, learn_additional_noise=True, num_data=12,
                              robust_c=MC)
    with pytest.raises(NotImplementedError):
        h.condition_on_observations(Xt, yt, nt, inplace=True)
    # fantasies (batched X) ignore robust_c; the wrappers pass the arguments through
    fant = m.condition_on_observations(Xt[None], yt[None], nt[None])
    assert fant is not None and m.last_robust_weights is None
    b = OnlineSKIBotorchModel(Xt, yt[:, None], nt[:, None], grid_bounds=torch.tensor(GB), grid_size=GS, robust_c=MC, robust_scale="predictive")
    assert b.robust_c == MC and b.robust_scale == "predictive"
