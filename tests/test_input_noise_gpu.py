"""GPU: noisy-input observations -- every point of a batch enters at a noise inflated by the slope of the posterior
before it, inside the launch that absorbs it -- against the fp64 reference of tests/input_noise_reference.py: the kernel through the C
ABI, the contract, the model surface, and the toy stream on which the feature has to pay.

Bounds.  Statistics: those of tests/test_grad_obs_gpu.py (scatter 1e-11 / 2e-4, x 10, relative to max |reference|).  Sites in fp64: 1e-9
relative -- omega, log Z and the slope each of its own value; a slope whose dot product has cancelled below 1e-3 of its magnitude
sum_a |v_k[a] u[a]| is held to 1e-9 of that magnitude instead (relative to itself it would measure the cancellation).  Sites in
fp32 get no hand-picked number: the reference gives per point the running error bound of the kernel's fp32 dot products,
(4^d + 2) eps32 sum_a |v[a] u[a]|, propagated through the site (input_noise_reference.fp32_bounds).  Model:
1e-4 / 1e-2, MLL 1e-7 dense, 0.05 matrix-free (the interval form's bounds).  The measured deviations are tabulated in DESIGN.md 3.24.
"""
import ctypes

import numpy as np
import pytest
import torch

import input_noise_reference as nref
from input_noise_reference import HUGE, KGRIDS, KS2, N, NANXI, OUTSIDE, ZERO
import sample_paths_reference as spr
from oracle import dataspace, spec

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [(torch.float64, 1e-11), (torch.float32, 2e-4)]          # the scatter tolerances of tests/test_grad_obs_gpu.py
RTOL = {torch.float64: 1e-4, torch.float32: 1e-2}
MLL_DENSE, MLL_FREE = 1e-7, 0.05
KEYS = ("A", "b", "cnt", "stats", "res")
FP64_SITE = 1e-9


# ------------------------------------------------------------------------------------------------------------------ the kernel
_kernel_case = nref.kernel_case


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


@pytest.mark.parametrize("with_gvar", [True, False])
@pytest.mark.parametrize("tdt,tol", DTYPES)
@pytest.mark.parametrize("name", list(KGRIDS))
def test_kernel_matches_the_dense_reference(name, tdt, tol, with_gvar):
    """fp64: 1e-9 relative.  fp32: the per-point bound of input_noise_reference.fp32_bounds around the fp64 reference -- the rounding of
    the kernel's fp32 dot products and of the stored values, nothing for the weights: the fp32 sweep of this site evaluates its
    interpolation weights in double (SiteInputNoise::refine), without which the slope lay 1.7 times the bound off at d = 1."""
    from online_gp_amd import grid_ops

    c = _kernel_case(name)
    grid, ok, d = c["grid"], c["ok"], c["d"]
    ref = c["ref" if with_gvar else "ref_mean"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    X, y, xvar, gvar, wa, noise, pvar, u = (mk(c[k]) for k in ("X", "y", "xvar", "gvar", "wa", "noise", "pvar", "u"))
    gv = gvar if with_gvar else None
    rname = dict(ref, A=ref["A_half"])
    got, err = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    mean = torch.full((N,), float("nan"), device=DEV, dtype=tdt)
    omega, log_z, grad = grid_ops.scatter_stats_input_noise(grid, X, y, xvar, gv, pvar, KS2, wa, wa, noise, got["b"], got["A"], got["cnt"], got["stats"],
                                                            err, u, res=got["res"], mean_out=mean, want_grad=True)
    assert omega.dtype == tdt and grad.dtype == tdt and log_z.dtype == torch.float64 and tuple(grad.shape) == (N, d)
    om, lz, gr = (t.double().cpu().numpy() for t in (omega, log_z, grad))
    fin = np.isfinite(ref["log_z"])
    # the site bounds, per point
    site_ref = ref
    if tdt == torch.float64:
        # the slope: 1e-9 of the magnitude its dot product is relative to, AND 1e-9 of the slope itself wherever the dot product has not
        # cancelled away (|g| at least 1e-3 of the magnitude; below that "relative to |g|" measures the cancellation, not the kernel)
        kept = np.abs(ref["grad"]) >= 1e-3 * ref["abs_grad"]
        bound = dict(grad=FP64_SITE * np.where(kept, np.abs(ref["grad"]), ref["abs_grad"]), omega=FP64_SITE * ref["omega"],
                     log_z=FP64_SITE * np.abs(np.where(fin, ref["log_z"], 0.0)))
    else:
        bound = nref.fp32_bounds(ref, c["y"], c["xvar"], c["pvar"], c["dn"], d)
    dev = dict(grad=np.abs(gr - site_ref["grad"]), omega=np.abs(om - site_ref["omega"]), log_z=np.abs(np.where(fin, lz - site_ref["log_z"], 0.0)))
    for k in dev:
        worst = float((dev[k] / np.where(bound[k] > 0, bound[k], 1.0))[bound[k] > 0].max()) if (bound[k] > 0).any() else 0.0
        scale = dict(grad=site_ref["abs_grad"], omega=np.where(site_ref["omega"] > 0, site_ref["omega"], 1.0),
                     log_z=np.abs(np.where(fin & (site_ref["log_z"] != 0), site_ref["log_z"], 1.0)))[k]
        print(f"{name} {tdt} gvar={with_gvar} {k}: largest deviation {float(dev[k].max()):.3e}, relative {float((dev[k] / np.where(scale > 0, scale, 1.0)).max()):.3e}, "
              f"largest deviation / bound {worst:.3f}")
    _compare(dict(got, mean_out=mean), rname, tol, KEYS + ("mean_out",), f"{name} zero-init")
    assert np.array_equal(om == 0.0, ref["omega"] == 0.0)             # who is skipped (and who is outside): exactly the reference's
    assert (om[list(ZERO)] == 1.0).all()                              # xvar = 0: exactly one
    assert np.array_equal(np.isnan(lz), np.isnan(ref["log_z"])) and lz[OUTSIDE] == 0.0 and (gr[OUTSIDE] == 0.0).all()
    for q in range(d):
        assert gr[4 + q, q] == 0.0 and gr[20 + q, q] == 0.0
    assert int(err.item()) == ref["err"] == 1 + 2 * 1                # bit 0 | one point dropped; a skipped point is not flagged
    for k in dev:
        assert (dev[k] <= bound[k]).all(), (name, k, int(np.argmax(dev[k] - bound[k])), float((dev[k] - bound[k]).max()))
    # on top of non-zero buffers: every statistic is added, none assigned; the sites do not depend on what the buffers hold
    rng = np.random.default_rng(5)
    init = {k: 0.5 * float(np.abs(rname[k]).max()) * rng.standard_normal(np.shape(rname[k])) for k in KEYS}
    got = _buffers(grid, tdt, init)
    start = {k: v.double().cpu().numpy().copy() for k, v in got.items()}
    err.zero_()
    om2, lz2 = grid_ops.scatter_stats_input_noise(grid, X, y, xvar, gv, pvar, KS2, wa, wa, noise, got["b"], got["A"], got["cnt"], got["stats"], err, u, res=got["res"])
    _compare(got, {k: start[k] + rname[k] for k in KEYS}, tol, KEYS, f"{name} on top")
    assert torch.equal(omega, om2) and torch.equal(torch.nan_to_num(log_z, nan=7.0), torch.nan_to_num(lz2, nan=7.0))


@pytest.mark.parametrize("tdt,tol", DTYPES)
@pytest.mark.parametrize("name", list(KGRIDS))
def test_kernel_with_zero_input_variance_is_the_plain_absorb(name, tdt, tol):
    from online_gp_amd import grid_ops

    c = _kernel_case(name)
    grid = c["grid"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    X, y, gvar, wa, noise, pvar, u = (mk(c[k]) for k in ("X", "y", "gvar", "wa", "noise", "pvar", "u"))
    got, want = _buffers(grid, tdt), _buffers(grid, tdt)
    e1, e2 = grid_ops.new_err_flag(DEV), grid_ops.new_err_flag(DEV)
    omega, _ = grid_ops.scatter_stats_input_noise(grid, X, y, torch.zeros_like(gvar), gvar, pvar, KS2, wa, wa, noise, got["b"], got["A"], got["cnt"], got["stats"],
                                                  e1, u, res=got["res"])
    grid_ops.scatter_stats_cnt(grid, X, y, wa, wa, noise, want["b"], want["A"], True, want["cnt"], want["stats"], e2, u=u, res=want["res"])
    _compare(got, {k: v.double().cpu().numpy() for k, v in want.items()}, tol, KEYS, f"{name} zero variance")
    assert int(e1.item()) == int(e2.item()) == 3
    assert np.array_equal(omega.double().cpu().numpy(), c["ok"].astype(np.float64))


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64])
def test_absorb_refuses_the_input_noise_group_with_what_the_kernel_does_not_do(tdt):
    """Through the full argument record plus the group (wiski_absorb_input_noise): every combination the contract refuses is
    WISKI_E_BADARG before any launch -- every buffer untouched -- while the record without the offending field runs and equals
    grid_ops.scatter_stats_input_noise; res, mean_out, gvar and grad_out are optional."""
    from online_gp_amd import _hip, grid_ops

    c = _kernel_case("d3")
    grid = c["grid"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    X, y, xvar, gvar, wa, noise, pvar, u = (mk(c[k]) for k in ("X", "y", "xvar", "gvar", "wa", "noise", "pvar", "u"))
    buf, err = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    nan = lambda dt=tdt, *s: torch.full(s or (N,), float("nan"), device=DEV, dtype=dt)
    mean, omega, logz, grad = nan(), nan(), nan(torch.float64), nan(tdt, N, 3)
    full = torch.zeros((grid.R, grid.m), device=DEV, dtype=tdt)
    guard = torch.tensor([7], device=DEV, dtype=torch.int64)
    z1 = torch.full((2,), 0x01010101, device=DEV, dtype=torch.int32)
    bin_ws = torch.zeros(1 << 16, device=DEV, dtype=torch.uint8)
    p = lambda t: t.data_ptr()
    stream = _hip.stream_ptr(torch.device("cuda", torch.cuda.current_device()))

    def call(xvar_=xvar, gvar_=gvar, pvar_=pvar, sigma2=KS2, omega_=omega, logz_=logz, grad_=grad, **kw):
        a = _hip.wiski_absorb_args(d_x=p(X), d_y=p(y), d_wa=p(wa), d_wb=p(wa), d_noise=p(noise), n=N, d_b=p(buf["b"]), d_A=p(buf["A"]), half=1,
                                   channels=0, d_cnt=p(buf["cnt"]), d_stats=p(buf["stats"]), d_err=p(err), d_u=p(u), d_res=p(buf["res"]),
                                   d_mean_out=p(mean), nout=1)
        for k, v in kw.items():
            setattr(a, k, v)
        return _hip.fn("wiski_absorb_input_noise", tdt)(grid.ref, ctypes.byref(a), _hip.dptr(xvar_), _hip.dptr(gvar_), _hip.dptr(pvar_), ctypes.c_double(sigma2),
                                                        _hip.dptr(omega_), _hip.dptr(logz_), _hip.dptr(grad_), stream)

    refused = [("no u", call(d_u=None, d_res=None, d_mean_out=None)), ("full stencil", call(half=0, d_A=p(full))), ("no A", call(d_A=None)),
               ("no cnt", call(d_cnt=None)), ("no y", call(d_y=None)), ("nout = 2", call(nout=2, d_mean_out=None)), ("channels", call(channels=4)),
               ("guard", call(d_guard=p(guard), guard_expect=7)), ("zero region", call(z1=p(z1), n1_bytes=8)), ("shard", call(g_lo=0, g_hi=3)),
               ("owner workspace", call(d_bin=p(bin_ws), bin_bytes=bin_ws.numel())), ("sigma2 = 0", call(sigma2=0.0)), ("sigma2 < 0", call(sigma2=-1.0)),
               ("sigma2 = inf", call(sigma2=float("inf"))), ("sigma2 = nan", call(sigma2=float("nan"))), ("no xvar", call(xvar_=None)),
               ("no pvar", call(pvar_=None)), ("no omega_out", call(omega_=None)), ("no logz_out", call(logz_=None))]
    torch.cuda.synchronize()
    assert [(what, rc) for what, rc in refused if rc != -1] == []
    assert all(float(v.abs().max()) == 0.0 for v in buf.values()) and float(full.abs().max()) == 0.0 and int(err.item()) == 0
    assert all(bool(torch.isnan(t).all()) for t in (mean, omega, logz, grad)) and bool((z1 == 0x01010101).all())
    assert call() == 0
    want, e2 = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    sites = grid_ops.scatter_stats_input_noise(grid, X, y, xvar, gvar, pvar, KS2, wa, wa, noise, want["b"], want["A"], want["cnt"], want["stats"], e2, u,
                                               res=want["res"], want_grad=True)
    _compare(buf, {k: v.double().cpu().numpy() for k, v in want.items()}, dict(DTYPES)[tdt], KEYS, "record")
    same = lambda a, b: torch.equal(torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0))
    assert all(same(a, b) for a, b in zip(sites, (omega, logz, grad))) and int(err.item()) == int(e2.item()) == 3
    assert call(d_res=None, d_mean_out=None, gvar_=None, grad_=None) == 0       # u alone is a complete request; no slope variance, no slopes reported
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- the model
GB, GS = [[-1.0, 1.0], [-1.0, 1.0]], [12, 12]
N0, Q, NB = 40, 16, 3
SX = 0.05


def _f(X):
    return np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.5 * X[:, 1]


def _stream(seed=4):
    """40 points at exact locations, then 3 batches of 16 whose recorded locations are off by N(0, xvar_ik), xvar between (SX / 2)^2 and
    (2 SX)^2 per point and dimension; 50 queries.  The declared noise is drawn from U(0.5, 2) for the reason
    tests/test_grad_obs_gpu.py::_data gives: the MLL bounds are relative."""
    rng = np.random.default_rng(seed)
    n = N0 + NB * Q
    Xt = rng.uniform(-0.9, 0.9, (n, 2))
    noise = rng.uniform(0.5, 2.0, n)
    y = _f(Xt) + 0.05 * rng.standard_normal(n)
    xvar = (SX * rng.uniform(0.5, 2.0, (n, 2))) ** 2
    X = Xt + np.sqrt(xvar) * rng.standard_normal((n, 2))
    X[:N0] = Xt[:N0]
    return X, y, noise, xvar, rng.uniform(-0.9, 0.9, (50, 2))


def _t(a, dtype):
    return torch.as_tensor(a, device=DEV, dtype=dtype)


def _model(X, y, nz, dtype, **kw):
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    return FixedNoiseOnlineSKIGP(_t(X, dtype), _t(y, dtype)[:, None], _t(nz, dtype)[:, None], grid_bounds=torch.tensor(kw.pop("bounds", GB)),
                                 grid_size=kw.pop("size", GS), learn_additional_noise=True, **kw)


def _hyp(m):
    k = m.covar_module.base_kernel
    return (tuple(float(v) for v in k.base_kernel.lengthscale.detach().cpu().reshape(-1)), float(k.outputscale), float(m.likelihood.second_noise))


def _mll(m):
    from online_gp_amd.mlls import BatchedWoodburyMarginalLogLikelihood

    m.train()
    v = float(BatchedWoodburyMarginalLogLikelihood(m.likelihood, m)(m(None), None).detach())
    m.eval()
    return v


_refs = {}


def _reference_stream(hyp, gamma=None, nb=NB, slope="posterior", bounds=GB, size=GS):
    """The stream through the dense reference model: per batch (sites, mean and variance at the queries, MLL, points held, the
    prediction at uncertain queries); computed once per setting."""
    key = (hyp, gamma, nb, slope, str(bounds), str(size))
    if key in _refs:
        return _refs[key]
    X, y, noise, xvar, Xs = _stream()
    M = nref.DenseStream(bounds, size, list(hyp[0]), hyp[1], hyp[2], slope=slope, gamma=gamma)
    M.absorb(X[:N0], y[:N0], noise[:N0], plain=True)
    steps = []
    for k in range(nb):
        sl = slice(N0 + k * Q, N0 + (k + 1) * Q)
        M.absorb(X[sl], y[sl], noise[sl], xvar[sl])
        mo, vo = M.predict(Xs)
        steps.append(dict(sites=M.last, mean=mo, var=vo, mll=M.mll(), n=M.y.shape[0], noisy=M.predict_noisy_input(Xs, [SX ** 2, 4 * SX ** 2])))
    _refs[key] = steps
    return steps


def _check_against(m, step, Xs, dtype, label, mll_bound, sites=True):
    if sites:
        om, lz, gr = (t.double().cpu().numpy() for t in m.last_input_noise_sites)
        st = step["sites"]
        e_o, e_l = np.abs(om - st["omega"]).max(), np.abs(lz - st["log_z"]).max() / np.abs(st["log_z"]).max()
        e_g = np.abs(gr - st["grad"]).max() / np.abs(st["grad"]).max()
        print(f"{label} {dtype}: omega {e_o:.3e}  log Z {e_l:.3e}  slope {e_g:.3e}  (bound {RTOL[dtype]:.0e}; omega {st['omega'].min():.4f} .. {st['omega'].max():.4f})")
        assert e_o <= RTOL[dtype] and e_l <= RTOL[dtype] and e_g <= RTOL[dtype]
        assert np.array_equal(om == 0.0, st["skipped"]) and m.num_data == step["n"]
    mvn = m(_t(Xs, dtype))
    mean, var = mvn.mean.detach().double().cpu().numpy(), mvn.variance.detach().double().cpu().numpy()
    e_m, e_v = np.abs(mean - step["mean"]).max() / np.abs(step["mean"]).max(), np.abs(var - step["var"]).max() / np.abs(step["var"]).max()
    print(f"{label} {dtype}: mean {e_m:.3e}  var {e_v:.3e}  (bound {RTOL[dtype]:.0e})")
    assert e_m <= RTOL[dtype] and e_v <= RTOL[dtype]
    if dtype == torch.float64 and mll_bound is not None:
        v, r = _mll(m), step["mll"]
        print(f"{label}: mll {v:.10f}  reference {r:.10f}  rel {abs(v - r) / abs(r):.3e}  (bound {mll_bound:.0e})")
        assert abs(v - r) <= mll_bound * abs(r)


def _absorb_batch(m, k, dtype, inplace=True, **kw):
    X, y, noise, xvar, Xs = _stream()
    sl = slice(N0 + k * Q, N0 + (k + 1) * Q)
    return m.condition_on_observations(_t(X[sl], dtype), _t(y[sl], dtype), _t(noise[sl], dtype), input_var=_t(xvar[sl], dtype), inplace=inplace, **kw)


def _check_regime(dtype, label, mll_bound, slope="posterior", **kw):
    X, y, noise, xvar, Xs = _stream()
    m = _model(X[:N0], y[:N0], noise[:N0], dtype, input_noise_slope=slope, **kw).eval()
    assert m.last_input_noise_sites is None                          # the initial data is absorbed plainly
    steps = _reference_stream(_hyp(m), kw.get("forgetting_factor"), slope=slope)
    for k, step in enumerate(steps):
        assert 0.0 < step["sites"]["omega"].min() and step["sites"]["omega"].max() < 1.0
        _absorb_batch(m, k, dtype)
        assert [tuple(t.shape) for t in m.last_input_noise_sites] == [(Q,), (Q,), (Q, 2)] and all(t.is_cuda for t in m.last_input_noise_sites)
        _check_against(m, step, Xs, dtype, f"{label} batch {k}", mll_bound)
    return m


@pytest.mark.parametrize("slope", ["posterior", "mean"])
def test_dense_regime_matches_the_reference_model_2d(slope):
    """12 x 12 grid, 40 exact points, 3 batches of 16 at uncertain locations, 50 queries; both slope rules; figures before the asserts."""
    _check_regime(torch.float64, f"dense 2-d {slope}", MLL_DENSE, slope=slope)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_matrix_free_regime_matches_the_reference_model(dtype):
    from online_gp_amd import settings
    from online_gp_amd.mlls.batched_woodbury_marginal_log_likelihood import num_trace_samples

    with settings.dense_small_grids(False), settings.spectral_factor(False), num_trace_samples(64), \
            settings.cg_tolerance(1e-10 if dtype == torch.float64 else 1e-6):
        m = _check_regime(dtype, "matrix-free", MLL_FREE)
        assert m._mean_state is not None


# the toy problem of the design: tanh(12 (x - 1/2)) recorded at locations off by sigma_x = 0.03, 8 batches of 16 from a cold start
def _toy_model(dtype, seed, input_var, slope="posterior"):
    """The model of the toy problem, started from one point that says nothing (noise 1e6), fed the stream of `seed`; returns it and the
    per-batch sites."""
    from online_gp_amd.kernels import GridInterpolationKernel, RBFKernel, ScaleKernel
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    T = nref.TOY
    X, y, Xs = nref.toy_stream(seed)
    with torch.no_grad():
        k = GridInterpolationKernel(ScaleKernel(RBFKernel(ard_num_dims=1)), grid_size=T["size"], num_dims=1, grid_bounds=torch.tensor(T["bounds"]))
        k.base_kernel.outputscale = T["osc"]
        k.base_kernel.base_kernel.lengthscale = torch.as_tensor(T["ell"])
        m = FixedNoiseOnlineSKIGP(_t([[0.5]], dtype), _t([[0.0]], dtype), _t([[1e6]], dtype), covar_module=k, learn_additional_noise=True,
                                  input_var=input_var, input_noise_slope=slope)
        m.likelihood.second_noise = T["sigma_y"] ** 2
        m.eval()
        sites = []
        for a in range(0, X.shape[0], T["q"]):
            m.condition_on_observations(_t(X[a:a + T["q"]], dtype), _t(y[a:a + T["q"]], dtype), torch.ones(T["q"], device=DEV, dtype=dtype), inplace=True)
            sites.append(m.last_input_noise_sites)
    return m, sites


_toy_ref = {}


def _toy_reference(seed, slope, hyp):
    """hyp: the hyper-parameters as the model holds them (_hyp: its parameters are stored in single precision, so a lengthscale set to
    0.08 is 0.08 (1 - 2e-8), which the MLL bound of 1e-7 sees)."""
    if (seed, slope, hyp) not in _toy_ref:
        T = nref.TOY
        X, y, Xs = nref.toy_stream(seed)
        M = nref.DenseStream(T["bounds"], T["size"], list(hyp[0]), hyp[1], hyp[2], slope=slope)
        M.absorb([[0.5]], [0.0], [1e6], plain=True)
        steps = []
        for a in range(0, X.shape[0], T["q"]):
            M.absorb(X[a:a + T["q"]], y[a:a + T["q"]], xvar=T["sigma_x"] ** 2)
            steps.append(M.last)
        mean, var = M.predict(Xs)
        _toy_ref[(seed, slope, hyp)] = dict(steps=steps, mean=mean, var=var, mll=M.mll(), nlpd=nref.nlpd(nref.toy_truth(Xs[:, 0]), mean, var))
    return _toy_ref[(seed, slope, hyp)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_toy_stream_matches_the_reference_model_and_pays(dtype):
    """Seed 0, dense regime, 8 batches from a cold start: sites per batch, posterior mean, variance and MLL against the reference model;
    and the NLPD of the noise-free truth gains over a plain model on the same stream at least half of what the reference gains.
    The reference is given the hyper-parameters as the model holds them.  DESIGN.md 3.24."""
    T = nref.TOY
    X, y, Xs = nref.toy_stream(0)
    m, sites = _toy_model(dtype, 0, T["sigma_x"] ** 2)
    R, P = _toy_reference(0, "posterior", _hyp(m)), _toy_reference(0, None, _hyp(m))
    for k, (got, want) in enumerate(zip(sites, R["steps"])):
        om, lz, gr = (t.double().cpu().numpy() for t in got)
        e_o, e_l = np.abs(om - want["omega"]).max(), np.abs(lz - want["log_z"]).max() / np.abs(want["log_z"]).max()
        print(f"toy {dtype} batch {k}: omega {e_o:.3e}  log Z {e_l:.3e}  (bound {RTOL[dtype]:.0e}; omega {want['omega'].min():.4f} .. {want['omega'].max():.4f})")
        assert e_o <= RTOL[dtype] and e_l <= RTOL[dtype]
    assert m.num_data == 1 + X.shape[0]
    _check_against(m, dict(mean=R["mean"], var=R["var"], mll=R["mll"]), Xs, dtype, "toy", MLL_DENSE, sites=False)
    plain, _ = _toy_model(dtype, 0, None)
    assert plain.last_input_noise_sites is None
    truth = nref.toy_truth(Xs[:, 0])
    nl = {}
    for name, mod in (("input noise", m), ("plain", plain)):
        mvn = mod(_t(Xs, dtype))
        nl[name] = nref.nlpd(truth, mvn.mean.detach().double().cpu().numpy(), mvn.variance.detach().double().cpu().numpy())
    gain, ref_gain = nl["plain"] - nl["input noise"], P["nlpd"] - R["nlpd"]
    print(f"toy {dtype}: NLPD plain {nl['plain']:+.3f}  input noise {nl['input noise']:+.3f}  gain {gain:.3f}; reference {P['nlpd']:+.3f} / {R['nlpd']:+.3f}  gain {ref_gain:.3f}")
    assert ref_gain >= 0.5 and gain >= 0.5 * ref_gain


def test_functional_form_and_forgetting():
    """forgetting_factor = 0.9 over two batches: the reference ages the effective noise by 1 / gamma per batch and takes the sites of
    a batch against the decayed posterior; the second batch functional -- the parent untouched, the sites on the child -- and in place."""
    dtype, gam = torch.float64, 0.9
    X, y, noise, xvar, Xs = _stream()
    m = _model(X[:N0], y[:N0], noise[:N0], dtype, forgetting_factor=gam).eval()
    steps = _reference_stream(_hyp(m), gam, nb=2)
    assert np.abs(steps[1]["mean"] - _reference_stream(_hyp(m), None, nb=2)[1]["mean"]).max() > 10 * RTOL[dtype] * np.abs(steps[1]["mean"]).max()
    _absorb_batch(m, 0, dtype)
    _check_against(m, steps[0], Xs, dtype, "forgetting batch 0", MLL_DENSE)
    before = [t.clone() for t in m.stats_buffers()]
    kept = m.last_input_noise_sites
    child = _absorb_batch(m, 1, dtype, inplace=False)
    assert all(torch.equal(a, b) for a, b in zip(before, m.stats_buffers())) and m.num_data == N0 + Q and m.last_input_noise_sites is kept
    _check_against(child.eval(), steps[1], Xs, dtype, "forgetting batch 1, functional", MLL_DENSE)
    _absorb_batch(m, 1, dtype)
    _check_against(m, steps[1], Xs, dtype, "forgetting batch 1, in place", MLL_DENSE)


def test_grow_grid_takes_a_batch_beyond_the_grid():
    """grow_grid=True and a batch with two points beyond the grid: the grid grows by whole nodes first (exactly: the SKI kernel of the
    points held does not change), so the reference model on the grown grid is the yardstick."""
    dtype = torch.float64
    X, y, noise, xvar, Xs = _stream()
    m = _model(X[:N0], y[:N0], noise[:N0], dtype, grow_grid=True).eval()
    hyp = _hyp(m)
    sl = slice(N0, N0 + Q)
    Xb = X[sl].copy()
    Xb[0], Xb[1] = [1.21, 0.3], [-0.2, -1.3]
    m.condition_on_observations(_t(Xb, dtype), _t(y[sl], dtype), _t(noise[sl], dtype), input_var=_t(xvar[sl], dtype), inplace=True)
    g = m._grid
    assert list(g.g) != GS and m.num_data == N0 + Q and float(m.last_input_noise_sites[0].min()) > 0.0
    M = nref.DenseStream(None, None, list(hyp[0]), hyp[1], hyp[2], grid=nref.Grid(g.g0, g.h, g.g))
    M.absorb(X[:N0], y[:N0], noise[:N0], plain=True)
    M.absorb(Xb, y[sl], noise[sl], xvar[sl])
    mo, vo = M.predict(Xs)
    _check_against(m, dict(sites=M.last, mean=mo, var=vo, mll=M.mll(), n=N0 + Q), Xs, dtype, "grown grid", MLL_DENSE)


def test_zero_input_variance_is_the_plain_model():
    dtype = torch.float64
    X, y, noise, xvar, Xs = _stream()
    a, b = _model(X[:N0], y[:N0], noise[:N0], dtype).eval(), _model(X[:N0], y[:N0], noise[:N0], dtype, input_var=0.0).eval()
    for k in range(NB):
        sl = slice(N0 + k * Q, N0 + (k + 1) * Q)
        a.condition_on_observations(_t(X[sl], dtype), _t(y[sl], dtype), _t(noise[sl], dtype), inplace=True)
        b.condition_on_observations(_t(X[sl], dtype), _t(y[sl], dtype), _t(noise[sl], dtype), inplace=True)
        assert bool((b.last_input_noise_sites[0] == 1.0).all()) and a.last_input_noise_sites is None
    pa, pb = a(_t(Xs, dtype)), b(_t(Xs, dtype))
    e_m = float((pa.mean - pb.mean).abs().max() / pa.mean.abs().max())
    e_v = float((pa.variance - pb.variance).abs().max() / pa.variance.abs().max())
    print(f"input_var = 0 against the plain model: mean {e_m:.3e}  variance {e_v:.3e}  (bound 1e-12)")
    assert e_m <= 1e-12 and e_v <= 1e-12 and a.num_data == b.num_data


def test_default_model_never_enters_the_input_noise_path(monkeypatch):
    """Without input_var the launch is never made (the binding is replaced by one that raises), no site is recorded, and the streaming
    step keeps its fast path; a model built with input_var takes the step's unfused fallback and does enter."""
    from online_gp_amd import grid_ops

    def forbidden(*a, **k):
        raise AssertionError("the noisy-input absorb was launched by a model that was given no input_var")

    monkeypatch.setattr(grid_ops, "scatter_stats_input_noise", forbidden)
    dtype = torch.float64
    X, y, noise, xvar, Xs = _stream()
    m = _model(X[:N0], y[:N0], noise[:N0], dtype).eval()
    for a in range(N0, N0 + NB * Q, Q):
        m.condition_on_observations(_t(X[a:a + Q], dtype), _t(y[a:a + Q], dtype), _t(noise[a:a + Q], dtype), inplace=True)
    child = m.condition_on_observations(_t(X[:Q], dtype), _t(y[:Q], dtype), _t(noise[:Q], dtype))
    m.stream_step(_t(X[:Q], dtype), _t(y[:Q], dtype))
    assert m.last_input_noise_sites is None and child.last_input_noise_sites is None and m.num_data == N0 + NB * Q + Q
    with pytest.raises(AssertionError):                             # (and the replacement is what a batch with input_var would have called)
        m.condition_on_observations(_t(X[:Q], dtype), _t(y[:Q], dtype), _t(noise[:Q], dtype), input_var=0.01, inplace=True)
    v = _model(X[:N0], y[:N0], noise[:N0], dtype, input_var=[0.01, 0.02]).eval()
    assert v._stream_fast_state(_t(X[:Q], dtype), _t(y[:Q], dtype)) is None
    with pytest.raises(AssertionError):
        v.stream_step(_t(X[N0:N0 + Q], dtype), _t(y[N0:N0 + Q], dtype))


def test_stream_step_of_a_model_with_input_var_is_the_conditioned_model():
    dtype = torch.float64
    X, y, noise, xvar, Xs = _stream()
    one = torch.ones(Q, device=DEV, dtype=dtype)
    a, b = (_model(X[:N0], y[:N0], noise[:N0], dtype, input_var=[SX ** 2, 4 * SX ** 2]).eval() for _ in range(2))
    sl = slice(N0, N0 + Q)
    a.stream_step(_t(X[sl], dtype), _t(y[sl], dtype))
    b.condition_on_observations(_t(X[sl], dtype), _t(y[sl], dtype), one, inplace=True)
    close = lambda s, t: bool(((s - t).abs().max() <= 1e-10 * t.abs().max()).item())      # (two models: the order of the atomics differs)
    assert close(a.last_input_noise_sites[0], b.last_input_noise_sites[0]) and float(a.last_input_noise_sites[0].max()) < 1.0
    assert all(close(s, t) for s, t in zip(a.stats_buffers(), b.stats_buffers())) and a.num_data == b.num_data == N0 + Q


def test_refusals():
    from online_gp_amd.distributed import ShardedStatsUpdater
    from online_gp_amd.models import FixedNoiseOnlineSKIGP, OnlineSKIBotorchModel, OnlineSKIRegression
    from online_gp_amd.models.stems import Identity

    dtype = torch.float64
    X, y, noise, xvar, Xs = _stream()
    Xt, yt, nt, vt = _t(X[:12], dtype), _t(y[:12], dtype), _t(noise[:12], dtype), _t(xvar[:12], dtype)
    two = FixedNoiseOnlineSKIGP(Xt, torch.stack([yt, yt], 1), None, grid_bounds=torch.tensor(GB), grid_size=GS)
    with pytest.raises(NotImplementedError):                        # several outputs
        two.condition_on_observations(Xt, torch.stack([yt, yt], 1), None, input_var=vt, inplace=True)
    m = _model(X[:12], y[:12], noise[:12], dtype)
    before = [t.clone() for t in m.stats_buffers()]
    for kw in (dict(grad_Y=torch.zeros(12, 2, device=DEV, dtype=dtype)), dict(lower=yt - 0.1, upper=yt + 0.1), dict(counts=yt.abs().round()),
               dict(counts=yt.abs().round(), trials=yt.abs().round() + 1)):
        with pytest.raises(NotImplementedError):                    # derivative observations, bounds, counts
            m.condition_on_observations(Xt, yt, nt, input_var=vt, inplace=True, **kw)
    with pytest.raises(NotImplementedError):                        # fantasies (batched X)
        m.condition_on_observations(Xt[None], yt[None], nt[None], input_var=vt)
    with pytest.raises(NotImplementedError):                        # the data-parallel statistics exchange
        m._absorb_input_noise(m._kernel_cache, Xt, yt, vt, nt, m, half_delta=m._half_buffers())
    with pytest.raises(NotImplementedError):
        ShardedStatsUpdater(m).update(Xt, yt, nt, input_var=vt)
    with pytest.raises(ValueError):                                 # a shape that is none of scalar, [d], [n], [n, d]
        m.condition_on_observations(Xt, yt, nt, input_var=torch.ones(5, device=DEV, dtype=dtype), inplace=True)
    with pytest.raises(ValueError):
        _model(X[:12], y[:12], noise[:12], dtype, input_noise_slope="variance")
    with pytest.raises(ValueError):
        _model(X[:12], y[:12], noise[:12], dtype, input_var=-1.0)
    with pytest.raises(ValueError):                                 # one value per dimension, checked when the model is built
        _model(X[:12], y[:12], noise[:12], dtype, input_var=[0.01, 0.02, 0.03])
    for kw in (dict(robust_c=2.0), dict(window=64), dict(trend="linear")):
        r = _model(X[:12], y[:12], noise[:12], dtype, **kw)
        with pytest.raises(NotImplementedError):
            r.condition_on_observations(Xt, yt, nt, input_var=vt, inplace=True)
    assert all(torch.equal(a, b) for a, b in zip(before, m.stats_buffers())) and m.num_data == 12 and m.last_input_noise_sites is None
    # a handed-over full-stencil cache
    cache = m._clone_cache(m._kernel_cache)
    op = cache["WtW"]
    full = torch.zeros((m._grid.R, m._grid.m), device=DEV, dtype=dtype)
    cache["WtW"] = type(op)(m._grid, full)
    h = FixedNoiseOnlineSKIGP(covar_module=m.covar_module, kernel_cache=cache, likelihood=m.likelihood, learn_additional_noise=True, num_data=12)
    with pytest.raises(NotImplementedError):
        h.condition_on_observations(Xt, yt, nt, input_var=vt, inplace=True)
    # the BoTorch-facing wrapper and the regression surface pass the variance through
    b = OnlineSKIBotorchModel(Xt, yt[:, None], nt[:, None], grid_bounds=torch.tensor(GB), grid_size=GS)
    b.eval()
    b.condition_on_observations(Xt, yt, nt, input_var=vt, inplace=True)
    assert b.num_data == 24 and 0.0 < float(b.last_input_noise_sites[0].min()) and float(b.last_input_noise_sites[0].max()) < 1.0
    r = OnlineSKIRegression(Identity(2), Xt, yt[:, None], 1e-2, 12, 1.0, input_var=SX ** 2)
    r.update(Xt, yt[:, None], update_stem=False, update_gp=False)
    assert r.gp.num_data == 24 and float(r.gp.last_input_noise_sites[0].max()) < 1.0


def test_path_probes_receive_the_effective_weights():
    """num_path_probes > 0, PCG route: after a batch at uncertain locations the sample paths equal Matheron's rule in data space at the
    weights omega_i / d_i, path by path -- the probes entered with sqrt(wa omega), so cov(P) is still A.  The check and its bound are
    those of tests/test_interval_gpu.py: 1e-4 of max |reference path|; paths drawn at the plain weights must lie further than 1e-2 away."""
    from online_gp_amd import settings
    from online_gp_amd.kernels import GridInterpolationKernel, MaternKernel, ScaleKernel
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    dtype, S, seed, ell, osc, s2 = torch.float64, 8, 21, [0.35, 0.5], 1.2, 0.3
    X, y, noise, xvar, Xs = _stream()
    xvar = 16.0 * xvar                                               # (weights well away from one, so that the last assert can tell)
    n = N0 + Q
    with settings.dense_small_grids(False), settings.spectral_factor(False), settings.cg_tolerance(1e-10), torch.no_grad():
        k = GridInterpolationKernel(ScaleKernel(MaternKernel(nu=2.5, ard_num_dims=2)), grid_size=GS, num_dims=2, grid_bounds=torch.tensor(GB))
        k.base_kernel.outputscale = osc
        k.base_kernel.base_kernel.lengthscale = torch.as_tensor(ell)
        m = FixedNoiseOnlineSKIGP(_t(X[:N0], dtype), _t(y[:N0], dtype)[:, None], _t(noise[:N0], dtype)[:, None], covar_module=k,
                                  learn_additional_noise=True, num_path_probes=S, path_seed=seed)
        m.likelihood.second_noise = s2
        m.eval()
        m.condition_on_observations(_t(X[N0:n], dtype), _t(y[N0:n], dtype), _t(noise[N0:n], dtype), input_var=_t(xvar[N0:n], dtype), inplace=True)
        M = nref.DenseStream(GB, GS, ell, osc, s2, kind="matern52")
        M.absorb(X[:N0], y[:N0], noise[:N0], plain=True)
        M.absorb(X[N0:n], y[N0:n], noise[N0:n], xvar[N0:n])
        om = M.last["omega"]
        assert not M.last["skipped"].any() and om.max() < 0.9
        assert np.abs(m.last_input_noise_sites[0].cpu().numpy() - om).max() <= RTOL[dtype]
        wts = np.concatenate([np.ones(N0), om]) / noise[:n]
        O = dataspace.DataSpaceGP(GB, GS, "matern52", ell, osc, s2).fit(X[:n], y[:n], 1.0 / wts)
        g0, h, gg = spec.make_grid(GB, GS)
        W, Kuu = spr.dense_w(g0, h, gg, X[:n]), spr.kuu_dense(O.cols)
        z = torch.randn((S, m._grid.m), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        paths = m.sample_paths(S, base_samples=z.to(DEV))
        assert paths.last_converged
        uo = spr.path_dataspace(Kuu, W, wts, y[:n], s2, (spr.sym_sqrt(Kuu) @ z.numpy().T).T, spr.normals(seed, np.arange(n), S))
        dev_path = np.abs(paths.values.cpu().numpy() - uo).max() / np.abs(uo).max()
        plain = spr.path_dataspace(Kuu, W, 1.0 / noise[:n], y[:n], s2, (spr.sym_sqrt(Kuu) @ z.numpy().T).T, spr.normals(seed, np.arange(n), S))
        print(f"noisy-input paths: path deviation {dev_path:.3e}; distance to the plainly weighted paths {np.abs(plain - uo).max() / np.abs(uo).max():.3e}")
        assert dev_path <= RTOL[dtype]
        assert np.abs(plain - uo).max() / np.abs(uo).max() > 1e-2      # (the check can tell the effective weights from the plain ones)


def test_prediction_at_an_uncertain_query():
    dtype = torch.float64
    X, y, noise, xvar, Xs = _stream()
    m = _model(X[:N0], y[:N0], noise[:N0], dtype).eval()
    steps = _reference_stream(_hyp(m))
    for k in range(NB):
        _absorb_batch(m, k, dtype)
    mean, var = m.posterior_noisy_input(_t(Xs, dtype), [SX ** 2, 4 * SX ** 2])
    rm, rv = steps[-1]["noisy"]
    plain = m(_t(Xs, dtype))
    e_m, e_v = float(np.abs(mean.cpu().numpy() - rm).max() / np.abs(rm).max()), float(np.abs(var.cpu().numpy() - rv).max() / np.abs(rv).max())
    print(f"posterior_noisy_input: mean {e_m:.3e}  variance {e_v:.3e}  (bound {RTOL[dtype]:.0e}); variance gained up to "
          f"{float(((var - plain.variance) / plain.variance).max()):.3f} of the plain one")
    assert e_m <= RTOL[dtype] and e_v <= RTOL[dtype] and torch.equal(mean, m.posterior_jet(_t(Xs, dtype)).mean[:, 0])
    assert bool((var > plain.variance).all())
    z_m, z_v = m.posterior_noisy_input(_t(Xs, dtype), 0.0)
    assert float((z_v - plain.variance).abs().max()) <= 1e-10 * float(plain.variance.abs().max())
