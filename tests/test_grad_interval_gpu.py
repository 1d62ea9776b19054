"""GPU: interval sites on values and partial derivatives -- every present channel of every point of a batch
moment-matched against the posterior before it, inside the one launch that absorbs them all -- against the fp64 reference of
tests/grad_interval_reference.py: the kernel through the C ABI, the contract, the model surface, and the toy on which it has to pay.

Bounds.  Statistics: those of tests/test_grad_obs_gpu.py (scatter 1e-11 / 2e-4, x 10, relative to max |reference|).  Sites in fp64:
those of tests/test_interval_gpu.py, 1e-9 on ytilde (of max |ytilde|) and on omega (of each omega), 1e-11 on log Z (of each log Z).
Sites in fp32: the site is evaluated in fp64 in both precisions, but the predictive mean of the channel reaches it in fp32, and a site
far in a tail magnifies that; a derivative channel's mean is a sum of terms u / h that cancel, so it carries more
rounding than a value's.  FP32_SITE_DEV holds the deviations from the fp64 reference measured on one MI355X (same metrics; the
largest over d = 1..4), and the test asserts three times those, the project's rule for fp32 parity.  Model: 1e-4 / 1e-2, MLL 1e-7
dense, 0.05 matrix-free.  The measured deviations are tabulated in DESIGN.md 3.25.
"""
import ctypes

import numpy as np
import pytest
import torch

import grad_interval_reference as gir
import grad_obs_reference as gr

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")
DTYPES = [(torch.float64, 1e-11), (torch.float32, 2e-4)]          # the scatter tolerances of tests/test_grad_obs_gpu.py
RTOL = {torch.float64: 1e-4, torch.float32: 1e-2}
MLL_DENSE, MLL_FREE = 1e-7, 0.05
N, KS2 = gir.N, gir.KS2
KEYS = ("A", "b", "cnt", "stats", "res")
FP64_SITE = dict(ytilde=1e-9, omega=1e-9, log_z=1e-11)
# measured on one MI355X, fp32 against the fp64 reference, largest over the four grids
FP32_SITE_DEV = dict(ytilde=1.842e-07, omega=1.240e-05, log_z=2.275e-05)


# ------------------------------------------------------------------------------------------------------------------ the kernel
def _case(name):
    from online_gp_amd import grid_ops

    c = gir.kernel_case(name)
    if "spec" not in c:
        c["spec"] = grid_ops.GridSpec([[-1.0, 1.0 + 0.25 * q] for q in range(len(c["g"]))], c["g"])
    return c


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


def _site_deviation(sites, ref):
    """ytilde: largest error over max |ytilde|; omega, log Z: largest error relative to the reference value itself, where that is
    finite and not 0 (the others are compared exactly by the caller)."""
    yt, om, lz = (t.double().cpu().numpy() for t in sites)
    nz_o, nz_l = ref["omega"] != 0, np.isfinite(ref["log_z"]) & (ref["log_z"] != 0)
    return dict(ytilde=float(np.abs(yt - ref["ytilde"]).max() / np.abs(ref["ytilde"]).max()),
                omega=float((np.abs(om - ref["omega"])[nz_o] / ref["omega"][nz_o]).max()),
                log_z=float((np.abs(lz[nz_l] - ref["log_z"][nz_l]) / np.abs(ref["log_z"][nz_l])).max()))


def _same(a, b):
    """Bit for bit (the cases hold no NaN bound, so no site is NaN; -inf compares equal to itself)."""
    return torch.equal(a, b)


def _launch(c, tdt, buf, err, mean_out=None, res=True, **over):
    from online_gp_amd import grid_ops

    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    t = {k: mk(over.get(k, c[k])) for k in ("X", "lo", "hi", "wa", "noise", "pvar", "u")}
    return grid_ops.scatter_stats_grad_interval(c["spec"], t["X"], t["lo"], t["hi"], t["pvar"], KS2, t["wa"], t["wa"], t["noise"], buf["b"], buf["A"],
                                                buf["cnt"], buf["stats"], err, t["u"], res=buf["res"] if res else None, mean_out=mean_out)


@pytest.mark.parametrize("tdt,tol", DTYPES)
@pytest.mark.parametrize("name", list(gir.KGRIDS))
def test_kernel_matches_the_dense_reference(name, tdt, tol):
    from online_gp_amd import grid_ops

    c = _case(name)
    grid, ref = c["spec"], c["ref"]
    C = grid.d + 1
    rname = dict(ref, A=ref["A_half"])
    # from zero
    got, err = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    mean = torch.full((N, C), float("nan"), device=DEV, dtype=tdt)
    sites = _launch(c, tdt, got, err, mean_out=mean)
    assert all(t.shape == (N, C) for t in sites) and sites[0].dtype == tdt and sites[1].dtype == tdt and sites[2].dtype == torch.float64
    dev = _site_deviation(sites, ref)
    bound = FP64_SITE if tdt == torch.float64 else {k: (None if v is None else 3.0 * v) for k, v in FP32_SITE_DEV.items()}
    print(f"{name} {tdt} sites: " + "  ".join(f"{k} {dev[k]:.3e} (bound {bound[k]})" for k in dev))
    _compare(dict(got, mean_out=mean), rname, tol, KEYS + ("mean_out",), f"{name} zero-init")
    yt, om, lz = (t.double().cpu().numpy() for t in sites)
    mu = mean.double().cpu().numpy()
    assert np.array_equal(om == 0.0, ref["omega"] == 0.0)             # who enters: exactly the reference's channels
    sk, zero = ref["skipped"], ref["zero"]
    assert np.array_equal(yt[sk], mu[sk])                             # skipped: (mu, 0, log Z)
    assert not yt[zero].any() and not om[zero].any() and not lz[zero].any()     # absent, outside the grid: (0, 0, 0)
    nf = ~np.isfinite(ref["log_z"])
    assert np.array_equal(lz[nf], ref["log_z"][nf], equal_nan=True)   # lo > hi: -inf
    ex = (c["kind"] == "exact") & ~zero
    assert (om[ex] == 1.0).all() and np.array_equal(yt[ex], c["lo"][ex])          # exact values: exactly
    assert int(err.item()) == ref["err"] == 1 + 2 * 1                # bit 0 | one point dropped, counted once; a skipped channel is not flagged
    for k in dev:
        assert bound[k] is not None and dev[k] <= bound[k], (name, k, dev[k], bound[k])
    # on top of non-zero buffers: every statistic is added, none assigned; the sites do not depend on what the buffers hold
    rng = np.random.default_rng(5)
    init = {k: 0.5 * float(np.abs(rname[k]).max()) * rng.standard_normal(np.shape(rname[k])) for k in KEYS}
    got = _buffers(grid, tdt, init)
    start = {k: v.double().cpu().numpy().copy() for k, v in got.items()}
    err.zero_()
    sites2 = _launch(c, tdt, got, err)
    _compare(got, {k: start[k] + rname[k] for k in KEYS}, tol, KEYS, f"{name} on top")
    assert all(_same(a, b) for a, b in zip(sites, sites2))


@pytest.mark.parametrize("tdt,tol", DTYPES)
def test_all_channels_exact_is_the_derivative_absorb(tdt, tol):
    """Equal bounds on every present channel: the launch equals grid_ops.scatter_stats_grad on the same values, omega = 1 and
    ytilde = the value exactly (d = 3)."""
    from online_gp_amd import grid_ops

    c = _case("d3")
    grid = c["spec"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    Yn = np.where(c["present"], np.where(np.isfinite(c["lo"]), c["lo"], 0.25), 0.0)
    got, want = _buffers(grid, tdt), _buffers(grid, tdt)
    e1, e2 = grid_ops.new_err_flag(DEV), grid_ops.new_err_flag(DEV)
    m1, m2 = torch.zeros((N, 4), device=DEV, dtype=tdt), torch.zeros((N, 4), device=DEV, dtype=tdt)
    yt, omega, _ = _launch(c, tdt, got, e1, mean_out=m1, lo=Yn, hi=Yn)
    grid_ops.scatter_stats_grad(grid, mk(c["X"]), mk(Yn), mk(c["wa"]), mk(c["wa"]), mk(c["noise"]), want["b"], want["A"], want["cnt"], want["stats"], e2,
                                u=mk(c["u"]), res=want["res"], mean_out=m2)
    _compare(got, {k: v.double().cpu().numpy() for k, v in want.items()}, tol, KEYS, "all exact")
    assert int(e1.item()) == int(e2.item()) == 3 and torch.equal(m1, m2)
    pres = c["present"] & c["ok"][:, None]
    assert np.array_equal(omega.double().cpu().numpy(), pres.astype(np.float64))
    assert np.array_equal(yt.double().cpu().numpy(), np.where(pres, Yn, 0.0))


@pytest.mark.parametrize("tdt,tol", DTYPES)
def test_only_the_value_channel_is_the_interval_absorb(tdt, tol):
    """Channel 0 alone present: the sites equal those of grid_ops.scatter_stats_interval bit for bit, the statistics to the bounds (d = 3)."""
    from online_gp_amd import grid_ops

    c = _case("d3")
    grid = c["spec"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    only = np.zeros_like(c["present"])
    only[:, 0] = c["present"][:, 0]
    wa, noise = np.where(only, c["wa"], 0.0), np.where(only, c["noise"], 1.0)
    got, want = _buffers(grid, tdt), _buffers(grid, tdt)
    e1, e2 = grid_ops.new_err_flag(DEV), grid_ops.new_err_flag(DEV)
    sites = _launch(c, tdt, got, e1, wa=wa, noise=noise)
    keep = only[:, 0]                                                 # (the interval form has no absent points: they are left out of its batch)
    col = lambda k: mk(np.ascontiguousarray(c[k][keep, 0]))
    w0 = col("wa")
    s1 = grid_ops.scatter_stats_interval(grid, mk(c["X"][keep]), col("lo"), col("hi"), col("pvar"), KS2, w0, w0, col("noise"), want["b"], want["A"],
                                         want["cnt"], want["stats"], e2, mk(c["u"]), res=want["res"])
    _compare(got, {k: v.double().cpu().numpy() for k, v in want.items()}, tol, KEYS, "value only")
    assert int(e1.item()) == int(e2.item()) == 3
    kt = torch.as_tensor(keep, device=DEV)
    for a, b in zip(sites, s1):
        assert _same(a[kt, 0], b)                                     # bit for bit
        assert not bool(a[:, 1:].any()) and not bool(a[~kt, 0].any())
    assert float(s1[1].max()) == 1.0 and 0.0 < float(s1[1][s1[1] > 0].min()) < 1e-6


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64])
def test_absorb_refuses_the_group_with_what_the_kernel_does_not_do(tdt):
    """Through the full argument record plus the form's arguments (wiski_absorb_grad_interval): every combination the contract
    refuses is WISKI_E_BADARG before any launch -- every buffer untouched -- while the clean record runs and equals
    grid_ops.scatter_stats_grad_interval; res and mean_out are optional, the record's d_y is ignored."""
    from online_gp_amd import _hip, grid_ops

    c = _case("d3")
    grid = c["spec"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    X, lo, hi, wa, noise, pvar, u = (mk(c[k]) for k in ("X", "lo", "hi", "wa", "noise", "pvar", "u"))
    buf, err = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    nan = lambda dt=tdt: torch.full((N, 4), float("nan"), device=DEV, dtype=dt)
    mean, yt, omega, logz = nan(), nan(), nan(), nan(torch.float64)
    full = torch.zeros((grid.R, grid.m), device=DEV, dtype=tdt)
    guard = torch.tensor([7], device=DEV, dtype=torch.int64)
    z1 = torch.full((2,), 0x01010101, device=DEV, dtype=torch.int32)
    bin_ws = torch.zeros(1 << 16, device=DEV, dtype=torch.uint8)
    p = lambda t: t.data_ptr()
    stream = _hip.stream_ptr(torch.device("cuda", torch.cuda.current_device()))

    def call(lo_=lo, hi_=hi, pvar_=pvar, sigma2=KS2, yt_=yt, omega_=omega, logz_=logz, **kw):
        a = _hip.wiski_absorb_args(d_x=p(X), d_y=None, d_wa=p(wa), d_wb=p(wa), d_noise=p(noise), n=N, d_b=p(buf["b"]), d_A=p(buf["A"]), half=1,
                                   channels=4, d_cnt=p(buf["cnt"]), d_stats=p(buf["stats"]), d_err=p(err), d_u=p(u), d_res=p(buf["res"]),
                                   d_mean_out=p(mean), nout=1)
        for k, v in kw.items():
            setattr(a, k, v)
        return _hip.fn("wiski_absorb_grad_interval", tdt)(grid.ref, ctypes.byref(a), _hip.dptr(lo_), _hip.dptr(hi_), _hip.dptr(pvar_), ctypes.c_double(sigma2),
                                                          _hip.dptr(yt_), _hip.dptr(omega_), _hip.dptr(logz_), stream)

    refused = [("channels = 0", call(channels=0)), ("channels = d", call(channels=3)), ("channels = d + 2", call(channels=5)),
               ("no u", call(d_u=None, d_res=None, d_mean_out=None)), ("no A", call(d_A=None)), ("no cnt", call(d_cnt=None)),
               ("full stencil", call(half=0, d_A=p(full))), ("guard", call(d_guard=p(guard), guard_expect=7)), ("zero region", call(z1=p(z1), n1_bytes=8)),
               ("shard", call(g_lo=0, g_hi=3)), ("owner workspace", call(d_bin=p(bin_ws), bin_bytes=bin_ws.numel())), ("nout = 2", call(nout=2, d_mean_out=None)),
               ("sigma2 = 0", call(sigma2=0.0)), ("sigma2 < 0", call(sigma2=-1.0)), ("sigma2 = inf", call(sigma2=float("inf"))),
               ("sigma2 = nan", call(sigma2=float("nan"))), ("no lo", call(lo_=None)), ("no hi", call(hi_=None)), ("no pvar", call(pvar_=None)),
               ("no ytilde_out", call(yt_=None)), ("no omega_out", call(omega_=None)), ("no logz_out", call(logz_=None))]
    torch.cuda.synchronize()
    assert [(what, rc) for what, rc in refused if rc != -1] == []
    assert all(float(v.abs().max()) == 0.0 for v in buf.values()) and float(full.abs().max()) == 0.0 and int(err.item()) == 0
    assert all(bool(torch.isnan(t).all()) for t in (mean, yt, omega, logz)) and bool((z1 == 0x01010101).all())
    # the refusals earlier forms pin stay: the interval entry with channels, the plain entry with a wrong channel count
    a = _hip.wiski_absorb_args(d_x=p(X), d_y=p(lo), d_wa=p(wa), d_wb=p(wa), d_noise=p(noise), n=N, d_b=p(buf["b"]), d_A=p(buf["A"]), half=1, channels=4,
                               d_cnt=p(buf["cnt"]), d_stats=p(buf["stats"]), d_err=p(err), d_u=p(u), d_res=p(buf["res"]), nout=1)
    assert _hip.fn("wiski_absorb_interval", tdt)(grid.ref, ctypes.byref(a), _hip.dptr(lo), _hip.dptr(hi), _hip.dptr(pvar), ctypes.c_double(KS2), _hip.dptr(yt),
                                                 _hip.dptr(omega), _hip.dptr(logz), stream) == -1
    a.channels = 3
    assert _hip.fn("wiski_absorb", tdt)(grid.ref, ctypes.byref(a), stream) == -1
    torch.cuda.synchronize()
    assert all(float(v.abs().max()) == 0.0 for v in buf.values())
    assert call() == 0
    want, e2 = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    sites = _launch(c, tdt, want, e2)
    _compare(buf, {k: v.double().cpu().numpy() for k, v in want.items()}, dict(DTYPES)[tdt], KEYS, "record")
    assert all(_same(a, b) for a, b in zip(sites, (yt, omega, logz))) and int(err.item()) == int(e2.item()) == 3
    assert call(d_res=None, d_mean_out=None) == 0                    # u alone is a complete request: res and mean_out are optional
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- the model
GB = {1: [[-1.0, 1.0]], 2: [[-1.0, 1.0], [-1.0, 1.0]]}
GS = {1: [32], 2: [12, 12]}
N0, Q, NB, NQ = 30, 12, 3, 23


def _f(X):
    return np.sin(2 * X[:, 0]) + 0.5 * X[:, 0] if X.shape[1] == 1 else np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.5 * X[:, 1]


def _df(X):
    if X.shape[1] == 1:
        return (2 * np.cos(2 * X[:, 0]) + 0.5)[:, None]
    return np.stack([2 * np.cos(2 * X[:, 0]) * np.cos(X[:, 1]), -np.sin(2 * X[:, 0]) * np.sin(X[:, 1]) + 0.5], 1)


_streams = {}


def _stream(d, reach=0.9):
    """30 points with values, then 3 batches of 12: values with a lower bound on every partial; binned values with two-sided slope
    bounds; bounds on a random subset of the partials alone.  The declared noise is drawn from U(0.5, 2) for the reason
    tests/test_grad_obs_gpu.py::_data gives: the MLL bounds are relative.  Returns (X0, y0, noise0, batches, queries), a batch being
    (X, keywords of condition_on_observations as numpy arrays)."""
    if (d, reach) in _streams:
        return _streams[(d, reach)]
    rng = np.random.default_rng(40 + d)
    n = N0 + NB * Q
    X = rng.uniform(-0.9, 0.9, (n, d))
    X[N0:] *= reach / 0.9
    noise = rng.uniform(0.5, 2.0, n)
    y = _f(X) + 0.05 * rng.standard_normal(n)
    g = _df(X) + 0.05 * rng.standard_normal((n, d))
    sl = [slice(N0 + k * Q, N0 + (k + 1) * Q) for k in range(NB)]
    lo = np.floor(y / 0.25) * 0.25
    mask = rng.uniform(size=(Q, d)) < 0.6
    mask[0] = True
    batches = [(X[sl[0]], dict(Y=y[sl[0]], noise=noise[sl[0]], grad_lower=g[sl[0]] - 0.3, grad_noise=rng.uniform(0.5, 2.0, (Q, d)))),
               (X[sl[1]], dict(lower=lo[sl[1]], upper=lo[sl[1]] + 0.25, noise=noise[sl[1]], grad_lower=g[sl[1]] - 0.5, grad_upper=g[sl[1]] + 0.5)),
               (X[sl[2]], dict(noise=noise[sl[2]], grad_lower=np.zeros(d), grad_upper=g[sl[2]] + 1.0, grad_mask=mask))]
    _streams[(d, reach)] = (X[:N0], y[:N0], noise[:N0], batches, rng.uniform(-0.9, 0.9, (NQ, d)))
    return _streams[(d, reach)]


def _t(a, dtype):
    return torch.as_tensor(a, device=DEV, dtype=dtype)


def _model(d, dtype, **kw):
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    X0, y0, n0 = _stream(d)[:3]
    return FixedNoiseOnlineSKIGP(_t(X0, dtype), _t(y0, dtype)[:, None], _t(n0, dtype)[:, None], grid_bounds=torch.tensor(GB[d]), grid_size=GS[d],
                                 learn_additional_noise=True, **kw).eval()


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


def _reference(d, hyp, gamma=None, nb=NB, reach=0.9, grid=None):
    """The stream through DenseStream (fp64): per batch the sites, mean, variance and mean gradient at the queries, the MLL and the
    number of scalar observations held; computed once per setting."""
    key = (d, hyp, gamma, nb, reach, None if grid is None else (tuple(grid.g0), tuple(grid.h), tuple(grid.g)))
    if key not in _refs:
        X0, y0, n0, batches, Xs = _stream(d, reach)
        grid = gir.Grid.from_bounds(GB[d], GS[d]) if grid is None else grid
        S = gir.DenseStream(grid, gr.dense_kuu(grid, "rbf", np.array(hyp[0]), hyp[1]), hyp[2]).add_values(X0, y0, n0)
        steps = []
        for X, kw in batches[:nb]:
            st = S.condition(X, *gir.channels(Q, d, **kw), gamma=gamma)
            mean, var, grad = S.predict(Xs)
            steps.append(dict(sites=st, mean=mean, var=var, grad=grad, mll=S.mll(), n=S.n))
        _refs[key] = steps
    return _refs[key]


def _absorb_batch(m, d, k, dtype, inplace=True, reach=0.9):
    X, kw = _stream(d, reach)[3][k]
    kw = {a: (_t(v, torch.bool) if a == "grad_mask" else _t(v, dtype)) for a, v in kw.items()}
    return m.condition_on_observations(_t(X, dtype), kw.pop("Y", None), kw.pop("noise"), inplace=inplace, **kw)


def _check_against(m, step, Xs, dtype, label, mll_bound):
    yt, om, lz = (t.double().cpu().numpy() for t in m.last_grad_interval_sites)
    st = step["sites"]
    e_y, e_o = np.abs(yt - st["ytilde"]).max() / np.abs(st["ytilde"]).max(), np.abs(om - st["omega"]).max()
    e_l = np.abs(lz - st["log_z"]).max() / np.abs(st["log_z"]).max()
    ent = st["omega"] > 0
    print(f"{label} {dtype}: ytilde {e_y:.3e}  omega {e_o:.3e}  log Z {e_l:.3e}  (bound {RTOL[dtype]:.0e}; {int(ent.sum())} of {int((~st['zero']).sum())} "
          f"present channels enter, omega {st['omega'][ent].min():.4f} .. {st['omega'].max():.4f})")
    assert e_y <= RTOL[dtype] and e_o <= RTOL[dtype] and e_l <= RTOL[dtype]
    assert np.array_equal(om > 0.0, ent) and m.num_data == step["n"]
    mvn = m(_t(Xs, dtype))
    mean, var = mvn.mean.detach().double().cpu().numpy(), mvn.variance.detach().double().cpu().numpy()
    grad = m.posterior_jet(_t(Xs, dtype)).mean[:, 1:].double().cpu().numpy()
    e_m, e_v = np.abs(mean - step["mean"]).max() / np.abs(step["mean"]).max(), np.abs(var - step["var"]).max() / np.abs(step["var"]).max()
    e_g = np.abs(grad - step["grad"]).max() / np.abs(step["grad"]).max()
    print(f"{label} {dtype}: mean {e_m:.3e}  var {e_v:.3e}  mean gradient {e_g:.3e}  (bound {RTOL[dtype]:.0e})")
    assert e_m <= RTOL[dtype] and e_v <= RTOL[dtype] and e_g <= RTOL[dtype]
    if dtype == torch.float64 and mll_bound is not None:
        v, r = _mll(m), step["mll"]
        print(f"{label}: mll {v:.10f}  reference {r:.10f}  rel {abs(v - r) / abs(r):.3e}  (bound {mll_bound:.0e})")
        assert abs(v - r) <= mll_bound * abs(r)


def _check_regime(d, dtype, label, mll_bound, **kw):
    m = _model(d, dtype, **kw)
    assert m.last_grad_interval_sites is None                        # the initial data is absorbed plainly
    steps = _reference(d, _hyp(m), kw.get("forgetting_factor"))
    Xs = _stream(d)[4]
    for k, step in enumerate(steps):
        _absorb_batch(m, d, k, dtype)
        assert all(t.shape == (Q, d + 1) and t.is_cuda for t in m.last_grad_interval_sites)
        _check_against(m, step, Xs, dtype, f"{label} d = {d} batch {k}", mll_bound)
    return m


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("d", [1, 2])
def test_dense_regime_matches_the_streamed_reference(d, dtype):
    _check_regime(d, dtype, "dense", MLL_DENSE)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("d", [1, 2])
def test_matrix_free_regime_matches_the_streamed_reference(d, dtype):
    from online_gp_amd import settings
    from online_gp_amd.mlls.batched_woodbury_marginal_log_likelihood import num_trace_samples

    with settings.dense_small_grids(False), settings.spectral_factor(False), num_trace_samples(64), \
            settings.cg_tolerance(1e-10 if dtype == torch.float64 else 1e-6):
        m = _check_regime(d, dtype, "matrix-free", MLL_FREE)
        assert m._mean_state is not None


def test_functional_form_leaves_the_parent_alone_and_sets_the_sites_on_the_child():
    d, dtype = 2, torch.float64
    m = _model(d, dtype)
    step = _reference(d, _hyp(m), nb=1)[0]
    Xs = _stream(d)[4]
    before = [t.clone() for t in m.stats_buffers()]
    child = _absorb_batch(m, d, 0, dtype, inplace=False)
    assert all(torch.equal(a, b) for a, b in zip(before, m.stats_buffers())) and m.num_data == N0 and m.last_grad_interval_sites is None
    _check_against(child.eval(), step, Xs, dtype, "functional", MLL_DENSE)
    _absorb_batch(m, d, 0, dtype)
    _check_against(m, step, Xs, dtype, "in place", MLL_DENSE)


def test_forgetting_decays_before_the_sites_are_matched():
    d, dtype, gam = 2, torch.float64, 0.9
    m = _model(d, dtype, forgetting_factor=gam)
    steps = _reference(d, _hyp(m), gam, nb=2)
    Xs = _stream(d)[4]
    assert np.abs(steps[1]["mean"] - _reference(d, _hyp(m), None, nb=2)[1]["mean"]).max() > 10 * RTOL[dtype] * np.abs(steps[1]["mean"]).max()
    _absorb_batch(m, d, 0, dtype)
    _check_against(m, steps[0], Xs, dtype, "forgetting batch 0", MLL_DENSE)
    child = _absorb_batch(m, d, 1, dtype, inplace=False)
    _check_against(child.eval(), steps[1], Xs, dtype, "forgetting batch 1, functional", MLL_DENSE)
    _absorb_batch(m, d, 1, dtype)
    _check_against(m, steps[1], Xs, dtype, "forgetting batch 1, in place", MLL_DENSE)


def test_grow_grid_grows_before_the_sites_are_matched():
    """Batches that reach to +-1.3 on a grid over [-1, 1]: the model grows its grid first (exactly), and equals the reference run on the
    grown grid from the start."""
    d, dtype, reach = 2, torch.float64, 1.3
    m = _model(d, dtype, grow_grid=True)
    g_before = list(m._grid.g)
    _absorb_batch(m, d, 0, dtype, reach=reach)
    assert list(m._grid.g) != g_before
    grid = gir.Grid(m._grid.g0, m._grid.h, m._grid.g)
    step = _reference(d, _hyp(m), nb=1, reach=reach, grid=grid)[0]
    assert not step["sites"]["zero"][:, 0].any()                      # no point is outside the grown grid
    _check_against(m, step, _stream(d, reach)[4], dtype, "grown", MLL_DENSE)


def test_gradient_interval_probability_against_scipy():
    from scipy import special as sp

    d, dtype = 2, torch.float64
    m = _model(d, dtype)
    Xs = _stream(d)[4]
    jet = m.posterior_jet(_t(Xs, dtype))
    mean = jet.mean[:, 1:].cpu().numpy()
    var = torch.diagonal(jet.covariance, dim1=-2, dim2=-1)[:, 1:].cpu().numpy()
    rng = np.random.default_rng(8)
    nz = rng.uniform(0.5, 2.0, (NQ, d))
    s = np.sqrt(np.maximum(var, 0.0) + _hyp(m)[2] * nz)
    a = rng.uniform(-4.0, 3.0, (NQ, d))
    b = a + rng.uniform(0.1, 3.0, (NQ, d))
    lo_q, hi_q = mean + s * a, mean + s * b
    lo_q[:5], hi_q[5:10] = -INF, INF
    a[:5], b[5:10] = -INF, INF
    want = np.log(sp.ndtr(b) - sp.ndtr(a))
    want[:5], want[5:10] = sp.log_ndtr(b[:5]), sp.log_ndtr(-a[5:10])
    got = m.gradient_interval_probability(_t(Xs, dtype), _t(lo_q, dtype), _t(hi_q, dtype), noise=_t(nz, dtype)).cpu().numpy()
    e = np.abs(got - want).max() / np.abs(want).max()
    print(f"gradient_interval_probability: {e:.3e} of max |log P| = {np.abs(want).max():.3f}")
    assert got.shape == (NQ, d) and e <= 1e-10


def test_default_model_never_enters_the_gradient_interval_path(monkeypatch):
    """Without grad_lower / grad_upper the method is never reached (it is replaced by one that raises): a value, a grad_Y and a
    lower= update take the paths they took."""
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    def forbidden(*a, **k):
        raise AssertionError("_absorb_grad_interval was reached by a model that was given no gradient bounds")

    monkeypatch.setattr(FixedNoiseOnlineSKIGP, "_absorb_grad_interval", forbidden)
    d, dtype = 2, torch.float64
    m = _model(d, dtype)
    X, kw = _stream(d)[3][0]
    Xt, yt, nt = _t(X, dtype), _t(kw["Y"], dtype), _t(kw["noise"], dtype)
    m.condition_on_observations(Xt, yt, nt, inplace=True)
    m.condition_on_observations(Xt, yt, nt, grad_Y=_t(kw["grad_lower"], dtype), inplace=True)
    m.condition_on_observations(Xt, None, nt, lower=yt - 0.1, upper=yt + 0.1, inplace=True)
    child = m.condition_on_observations(Xt, yt, nt)
    assert m.last_grad_interval_sites is None and child.last_grad_interval_sites is None and m.num_data == N0 + Q + 3 * Q + Q
    with pytest.raises(AssertionError):                             # (and the replacement is what a batch of gradient bounds would have called)
        m.condition_on_observations(Xt, yt, nt, grad_lower=0.0, inplace=True)


def test_refusals():
    from online_gp_amd.distributed import ShardedStatsUpdater
    from online_gp_amd.models import FixedNoiseOnlineSKIGP, OnlineSKIBotorchModel

    d, dtype = 2, torch.float64
    X0, y0, n0 = _stream(d)[:3]
    Xt, yt, nt = _t(X0[:12], dtype), _t(y0[:12], dtype), _t(n0[:12], dtype)
    gl = torch.zeros(12, 2, device=DEV, dtype=dtype)
    two = FixedNoiseOnlineSKIGP(Xt, torch.stack([yt, yt], 1), None, grid_bounds=torch.tensor(GB[d]), grid_size=GS[d])
    with pytest.raises(NotImplementedError):                        # several outputs
        two.condition_on_observations(Xt, torch.stack([yt, yt], 1), nt, grad_lower=gl, inplace=True)
    m = _model(d, dtype)
    before = [t.clone() for t in m.stats_buffers()]
    with pytest.raises(NotImplementedError):                        # an exact partial is equal bounds
        m.condition_on_observations(Xt, yt, nt, grad_Y=gl, grad_lower=gl, inplace=True)
    with pytest.raises(NotImplementedError):                        # targets and bounds on the value
        m.condition_on_observations(Xt, yt, nt, lower=yt - 0.1, grad_lower=gl, inplace=True)
    with pytest.raises(NotImplementedError, match="interval observations bound values only"):      # as before this form existed
        m.condition_on_observations(Xt, None, nt, lower=yt, grad_Y=gl)
    with pytest.raises(NotImplementedError):                        # fantasies (batched X)
        m.condition_on_observations(Xt[None], yt[None], nt[None], grad_lower=gl[None])
    with pytest.raises(NotImplementedError):                        # noisy inputs
        m.condition_on_observations(Xt, yt, nt, grad_lower=gl, input_var=0.01, inplace=True)
    with pytest.raises(NotImplementedError):                        # counts
        m.condition_on_observations(Xt, None, None, counts=torch.ones(12, device=DEV, dtype=dtype), grad_lower=gl, inplace=True)
    with pytest.raises(NotImplementedError):                        # the data-parallel statistics exchange
        ShardedStatsUpdater(m).update(Xt, yt, nt, grad_lower=gl)
    with pytest.raises(ValueError):                                 # shapes
        m.condition_on_observations(Xt, yt, nt, grad_lower=torch.zeros(5, 2, device=DEV, dtype=dtype), inplace=True)
    with pytest.raises(ValueError):
        m.condition_on_observations(Xt, yt, nt, grad_lower=gl, grad_mask=torch.ones(12, 3, device=DEV, dtype=torch.bool), inplace=True)
    for kw in (dict(robust_c=2.0), dict(window=64), dict(num_path_probes=4), dict(trend="linear")):
        r = _model(d, dtype, **kw)
        with pytest.raises(NotImplementedError):
            r.condition_on_observations(Xt, yt, nt, grad_lower=gl, inplace=True)
    assert all(torch.equal(a, b) for a, b in zip(before, m.stats_buffers())) and m.num_data == N0 and m.last_grad_interval_sites is None
    # a handed-over full-stencil cache
    cache = m._clone_cache(m._kernel_cache)
    op = cache["WtW"]
    cache["WtW"] = type(op)(m._grid, torch.zeros((m._grid.R, m._grid.m), device=DEV, dtype=dtype))
    h = FixedNoiseOnlineSKIGP(covar_module=m.covar_module, kernel_cache=cache, likelihood=m.likelihood, learn_additional_noise=True, num_data=N0)
    with pytest.raises(NotImplementedError):
        h.condition_on_observations(Xt, yt, nt, grad_lower=gl, inplace=True)
    # the BoTorch-facing wrapper passes the keywords through
    from online_gp_amd.models import monotone_bounds

    b = OnlineSKIBotorchModel(Xt, yt[:, None], nt[:, None], grid_bounds=torch.tensor(GB[d]), grid_size=GS[d])
    b.eval()
    lo, hi, mask = monotone_bounds(12, 2, [1])
    b.condition_on_observations(Xt, yt, nt, grad_lower=lo, grad_upper=hi, grad_mask=mask, grad_noise=0.01, inplace=True)
    om = b.last_grad_interval_sites[1]
    assert bool((om[:, 0] == 1).all()) and not bool(om[:, 1].any()) and b.num_data == 12 + 12 + int((om[:, 2] > 0).sum())


# ------------------------------------------------------------------------------------------------------- where it has to pay
def _toy_model(seed, constrained):
    from online_gp_amd.kernels import GridInterpolationKernel, RBFKernel, ScaleKernel
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    dtype = torch.float64
    X, y, Xs = gir.toy(seed)
    with torch.no_grad():
        k = GridInterpolationKernel(ScaleKernel(RBFKernel(ard_num_dims=1)), grid_size=gir.TG, num_dims=1, grid_bounds=torch.tensor(gir.TB))
        k.base_kernel.outputscale = gir.TOSC
        k.base_kernel.base_kernel.lengthscale = torch.as_tensor([gir.TELL])
        m = FixedNoiseOnlineSKIGP(_t([[0.5]], dtype), _t([[0.0]], dtype), _t([[1e6]], dtype), covar_module=k, learn_additional_noise=True)
        m.likelihood.second_noise = gir.TS2
        m.eval()
        for a in range(0, gir.TNB * gir.TQ, gir.TQ):
            kw = dict(grad_lower=0.0, grad_noise=gir.TNU) if constrained else {}
            m.condition_on_observations(_t(X[a:a + gir.TQ], dtype), _t(y[a:a + gir.TQ], dtype), torch.ones(gir.TQ, device=DEV, dtype=dtype), inplace=True, **kw)
        jet = m.posterior_jet(_t(Xs, dtype)).mean.cpu().numpy()
    return gir.toy_figures(jet[:, 0], jet[:, 1], Xs)


def test_monotone_toy_pays_as_the_reference_says():
    """tanh(4x - 2) + x from 24 noisy points under a prior that wiggles (RBF lengthscale 0.1), with and without "the slope is
    positive at the points of each batch".  The model reproduces the reference's RMSE and its share of queries with a negative
    slope to 1e-6 on each of the five seeds, and on each the constrained model wins both -- by at least half the reference's
    smallest gain: its worst RMSE ratio is 0.981 (threshold sqrt(0.981)), its smallest drop of the share 0.06 (threshold 0.03)."""
    ref = {s: (gir.toy_reference(s, True), gir.toy_reference(s, False)) for s in gir.TSEEDS}
    worst_ratio = max(c[0] / u[0] for c, u in ref.values())
    least_drop = min(u[1] - c[1] for c, u in ref.values())
    print(f"reference: worst RMSE ratio {worst_ratio:.4f}, smallest drop of the negative-slope share {least_drop:.3f}")
    assert worst_ratio < 1.0 and least_drop > 0.0
    for s in gir.TSEEDS:
        got = (_toy_model(s, True), _toy_model(s, False))
        print(f"seed {s}: model RMSE {got[0][0]:.6f} / {got[1][0]:.6f}  share {got[0][1]:.2f} / {got[1][1]:.2f};  "
              f"reference RMSE {ref[s][0][0]:.6f} / {ref[s][1][0]:.6f}  share {ref[s][0][1]:.2f} / {ref[s][1][1]:.2f}")
        for g, r in zip(got, ref[s]):
            assert abs(g[0] - r[0]) <= 1e-6 and abs(g[1] - r[1]) <= 1e-6
        assert got[0][0] <= np.sqrt(worst_ratio) * got[1][0] and got[0][1] <= got[1][1] - 0.5 * least_drop
