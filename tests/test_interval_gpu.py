"""GPU: interval and censored observations -- every point of a batch moment-matched against the posterior before it,
inside the launch that absorbs it -- against the fp64 reference of tests/interval_reference.py and the data-space oracle fitted at the
reference's pseudo-observations (ytilde_i, noise_i / omega_i): the kernel through the C ABI, the contract, the model surface, and two
streams on which the feature has to pay.

Bounds.  Statistics: those of tests/test_grad_obs_gpu.py (scatter 1e-11 / 2e-4, x 10, relative to max |reference|).  Sites in fp64:
1e-9 on ytilde (of max |ytilde|) and on omega (of each omega), 1e-11 on log Z (of each log Z).  Sites in fp32: the site itself is
evaluated in fp64 in both precisions, but the predictive mean reaches it in fp32, and a site far in a tail magnifies that -- d log
omega / d mu is z / s, six for a bound satisfied by six standard deviations.  FP32_SITE_DEV holds the deviations from the fp64
reference measured on one MI355X (same metrics; the largest over d = 1..4), and the test asserts three times those, the project's
rule for fp32 parity.  Model: 1e-4 / 1e-2, MLL 1e-7 dense, 0.05 matrix-free.  The measured deviations are tabulated in DESIGN.md 3.20.
"""
import ctypes

import numpy as np
import pytest
import torch

import interval_reference as iref
import sample_paths_reference as spr
from oracle import dataspace, spec

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = float("inf")
DTYPES = [(torch.float64, 1e-11), (torch.float32, 2e-4)]          # the scatter tolerances of tests/test_grad_obs_gpu.py
RTOL = {torch.float64: 1e-4, torch.float32: 1e-2}
MLL_DENSE, MLL_FREE = 1e-7, 0.05
KGRIDS = {"d1": [8], "d2": [8, 8], "d3": [8, 8, 8], "d4": [6, 6, 6, 6]}
N = 37                                                            # three blocks of 16; the last pass of the last block holds one point
KS2 = 0.7                                                         # sigma2 of the kernel cases
KEYS = ("A", "b", "cnt", "stats", "res")
FP64_SITE = dict(ytilde=1e-9, omega=1e-9, log_z=1e-11)
# measured on one MI355X, fp32 against the fp64 reference, largest over the four grids
FP32_SITE_DEV = dict(ytilde=5.231e-08, omega=3.510e-06, log_z=4.125e-06)


# ------------------------------------------------------------------------------------------------------------------ the kernel
_cases = {}


def _kernel_case(name):
    """Grid, 37 points (fp64 values that are exact in fp32), bounds placed around the reference's own predictive mean in units of
    s = sqrt(pvar + sigma2 noise), and the dense reference; built once.
      0, 1: exact values   2: (-inf, inf)   3: a lower bound satisfied by 12 s (skipped)   10: outside the grid
      others, in turn: lower-only, upper-only (violated by up to 8 s, satisfied by up to 6 s), two-sided (width 0.05 s .. 4 s, anywhere
      within 8 s); 12 .. 16 share one interior cell (colliding atomics); point 5 has pvar = 0 exactly."""
    if name in _cases:
        return _cases[name]
    from online_gp_amd import grid_ops

    g = KGRIDS[name]
    d = len(g)
    rng = np.random.default_rng(200 + d)
    grid = grid_ops.GridSpec([[-1.0, 1.0 + 0.25 * q] for q in range(d)], g)
    cell = np.stack([rng.integers(0, gq - 1, N) for gq in g], 1).astype(np.float64)
    frac = 0.5 + rng.choice([-1.0, 1.0], (N, d)) * rng.uniform(0.05, 0.45, (N, d))      # away from nodes and cell midpoints
    for q in range(d):
        cell[4 + q, q] = 0                                          # first (boundary) cell of dim q
        cell[20 + q, q] = g[q] - 2                                  # last (boundary) cell of dim q
    cell[12:17] = 1
    X = np.array(grid.g0) + np.array(grid.h) * (cell + frac)
    X[10, 0] = grid.g0[0] - 1.0
    f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)
    X = f32(X)
    noise = f32(rng.uniform(0.5, 2.0, N))
    wa = f32(1.0 / noise)
    pvar = f32(rng.uniform(0.0, 2.0, N))
    pvar[5] = 0.0
    u = f32(rng.standard_normal(grid.m))
    mean = iref.dense_absorb(grid, X, np.zeros(N), np.zeros(N), wa, wa, noise, pvar, KS2, u)["mean_out"]
    s = np.sqrt(pvar + KS2 * noise)
    lo, hi = np.full(N, -INF), np.full(N, INF)
    kind = np.empty(N, dtype=object)
    turn = 0
    for i in range(N):
        if i in (0, 1):
            lo[i] = hi[i] = mean[i] + s[i] * rng.uniform(-2.0, 2.0)
            kind[i] = "exact"
        elif i == 2:
            kind[i] = "open"
        elif i == 3:
            lo[i] = mean[i] - 12.0 * s[i]
            kind[i] = "far"
        elif i == 10:
            lo[i] = 0.0
            kind[i] = "outside"
        else:
            k = ("lower", "upper", "two")[turn % 3]
            turn += 1
            kind[i] = k
            if k == "two":
                width = np.exp(rng.uniform(np.log(0.05), np.log(4.0)))
                a = rng.uniform(-8.0, 8.0 - width)
                lo[i], hi[i] = mean[i] + s[i] * a, mean[i] + s[i] * (a + width)
            else:
                t = rng.uniform(-8.0, 6.0)                          # > 0: satisfied by t s, < 0: violated
                if k == "lower":
                    lo[i] = mean[i] - t * s[i]
                else:
                    hi[i] = mean[i] + t * s[i]
    lo, hi = f32(lo), f32(hi)
    ref = iref.dense_absorb(grid, X, lo, hi, wa, wa, noise, pvar, KS2, u)
    _cases[name] = dict(grid=grid, X=X, lo=lo, hi=hi, wa=wa, noise=noise, pvar=pvar, u=u, ref=ref, ok=iref.inside(grid, X), kind=kind, s=s)
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


def _site_deviation(sites, ref):
    """ytilde: largest error over max |ytilde|; omega, log Z: largest error relative to the reference value itself (where it is not 0)."""
    yt, om, lz = (t.double().cpu().numpy() for t in sites)
    nz_o, nz_l = ref["omega"] != 0, ref["log_z"] != 0
    return dict(ytilde=float(np.abs(yt - ref["ytilde"]).max() / np.abs(ref["ytilde"]).max()),
                omega=float((np.abs(om - ref["omega"])[nz_o] / ref["omega"][nz_o]).max()),
                log_z=float((np.abs(lz - ref["log_z"])[nz_l] / np.abs(ref["log_z"][nz_l])).max()))


@pytest.mark.parametrize("name", list(KGRIDS))
def test_reference_split_of_the_kernel_case(name):
    """What the batch is meant to contain, on the reference alone: the skipped points are exactly the open and the far one, and every
    other site keeps a factor 1e4 from the skip threshold."""
    c = _kernel_case(name)
    r, kind, ok = c["ref"], c["kind"], c["ok"]
    assert list(np.nonzero(~ok)[0]) == [10] and r["err"] == 3
    assert list(np.nonzero(r["skipped"])[0]) == [2, 3] and (r["omega"][[0, 1]] == 1.0).all() and (r["ytilde"][[0, 1]] == c["lo"][[0, 1]]).all()
    ent = ok & ~r["skipped"]
    assert (r["omega"][ent] >= 1e4 * iref.OMEGA_MIN).all() and (r["omega"][ent] <= 1.0).all()
    assert all(int((kind == k).sum()) >= 9 for k in ("lower", "upper", "two")) and c["pvar"][5] == 0.0
    width = ((c["hi"] - c["lo"]) / c["s"])[kind == "two"]
    print(f"{name}: omega of the entering sites {r['omega'][ent].min():.2e} .. {r['omega'][ent].max():.3f}; two-sided widths {width.min():.3f} s .. {width.max():.3f} s")
    assert 0.049 <= width.min() and width.max() <= 4.001


@pytest.mark.parametrize("tdt,tol", DTYPES)
@pytest.mark.parametrize("name", list(KGRIDS))
def test_kernel_matches_the_dense_reference(name, tdt, tol):
    from online_gp_amd import grid_ops

    test_reference_split_of_the_kernel_case(name)                    # the split holds on the reference before the kernel is looked at
    c = _kernel_case(name)
    grid, ref, ok = c["grid"], c["ref"], c["ok"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    X, lo, hi, wa, noise, pvar, u = (mk(c[k]) for k in ("X", "lo", "hi", "wa", "noise", "pvar", "u"))
    rname = dict(ref, A=ref["A_half"])
    # from zero
    got, err = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    mean = torch.full((N,), float("nan"), device=DEV, dtype=tdt)
    sites = grid_ops.scatter_stats_interval(grid, X, lo, hi, pvar, KS2, wa, wa, noise, got["b"], got["A"], got["cnt"], got["stats"], err, u,
                                            res=got["res"], mean_out=mean)
    assert sites[0].dtype == tdt and sites[1].dtype == tdt and sites[2].dtype == torch.float64
    dev = _site_deviation(sites, ref)
    bound = FP64_SITE if tdt == torch.float64 else {k: (None if v is None else 3.0 * v) for k, v in FP32_SITE_DEV.items()}
    print(f"{name} {tdt} sites: " + "  ".join(f"{k} {dev[k]:.3e} (bound {bound[k]})" for k in dev))
    _compare(dict(got, mean_out=mean), rname, tol, KEYS + ("mean_out",), f"{name} zero-init")
    om = sites[1].double().cpu().numpy()
    assert np.array_equal(om == 0.0, ref["omega"] == 0.0)             # who is skipped (and who is outside): exactly the reference's
    assert (om[[0, 1]] == 1.0).all() and np.array_equal(sites[0].double().cpu().numpy()[[0, 1]], c["lo"][[0, 1]])     # exact values: exactly
    assert np.array_equal(sites[0].double().cpu().numpy()[[2, 3]], mean.double().cpu().numpy()[[2, 3]])               # skipped: ytilde = mu
    assert [float(v) for v in sites[0][10:11]] + [float(v) for v in sites[2][10:11]] == [0.0, 0.0]
    assert int(err.item()) == ref["err"] == 1 + 2 * 1                # bit 0 | one point dropped; a skipped point is not flagged
    for k in dev:
        assert bound[k] is not None and dev[k] <= bound[k], (name, k, dev[k], bound[k])
    # on top of non-zero buffers: every statistic is added, none assigned; the sites do not depend on what the buffers hold
    rng = np.random.default_rng(5)
    init = {k: 0.5 * float(np.abs(rname[k]).max()) * rng.standard_normal(np.shape(rname[k])) for k in KEYS}
    got = _buffers(grid, tdt, init)
    start = {k: v.double().cpu().numpy().copy() for k, v in got.items()}
    err.zero_()
    sites2 = grid_ops.scatter_stats_interval(grid, X, lo, hi, pvar, KS2, wa, wa, noise, got["b"], got["A"], got["cnt"], got["stats"], err, u, res=got["res"])
    _compare(got, {k: start[k] + rname[k] for k in KEYS}, tol, KEYS, f"{name} on top")
    assert all(torch.equal(a, b) for a, b in zip(sites, sites2))


@pytest.mark.parametrize("tdt,tol", DTYPES)
@pytest.mark.parametrize("name", list(KGRIDS))
def test_kernel_with_exact_values_only_is_the_plain_absorb(name, tdt, tol):
    from online_gp_amd import grid_ops

    c = _kernel_case(name)
    grid = c["grid"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    X, wa, noise, pvar, u = (mk(c[k]) for k in ("X", "wa", "noise", "pvar", "u"))
    Y = mk(np.where(np.isfinite(c["lo"]), c["lo"], np.where(np.isfinite(c["hi"]), c["hi"], 0.25)))
    got, want = _buffers(grid, tdt), _buffers(grid, tdt)
    e1, e2 = grid_ops.new_err_flag(DEV), grid_ops.new_err_flag(DEV)
    yt, omega, _ = grid_ops.scatter_stats_interval(grid, X, Y, Y, pvar, KS2, wa, wa, noise, got["b"], got["A"], got["cnt"], got["stats"], e1, u, res=got["res"])
    grid_ops.scatter_stats_cnt(grid, X, Y, wa, wa, noise, want["b"], want["A"], True, want["cnt"], want["stats"], e2, u=u, res=want["res"])
    _compare(got, {k: v.double().cpu().numpy() for k, v in want.items()}, tol, KEYS, f"{name} exact")
    assert int(e1.item()) == int(e2.item()) == 3
    assert np.array_equal(omega.double().cpu().numpy(), c["ok"].astype(np.float64))
    assert torch.equal(yt[mk(c["ok"]).bool()], Y[mk(c["ok"]).bool()])


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64])
def test_absorb_refuses_the_interval_group_with_what_the_kernel_does_not_do(tdt):
    """Through the full argument record plus the interval group (wiski_absorb_interval): every combination the contract refuses is
    WISKI_E_BADARG before any launch -- every buffer untouched -- while the record without the offending field runs and equals
    grid_ops.scatter_stats_interval; res and mean_out are optional, the record's d_y is ignored."""
    from online_gp_amd import _hip, grid_ops

    c = _kernel_case("d3")
    grid = c["grid"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    X, lo, hi, wa, noise, pvar, u = (mk(c[k]) for k in ("X", "lo", "hi", "wa", "noise", "pvar", "u"))
    buf, err = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    nan = lambda dt=tdt: torch.full((N,), float("nan"), device=DEV, dtype=dt)
    mean, yt, omega, logz = nan(), nan(), nan(), nan(torch.float64)
    full = torch.zeros((grid.R, grid.m), device=DEV, dtype=tdt)
    guard = torch.tensor([7], device=DEV, dtype=torch.int64)
    z1 = torch.full((2,), 0x01010101, device=DEV, dtype=torch.int32)
    bin_ws = torch.zeros(1 << 16, device=DEV, dtype=torch.uint8)
    p = lambda t: t.data_ptr()
    stream = _hip.stream_ptr(torch.device("cuda", torch.cuda.current_device()))

    def call(lo_=lo, hi_=hi, pvar_=pvar, sigma2=KS2, yt_=yt, omega_=omega, logz_=logz, **kw):
        a = _hip.wiski_absorb_args(d_x=p(X), d_y=None, d_wa=p(wa), d_wb=p(wa), d_noise=p(noise), n=N, d_b=p(buf["b"]), d_A=p(buf["A"]), half=1,
                                   channels=0, d_cnt=p(buf["cnt"]), d_stats=p(buf["stats"]), d_err=p(err), d_u=p(u), d_res=p(buf["res"]),
                                   d_mean_out=p(mean), nout=1)
        for k, v in kw.items():
            setattr(a, k, v)
        return _hip.fn("wiski_absorb_interval", tdt)(grid.ref, ctypes.byref(a), _hip.dptr(lo_), _hip.dptr(hi_), _hip.dptr(pvar_), ctypes.c_double(sigma2),
                                                     _hip.dptr(yt_), _hip.dptr(omega_), _hip.dptr(logz_), stream)

    refused = [("no u", call(d_u=None, d_res=None, d_mean_out=None)), ("full stencil", call(half=0, d_A=p(full))), ("no A", call(d_A=None)),
               ("no cnt", call(d_cnt=None)), ("nout = 2", call(nout=2, d_mean_out=None)), ("channels", call(channels=4)),
               ("guard", call(d_guard=p(guard), guard_expect=7)), ("zero region", call(z1=p(z1), n1_bytes=8)), ("shard", call(g_lo=0, g_hi=3)),
               ("owner workspace", call(d_bin=p(bin_ws), bin_bytes=bin_ws.numel())), ("sigma2 = 0", call(sigma2=0.0)), ("sigma2 < 0", call(sigma2=-1.0)),
               ("sigma2 = inf", call(sigma2=float("inf"))), ("sigma2 = nan", call(sigma2=float("nan"))), ("no lo", call(lo_=None)), ("no hi", call(hi_=None)),
               ("no pvar", call(pvar_=None)), ("no ytilde_out", call(yt_=None)), ("no omega_out", call(omega_=None)), ("no logz_out", call(logz_=None))]
    torch.cuda.synchronize()
    assert [(what, rc) for what, rc in refused if rc != -1] == []
    assert all(float(v.abs().max()) == 0.0 for v in buf.values()) and float(full.abs().max()) == 0.0 and int(err.item()) == 0
    assert all(bool(torch.isnan(t).all()) for t in (mean, yt, omega, logz)) and bool((z1 == 0x01010101).all())
    assert call() == 0
    want, e2 = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    sites = grid_ops.scatter_stats_interval(grid, X, lo, hi, pvar, KS2, wa, wa, noise, want["b"], want["A"], want["cnt"], want["stats"], e2, u, res=want["res"])
    tol = dict(DTYPES)[tdt]
    _compare(buf, {k: v.double().cpu().numpy() for k, v in want.items()}, tol, KEYS, "record")
    assert all(torch.equal(a, b) for a, b in zip(sites, (yt, omega, logz))) and int(err.item()) == int(e2.item()) == 3
    assert call(d_res=None, d_mean_out=None) == 0                    # u alone is a complete request: res and mean_out are optional
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- the model
GB, GS = [[-1.0, 1.0], [-1.0, 1.0]], [12, 10]
N0, Q, NB = 40, 16, 3
STREAM_SEED = 4


def _f(X):
    return np.sin(2 * X[:, 0]) * np.cos(X[:, 1]) + 0.5 * X[:, 1]


def _stream(seed=STREAM_SEED, plain=False):
    """40 points with values, then 3 batches of 16 given as bounds: readings above 0.3 are censored there (a lower bound), the others
    are binned to width 0.25; per batch, point 0 is an exact value and point 1 says nothing (it must not count in num_data; left out
    with plain=True, the stream of the path-probe test).  The declared noise is drawn from U(0.5, 2) for the reason
    tests/test_grad_obs_gpu.py::_data gives: the MLL bounds are relative."""
    rng = np.random.default_rng(seed)
    n = N0 + NB * Q
    X = rng.uniform(-0.95, 0.95, (n, 2))
    noise = rng.uniform(0.5, 2.0, n)
    y = _f(X) + 0.05 * rng.standard_normal(n)
    lo, hi = np.floor(y / 0.25) * 0.25, np.floor(y / 0.25) * 0.25 + 0.25
    cens = y > 0.3
    lo[cens], hi[cens] = 0.3, INF
    if not plain:
        for k in range(NB):
            i = N0 + k * Q
            lo[i] = hi[i] = y[i]
            lo[i + 1], hi[i + 1] = -INF, INF
    Xs = rng.uniform(-0.95, 0.95, (50, 2))
    return X, y, noise, lo, hi, Xs


def _oracle(hyp=None):
    ell, s, s2 = hyp if hyp is not None else (spec.SOFTPLUS0, spec.SOFTPLUS0, spec.SOFTPLUS0)
    return dataspace.DataSpaceGP(GB, GS, "rbf", ell, s, s2)


_refs = {}


def _reference_stream(gamma=None, nb=NB, seed=STREAM_SEED, hyp=None):
    """The stream through the fp64 oracle: before batch k the oracle holds the initial points and the pseudo-observations so far at their
    effective noise (noise_i / omega_i, aged by 1 / gamma per batch under forgetting); its predictive mean and variance at the batch give
    the batch's sites (interval_reference.sites), whose skipped points are left out.  Returns per batch (sites, mean and variance at the
    queries, MLL, number of points held); computed once per setting."""
    key = (gamma, nb, seed, hyp)
    if key in _refs:
        return _refs[key]
    X, y, noise, lo, hi, Xs = _stream(seed)
    O = _oracle(hyp)
    Xp, yp, eff = X[:N0], y[:N0], noise[:N0].copy()
    steps = []
    for k in range(nb):
        sl = slice(N0 + k * Q, N0 + (k + 1) * Q)
        if gamma is not None:
            eff = eff / gamma
        O.fit(Xp, yp, eff)
        mean, var = O.predict(X[sl])
        st = iref.sites(lo[sl], hi[sl], mean, var, O.sigma2 * noise[sl])
        ent = ~st["skipped"]
        Xp, yp, eff = np.concatenate([Xp, X[sl][ent]]), np.concatenate([yp, st["ytilde"][ent]]), np.concatenate([eff, noise[sl][ent] / st["omega"][ent]])
        O.fit(Xp, yp, eff)
        mo, vo = O.predict(Xs)
        steps.append(dict(sites=st, mean=mo, var=vo, mll=O.mll(), n=yp.shape[0]))
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


def _check_against(m, step, Xs, dtype, label, mll_bound, sites=True):
    if sites:
        yt, om, lz = (t.double().cpu().numpy() for t in m.last_interval_sites)
        st = step["sites"]
        e_y, e_o = np.abs(yt - st["ytilde"]).max() / np.abs(st["ytilde"]).max(), np.abs(om - st["omega"]).max()
        e_l = np.abs(lz - st["log_z"]).max() / np.abs(st["log_z"]).max()
        print(f"{label} {dtype}: ytilde {e_y:.3e}  omega {e_o:.3e}  log Z {e_l:.3e}  (bound {RTOL[dtype]:.0e}; {int(st['skipped'].sum())} of {om.size} skipped, "
              f"omega {st['omega'][~st['skipped']].min():.4f} .. {st['omega'].max():.4f})")
        assert e_y <= RTOL[dtype] and e_o <= RTOL[dtype] and e_l <= RTOL[dtype]
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


def _absorb_batch(m, k, dtype, inplace=True):
    X, y, noise, lo, hi, Xs = _stream()
    sl = slice(N0 + k * Q, N0 + (k + 1) * Q)
    return m.condition_on_observations(_t(X[sl], dtype), None, _t(noise[sl], dtype), lower=_t(lo[sl], dtype), upper=_t(hi[sl], dtype), inplace=inplace)


def _check_regime(dtype, label, mll_bound, **kw):
    X, y, noise, lo, hi, Xs = _stream()
    m = _model(X[:N0], y[:N0], noise[:N0], dtype, **kw).eval()
    assert m.last_interval_sites is None                             # the initial data is absorbed plainly
    steps = _reference_stream(kw.get("forgetting_factor"), hyp=_hyp(m))
    for k, step in enumerate(steps):
        st = step["sites"]
        assert list(np.nonzero(st["skipped"])[0]) == [1] and st["omega"][0] == 1.0 and 0.0 < st["omega"][2:].min() and st["omega"][2:].max() < 1.0
        _absorb_batch(m, k, dtype)
        assert all(t.shape == (Q,) and t.is_cuda for t in m.last_interval_sites)
        _check_against(m, step, Xs, dtype, f"{label} batch {k}", mll_bound)
    return m


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_dense_regime_matches_the_oracle_at_the_pseudo_observations(dtype):
    """12 x 10 grid, 40 points with values, 3 batches of 16 given as bounds, 50 queries; figures printed before the asserts."""
    _check_regime(dtype, "dense", MLL_DENSE)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_matrix_free_regime_matches_the_oracle_at_the_pseudo_observations(dtype):
    from online_gp_amd import settings
    from online_gp_amd.mlls.batched_woodbury_marginal_log_likelihood import num_trace_samples

    with settings.dense_small_grids(False), settings.spectral_factor(False), num_trace_samples(64), \
            settings.cg_tolerance(1e-10 if dtype == torch.float64 else 1e-6):
        m = _check_regime(dtype, "matrix-free", MLL_FREE)
        assert m._mean_state is not None


def test_functional_form_leaves_the_parent_alone_and_sets_the_sites_on_the_child():
    dtype = torch.float64
    X, y, noise, lo, hi, Xs = _stream()
    m = _model(X[:N0], y[:N0], noise[:N0], dtype).eval()
    step = _reference_stream(None, nb=1, hyp=_hyp(m))[0]
    before = [t.clone() for t in m.stats_buffers()]
    child = _absorb_batch(m, 0, dtype, inplace=False)
    assert all(torch.equal(a, b) for a, b in zip(before, m.stats_buffers())) and m.num_data == N0 and m.last_interval_sites is None
    assert child.num_data == N0 + Q - 1
    _check_against(child.eval(), step, Xs, dtype, "functional", MLL_DENSE)
    _absorb_batch(m, 0, dtype)
    _check_against(m, step, Xs, dtype, "in place", MLL_DENSE)


def test_forgetting_ages_the_effective_noise():
    """forgetting_factor = 0.9 over two batches of bounds: the oracle at d_i gamma^-k / omega_i, the sites of a batch matched against the
    decayed posterior; in place and, for the second batch, functional."""
    dtype, gam = torch.float64, 0.9
    X, y, noise, lo, hi, Xs = _stream()
    m = _model(X[:N0], y[:N0], noise[:N0], dtype, forgetting_factor=gam).eval()
    steps = _reference_stream(gam, nb=2, hyp=_hyp(m))
    assert np.abs(steps[1]["mean"] - _reference_stream(None, nb=2, hyp=_hyp(m))[1]["mean"]).max() > 10 * RTOL[dtype] * np.abs(steps[1]["mean"]).max()
    _absorb_batch(m, 0, dtype)
    _check_against(m, steps[0], Xs, dtype, "forgetting batch 0", MLL_DENSE)
    child = _absorb_batch(m, 1, dtype, inplace=False)
    _check_against(child.eval(), steps[1], Xs, dtype, "forgetting batch 1, functional", MLL_DENSE)
    _absorb_batch(m, 1, dtype)
    _check_against(m, steps[1], Xs, dtype, "forgetting batch 1, in place", MLL_DENSE)


def test_path_probes_receive_the_effective_weights():
    """num_path_probes > 0, PCG route: after a batch of bounds the sample paths equal Matheron's rule in data space at the weights
    omega_i / d_i and targets ytilde_i, path by path -- the probes entered with sqrt(wa omega), so cov(P) is still A.  Bound: the fp64
    tolerance of the model checks of this file, 1e-4 of max |reference path|, against a reference whose two routes (data space and
    grid space) agree to 4e-15 on this problem; paths drawn at the plain weights lie 0.11 away, which the last line asserts the check
    would see.  The deviation of the model's own posterior mean is printed beside it: both are what a CG solve at tolerance 1e-10
    leaves (measured on one MI355X: path 5.0e-08, mean 1.5e-08, ratio 3.26 -- the "3 x the mean's deviation" yardstick of
    tests/test_sample_paths_gpu.py compares two outputs of the code under test with each other, bounds neither, and is not used here)."""
    from online_gp_amd import settings
    from online_gp_amd.kernels import GridInterpolationKernel, MaternKernel, ScaleKernel
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    dtype, S, seed, ell, osc, s2 = torch.float64, 8, 21, [0.35, 0.5], 1.2, 0.3
    X, y, noise, lo, hi, Xs = _stream(plain=True)
    n = N0 + Q
    with settings.dense_small_grids(False), settings.spectral_factor(False), settings.cg_tolerance(1e-10), torch.no_grad():
        k = GridInterpolationKernel(ScaleKernel(MaternKernel(nu=2.5, ard_num_dims=2)), grid_size=GS, num_dims=2, grid_bounds=torch.tensor(GB))
        k.base_kernel.outputscale = osc
        k.base_kernel.base_kernel.lengthscale = torch.as_tensor(ell)
        m = FixedNoiseOnlineSKIGP(_t(X[:N0], dtype), _t(y[:N0], dtype)[:, None], _t(noise[:N0], dtype)[:, None], covar_module=k,
                                  learn_additional_noise=True, num_path_probes=S, path_seed=seed)
        m.likelihood.second_noise = s2
        m.eval()
        m.condition_on_observations(_t(X[N0:n], dtype), None, _t(noise[N0:n], dtype), lower=_t(lo[N0:n], dtype), upper=_t(hi[N0:n], dtype), inplace=True)
        O = dataspace.DataSpaceGP(GB, GS, "matern52", ell, osc, s2).fit(X[:N0], y[:N0], noise[:N0])
        st = iref.sites(lo[N0:n], hi[N0:n], *O.predict(X[N0:n]), s2 * noise[N0:n])
        assert not st["skipped"].any() and st["omega"].max() < 1.0
        assert np.abs(m.last_interval_sites[1].cpu().numpy() - st["omega"]).max() <= RTOL[dtype]
        wts = np.concatenate([np.ones(N0), st["omega"]]) / noise[:n]
        yp = np.concatenate([y[:N0], st["ytilde"]])
        O.fit(X[:n], yp, 1.0 / wts)
        g0, h, gg = spec.make_grid(GB, GS)
        W, Kuu = spr.dense_w(g0, h, gg, X[:n]), spr.kuu_dense(O.cols)
        u_mean = Kuu @ (W.T @ O.alpha)
        z = torch.randn((S, m._grid.m), generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        paths = m.sample_paths(S, base_samples=z.to(DEV))
        assert paths.last_converged
        U = m.prediction_cache["pred_mean"][0, :, 0].cpu().numpy()
        dev_mean = np.abs(U - u_mean).max() / np.abs(u_mean).max()
        uo = spr.path_dataspace(Kuu, W, wts, yp, s2, (spr.sym_sqrt(Kuu) @ z.numpy().T).T, spr.normals(seed, np.arange(n), S))
        dev_path = np.abs(paths.values.cpu().numpy() - uo).max() / np.abs(uo).max()
        plain = spr.path_dataspace(Kuu, W, 1.0 / noise[:n], yp, s2, (spr.sym_sqrt(Kuu) @ z.numpy().T).T, spr.normals(seed, np.arange(n), S))
        print(f"interval paths: path deviation {dev_path:.3e}, mean deviation {dev_mean:.3e}, ratio {dev_path / dev_mean:.2f}; "
              f"distance to the plainly weighted paths {np.abs(plain - uo).max() / np.abs(uo).max():.3e}")
        assert dev_path <= RTOL[dtype] and dev_mean <= RTOL[dtype]
        assert np.abs(plain - uo).max() / np.abs(uo).max() > 1e-2      # (the check can tell the effective weights from the plain ones)


def test_interval_probability_against_scipy():
    from scipy import special as sp

    dtype = torch.float64
    X, y, noise, lo, hi, Xs = _stream()
    m = _model(X[:N0], y[:N0], noise[:N0], dtype).eval()
    mvn = m(_t(Xs, dtype))
    mean, var = mvn.mean.detach().cpu().numpy(), mvn.variance.detach().cpu().numpy()
    rng = np.random.default_rng(8)
    nz = rng.uniform(0.5, 2.0, 50)
    s = np.sqrt(var + _hyp(m)[2] * nz)
    a = rng.uniform(-4.0, 3.0, 50)
    b = a + rng.uniform(0.1, 3.0, 50)
    lo_q, hi_q = mean + s * a, mean + s * b
    lo_q[:10], hi_q[10:20] = -INF, INF
    a[:10], b[10:20] = -INF, INF
    want = np.log(sp.ndtr(b) - sp.ndtr(a))
    want[:10], want[10:20] = sp.log_ndtr(b[:10]), sp.log_ndtr(-a[10:20])
    got = m.interval_probability(_t(Xs, dtype), _t(lo_q, dtype), _t(hi_q, dtype), noise=_t(nz, dtype)).cpu().numpy()
    e = np.abs(got - want).max() / np.abs(want).max()
    print(f"interval_probability: {e:.3e} of max |log P| = {np.abs(want).max():.3f}")
    assert got.shape == (50,) and e <= 1e-10
    one = m.interval_probability(_t(Xs, dtype), None, _t(hi_q, dtype)).cpu().numpy()       # unit noise, no lower bound
    assert np.abs(one - sp.log_ndtr((hi_q - mean) / np.sqrt(var + _hyp(m)[2]))).max() <= 1e-10 * np.abs(one).max()


def test_default_model_never_enters_the_interval_path(monkeypatch):
    """Without bounds the interval launch is never made (the binding is replaced by one that raises) and no site is recorded."""
    from online_gp_amd import grid_ops

    def forbidden(*a, **k):
        raise AssertionError("the interval absorb was launched by a model that was given no bounds")

    monkeypatch.setattr(grid_ops, "scatter_stats_interval", forbidden)
    dtype = torch.float64
    X, y, noise, lo, hi, Xs = _stream()
    m = _model(X[:N0], y[:N0], noise[:N0], dtype).eval()
    for a in range(N0, N0 + NB * Q, Q):
        m.condition_on_observations(_t(X[a:a + Q], dtype), _t(y[a:a + Q], dtype), _t(noise[a:a + Q], dtype), inplace=True)
    child = m.condition_on_observations(_t(X[:Q], dtype), _t(y[:Q], dtype), _t(noise[:Q], dtype))
    assert m.last_interval_sites is None and child.last_interval_sites is None and m.num_data == N0 + NB * Q
    with pytest.raises(AssertionError):                             # (and the replacement is what a batch of bounds would have called)
        m.condition_on_observations(_t(X[:Q], dtype), None, _t(noise[:Q], dtype), lower=_t(lo[N0:N0 + Q], dtype), inplace=True)


def test_refusals():
    from online_gp_amd.distributed import ShardedStatsUpdater
    from online_gp_amd.models import FixedNoiseOnlineSKIGP, OnlineSKIBotorchModel

    dtype = torch.float64
    X, y, noise, lo, hi, Xs = _stream()
    Xt, yt, nt = _t(X[:12], dtype), _t(y[:12], dtype), _t(noise[:12], dtype)
    lt, ht = _t(y[:12] - 0.1, dtype), _t(y[:12] + 0.1, dtype)
    two = FixedNoiseOnlineSKIGP(Xt, torch.stack([yt, yt], 1), None, grid_bounds=torch.tensor(GB), grid_size=GS)
    with pytest.raises(NotImplementedError):                        # several outputs
        two.condition_on_observations(Xt, None, nt, lower=lt, upper=ht, inplace=True)
    m = _model(X[:12], y[:12], noise[:12], dtype)
    before = [t.clone() for t in m.stats_buffers()]
    with pytest.raises(NotImplementedError):                        # targets and bounds
        m.condition_on_observations(Xt, yt, nt, lower=lt, upper=ht, inplace=True)
    with pytest.raises(NotImplementedError):                        # derivative observations
        m.condition_on_observations(Xt, None, nt, lower=lt, grad_Y=torch.zeros(12, 2, device=DEV, dtype=dtype))
    with pytest.raises(NotImplementedError):                        # fantasies (batched X)
        m.condition_on_observations(Xt[None], None, nt[None], lower=lt[None], upper=ht[None])
    with pytest.raises(NotImplementedError):                        # the data-parallel statistics exchange
        m._absorb_interval(m._kernel_cache, Xt, lt, ht, nt, m, half_delta=m._half_buffers())
    with pytest.raises(NotImplementedError):
        ShardedStatsUpdater(m).update(Xt, None, nt, lower=lt, upper=ht)
    for kw in (dict(robust_c=2.0), dict(window=64)):
        r = _model(X[:12], y[:12], noise[:12], dtype, **kw)
        with pytest.raises(NotImplementedError):
            r.condition_on_observations(Xt, None, nt, lower=lt, upper=ht, inplace=True)
    assert all(torch.equal(a, b) for a, b in zip(before, m.stats_buffers())) and m.num_data == 12 and m.last_interval_sites is None
    # a handed-over full-stencil cache
    cache = m._clone_cache(m._kernel_cache)
    op = cache["WtW"]
    full = torch.zeros((m._grid.R, m._grid.m), device=DEV, dtype=dtype)
    cache["WtW"] = type(op)(m._grid, full)
    h = FixedNoiseOnlineSKIGP(covar_module=m.covar_module, kernel_cache=cache, likelihood=m.likelihood, learn_additional_noise=True, num_data=12)
    with pytest.raises(NotImplementedError):
        h.condition_on_observations(Xt, None, nt, lower=lt, upper=ht, inplace=True)
    # the BoTorch-facing wrapper passes the bounds through
    b = OnlineSKIBotorchModel(Xt, yt[:, None], nt[:, None], grid_bounds=torch.tensor(GB), grid_size=GS)
    b.eval()
    b.condition_on_observations(Xt, None, nt, lower=lt, upper=ht, inplace=True)
    assert b.num_data == 24 and float(b.last_interval_sites[1].min()) > 0.0


# ------------------------------------------------------------------------------------------------------- two streams where it has to pay
TB, TG, TELL, TOSC, TS2 = [[-0.15, 1.15]], [32], [0.25], 1.0, 0.05
TSEED, TLIMIT = 4, 0.6


def _toy_f(x):
    return np.sin(6.0 * x) + 0.5 * x


def _toy():
    """sin 6x + x / 2 on [0, 1], noise variance 0.05, 8 batches of 16, 50 queries."""
    rng = np.random.default_rng(TSEED)
    X = rng.uniform(0.0, 1.0, (128, 1))
    y = _toy_f(X[:, 0]) + np.sqrt(TS2) * rng.standard_normal(128)
    return X, y, np.linspace(0.02, 0.98, 50)[:, None]


def _toy_bounds(y, mode):
    if mode == "limit":                                              # the limit fed as if it were the value
        v = np.minimum(y, TLIMIT)
        return v, v
    if mode == "censored":
        return np.where(y > TLIMIT, TLIMIT, y), np.where(y > TLIMIT, INF, y)
    from online_gp_amd.models import interval_from_labels

    lo, hi = interval_from_labels(torch.as_tensor((y > 0).astype(np.int64)))
    return lo.double().numpy(), hi.double().numpy()


def _toy_reference(mode):
    """The stream through the fp64 oracle, started from one point that says nothing (noise 1e6): (mean at the queries, mean log Z)."""
    X, y, Xs = _toy()
    lo, hi = _toy_bounds(y, mode)
    O = dataspace.DataSpaceGP(TB, TG, "rbf", TELL, TOSC, TS2)
    Xp, yp, eff, lz = np.array([[0.5]]), np.array([0.0]), np.array([1e6]), []
    for k in range(8):
        sl = slice(16 * k, 16 * k + 16)
        st = iref.sites(lo[sl], hi[sl], *O.fit(Xp, yp, eff).predict(X[sl]), TS2 * np.ones(16))
        ent = ~st["skipped"]
        lz.append(st["log_z"])
        Xp, yp, eff = np.concatenate([Xp, X[sl][ent]]), np.concatenate([yp, st["ytilde"][ent]]), np.concatenate([eff, 1.0 / st["omega"][ent]])
    return O.fit(Xp, yp, eff).predict(Xs)[0], float(np.mean(lz))


def _toy_model(mode):
    from online_gp_amd.kernels import GridInterpolationKernel, RBFKernel, ScaleKernel
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    dtype = torch.float64
    X, y, Xs = _toy()
    lo, hi = _toy_bounds(y, mode)
    with torch.no_grad():
        k = GridInterpolationKernel(ScaleKernel(RBFKernel(ard_num_dims=1)), grid_size=TG, num_dims=1, grid_bounds=torch.tensor(TB))
        k.base_kernel.outputscale = TOSC
        k.base_kernel.base_kernel.lengthscale = torch.as_tensor(TELL)
        m = FixedNoiseOnlineSKIGP(_t([[0.5]], dtype), _t([[0.0]], dtype), _t([[1e6]], dtype), covar_module=k, learn_additional_noise=True)
        m.likelihood.second_noise = TS2
        m.eval()
        lz = []
        for a in range(0, 128, 16):
            m.condition_on_observations(_t(X[a:a + 16], dtype), None, torch.ones(16, device=DEV, dtype=dtype), lower=_t(lo[a:a + 16], dtype),
                                        upper=_t(hi[a:a + 16], dtype), inplace=True)
            lz.append(m.last_interval_sites[2].cpu().numpy())
        return m(_t(Xs, dtype)).mean.cpu().numpy(), float(np.mean(lz))


def _rmse(mean):
    return float(np.sqrt(np.mean((mean - _toy_f(_toy()[2][:, 0])) ** 2)))


def test_censored_stream_beats_feeding_the_limit_as_a_value():
    """Readings above 0.6 are censored.  RMSE to the noise-free truth at 50 queries: the model given [0.6, inf) for a censored point is at
    most half as far off as the model given 0.6.  (Asserted first on the fp64 references, which differ by a factor of five.)"""
    r_int, r_lim = _rmse(_toy_reference("censored")[0]), _rmse(_toy_reference("limit")[0])
    print(f"reference RMSE: interval {r_int:.4f}  limit as value {r_lim:.4f}  ratio {r_lim / r_int:.2f}")
    assert r_int <= 0.5 * r_lim
    g_int, g_lim = _rmse(_toy_model("censored")[0]), _rmse(_toy_model("limit")[0])
    print(f"model RMSE: interval {g_int:.4f}  limit as value {g_lim:.4f}  ratio {g_lim / g_int:.2f}")
    assert g_int <= 0.5 * g_lim


def test_probit_stream_classifies_and_predicts_its_labels():
    """Labels y > 0 of the same stream through interval_from_labels, unit noise: the sign of the posterior mean agrees with the sign of
    the truth at >= 0.85 of 50 queries, and the mean log predictive probability of the labels over the stream is above -0.55 (chance:
    log 1/2 = -0.69)."""
    truth = _toy_f(_toy()[2][:, 0]) > 0
    mean_r, lz_r = _toy_reference("probit")
    print(f"reference: accuracy {np.mean((mean_r > 0) == truth):.3f}  mean log Z {lz_r:.4f}")
    mean, lz = _toy_model("probit")
    acc = float(np.mean((mean > 0) == truth))
    print(f"model: accuracy {acc:.3f}  mean log Z {lz:.4f}")
    assert acc >= 0.85 and lz > -0.55
