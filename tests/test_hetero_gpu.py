"""GPU: the heteroscedastic absorb -- a second field on the same grid, g = log of the noise multiplier, learned from
the stream's own residuals inside the launch that absorbs the batch -- against the fp64 reference of tests/hetero_reference.py (pinned
to 50 digits in tests/test_hetero_host.py) and the data-space oracle fitted at the reference's effective noises and pseudo-targets:
the evaluator alone on the specified box, the kernel through the C ABI, the contract, the model surface, and the stream on which the
feature has to pay.

Bounds.  Evaluator: three times the deviations measured on one MI355X (FP64_DEV, FP32_DEV below; DESIGN.md 3.27 tabulates them), in the
quantities the posterior receives; no fp64 figure may exceed 1e-6.  Statistics of BOTH models: those of tests/test_grad_obs_gpu.py
(scatter 1e-11 / 2e-4, x 10, relative to max |reference|).  Sites of the kernel cases in fp64: 1e-9, what the reference itself is
pinned to; in fp32 the predictive means reach the site in fp32, and the test asserts three times FP32_SITE_DEV, measured likewise.
Model: the bounds of tests/test_count_gpu.py, 1e-4 / 1e-2.
"""
import ctypes

import numpy as np
import pytest
import torch

import hetero_reference as href
from oracle import dataspace

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [(torch.float64, 1e-11), (torch.float32, 2e-4)]          # the scatter tolerances of tests/test_grad_obs_gpu.py
RTOL = {torch.float64: 1e-4, torch.float32: 1e-2}
f32 = lambda a: np.asarray(a).astype(np.float32).astype(np.float64)

# ------------------------------------------------------------------------------------------------------------- the evaluator alone
NSWEEP = 400
# measured on one MI355X against hetero_reference.sites, 400 box cases: |mhat - mhat_ref| / sqrt Vhat_ref,
# |Vhat - Vhat_ref| / Vhat_ref, log Z relative, tau relative where v tau <= 1 and at v = 0
FP64_DEV = dict(m=4.602e-15, V=9.298e-16, log_z=5.743e-14, tau=1.159e-13)
# (fp32: ytilde and tau are stored in fp32; log Z is a double in both precisions and the inputs are exact in fp32)
FP32_DEV = dict(m=7.859e-07, V=4.669e-08, log_z=5.743e-14, tau=5.570e-08)
FP64_CEILING = 1e-6
_sweep_cache = []


def _sweep():
    """400 box cases rounded to fp32, so that both precisions see the same inputs, and their reference sites; once."""
    if not _sweep_cache:
        rho, nu, mu, v = (f32(a) for a in href.box_cases(NSWEEP, 41))
        _sweep_cache.append((rho, nu, mu, v, href.sites(rho, nu, mu, v)))
    return _sweep_cache[0]


@pytest.mark.parametrize("tdt", [torch.float64, torch.float32])
def test_evaluator_on_the_box(tdt):
    from online_gp_amd import grid_ops

    rho, nu, mu, v, ref = _sweep()
    assert not ref["skipped"].any() and (v <= 9.0).all() and int((v == 0).sum()) == NSWEEP // 20 and set(nu) == {1.0, 4.0}
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    yt, tau, lz = grid_ops.hetero_sites(mk(mu), mk(v), mk(rho), mk(nu))
    assert yt.dtype == tdt and tau.dtype == tdt and lz.dtype == torch.float64
    got = dict(ytilde=yt.double().cpu().numpy(), tau=tau.double().cpu().numpy(), log_z=lz.cpu().numpy())
    dev = href.deviation(got, ref, mu, v)
    measured = FP64_DEV if tdt == torch.float64 else FP32_DEV
    print(f"log-variance {tdt} evaluator: " + "  ".join(f"{k} {dev[k]:.3e} (bound {3 * measured[k]:.3e})" for k in dev))
    assert (got["tau"] > 0).all()
    if tdt == torch.float64:
        assert max(measured.values()) <= FP64_CEILING and max(dev.values()) <= FP64_CEILING
    for k in dev:
        assert dev[k] <= 3.0 * measured[k], (tdt, k, dev[k], measured[k])


# ------------------------------------------------------------------------------------------------------------------ the kernel
KGRIDS = {"d1": [8], "d2": [8, 8], "d3": [8, 8, 8], "d4": [6, 6, 6, 6]}
N = 37                                                            # three blocks of 16; the last pass of the last block holds one point
KS2, G0 = 0.75, 0.25                                              # sigma2 and the prior mean of g of the kernel cases
KEYS = ("A", "b", "cnt", "stats", "res")
SITE_KEYS = ("e", "ytilde", "tau", "log_z", "log_zy")
FP64_SITE = {k: 1e-9 for k in SITE_KEYS}
# measured on one MI355X, fp32 against the fp64 reference, largest over the four grids
# (ytilde and tau: a residual of 1e-2 of its scale is the difference of two fp32 numbers, and rho is its square)
FP32_SITE_DEV = dict(e=7.765e-07, ytilde=6.735e-05, tau=6.734e-05, log_z=1.124e-06, log_zy=3.478e-07)
_cases = {}


def _kernel_case(name):
    """Grid, 37 points (fp64 values that are exact in fp32) and the dense reference; once.
      0: in the first cell of every dim, where the row collapses to the one-hot of node 0, with y = mu_f = u[0] exactly (rho = 0: f
         enters, g is skipped)   1: a 20-sigma residual   3: y = NaN
      5: pvar_f = 0   6: pvar_g = 0   10: outside the grid   12 .. 16 share one interior cell (colliding atomics)
      4 + q / 20 + q: first / last cell of dim q.  noise_p is non-unit throughout."""
    if name in _cases:
        return _cases[name]
    from online_gp_amd import grid_ops

    g = KGRIDS[name]
    d = len(g)
    rng = np.random.default_rng(700 + d)
    grid = grid_ops.GridSpec([[-1.0, 1.0 + 0.25 * q] for q in range(d)], g)
    cell = np.stack([rng.integers(0, gq - 1, N) for gq in g], 1).astype(np.float64)
    frac = 0.5 + rng.choice([-1.0, 1.0], (N, d)) * rng.uniform(0.05, 0.45, (N, d))      # away from nodes and cell midpoints
    for q in range(d):
        cell[4 + q, q] = 0                                          # first (boundary) cell of dim q
        cell[20 + q, q] = g[q] - 2                                  # last (boundary) cell of dim q
    cell[12:17] = 1
    cell[0], frac[0] = 0, 0.3                                       # a boundary cell of every dim: the row is the one-hot of node 0
    X = np.array(grid.g0) + np.array(grid.h) * (cell + frac)
    X[10, 0] = grid.g0[0] - 1.0
    X = f32(X)
    noise = f32(rng.uniform(0.5, 2.0, N))
    wa = f32(1.0 / noise)
    pvar, pvar2 = f32(rng.uniform(0.0, 2.0, N)), f32(rng.uniform(0.0, 1.5, N))
    pvar[5], pvar2[6] = 0.0, 0.0
    u, u2 = f32(rng.standard_normal(grid.m)), f32(0.7 * rng.standard_normal(grid.m))
    probe = href.dense_absorb(grid, X, np.zeros(N), wa, wa, noise, pvar, pvar2, KS2, G0, u, u2)
    sd = np.sqrt(np.maximum(pvar, 0) + KS2 * noise * probe["e"])
    y = probe["mean_out"] + sd * rng.standard_normal(N)
    y[1] = probe["mean_out"][1] + 20.0 * sd[1]
    y = f32(y)
    y[0], y[3] = probe["mean_out"][0], np.nan
    assert y[0] == u[0]
    ref = href.dense_absorb(grid, X, y, wa, wa, noise, pvar, pvar2, KS2, G0, u, u2)
    _cases[name] = dict(grid=grid, X=X, y=y, wa=wa, noise=noise, pvar=pvar, pvar2=pvar2, u=u, u2=u2, ref=ref, ok=href.inside(grid, X))
    return _cases[name]


def _buffers(grid, tdt, init=None):
    H = (grid.R + 1) // 2
    z = lambda *s: torch.zeros(s, device=DEV, dtype=tdt)
    out = dict(b=z(grid.m), A=z(H * grid.m), cnt=z(grid.m), res=z(grid.m), stats=torch.zeros(2, device=DEV, dtype=torch.float64))
    if init is not None:
        for k, v in out.items():
            v.copy_(torch.as_tensor(init[k]).to(v))
    return out


def _set(buf, u):
    return (buf["b"], buf["A"], buf["cnt"], buf["stats"], u, buf["res"])


def _compare(got, ref, tol, keys, label):
    for k in keys:
        r = np.asarray(ref[k], dtype=np.float64)
        e = float(np.abs(got[k].double().cpu().numpy() - r).max())
        bound = 10 * tol * float(np.abs(r).max())
        print(f"{label} {k}: max err {e:.3e}  bound {bound:.3e}")
        assert e <= bound, (label, k, e, bound)


def _site_deviation(sites, ref):
    """ytilde: largest error over max |ytilde|; e, tau, log Z, log Z_y: largest error relative to the reference value itself (where it
    is finite and not 0)."""
    got = {k: t.double().cpu().numpy() for k, t in zip(SITE_KEYS, sites)}
    out = dict(ytilde=float(np.abs(got["ytilde"] - ref["ytilde"]).max() / np.abs(ref["ytilde"]).max()))
    for k in ("e", "tau", "log_z", "log_zy"):
        nz = np.isfinite(ref[k]) & (ref[k] != 0)
        out[k] = float((np.abs(got[k] - ref[k])[nz] / np.abs(ref[k][nz])).max())
    return {k: out[k] for k in SITE_KEYS}


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))


@pytest.mark.parametrize("name", list(KGRIDS))
def test_reference_split_of_the_kernel_case(name):
    """What the batch is meant to contain, on the reference alone."""
    c = _kernel_case(name)
    r, ok = c["ref"], c["ok"]
    assert list(np.nonzero(~ok)[0]) == [10] and r["err"] == 3
    assert list(np.nonzero(ok & ~r["entered_f"])[0]) == [3] and np.isnan(r["log_z"][3]) and np.isnan(r["log_zy"][3])
    assert list(np.nonzero(r["skipped"])[0]) == [0] and r["tau"][0] == 0.0 and np.isfinite(r["log_z"][0])     # rho = 0: f enters, g is skipped
    ent = r["entered_g"]
    assert (r["tau"][ent] >= 1e4 * href.OMEGA_MIN).all() and np.isfinite(r["log_z"][ent]).all() and int(ent.sum()) == N - 3
    assert c["pvar"][5] == 0.0 and c["pvar2"][6] == 0.0 and ent[5] and ent[6] and ent[1] and r["log_zy"][1] < -150.0
    print(f"{name}: tau of the entering sites {r['tau'][ent].min():.2e} .. {r['tau'][ent].max():.3f}, e {r['e'][ok].min():.3f} .. {r['e'][ok].max():.3f}")


def _launch(c, tdt, f, g, err, mean=None):
    from online_gp_amd import grid_ops

    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    X, y, wa, noise, pvar, pvar2, u, u2 = (mk(c[k]) for k in ("X", "y", "wa", "noise", "pvar", "pvar2", "u", "u2"))
    return grid_ops.scatter_stats_hetero(c["grid"], X, y, pvar, pvar2, KS2, G0, wa, wa, noise, _set(f, u), _set(g, u2), err, mean_out=mean)


@pytest.mark.parametrize("tdt,tol", DTYPES)
@pytest.mark.parametrize("name", list(KGRIDS))
def test_kernel_matches_the_dense_reference(name, tdt, tol):
    from online_gp_amd import grid_ops

    test_reference_split_of_the_kernel_case(name)
    c = _kernel_case(name)
    grid, ref = c["grid"], c["ref"]
    rf, rg = dict(ref["f"], A=ref["f"]["A_half"], mean_out=ref["mean_out"]), dict(ref["g"], A=ref["g"]["A_half"])
    # from zero
    f, g, err = _buffers(grid, tdt), _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    mean = torch.full((N,), float("nan"), device=DEV, dtype=tdt)
    sites = _launch(c, tdt, f, g, err, mean)
    assert all(s.dtype == tdt for s in sites[:3]) and sites[3].dtype == torch.float64 and sites[4].dtype == torch.float64
    dev = _site_deviation(sites, ref)
    bound = FP64_SITE if tdt == torch.float64 else {k: 3.0 * v for k, v in FP32_SITE_DEV.items()}
    print(f"{name} {tdt} sites: " + "  ".join(f"{k} {dev[k]:.3e} (bound {bound[k]:.1e})" for k in dev))
    _compare(dict(f, mean_out=mean), rf, tol, KEYS + ("mean_out",), f"{name} f zero-init")
    _compare(g, rg, tol, KEYS, f"{name} g zero-init")
    e, yt, tau, lz, lzy = (s.double().cpu().numpy() for s in sites)
    assert np.array_equal(tau == 0.0, ref["tau"] == 0.0)             # whose noise site is skipped (0), dropped (3, 10): exactly the reference's
    assert np.array_equal(np.isnan(lz), np.isnan(ref["log_z"])) and np.array_equal(np.isnan(lzy), np.isnan(ref["log_zy"]))
    assert [e[10], yt[10], tau[10], lz[10], lzy[10]] == [0.0] * 5      # outside the grid: zeros
    assert int(err.item()) == ref["err"] == 1 + 2 * 1                # bit 0 | one point dropped, counted once; a skipped point is not flagged
    for k in dev:
        assert dev[k] <= bound[k], (name, k, dev[k], bound[k])
    # on top of non-zero buffers: every statistic of both models is added, none assigned; the sites do not depend on what the buffers hold
    rng = np.random.default_rng(5)
    init = [{k: 0.5 * float(np.abs(r[k]).max()) * rng.standard_normal(np.shape(r[k])) for k in KEYS} for r in (rf, rg)]
    f2, g2 = _buffers(grid, tdt, init[0]), _buffers(grid, tdt, init[1])
    start = [{k: v.double().cpu().numpy().copy() for k, v in b.items()} for b in (f2, g2)]
    err.zero_()
    sites2 = _launch(c, tdt, f2, g2, err)
    _compare(f2, {k: start[0][k] + rf[k] for k in KEYS}, tol, KEYS, f"{name} f on top")
    _compare(g2, {k: start[1][k] + rg[k] for k in KEYS}, tol, KEYS, f"{name} g on top")
    assert all(_same(a, b) for a, b in zip(sites, sites2))


@pytest.mark.parametrize("tdt,tol", DTYPES)
@pytest.mark.parametrize("name", list(KGRIDS))
def test_the_launch_is_a_plain_absorb_of_each_model(name, tdt, tol):
    """Composition.  The f statistics equal a plain half-stencil absorb of y at noise noise_p e_p (weights wa / e, wb / e), e the
    multiplier the launch reports; the g statistics equal the sites of wiski_hetero_sites at the reference's (mu_g, rho) absorbed
    plainly as ytilde - g0 at noise 1 / tau.  Both within the scatter bound."""
    from online_gp_amd import grid_ops

    c = _kernel_case(name)
    grid, ref = c["grid"], c["ref"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    f, g, err = _buffers(grid, tdt), _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    e, yt, tau, lz, lzy = _launch(c, tdt, f, g, err)
    X, y, wa, noise, u, u2 = (mk(c[k]) for k in ("X", "y", "wa", "noise", "u", "u2"))
    inn = torch.isfinite(lzy) & (e > 0)
    zero, one = torch.zeros_like(e), torch.ones_like(e)
    om = torch.where(inn, 1.0 / torch.where(inn, e, one), zero)
    pf, e2 = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    grid_ops.scatter_stats_cnt(grid, X, torch.where(inn, y, zero), wa * om, wa * om, torch.where(inn, noise * e, one), pf["b"], pf["A"], True, pf["cnt"],
                               pf["stats"], e2, u=u, res=pf["res"])
    _compare(f, {k: v.double().cpu().numpy() for k, v in pf.items()}, tol, KEYS, f"{name} {tdt} f against the plain absorb")
    assert int(e2.item()) == int(err.item()) == 3
    ok = c["ok"] & ref["entered_f"]
    W_u2 = href.ir.dense_rows(grid, torch.as_tensor(c["X"])).numpy() @ c["u2"]
    ps = href.point_sites(c["y"], ref["mean_out"], c["pvar"], W_u2, c["pvar2"], c["noise"], KS2, G0)
    rho = np.where(ok, ps["rho"], -1.0)                               # (an invalid datum where nothing entered: the site is skipped)
    s_yt, s_tau, _ = grid_ops.hetero_sites(mk(G0 + W_u2), mk(c["pvar2"]), mk(rho), one)
    pg, e3 = _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    ent = s_tau > 0
    grid_ops.scatter_stats_cnt(grid, X, torch.where(ent, s_yt - G0, zero), s_tau, s_tau, torch.where(ent, 1.0 / torch.where(ent, s_tau, one), one), pg["b"], pg["A"],
                               True, pg["cnt"], pg["stats"], e3, u=u2, res=pg["res"])
    _compare(g, {k: v.double().cpu().numpy() for k, v in pg.items()}, tol, KEYS, f"{name} {tdt} g against sites + plain absorb")


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64])
@pytest.mark.parametrize("level", [100.0, -100.0])
def test_a_multiplier_beyond_the_working_precision_skips_the_point(level, tdt):
    """u_g = +-100 on every node (rows sum to one: mu_g = +-100): e = exp(mu_g) and 1 / e are finite doubles, and one of them is beyond
    fp32.  In fp32 such a point would enter at weight 0 or inf while e_out says otherwise: it is skipped for both models instead
    (both log Z = NaN, nothing anywhere, no flag).  In fp64 the same points enter."""
    from online_gp_amd import grid_ops

    grid = grid_ops.GridSpec([[-1.0, 1.0]], [8])
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    X, y, one = mk([[-0.5], [0.55], [0.1]]), mk([0.3, -0.2, 0.1]), mk([1.0, 1.0, 1.0])
    f, g, err = _buffers(grid, tdt), _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    e, yt, tau, lz, lzy = grid_ops.scatter_stats_hetero(grid, X, y, one * 0.5, one * 0.0, 1.0, 0.0, one, one, one, _set(f, torch.zeros(grid.m, device=DEV, dtype=tdt)),
                                                      _set(g, torch.full((grid.m,), level, device=DEV, dtype=tdt)), err)
    assert int(err.item()) == 0
    if tdt == torch.float64:
        assert bool(torch.isfinite(lzy).all()) and bool(torch.isfinite(e).all()) and bool((e > 0).all()) and float(f["cnt"].abs().max()) > 0
        return
    assert bool(torch.isnan(lzy).all()) and bool(torch.isnan(lz).all()) and float(tau.abs().max()) == 0.0
    assert bool((e == float("inf")).all()) if level > 0 else float(e.max()) < 1e-37
    assert all(float(v.abs().max()) == 0.0 for b in (f, g) for v in b.values())


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64])
def test_absorb_refuses_the_hetero_group_with_what_the_kernel_does_not_do(tdt):
    """Through the full argument record plus the hetero group (wiski_absorb_hetero): every combination the contract refuses is
    WISKI_E_BADARG before any launch -- every buffer of both models untouched -- while the record without the offending field runs
    and equals grid_ops.scatter_stats_hetero; res, res2 and mean_out are optional; n = 0 does nothing."""
    from online_gp_amd import _hip, grid_ops

    c = _kernel_case("d3")
    grid = c["grid"]
    mk = lambda a: torch.as_tensor(a, device=DEV, dtype=tdt)
    X, y, wa, noise, pvar, pvar2, u, u2 = (mk(c[k]) for k in ("X", "y", "wa", "noise", "pvar", "pvar2", "u", "u2"))
    f, g, err = _buffers(grid, tdt), _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    nan = lambda dt=tdt: torch.full((N,), float("nan"), device=DEV, dtype=dt)
    mean, e, yt, tau, logz, logzy = nan(), nan(), nan(), nan(), nan(torch.float64), nan(torch.float64)
    full = torch.zeros((grid.R, grid.m), device=DEV, dtype=tdt)
    guard = torch.tensor([7], device=DEV, dtype=torch.int64)
    z1 = torch.full((2,), 0x01010101, device=DEV, dtype=torch.int32)
    bin_ws = torch.zeros(1 << 16, device=DEV, dtype=torch.uint8)
    p = lambda a: None if a is None else a.data_ptr()
    stream = _hip.stream_ptr(torch.device("cuda", torch.cuda.current_device()))
    G = dict(pvar=pvar, pvar2=pvar2, sigma2=KS2, g0=G0, b2=g["b"], A2=g["A"], cnt2=g["cnt"], u2=u2, res2=g["res"], stats2=g["stats"], e=e, yt=yt, tau=tau,
             logz=logz, logzy=logzy)

    def call(n=N, y_=y, **kw):
        a = _hip.wiski_absorb_args(d_x=p(X), d_y=p(y_), d_wa=p(wa), d_wb=p(wa), d_noise=p(noise), n=n, d_b=p(f["b"]), d_A=p(f["A"]), half=1, channels=0,
                                   d_cnt=p(f["cnt"]), d_stats=p(f["stats"]), d_err=p(err), d_u=p(u), d_res=p(f["res"]), d_mean_out=p(mean), nout=1)
        h = dict(G)
        for k, v in kw.items():
            if k in h:
                h[k] = v
            else:
                setattr(a, k, v)
        return _hip.fn("wiski_absorb_hetero", tdt)(grid.ref, ctypes.byref(a), p(h["pvar"]), p(h["pvar2"]), h["sigma2"], h["g0"], p(h["b2"]), p(h["A2"]),
                                                   p(h["cnt2"]), p(h["u2"]), p(h["res2"]), p(h["stats2"]), p(h["e"]), p(h["yt"]), p(h["tau"]), p(h["logz"]),
                                                   p(h["logzy"]), stream)

    inf, nanf = float("inf"), float("nan")
    refused = [("no u", call(d_u=None, d_res=None, d_mean_out=None)), ("full stencil", call(half=0, d_A=p(full))), ("no A", call(d_A=None)),
               ("no cnt", call(d_cnt=None)), ("nout = 2", call(nout=2, d_mean_out=None)), ("channels", call(channels=4)),
               ("guard", call(d_guard=p(guard), guard_expect=7)), ("zero region", call(z1=p(z1), n1_bytes=8)), ("shard", call(g_lo=0, g_hi=3)),
               ("owner workspace", call(d_bin=p(bin_ws), bin_bytes=bin_ws.numel())), ("sigma2 = 0", call(sigma2=0.0)), ("sigma2 < 0", call(sigma2=-1.0)),
               ("sigma2 = inf", call(sigma2=inf)), ("sigma2 = nan", call(sigma2=nanf)), ("g0 = inf", call(g0=inf)), ("g0 = nan", call(g0=nanf)),
               ("no y", call(y_=None)), ("no pvar", call(pvar=None)), ("no pvar2", call(pvar2=None)), ("no b2", call(b2=None)), ("no A2", call(A2=None)),
               ("no cnt2", call(cnt2=None)), ("no u2", call(u2=None)), ("no stats2", call(stats2=None)), ("no e_out", call(e=None)),
               ("no ytilde_out", call(yt=None)), ("no omega_out", call(tau=None)), ("no logz_out", call(logz=None)), ("no logzy_out", call(logzy=None))]
    torch.cuda.synchronize()
    assert [(what, rc) for what, rc in refused if rc != -1] == []
    assert call(n=0) == 0 and call(n=0, d_u=None, d_cnt=None, pvar=None, b2=None) == 0     # n = 0 does nothing, whatever the other fields hold
    torch.cuda.synchronize()
    assert all(float(v.abs().max()) == 0.0 for b in (f, g) for v in b.values()) and float(full.abs().max()) == 0.0 and int(err.item()) == 0
    assert all(bool(torch.isnan(a).all()) for a in (mean, e, yt, tau, logz, logzy)) and bool((z1 == 0x01010101).all())
    assert call() == 0
    wf, wg, e2 = _buffers(grid, tdt), _buffers(grid, tdt), grid_ops.new_err_flag(DEV)
    sites = _launch(c, tdt, wf, wg, e2)
    tol = dict(DTYPES)[tdt]
    _compare(f, {k: v.double().cpu().numpy() for k, v in wf.items()}, tol, KEYS, "record f")
    _compare(g, {k: v.double().cpu().numpy() for k, v in wg.items()}, tol, KEYS, "record g")
    assert all(_same(a, b) for a, b in zip(sites, (e, yt, tau, logz, logzy))) and int(err.item()) == int(e2.item()) == 3
    assert call(d_res=None, res2=None, d_mean_out=None) == 0         # the residuals and the mean are optional
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------- the model
REGIMES = {"dense-1d": ([[0.0, 1.0]], [40]), "dense-2d": ([[-1.0, 1.0], [-1.0, 1.0]], [24, 24]), "matrix-free-3d": ([[-1.0, 1.0]] * 3, [14, 14, 14])}
N0, Q, NB = 40, 37, 4
M_G0 = -0.5
ELL_G, OS_G = 0.6, 2.0


def _mf(X):
    return np.sin(3.0 * X[:, 0]) + (0.5 * np.cos(2.0 * X[:, 1]) if X.shape[1] > 1 else 0.0)


def _mstream(regime, seed=9):
    """40 points with values at known noise, then 4 batches of 37 whose noise standard deviation grows with x_0; 50 queries."""
    gb, gs = REGIMES[regime]
    d = len(gs)
    rng = np.random.default_rng(seed + d)
    n = N0 + NB * Q
    lo, hi = np.array(gb)[:, 0], np.array(gb)[:, 1]
    U = lambda k: lo + (hi - lo) * rng.uniform(0.05, 0.95, (k, d))
    X = U(n)
    sd = 0.05 + 0.4 * ((X[:, 0] - lo[0]) / (hi[0] - lo[0])) ** 2
    y = _mf(X) + sd * rng.standard_normal(n)
    noise = rng.uniform(0.5, 2.0, n)
    return X, y, noise, U(50)


def _t(a, dtype):
    return torch.as_tensor(a, device=DEV, dtype=dtype)


def _noise_kernel(d):
    from online_gp_amd.kernels import RBFKernel, ScaleKernel

    k = ScaleKernel(RBFKernel(ard_num_dims=d))
    k.base_kernel.lengthscale = ELL_G
    k.outputscale = OS_G
    return k


def _model(regime, dtype, nb0=N0, **kw):
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    gb, gs = REGIMES[regime]
    X, y, noise, _ = _mstream(regime)
    return FixedNoiseOnlineSKIGP(_t(X[:nb0], dtype), _t(y[:nb0], dtype)[:, None], _t(noise[:nb0], dtype)[:, None], grid_bounds=torch.tensor(gb), grid_size=gs,
                                 learn_additional_noise=True, heteroscedastic=True, noise_kernel=_noise_kernel(len(gs)), log_noise_mean=M_G0, **kw)


def _hyp(m):
    k = m.covar_module.base_kernel
    return (tuple(float(v) for v in k.base_kernel.lengthscale.detach().cpu().reshape(-1)), float(k.outputscale.detach()), float(m.likelihood.second_noise.detach()))


_refs = {}


def _reference_stream(regime, hyp, gamma=None):
    """The stream through two fp64 oracles: before batch k the oracle of f holds the initial points and the batches so far at their
    effective noise noise_p e_p (aged by 1 / gamma per batch under forgetting), the oracle of g the noise sites so far as
    (ytilde - g0, 1 / tau); their predictive moments at the batch give the batch's sites (hetero_reference.point_sites).  Per batch:
    the sites and both posteriors at the queries."""
    key = (regime, hyp, gamma)
    if key in _refs:
        return _refs[key]
    gb, gs = REGIMES[regime]
    X, y, noise, Xs = _mstream(regime)
    ell, s, s2 = hyp
    Of, Og = dataspace.DataSpaceGP(gb, gs, "rbf", ell, s, s2), dataspace.DataSpaceGP(gb, gs, "rbf", ELL_G, OS_G, 1.0)
    Xf, yf, ef = X[:N0], y[:N0], noise[:N0].copy()
    Xg, yg, eg = np.zeros((0, len(gs))), np.zeros(0), np.zeros(0)
    steps = []
    for k in range(NB):
        sl = slice(N0 + k * Q, N0 + (k + 1) * Q)
        if gamma is not None:
            ef, eg = ef / gamma, eg / gamma
        Of.fit(Xf, yf, ef)
        mf, vf = Of.predict(X[sl])
        if len(yg):
            Og.fit(Xg, yg, eg)
            mg, vg = Og.predict(X[sl])
        else:
            mg, vg = np.zeros(Q), np.diag(Og.cross(X[sl], X[sl])).copy()
        ps = href.point_sites(y[sl], mf, vf, mg, vg, noise[sl], s2, M_G0)
        assert ps["enters"].all() and not ps["skipped"].any()
        Xf, yf, ef = np.concatenate([Xf, X[sl]]), np.concatenate([yf, y[sl]]), np.concatenate([ef, noise[sl] * ps["e"]])
        Xg, yg, eg = np.concatenate([Xg, X[sl]]), np.concatenate([yg, ps["ytilde"] - M_G0]), np.concatenate([eg, 1.0 / ps["tau"]])
        Of.fit(Xf, yf, ef)
        Og.fit(Xg, yg, eg)
        mo, vo = Of.predict(Xs)
        go, wo = Og.predict(Xs)
        steps.append(dict(sites=ps, mean=mo, var=vo, gmean=go + M_G0, gvar=wo, n=len(yf), ng=len(yg)))
    _refs[key] = steps
    return steps


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _check_against(m, step, Xs, dtype, label):
    e, yt, tau, lz, lzy = (a.double().cpu().numpy() for a in m.last_hetero_sites)
    st = step["sites"]
    errs = dict(e=_rel(e, st["e"]), ytilde=_rel(yt, st["ytilde"]), tau=_rel(tau, st["tau"]), log_z=_rel(lz, st["log_z"]), log_zy=_rel(lzy, st["log_zy"]))
    print(f"{label} {dtype} sites: " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f"  (bound {RTOL[dtype]:.0e})")
    assert max(errs.values()) <= RTOL[dtype] and m.num_data == step["n"] and m.noise_model.num_data == step["ng"]
    mvn = m(_t(Xs, dtype))
    mean, var = mvn.mean.detach().double().cpu().numpy(), mvn.variance.detach().double().cpu().numpy()
    gm, gv = (a.detach().double().cpu().numpy() for a in m.noise_posterior(_t(Xs, dtype)))
    errs = dict(mean=_rel(mean, step["mean"]), var=_rel(var, step["var"]), g_mean=_rel(gm, step["gmean"]), g_var=_rel(gv, step["gvar"]))
    print(f"{label} {dtype} posteriors: " + "  ".join(f"{k} {v:.3e}" for k, v in errs.items()) + f"  (bound {RTOL[dtype]:.0e})")
    assert max(errs.values()) <= RTOL[dtype]


def _batch(regime, k, dtype):
    X, y, noise, _ = _mstream(regime)
    sl = slice(N0 + k * Q, N0 + (k + 1) * Q)
    return _t(X[sl], dtype), _t(y[sl], dtype), _t(noise[sl], dtype)


def _check_regime(regime, dtype, **kw):
    m = _model(regime, dtype, **kw).eval()
    assert m.last_hetero_sites is None and m.noise_model.num_data == 0 and m.noise_model._grid is m._grid     # the initial data is absorbed plainly
    steps = _reference_stream(regime, _hyp(m), kw.get("forgetting_factor"))
    Xs = _mstream(regime)[3]
    for k, step in enumerate(steps):
        m.condition_on_observations(*_batch(regime, k, dtype), inplace=True)
        assert all(a.shape == (Q,) and a.is_cuda for a in m.last_hetero_sites)
        _check_against(m, step, Xs, dtype, f"{regime} batch {k}")
    return m


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("regime", ["dense-1d", "dense-2d"])
def test_dense_regime_matches_the_oracles_at_the_effective_noises(regime, dtype):
    _check_regime(regime, dtype)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_matrix_free_regime_matches_the_oracles_at_the_effective_noises(dtype):
    from online_gp_amd import settings

    assert 14 ** 3 > settings.max_cholesky_size.value()
    with settings.spectral_factor(False), settings.cg_tolerance(1e-10 if dtype == torch.float64 else 1e-6):
        m = _check_regime("matrix-free-3d", dtype)
        assert m._mean_state is not None and m.noise_model._mean_state is not None


def test_functional_form_equals_the_inplace_form_and_leaves_the_parent_alone():
    dtype, regime = torch.float64, "dense-2d"
    a, b = _model(regime, dtype).eval(), _model(regime, dtype).eval()
    Xs = _t(_mstream(regime)[3], dtype)
    for k in range(2):
        before = [t.clone() for t in b.stats_buffers() + b.noise_model.stats_buffers()]
        a.condition_on_observations(*_batch(regime, k, dtype), inplace=True)
        child = b.condition_on_observations(*_batch(regime, k, dtype))
        assert all(torch.equal(x, y) for x, y in zip(before, b.stats_buffers() + b.noise_model.stats_buffers()))     # the parent, bit for bit
        assert child.noise_model is not b.noise_model and child.num_data == a.num_data and child.noise_model.num_data == a.noise_model.num_data
        for x, y in zip(a.last_hetero_sites, child.last_hetero_sites):
            assert _rel(y.double().cpu().numpy(), x.double().cpu().numpy()) <= 1e-9
        for fa, fc in ((a.predictive, child.predictive), (a.noise_posterior, child.noise_posterior)):
            for x, y in zip(fa(Xs), fc(Xs)):
                assert _rel(y.double().cpu().numpy(), x.double().cpu().numpy()) <= 1e-8
        b = child


def test_forgetting_ages_both_models():
    _check_regime("dense-1d", torch.float64, forgetting_factor=0.9)


def test_forget_and_regrid_act_on_both_models():
    """Stream one model, then forget_ and regrid_ it.  A model BUILT on the regridded grid, streamed the same batches and decayed
    alike, holds the same statistics of both models and agrees with it: regrid_ is an index shift and forget_ a scaling, of f and of g."""
    from online_gp_amd.kernels import GridInterpolationKernel, RBFKernel, ScaleKernel

    dtype, regime = torch.float64, "dense-2d"
    gb, gs = REGIMES[regime]
    m = _model(regime, dtype).eval()
    for k in range(2):
        m.condition_on_observations(*_batch(regime, k, dtype), inplace=True)
    Xs = _t(_mstream(regime)[3], dtype)
    pf0, pg0 = m.predictive(Xs), m.noise_posterior(Xs)
    s_f, s_g = m._kernel_cache["_stats"].clone(), m.noise_model._kernel_cache["_stats"].clone()
    m.forget_(0.8)
    assert torch.allclose(m._kernel_cache["_stats"][0, 0], 0.8 * s_f[0, 0], rtol=1e-12)
    assert torch.allclose(m.noise_model._kernel_cache["_stats"][0, 0], 0.8 * s_g[0, 0], rtol=1e-12)
    pf1, pg1 = m.predictive(Xs), m.noise_posterior(Xs)
    m.regrid_(2, 1)
    assert m.noise_model._grid is m._grid and m.noise_model.covar_module.grid_spec is m._grid and list(m._grid.g) == [gs[0] + 3, gs[1] + 3]
    assert m.noise_model._kernel_cache["WtW"].grid is m._grid and m._kernel_cache["WtW"].grid is m._grid     # one grid object, operators included
    assert m.noise_model.last_regrid_dropped_mass == 0.0
    pf2, pg2 = m.predictive(Xs), m.noise_posterior(Xs)
    for x, y in zip(pf1 + pg1, pf2 + pg2):                              # the regrid moves neither posterior
        assert _rel(y.double().cpu().numpy(), x.double().cpu().numpy()) <= 1e-7
    assert _rel(pf1[1].cpu().numpy(), pf0[1].cpu().numpy()) > 1e-3 and _rel(pg1[1].cpu().numpy(), pg0[1].cpu().numpy()) > 1e-3     # the decay moves both
    kern = GridInterpolationKernel(base_kernel=ScaleKernel(RBFKernel(ard_num_dims=2)), grid_size=8, num_dims=2, grid_bounds=gb)
    kern.set_grid_spec(m._grid)
    fresh = _model(regime, dtype, covar_module=kern).eval()
    assert list(fresh._grid.g) == list(m._grid.g)
    for k in range(2):
        fresh.condition_on_observations(*_batch(regime, k, dtype), inplace=True)
    fresh.forget_(0.8)
    for x, y in zip(pf2 + pg2, fresh.predictive(Xs) + fresh.noise_posterior(Xs)):
        assert _rel(y.double().cpu().numpy(), x.double().cpu().numpy()) <= 1e-6
    for x, y in zip(m.stats_buffers() + m.noise_model.stats_buffers(), fresh.stats_buffers() + fresh.noise_model.stats_buffers()):
        assert x.shape == y.shape and float((x.double() - y.double()).abs().max()) <= 1e-6 * max(1.0, float(x.double().abs().max()))


def test_set_train_data_rebuilds_both_models():
    dtype, regime = torch.float64, "dense-1d"
    m = _model(regime, dtype).eval()
    m.condition_on_observations(*_batch(regime, 0, dtype), inplace=True)
    assert m.noise_model.num_data == Q
    X, y, noise, _ = _mstream(regime)
    m.set_train_data(_t(X[:N0], dtype), _t(y[:N0], dtype)[:, None], _t(noise[:N0], dtype)[:, None])
    assert m.noise_model.num_data == 0 and m.num_data == N0 and all(float(t.abs().max()) == 0.0 for t in m.noise_model.stats_buffers())
    steps = _reference_stream(regime, _hyp(m))
    m.condition_on_observations(*_batch(regime, 0, dtype), inplace=True)
    _check_against(m, steps[0], _mstream(regime)[3], dtype, "after set_train_data")


def test_predictive_and_log_probability():
    dtype, regime = torch.float64, "dense-1d"
    m = _model(regime, dtype).eval()
    m.condition_on_observations(*_batch(regime, 0, dtype), inplace=True)
    Xs = _t(_mstream(regime)[3], dtype)
    gm, gv = m.noise_posterior(Xs)
    s2 = _hyp(m)[2]
    nz = torch.full((50,), 1.5, device=DEV, dtype=dtype)
    assert torch.allclose(m.predict_noise(Xs), s2 * torch.exp(gm + 0.5 * gv), rtol=1e-12) and torch.allclose(m.predict_noise(Xs, nz), 1.5 * m.predict_noise(Xs), rtol=1e-12)
    mvn = m(Xs)
    mean, var = m.predictive(Xs, nz)
    assert torch.allclose(mean, mvn.mean, rtol=1e-12) and torch.allclose(var, mvn.variance + m.predict_noise(Xs, nz), rtol=1e-12)
    Y = mean + 0.3
    lp = m.hetero_log_probability(Xs, Y, nz)
    assert torch.allclose(lp, -0.5 * torch.log(2 * np.pi * var) - 0.5 * 0.09 / var, rtol=1e-12)
    # what the launch reports as log Z_y of a batch is this, for the batch about to be absorbed
    Xb, yb, nb = _batch(regime, 1, dtype)
    lp = m.hetero_log_probability(Xb, yb, nb)
    m.condition_on_observations(Xb, yb, nb, inplace=True)
    assert _rel(m.last_hetero_sites[4].cpu().numpy(), lp.cpu().numpy()) <= 1e-8


def test_default_model_never_enters_the_hetero_path(monkeypatch):
    from online_gp_amd import grid_ops
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    def boom(*a, **k):
        raise AssertionError("the heteroscedastic launch on a default model")

    monkeypatch.setattr(grid_ops, "scatter_stats_hetero", boom)
    gb, gs = REGIMES["dense-1d"]
    X, y, noise, _ = _mstream("dense-1d")
    m = FixedNoiseOnlineSKIGP(_t(X[:N0], torch.float64), _t(y[:N0], torch.float64)[:, None], _t(noise[:N0], torch.float64)[:, None], grid_bounds=torch.tensor(gb),
                              grid_size=gs).eval()
    assert m.noise_model is None
    m.condition_on_observations(*_batch("dense-1d", 0, torch.float64), inplace=True)
    with pytest.raises(RuntimeError):
        m.noise_posterior(_t(X[:3], torch.float64))


def test_refusals():
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    dtype, regime = torch.float64, "dense-2d"
    gb, gs = REGIMES[regime]
    X, y, noise, _ = _mstream(regime)
    base = dict(grid_bounds=torch.tensor(gb), grid_size=gs, heteroscedastic=True)
    args = (_t(X[:N0], dtype), _t(y[:N0], dtype)[:, None], _t(noise[:N0], dtype)[:, None])
    for kw in (dict(robust_c=2.0), dict(window=32), dict(trend="linear"), dict(input_var=0.01)):
        with pytest.raises(NotImplementedError):
            FixedNoiseOnlineSKIGP(*args, **base, **kw)
    with pytest.raises(NotImplementedError):
        FixedNoiseOnlineSKIGP(args[0], torch.cat([args[1], args[1]], 1), torch.cat([args[2], args[2]], 1), **base)
    with pytest.raises(ValueError):
        FixedNoiseOnlineSKIGP(*args, grid_bounds=torch.tensor(gb), grid_size=gs, log_noise_mean=1.0)
    m = _model(regime, dtype).eval()
    Xb, yb, nb = _batch(regime, 0, dtype)
    one = torch.ones_like(yb)
    for kw in (dict(lower=yb), dict(counts=one), dict(labels=one), dict(grad_Y=torch.zeros_like(Xb)), dict(input_var=0.01), dict(grad_lower=0.0)):
        with pytest.raises(NotImplementedError):
            m.condition_on_observations(Xb, yb, nb, inplace=True, **kw)
    with pytest.raises(NotImplementedError):
        m.condition_on_observations(Xb[None].expand(3, -1, -1), yb[None].expand(3, -1), inplace=False)
    with pytest.raises(NotImplementedError):
        m.get_fantasy_model(Xb[None].expand(3, -1, -1), yb[None].expand(3, -1))
    with pytest.raises(NotImplementedError):
        m.stream_step(Xb, yb[:, None])
    with pytest.raises(NotImplementedError):
        m.enter_stencil_shard(0, 2, lambda t, op: t)
    with pytest.raises(ValueError):
        m.condition_on_observations(Xb, None, inplace=True)
    assert m.num_data == N0 and m.noise_model.num_data == 0


def test_train_and_eval_reach_the_noise_model_and_its_kernel_is_no_parameter():
    m = _model("dense-1d", torch.float64)
    m.train()
    assert m.noise_model.training
    m.eval()
    assert not m.noise_model.training
    own = {id(p) for p in m.noise_model.covar_module.parameters()}         # (the likelihood object is shared, and unused by the noise model)
    assert own and not own & {id(p) for p in m.parameters()} and not any(k.startswith("noise_model") for k in m.state_dict())


def test_the_regression_wrapper_passes_the_feature_through():
    """OnlineSKIRegression(..., heteroscedastic=True, noise_kernel=, log_noise_mean=): update() absorbs heteroscedastically (it goes
    through condition_on_observations), predict() and evaluate() use the learned noise, fit() rebuilds both models; the default
    wrapper has no noise model."""
    from online_gp_amd.models import OnlineSKIRegression
    from online_gp_amd.models.stems import Identity

    dtype = torch.float64
    X, Y, _, _ = href.stream_data(5, n_batches=5, batch=32, held_out=8)
    Xt, Yt = _t(X, dtype).reshape(5, 32, 1) * 1.6 - 0.8, _t(Y, dtype).reshape(5, 32, 1)
    plain = OnlineSKIRegression(Identity(1), Xt[0], Yt[0], 1e-2, 24, 1.0)
    assert plain.gp.noise_model is None
    r = OnlineSKIRegression(Identity(1), Xt[0], Yt[0], 1e-2, 24, 1.0, heteroscedastic=True, noise_kernel=_noise_kernel(1), log_noise_mean=M_G0)
    assert r.gp.noise_model is not None and r.gp.log_noise_mean == M_G0 and r.gp.noise_model.num_data == 0
    for k in range(1, 4):
        r.update(Xt[k], Yt[k])
        assert r.gp.last_hetero_sites is not None and r.gp.num_data == 32 * (k + 1) and r.gp.noise_model.num_data == 32 * k
    mean, var = r.predict(Xt[4])
    pm, pv = r.gp.predictive(Xt[4])
    assert mean.shape == (32, 1) and torch.equal(mean[:, 0], pm) and torch.equal(var[:, 0], pv)
    latent = r(Xt[4]).variance.reshape(-1)
    assert torch.allclose(var[:, 0] - latent, r.gp.predict_noise(Xt[4]), rtol=1e-10) and float((var[:, 0] - latent).min()) > 0
    rmse, nll = r.evaluate(Xt[4], Yt[4])
    want = 0.5 * ((mean - Yt[4]) ** 2 / var + var.log() + np.log(2 * np.pi)).mean()
    assert abs(nll - float(want)) <= 1e-9 * abs(float(want)) and abs(rmse - float(((mean - Yt[4]) ** 2).mean().sqrt())) <= 1e-9
    r.fit(Xt[:2].reshape(-1, 1), Yt[:2].reshape(-1, 1), 1)
    assert r.gp.noise_model.num_data == 0 and r.gp.num_data == 64 and all(float(t.abs().max()) == 0.0 for t in r.gp.noise_model.stats_buffers())
    r.update(Xt[2], Yt[2])
    assert r.gp.noise_model.num_data == 32


# ------------------------------------------------------------------------------------------------------------------ the stream
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_the_stream_of_the_property_test_through_the_model(dtype):
    """The 1-D stream of tests/test_hetero_host.py through the model: the first batch builds it (absorbed plainly, at multiplier 1), the
    other nineteen are absorbed heteroscedastically.  Conditions (a) - (c) as there."""
    from online_gp_amd.kernels import RBFKernel, ScaleKernel
    from online_gp_amd.models import FixedNoiseOnlineSKIGP
    from test_hetero_host import STREAM_SEED

    S = href.STREAM
    X, Y, _, _ = href.stream_data(STREAM_SEED)

    def kern(ell, os_):
        k = ScaleKernel(RBFKernel(ard_num_dims=1))
        k.base_kernel.lengthscale, k.outputscale = ell, os_
        return k

    m = FixedNoiseOnlineSKIGP(_t(X[0], dtype)[:, None], _t(Y[0], dtype)[:, None], torch.ones(S["batch"], 1, device=DEV, dtype=dtype), covar_module=kern(S["ell_f"], S["os_f"]),
                              grid_bounds=torch.tensor(S["grid_bounds"]), grid_size=[S["grid_size"]], learn_additional_noise=True, heteroscedastic=True,
                              noise_kernel=kern(S["ell_g"], S["os_g"]), log_noise_mean=S["g0"]).eval()
    m.likelihood.second_noise = S["sigma2"]
    m.hyperparameters_changed()
    skipped = 0
    for xb, yb in zip(X[1:], Y[1:]):
        m.condition_on_observations(_t(xb, dtype)[:, None], _t(yb, dtype), inplace=True)
        skipped += int((m.last_hetero_sites[2] == 0).sum())

    def predictive(Xt):
        mean, var = m.predictive(_t(Xt, dtype)[:, None])
        return mean.double().cpu().numpy(), var.double().cpu().numpy()

    r = href.stream_report(predictive, STREAM_SEED)
    print(f"stream {dtype}: " + "  ".join(f"{k} {v:.4f}" for k, v in r.items()) + f"  skipped {skipped}")
    a, b = href.stream_conditions(r)
    assert a, r
    assert b, r
    assert skipped == 0 and m.num_data == X.size and m.noise_model.num_data == X.size - S["batch"]
