"""GPU: what each observation form does to the followers of the statistics -- the root pair, the noise-weight sum, num_data, the
carried residual, the spectral factor, the two-level block, parent and child of the functional route.  The five forms of
``condition_on_observations`` (plain, grad_Y, robust_c, lower / upper, window) share their host logic; the other suites check each
form's posterior, this one pins the follower list form by form, route by route.

Three set-ups, each built once per case and shared by the tests that look at it (``_dense`` / ``_free`` / ``_spectral`` return a
record of flags and figures; the tests only assert on it):

* dense: fp64, d = 2, 10 x 10 nodes on [-1.1, 1.1]^2, 300 seeded points and a batch of 12 -- the configuration of
  tests/test_dense_gpu.py::test_root_pair_is_dropped_when_the_stencil_is_rebuilt_or_all_reduced: with m = 100 a root pair exists and
  a batch of 12 <= m / 2 takes the rank-update branch.
* matrix-free: the fp64 12 x 12 configuration of tests/test_window_gpu.py::test_matrix_free_regime_is_the_gp_of_the_last_window_points
  (max_cholesky_size 64, no spectral factor): a mean state and its carried residual.
* spectral: d = 3, 14^3 nodes, the configuration of tests/test_grad_obs_gpu.py::test_spectral_factor_is_rebuilt_after_a_derivative_update,
  in which a posterior variance builds a spectral factor.

Vacuous by construction, and said here once: the matrix-free set-up switches the spectral factor off, so its "stale" flags have no
factor to look at (the spectral set-up is there for that, and asserts that a factor exists before every batch); the two-level block
belongs to fp32 d = 3 streams, so in these fp64 set-ups ``_two_level`` is absent throughout and "is None" holds trivially.

Flags and counters are compared exactly; figures that pass through atomics to a tolerance: L L^T against A within
1e-6 max(1, |A|max) (the bound of the test_dense_gpu.py test above), the noise-weight sum to 1e-12 relative (both sides are fp64 sums
of <= 312 positive terms), the posterior means of the two routes within RTOL = 1e-4 of test_robust_gpu.py (relative to max |mean|).
"""
import functools

import numpy as np
import pytest
import torch

from test_robust_gpu import RTOL
from test_window_gpu import W as FREE_W, _model as _free_model, _stream as _free_stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT = torch.float64
FORMS = ("plain", "grad", "robust", "interval", "window")
FOLLOW = ("plain", "robust", "interval")              # forms whose root pair and spectral factor follow the batch
ROUTES = ("inplace", "functional")
N0, Q, WIN, GAMMA = 300, 12, 64, 0.9
CASES = [(f, r, None) for f in FORMS for r in ROUTES] + [(f, r, GAMMA) for f in FORMS[:4] for r in ROUTES]     # (the window refuses forgetting)
IDS = [f"{f}-{r}-{'keep' if ff is None else 'forget'}" for f, r, ff in CASES]


def _t(a):
    return torch.as_tensor(a, device=DEV, dtype=DT)


def _kw(form, ff=None):
    kw = {} if ff is None else {"forgetting_factor": ff}
    if form == "robust":
        kw["robust_c"] = 2.0
    if form == "window":
        kw["window"] = WIN
    return kw


def _batch(form, X, y, noise, rng):
    """(args, kwargs) of condition_on_observations for one batch in the given form.  robust: two gross outliers; interval: two-sided,
    one-sided, an exact value and one point with nothing to say (which does not count in num_data)."""
    d = X.shape[1]
    if form == "grad":
        return (_t(X), _t(y), _t(noise)), {"grad_Y": _t(rng.standard_normal((X.shape[0], d)))}
    if form == "robust":
        y = y.copy()
        y[[1, 7]] += [25.0, -25.0]
    if form == "interval":
        lo, hi = y - 0.3, y + 0.3
        hi[2], lo[3] = np.inf, -np.inf
        lo[4] = hi[4] = y[4]
        lo[5], hi[5] = -np.inf, np.inf
        return (_t(X), None, _t(noise)), {"lower": _t(lo), "upper": _t(hi)}
    return (_t(X), _t(y), _t(noise)), {}


def _grown(form, q, d):
    """What num_data grows by: points; scalar observations for grad; entered + dropped for interval (one of the points of _batch has
    nothing to say).  (The window's count is its ring's.)"""
    return {"grad": q * (d + 1), "interval": q - 1}.get(form, q)


def _wsum_expected(form, model, w0, wq, ff):
    """The noise-weight sum after the batch, from the weights themselves (w0, wq: 1 / noise of the initial points and of the batch)."""
    if form == "grad":
        return float(model._kernel_cache["_cnt"].sum(dtype=torch.float64))
    if form == "window":
        return float(model._kernel_cache["_ring"].wa.sum(dtype=torch.float64))
    omega = {"robust": lambda: model.last_robust_weights, "interval": lambda: model.last_interval_sites[1]}.get(form, lambda: 1.0)()
    return float((1.0 if ff is None else ff) * w0.sum(dtype=torch.float64) + (wq * omega).sum(dtype=torch.float64))


def _sites(m):
    return m.last_robust_weights, m.last_interval_sites


# ------------------------------------------------------------------------------------------------------------------ dense
@functools.lru_cache(maxsize=None)
def _dense(form, route, ff):
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    g = torch.Generator(device="cpu").manual_seed(5)
    X = torch.rand(N0 + Q, 2, generator=g, dtype=DT) * 2 - 1
    noise = torch.rand(N0 + Q, generator=g, dtype=DT) * 1.5 + 0.5
    Xs = _t(torch.rand(8, 2, generator=g, dtype=DT) * 2 - 1)
    y = torch.sin(3 * X.sum(1)) + 0.05 * torch.randn(N0 + Q, generator=g, dtype=DT)
    X, y, noise = X.numpy(), y.numpy(), noise.numpy()
    model = FixedNoiseOnlineSKIGP(_t(X[:N0]), _t(y[:N0, None]), _t(noise[:N0, None]), grid_bounds=torch.tensor([[-1.1, 1.1]] * 2), grid_size=10,
                                  learn_additional_noise=True, **_kw(form, ff))
    op = model._kernel_cache["WtW"]
    L0 = op.root_decomposition().root.evaluate().clone()
    assert op.root is not None and op.inv_root is not None
    R0 = op.inv_root.clone()
    args, kw = _batch(form, X[N0:], y[N0:], noise[N0:], np.random.default_rng(3))
    rec = {"form": form, "d": 2}
    before = [t.clone() for t in model.stats_buffers()]
    n_before, wsum_before = model.num_data, model._wsum[0]
    if route == "functional":
        child_train = model.train().condition_on_observations(*args, **kw)
        child = model.eval().condition_on_observations(*args, **kw)
        rec.update(modes=(child_train.training, child.training),
                   parent_same=all(torch.equal(a, b) for a, b in zip(before, model.stats_buffers())),
                   parent_root_same=op.root is not None and torch.equal(op.root, L0) and torch.equal(op.inv_root, R0),
                   parent_counters_same=model.num_data == n_before and model._wsum[0] == wsum_before,
                   parent_sites=_sites(model))
        new = child
    else:
        assert model.eval().condition_on_observations(*args, inplace=True, **kw) is None
        new = model
    nop = new._kernel_cache["WtW"]
    rec.update(root=nop.root is not None, inv_root=nop.inv_root is not None, sites=_sites(new), num_data=new.num_data, n_before=n_before,
               wsum=new._wsum[0])
    w0 = 1.0 / _t(noise[:N0])
    rec["wsum_expected"] = _wsum_expected(form, new, w0, 1.0 / _t(noise[N0:]), ff)
    if nop.root is not None:
        A = nop.evaluate()
        rec.update(root_err=float(((nop.root @ nop.root.t()) - A).abs().max()), A_max=float(A.abs().max()))
    with torch.no_grad():
        rec["mean"] = new.eval()(Xs).mean.double().cpu().numpy()
    return rec


@pytest.mark.parametrize("form,route,ff", CASES, ids=IDS)
def test_root_pair_counters_and_sums(form, route, ff):
    r = _dense(form, route, ff)
    print({k: v for k, v in r.items() if k not in ("mean", "sites", "parent_sites")})
    # the root pair: followed with the effective weights, or dropped (by the decay before the batch, by grad / window always)
    if form in FOLLOW and ff is None:
        assert r["root"] and r["inv_root"]
        assert r["root_err"] < 1e-6 * max(1.0, r["A_max"])
    else:
        assert not r["root"] and not r["inv_root"]
    # counters and sums
    assert r["num_data"] == (WIN if form == "window" else r["n_before"] + _grown(form, Q, r["d"]))
    assert abs(r["wsum"] - r["wsum_expected"]) <= 1e-12 * r["wsum_expected"]
    # the sites land on the model that absorbed the batch
    assert (r["sites"][0] is not None) == (form == "robust") and (r["sites"][1] is not None) == (form == "interval")
    if form == "robust":
        assert r["sites"][0].shape == (Q,) and float(r["sites"][0].min()) < 1.0         # the outliers were down-weighted
    if form == "interval":
        assert int((r["sites"][1][1] > 0).sum()) == Q - 1
    if route == "functional":
        assert r["parent_same"] and r["parent_root_same"] and r["parent_counters_same"]
        assert r["modes"] == (True, False)                                               # the child is in the parent's mode
        assert r["parent_sites"] == (None, None)


@pytest.mark.parametrize("form,ff", [(f, ff) for f, r, ff in CASES if r == "inplace"], ids=[i for i, c in zip(IDS, CASES) if c[1] == "inplace"])
def test_both_routes_give_the_same_posterior_mean(form, ff):
    a, b = _dense(form, "inplace", ff)["mean"], _dense(form, "functional", ff)["mean"]
    dev = float(np.abs(a - b).max() / np.abs(a).max())
    print(f"{form} forgetting={ff}: in place vs functional mean {dev:.3e}  (bound {RTOL[DT]:.0e})")
    assert dev <= RTOL[DT]


# ------------------------------------------------------------------------------------------------------------ matrix-free
def _free_batch(form, X, y, noise, lo, hi):
    return _batch(form, X[lo:hi], y[lo:hi].copy(), noise[lo:hi], np.random.default_rng(4))


@functools.lru_cache(maxsize=None)
def _free(form, route):
    """64 points, a converged mean solve, then one batch of 16."""
    from online_gp_amd import settings

    X, y, noise, _ = _free_stream()
    kw = _kw(form)
    if form == "window":
        kw["window"] = FREE_W
    with settings.max_cholesky_size(64), settings.spectral_factor(False), settings.cg_tolerance(1e-10), torch.no_grad():
        m = _free_model(X[:64], y[:64], noise[:64], DT, [12, 12], **kw).eval()
        m.prediction_cache
        ms = m._mean_state
        rec = {"dense": m._use_dense(), "R_ok_before": ms is not None and ms["R_ok"]}
        args, bkw = _free_batch(form, X, y, noise, 64, 80)
        new = m.condition_on_observations(*args, inplace=route == "inplace", **bkw)
        if route == "inplace":
            rec["same_state"] = m._mean_state is ms
            new = m
        rec.update(R_ok=new._mean_state["R_ok"], parent_R_ok=m._mean_state["R_ok"], factors=len(new.__dict__.get("_spectral", {})),
                   two_level=new.__dict__.get("_two_level"), num_data=new.num_data)
    return rec


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("form", FORMS)
def test_carried_residual_in_place_and_on_the_child(form, route):
    r = _free(form, route)
    print(form, route, r)
    assert not r["dense"] and r["R_ok_before"]
    if route == "inplace":
        assert r["same_state"] and r["R_ok"] is True                 # every form's launch kept R = b - Z - A U exact
    else:
        assert r["R_ok"] is False and r["parent_R_ok"] is True       # the child's copy predates the batch; the parent's is untouched
    assert r["factors"] == 0 and r["two_level"] is None               # (vacuous here: see the module docstring)
    assert r["num_data"] == (FREE_W if form == "window" else 64 + _grown(form, 16, 2))


# --------------------------------------------------------------------------------------------------------------- spectral
@functools.lru_cache(maxsize=None)
def _spectral(form):
    from online_gp_amd import settings
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    d, g, n0 = 3, 14, 300
    rng = np.random.default_rng(11)
    X = rng.uniform(-1, 1, (n0 + Q, d))
    y = np.sin(2 * X.sum(1)) + 0.1 * rng.standard_normal(n0 + Q)
    noise = rng.uniform(0.5, 2.0, n0 + Q)
    Xs = rng.uniform(-1, 1, (50, d))
    with settings.cg_tolerance(1e-10), settings.spectral_max_rank(1024), torch.no_grad():
        m = FixedNoiseOnlineSKIGP(_t(X[:n0]), _t(y[:n0, None]), _t(noise[:n0, None]), grid_bounds=torch.tensor([[-1.1, 1.1]] * d), grid_size=g,
                                  learn_additional_noise=True, **_kw(form)).eval()
        m(_t(Xs)).variance
        fac = m.__dict__.get("_spectral", {}).get(0)
        rec = {"built": fac is not None and fac.ref is not None and not fac.stale}
        args, kw = _batch(form, X[n0:], y[n0:].copy(), noise[n0:], np.random.default_rng(6))
        m.condition_on_observations(*args, inplace=True, **kw)
        rec.update(stale=[f.stale for f in m.__dict__.get("_spectral", {}).values()], two_level=m.__dict__.get("_two_level"))
    return rec


@pytest.mark.parametrize("form", FORMS)
def test_spectral_factor_follows_or_is_marked_stale(form):
    r = _spectral(form)
    print(form, r)
    assert r["built"] and len(r["stale"]) == 1                       # not vacuous: a factor existed before the batch and is still there
    assert r["stale"] == [form not in FOLLOW]                         # grad / window: rebuilt from the stencil when next asked
    assert r["two_level"] is None                                     # (vacuous in fp64: see the module docstring)
