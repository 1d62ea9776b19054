"""No GPU: the site revisit in numpy fp64 -- the identity behind one launch, the fixed point of the sweeps, and what
the model refuses before it touches a device.

``revisit_reference.dense_revisit`` is what one launch adds.  It equals "absorb the old site negated, absorb the fresh site", each
assembled from ``interval_reference.dense_absorb``: a site (ytilde, omega) of a point at noise d is the exact value ytilde at noise
d / omega with the weights wa omega, wb omega.  The fixed point of the sweeps (``ep_stream``, the exact SKI GP in data space) does not
depend on how the stream was cut into batches: 1e-8 on the posterior mean after 15 sweeps.  On the SKI grid of 32 nodes the reference
alone reaches 5.9e-12 (128 censored points, one batch against eight) and 6.4e-14 (48 Poisson counts, one batch against four) at the
seeds used here; over seeds 0 - 5 the censored figure lies between 3e-12 and 3.8e-9."""
import ctypes
import os

import numpy as np
import pytest
import torch

import interval_reference as iref
import revisit_reference as rv
from oracle import dataspace, spec
from test_forgetting_host import G, GB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
S2 = 0.4


def _ring(n=24, seed=3):
    """A 2-D grid and a ring of n interval slots with plausible old sites (tau_old v in (0, 0.8)); slot 0: an exact value, 1: empty,
    2: omega_old = 0, 3: a Poisson slot, 4: outside the grid, 5: pvar = 0, 6: a cavity below CAVITY_MIN."""
    rng = np.random.default_rng(seed)
    g0, h, g = spec.make_grid(GB, G)
    grid = iref.Grid(g0, h, g)
    m = int(np.prod(g))
    X = rng.uniform(-0.9, 0.9, (n, 2))
    X[4] = [5.0, 0.0]
    noise = rng.uniform(0.5, 2.0, n)
    pvar = rng.uniform(0.1, 1.5, n)
    pvar[5] = 0.0
    tv = rng.uniform(0.05, 0.8, n)
    tv[2], tv[6] = 0.0, 1.0 - 1e-6
    u = rng.standard_normal(m)
    import interp_reference as ir

    mean = ir.dense_rows(grid, torch.as_tensor(X)).numpy() @ u
    omega = S2 * noise * tv / np.where(pvar > 0, pvar, 1.0)
    ytilde = mean + np.sqrt(pvar) * rng.uniform(-1, 1, n)
    lo = mean + rng.uniform(-2.0, 1.0, n)
    hi = np.where(rng.uniform(size=n) < 0.5, INF, lo + rng.uniform(0.1, 2.0, n))
    form = np.full(n, rv.INTERVAL)
    lo[0] = hi[0] = ytilde[0]
    omega[0] = 1.0
    form[1], form[3] = rv.EMPTY, rv.POISSON
    ring = dict(x=X, d0=lo, d1=hi, noise=noise, wa=1.0 / noise, wb=1.0 / noise, ytilde=ytilde, omega=omega, form=form)
    return grid, ring, pvar, u, mean


@pytest.mark.parametrize("damping", [1.0, 0.5])
def test_one_launch_is_the_old_site_negated_plus_the_new_site(damping):
    grid, ring, pvar, u, mean = _ring()
    r = rv.dense_revisit(grid, ring, rv.INTERVAL, pvar, S2, u, damping)
    t = r["touched"]
    assert set(np.nonzero(~t)[0]) == {0, 1, 3, 4, 5, 6} and list(np.nonzero(r["entered"])[0]) == [2]
    # the new sites, from the definitions: cavity, the form's own site function, damping in natural parameters
    dn = S2 * ring["noise"][t]
    tau, yo = ring["omega"][t] / dn, ring["ytilde"][t]
    p = 1.0 / pvar[t] - tau
    st = iref.sites(ring["d0"][t], ring["d1"][t], (mean[t] / pvar[t] - tau * yo) / p, 1.0 / p, dn)
    tau_n = (1 - damping) * tau + damping * st["omega"] / dn
    nu_n = (1 - damping) * tau * yo + damping * st["omega"] / dn * st["ytilde"]
    assert np.allclose(r["omega"][t], dn * tau_n, rtol=1e-13) and np.allclose(r["ytilde"][t], nu_n / tau_n, rtol=1e-12)
    assert np.array_equal(r["omega"][~t], ring["omega"][~t]) and np.array_equal(r["ytilde"][~t], ring["ytilde"][~t])
    if damping == 1.0:
        assert np.allclose(r["log_z"][t], st["log_z"], rtol=1e-13) and np.isnan(r["log_z"][~t]).all()

    # a site as an exact value at noise / omega with the weights wa omega, wb omega: interval_reference.dense_absorb's own pieces
    def as_values(yt, om):
        k = t & (om > 0)
        return iref.dense_absorb(grid, ring["x"][k], yt[k], yt[k], (ring["wa"] * om)[k], (ring["wb"] * om)[k], ring["noise"][k] / om[k], pvar[k], S2, u)

    old, new = as_values(ring["ytilde"], ring["omega"]), as_values(r["ytilde"], r["omega"])
    for k in ("A", "A_half", "b", "cnt", "res", "stats"):
        want = new[k] - old[k]
        assert np.abs(r[k] - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), k
    assert np.abs(r["A"]).max() > 0.01


def test_damping_zero_gives_zeros():
    grid, ring, pvar, u, _ = _ring()
    r = rv.dense_revisit(grid, ring, rv.INTERVAL, pvar, S2, u, 0.0)
    assert not r["touched"].any() and all(float(np.abs(r[k]).max()) == 0.0 for k in ("A", "A_half", "b", "cnt", "res", "stats", "change"))
    assert all(np.array_equal(r["ring"][k], ring[k]) for k in rv.RING_KEYS) and np.isnan(r["log_z"]).all()


TB, TG, TELL, TOSC, TS2 = [[-0.15, 1.15]], [32], [0.25], 1.0, 0.05     # the toy of DESIGN.md 3.20
TSEED = 4


def _toy(n, seed=TSEED):
    """sin 6x + x / 2 on [0, 1], noise variance 0.05; readings above 0.6 are censored, the others are exact values."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (n, 1))
    y = np.sin(6.0 * X[:, 0]) + 0.5 * X[:, 0] + np.sqrt(TS2) * rng.standard_normal(n)
    return X, np.where(y > 0.6, 0.6, y), np.where(y > 0.6, INF, y), np.linspace(0.02, 0.98, 50)[:, None]


def _oracle():
    return dataspace.DataSpaceGP(TB, TG, "rbf", TELL, TOSC, TS2)


def test_fixed_point_does_not_depend_on_the_batching_censored():
    X, lo, hi, Xs = _toy(128)
    one = rv.ep_stream(_oracle(), [(rv.INTERVAL, X, lo, hi)], 128, 15)
    eight = rv.ep_stream(_oracle(), [(rv.INTERVAL, X[a:a + 16], lo[a:a + 16], hi[a:a + 16]) for a in range(0, 128, 16)], 128, 15)
    adf = rv.ep_stream(_oracle(), [(rv.INTERVAL, X, lo, hi)], 128, 0)
    m1, m8, m0 = one.marginals(Xs)[0], eight.marginals(Xs)[0], adf.marginals(Xs)[0]
    e = float(np.abs(m1 - m8).max())
    print(f"censored, one batch against eight: {e:.3e}; changes {['%.1e' % c for c in one.changes]}; the sweeps move the mean by {np.abs(m1 - m0).max():.3f}")
    assert int(np.isinf(hi).sum()) >= 30 and np.abs(m1 - m0).max() > 0.05
    assert all(b <= a for a, b in zip(one.changes[1:], one.changes[2:])) and one.changes[-1] < 1e-6
    assert e <= 1e-8
    # exact values are never re-matched, and every point is in the posterior
    exact = lo == hi
    assert (one.ring["omega"][exact] == 1.0).all() and np.array_equal(one.ring["ytilde"][exact], lo[exact]) and one.num_data == 128


def test_fixed_point_does_not_depend_on_the_batching_counts():
    rng = np.random.default_rng(TSEED)
    X = rng.uniform(0.0, 1.0, (48, 1))
    y = rng.poisson(1.5 * np.exp(np.sin(6.0 * X[:, 0]) + 0.5 * X[:, 0] - 0.4)).astype(np.float64)
    t, Xs = np.full(48, 1.5), np.linspace(0.02, 0.98, 50)[:, None]
    one = rv.ep_stream(_oracle(), [(rv.POISSON, X, y, t)], 48, 15)
    four = rv.ep_stream(_oracle(), [(rv.POISSON, X[a:a + 12], y[a:a + 12], t[a:a + 12]) for a in range(0, 48, 12)], 48, 15)
    e = float(np.abs(one.marginals(Xs)[0] - four.marginals(Xs)[0]).max())
    print(f"counts, one batch against four: {e:.3e}; changes {['%.1e' % c for c in one.changes]}")
    assert one.changes[-1] < 1e-6 and e <= 1e-8


def test_an_evicted_site_stays_frozen():
    """A ring of 16 under three batches of 12: the 20 evicted points keep the sites they had when they left, the sweeps move the 16
    stored ones only."""
    X, lo, hi, Xs = _toy(36)
    S = rv.ep_stream(_oracle(), [(rv.INTERVAL, X[a:a + 12], lo[a:a + 12], hi[a:a + 12]) for a in range(0, 36, 12)], 16, 0)
    fy, feff = S.fy.copy(), S.feff.copy()
    assert S.fy.shape[0] == 20 and np.array_equal(S.ring["x"], X[20:]) and np.array_equal(S.fX, X[:20])
    for _ in range(5):
        S.sweep()
    assert np.array_equal(S.fy, fy) and np.array_equal(S.feff, feff) and S.changes[0] > 0.1


def test_constructor_refusals_need_no_device():
    from online_gp_amd.models import FixedNoiseOnlineSKIGP, OnlineSKIBotorchModel

    X, y = torch.rand(6, 1), torch.rand(6, 1)
    mk = lambda cls=FixedNoiseOnlineSKIGP, y_=y, **kw: cls(X, y_, torch.ones_like(y_), grid_bounds=torch.tensor([[-0.1, 1.1]]), grid_size=[16], **kw)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            mk(site_memory=bad)
    for kw in (dict(site_refine_sweeps=2), dict(site_refine_damping=0.5), dict(site_memory=8, site_refine_sweeps=-1),
               dict(site_memory=8, site_refine_damping=1.5)):
        with pytest.raises(ValueError):
            mk(**kw)
    for cls in (FixedNoiseOnlineSKIGP, OnlineSKIBotorchModel):
        for kw in (dict(forgetting_factor=0.9), dict(window=32), dict(robust_c=2.0), dict(trend="linear"), dict(heteroscedastic=True), dict(num_path_probes=4)):
            with pytest.raises(NotImplementedError, match="site_memory"):
                mk(cls, site_memory=8, **kw)
        with pytest.raises(NotImplementedError, match="site_memory"):
            mk(cls, torch.rand(6, 2), site_memory=8)                 # several outputs


def test_kernel_is_declared_and_listed_for_the_build():
    from online_gp_amd import _hip, grid_ops

    hdr = open(os.path.join(ROOT, "include", "wiski.h")).read()
    for name in ("wiski_absorb_revisit_f32", "wiski_absorb_revisit_f64", "wiski_site_ring"):
        assert name in hdr
    assert "scatter_revisit.h" in _hip._HEADERS and os.path.exists(os.path.join(ROOT, "online_gp_amd", "csrc", "scatter_revisit.h"))
    assert '#include "scatter_revisit.h"' in open(os.path.join(ROOT, "online_gp_amd", "csrc", "scatter_stats.hip")).read()
    assert callable(grid_ops.revisit_sites) and {"wiski_absorb_revisit" + s for s in ("_f32", "_f64")} <= set(_hip.ABSORB_SIGNATURES)
    assert grid_ops.SITE_FORMS == {"interval": rv.INTERVAL, "poisson": rv.POISSON, "binomial": rv.BINOMIAL}
    assert ctypes.sizeof(_hip.wiski_site_ring) == 80
    # the public argument record has not grown: callers built against the previous header keep working
    assert ctypes.sizeof(_hip.wiski_absorb_args) == 224
