"""GPU: exponential forgetting.  The decay kernel (wiski_decay_stats) element by element; the forgetting model
against oracle/dataspace.py at the inflated noise d_i gamma^-(batches since i) -- posterior, marginal likelihood, sample paths --;
the carried residual; the bookkeeping (functional form, fantasies, sharded updater, launches per step); a drifting stream.

Every comparison with the oracle prints its figures before it asserts (run with -s)."""
import math

import numpy as np
import pytest
import torch

import sample_paths_reference as ref
from oracle import dataspace, spec

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}


# ------------------------------------------------------------------------------------------------------------ the kernel
SHAPES = {"d1": ([8], 1), "d2_odd": ([5, 7], 1), "d3": ([12, 12, 12], 1), "d2_two_outputs": ([5, 7], 2)}


def _arena(g, out, dtype, S, seed, guard=3):
    """One buffer that holds, each between guard words, the regions a model decays: the half stencils [out, H, m], b, cnt [out, m],
    the probes [m, S] and the residual R [out, m].  Region lengths with odd m and the 3-word guards put most regions off a 16-byte
    boundary.  -> (arena, {name: (offset, length)})"""
    m = int(np.prod(g))
    H = (7 ** len(g) + 1) // 2
    sizes = [("pack", out * H * m), ("b", out * m), ("cnt", out * m), ("P", m * S), ("R", out * m)]
    where, off = {}, guard
    for name, n in sizes:
        where[name] = (off, n)
        off += n + guard
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(off, generator=gen, dtype=torch.float64) * 3.0).to(dtype).to(DEV), where, (out, H, m)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("gamma", [0.9, 2.0 ** -10], ids=["g0.9", "g2^-10"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_decay_kernel_element_wise(shape, gamma, dtype):
    from online_gp_amd import grid_ops

    g, out = SHAPES[shape]
    S = 4
    arena, where, (out, H, m) = _arena(g, out, dtype, S, seed=len(g) + out)
    before = arena.clone()
    view = lambda name: arena[where[name][0]:where[name][0] + where[name][1]]
    # Z: a buffer of its own; for the odd grid at a 16-byte phase that differs from R's (the kernel then reads it element-wise)
    zbuf = torch.randn(out * m + 4, generator=torch.Generator().manual_seed(9), dtype=torch.float64).to(dtype).to(DEV)
    zoff = 1 if shape == "d2_odd" else 0
    Z = zbuf[zoff:zoff + out * m]
    zbefore = zbuf.clone()
    pack = view("pack").view(out, H, m)
    # two outputs: the stencils go in as the per-output views pack[o] (what a cache whose stencils are not one tensor hands over)
    regions = [(pack[o], gamma) for o in range(out)] if out > 1 else [(pack, gamma)]
    regions += [(view("b"), gamma), (view("cnt"), gamma), (view("P").view(m, S), math.sqrt(gamma))]
    stats = torch.randn((out, 2), generator=torch.Generator().manual_seed(4), dtype=torch.float64).to(DEV) * 50.0
    stats0 = stats.clone()
    counts = [123.0 + 7 * o for o in range(out)]
    side = torch.tensor([3.25, 1.5][:out], dtype=torch.float64, device=DEV)
    side0 = side.clone()
    grid_ops.decay_stats(gamma, regions, stats=stats, counts=counts, R=view("R").view(out, m), Z=Z.view(out, m), side=side)
    torch.cuda.synchronize()
    # pure scalings: the correctly rounded product with the factor rounded once to the working precision, bit for bit
    want = before.clone()
    for name, f in (("pack", gamma), ("b", gamma), ("cnt", gamma), ("P", math.sqrt(gamma))):
        o, n = where[name]
        want[o:o + n] = before[o:o + n] * torch.tensor(f, dtype=dtype)
        assert torch.equal(arena[o:o + n], want[o:o + n]), name
    # the residual: gamma R - (1 - gamma) Z in fp64, within 4 eps (|gamma R| + |(1 - gamma) Z|) per element (a fused multiply-add is allowed)
    o, n = where["R"]
    tR, tZ = gamma * before[o:o + n].double(), (1.0 - gamma) * Z.double().reshape(-1)
    err = (arena[o:o + n].double() - (tR - tZ)).abs()
    bound = 4 * EPS[dtype] * (tR.abs() + tZ.abs())
    print(f"{shape} {dtype} gamma={gamma}: residual worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    # guard words before, between and after the regions, and Z, are untouched
    want[o:o + n] = arena[o:o + n]
    assert torch.equal(arena, want) and torch.equal(zbuf, zbefore)
    # the fp64 statistics: slot 0 times gamma, slot 1 moved by -n log gamma
    assert torch.equal(stats[:, 0], stats0[:, 0] * gamma) and torch.equal(side, side0 * gamma)
    for o_ in range(out):
        exp = float(stats0[o_, 1]) - counts[o_] * math.log(gamma)
        assert abs(float(stats[o_, 1]) - exp) <= 1e-14 * abs(exp)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_decay_kernel_gamma_one_and_bad_gammas(dtype):
    from online_gp_amd import grid_ops
    from online_gp_amd._hip import WiskiError

    arena, where, (out, H, m) = _arena([5, 7], 1, dtype, 4, seed=2)
    before = arena.clone()
    view = lambda name: arena[where[name][0]:where[name][0] + where[name][1]]
    stats = torch.tensor([[2.0, -3.0]], dtype=torch.float64, device=DEV)
    Z = torch.ones(m, dtype=dtype, device=DEV)
    args = lambda: dict(regions=[(view("pack"), 1.0), (view("b"), 1.0)], stats=stats, counts=[10.0], R=view("R"), Z=Z)
    grid_ops.decay_stats(1.0, **args())
    torch.cuda.synchronize()
    assert torch.equal(arena, before) and stats.tolist() == [[2.0, -3.0]]
    for bad in (0.0, 1.5, float("nan"), -0.5):
        with pytest.raises(WiskiError):
            grid_ops.decay_stats(bad, **args())
    with pytest.raises(WiskiError):                                   # a factor outside (0, 1]
        grid_ops.decay_stats(0.5, [(view("b"), 1.5)])
    torch.cuda.synchronize()
    assert torch.equal(arena, before) and stats.tolist() == [[2.0, -3.0]]


def test_decay_beyond_eight_regions_outputs_and_side_scalars():
    """Ten regions, ten stats rows and ten side scalars: grid_ops.decay_stats cuts them into launches of eight, every element decays once."""
    from online_gp_amd import grid_ops

    gamma, n = 0.9, 10
    gen = torch.Generator().manual_seed(5)
    bufs = [torch.randn(37 + i, generator=gen, dtype=torch.float64).to(DEV) for i in range(n)]
    stats = torch.randn((n, 2), generator=gen, dtype=torch.float64).to(DEV)
    side = torch.randn(n, generator=gen, dtype=torch.float64).to(DEV)
    before, stats0, side0 = [b.clone() for b in bufs], stats.clone(), side.clone()
    counts = [10.0 + o for o in range(n)]
    grid_ops.decay_stats(gamma, [(b, gamma) for b in bufs], stats=stats, counts=counts, side=side)
    torch.cuda.synchronize()
    assert all(torch.equal(b, b0 * gamma) for b, b0 in zip(bufs, before))
    assert torch.equal(stats[:, 0], stats0[:, 0] * gamma) and torch.equal(side, side0 * gamma)
    exp = stats0[:, 1] - torch.tensor(counts, dtype=torch.float64, device=DEV) * math.log(gamma)
    assert bool(((stats[:, 1] - exp).abs() <= 1e-14 * exp.abs()).all())


# ------------------------------------------------------------------------------------- the model against the oracle
def _kernel(d, gb, g, ell, osc):
    from online_gp_amd.kernels import GridInterpolationKernel, MaternKernel, ScaleKernel

    k = GridInterpolationKernel(ScaleKernel(MaternKernel(nu=2.5, ard_num_dims=d)), grid_size=g, num_dims=d, grid_bounds=gb)
    k.base_kernel.outputscale = osc
    k.base_kernel.base_kernel.lengthscale = torch.as_tensor(np.broadcast_to(ell, (d,)).copy())
    return k


CASES = {
    "d2": dict(d=2, g=[12, 14], ell=[0.35, 0.5], osc=1.2),
    "d3": dict(d=3, g=[8, 8, 8], ell=[0.6, 0.5, 0.7], osc=1.1),
}
S2 = 0.3
_DATA = {}


def _data(case, batches, q):
    """Heteroscedastic points of a case, computed once and shared: (X, y, noise) numpy fp64, test points Xs."""
    key = (case, batches, q)
    if key not in _DATA:
        d = CASES[case]["d"]
        rng = np.random.default_rng(40 + d)
        n = batches * q
        X = rng.uniform(-1.05, 1.05, (n, d))
        y = np.sin(2.5 * X.sum(1)) + 0.3 * rng.standard_normal(n)
        _DATA[key] = (X, y, rng.uniform(0.3, 2.5, n), rng.uniform(-1.0, 1.0, (24, d)))
    return _DATA[key]


def _stream(case, dtype, gamma, batches=6, q=40, probes=0, seed=21, refresh=True):
    """A model built from the first batch and updated with the others (in place, each update decays first)."""
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    c = CASES[case]
    X, y, noise, Xs = _data(case, batches, q)
    t = lambda a: torch.as_tensor(a, dtype=dtype, device=DEV)
    Xt, yt, nt = t(X), t(y)[:, None], t(noise)[:, None]
    gb = torch.tensor([[-1.1, 1.1]] * c["d"])
    model = FixedNoiseOnlineSKIGP(Xt[:q], yt[:q], nt[:q], covar_module=_kernel(c["d"], gb, c["g"], c["ell"], c["osc"]), learn_additional_noise=True,
                                  num_path_probes=probes, path_seed=seed, forgetting_factor=gamma)
    model.likelihood.second_noise = S2
    model.eval()
    for lo in range(q, batches * q, q):
        if refresh:
            model.prediction_cache                                    # (PCG: the update then carries the residual through the decay)
        model.condition_on_observations(Xt[lo:lo + q], yt[lo:lo + q], nt[lo:lo + q], inplace=True)
    return model


def _inflated(noise, gamma, batches, q):
    age = (batches - 1) - np.arange(batches * q) // q                  # decays a point has seen: one per later batch
    return noise * float(gamma) ** -age


def _oracle(case, noise_eff, batches=6, q=40):
    c = CASES[case]
    X, y, _, Xs = _data(case, batches, q)
    O = dataspace.DataSpaceGP([[-1.1, 1.1]] * c["d"], c["g"], "matern52", c["ell"], c["osc"], S2).fit(X, y, noise_eff)
    return O, O.predict(Xs)


def _deviation(model, ref_mv, Xs):
    mvn = model(torch.as_tensor(Xs, dtype=model._dtype, device=DEV))
    mo, vo = ref_mv
    dm = np.abs(mvn.mean.double().cpu().numpy() - mo).max() / np.abs(mo).max()
    dv = np.abs(mvn.variance.double().cpu().numpy() - vo).max() / np.abs(vo).max()
    return dm, dv


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("regime", ["d2-dense", "d2-pcg", "d3-pcg"])
def test_posterior_matches_the_inflated_noise_oracle(regime, dtype):
    """Six batches of 40 heteroscedastic points, gamma = 0.8 per update, against DataSpaceGP at the noise d_i 0.8^-(batches since i).
    Allowed deviation of mean and variance: 3 x what the same model with forgetting_factor=None shows against the plain-noise oracle
    on the same points.  Measured on an MI355X (forgetting / plain, mean and variance): see DESIGN.md 3.13."""
    from online_gp_amd import settings

    case, route = regime.split("-")
    gamma = 0.8
    _, _, noise, Xs = _data(case, 6, 40)
    tol = 1e-10 if dtype == torch.float64 else None
    with settings.dense_small_grids(route == "dense"), settings.spectral_factor(route == "dense"), settings.cg_tolerance(tol), torch.no_grad():
        plain = _stream(case, dtype, None)
        pm, pv = _deviation(plain, _oracle(case, noise)[1], Xs)
        model = _stream(case, dtype, gamma)
        assert hasattr(model.prediction_cache["pred_cov"], "dense") == (route == "dense")
        fm, fv = _deviation(model, _oracle(case, _inflated(noise, gamma, 6, 40))[1], Xs)
    print(f"{regime} {dtype}: forgetting mean {fm:.3e} var {fv:.3e} | plain mean {pm:.3e} var {pv:.3e}")
    assert model.num_data == plain.num_data == 240
    assert fm <= 3.0 * pm and fv <= 3.0 * pv, (regime, dtype, fm, pm, fv, pv)
    # and the decay did something: the forgetting posterior is not the plain one
    dm, _ = _deviation(model, _oracle(case, noise)[1], Xs)
    assert dm > 10.0 * max(fm, pm)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", ["d2", "d3"])
def test_stream_step_posterior_matches_the_inflated_noise_oracle(case, dtype):
    """The one-call streaming step -- the only path that keeps the prediction cache across a decay and hands the closed-form residual
    to the fused absorb and refresh: 400 unit-noise points, then five `stream_step`s of 40 with gamma = 0.8, every one on that path and
    every one with the residual carried (fewer than 16 steps: no recompute in between).  Mean and variance against DataSpaceGP at the
    noise 0.8^-(steps since i), under the rule of the test above: 3 x what the same stream with forgetting_factor=None shows against
    the unit-noise oracle.  The d = 3 fp32 case is a shape with a two-level preconditioner, which every decay drops."""
    from online_gp_amd import settings
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    gamma, n0, q, steps = 0.8, 400, 40, 5
    c = CASES[case]
    X, y, _, Xs = _data(case, n0 // q + steps, q)
    n = n0 + steps * q
    t = lambda a: torch.as_tensor(a, dtype=dtype, device=DEV)
    Xt, yt = t(X), t(y)[:, None]
    gb = [[-1.1, 1.1]] * c["d"]
    dev, fast, carried = {}, {}, {}
    with settings.dense_small_grids(False), settings.spectral_factor(False), settings.deferred_refresh(False), torch.no_grad(), \
            settings.cg_tolerance(1e-10 if dtype == torch.float64 else None):
        for f in (None, gamma):
            model = FixedNoiseOnlineSKIGP(Xt[:n0], yt[:n0], None, covar_module=_kernel(c["d"], torch.tensor(gb), c["g"], c["ell"], c["osc"]),
                                          learn_additional_noise=True, forgetting_factor=f)
            model.likelihood.second_noise = S2
            model.eval()
            model.prediction_cache
            fast[f] = carried[f] = 0
            for lo in range(n0, n, q):
                fast[f] += int(model._stream_fast_state(Xt[lo:lo + q], yt[lo:lo + q]) is not None)
                carried[f] += int(model._mean_state["R_ok"])
                model.stream_step(Xt[lo:lo + q], yt[lo:lo + q])
            age = np.minimum(steps, (n - 1 - np.arange(n)) // q)            # decays a point has seen: one per later step
            noise_eff = np.ones(n) if f is None else float(f) ** -age
            O = dataspace.DataSpaceGP(gb, c["g"], "matern52", c["ell"], c["osc"], S2).fit(X, y, noise_eff)
            dev[f] = _deviation(model, O.predict(Xs), Xs)
            assert model.num_data == n
    (pm, pv), (fm, fv) = dev[None], dev[gamma]
    print(f"stream_step {case} {dtype}: forgetting mean {fm:.3e} var {fv:.3e} | plain mean {pm:.3e} var {pv:.3e} | one-call steps {fast}")
    assert fast[gamma] == steps and carried[gamma] == steps
    assert fm <= 3.0 * pm and fv <= 3.0 * pv, (case, dtype, fm, pm, fv, pv)


def test_mll_matches_the_oracle_at_the_inflated_noise():
    """Dense d = 2 case; the margin is the one tests/test_mll_gpu.py applies to the undecayed model against DataSpaceGP.mll()
    (test_mll_learnable_noise_gradient_matches_finite_difference: 1e-7 relative)."""
    from online_gp_amd.mlls import BatchedWoodburyMarginalLogLikelihood

    gamma = 0.8
    X, y, noise, _ = _data("d2", 6, 40)
    model = _stream("d2", torch.float64, gamma)
    assert hasattr(model.prediction_cache["pred_cov"], "dense")
    mll = BatchedWoodburyMarginalLogLikelihood(model.likelihood, model)
    model.train()
    Xt = torch.as_tensor(X, device=DEV)
    v = float(mll(model(Xt), torch.as_tensor(y, device=DEV)[:, None]).detach())
    O, _ = _oracle("d2", _inflated(noise, gamma, 6, 40))
    O0, _ = _oracle("d2", noise)
    print(f"mll {v:.12f} oracle (inflated) {O.mll():.12f} oracle (plain) {O0.mll():.12f}")
    assert abs(v - O.mll()) < 1e-7 * abs(O.mll())
    assert abs(v - O0.mll()) > 1e-3 * abs(O0.mll())


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-9), (torch.float32, 2e-4)], ids=["f64", "f32"])
def test_carried_residual_survives_the_decay(dtype, tol):
    """PCG regime: after a converged refresh and forget_(0.7) the state's R is b - Z - A U of the decayed buffers (recomputed in fp64;
    tolerance of tests/test_model_gpu.py::test_residual_carry_over_tracks_true_residual: 50 tol max|b|), and the next refresh takes
    no more CG iterations than a cold solve of the same system.

    Shape: 3 000 points on 8^3 = 512 nodes.  The state that is carried is (U, Z) of the UNDECAYED system; it is a good start exactly where
    the posterior mean moves little under the decay, i.e. where the data outweigh the prior at most nodes -- which is where a stream
    that forgets lives (it holds q / (1 - gamma) points' worth of weight for ever).  With fewer points than nodes the prior term Z is
    as large as b, the start's residual gamma R - (1 - gamma) Z is no smaller than the cold one's gamma b, and a warm solve has no reason
    to be shorter (measured there, 300 points, fp64 at tol 1e-10: 32 iterations warm, 30 cold)."""
    from online_gp_amd import grid_ops, settings

    with settings.dense_small_grids(False), settings.spectral_factor(False), settings.cg_tolerance(1e-10 if dtype == torch.float64 else 1e-6), torch.no_grad():
        model = _stream("d3", dtype, None, batches=3, q=1000)
        model.prediction_cache
        ms = model._mean_state
        assert ms["R_ok"]
        U0 = ms["U"].clone()
        model.forget_(0.7)
        assert model._mean_state is ms and ms["R_ok"] and torch.equal(ms["U"], U0) and "prediction_cache" not in model._memo
        c = model._kernel_cache
        A64 = c["WtW"].stencil.double()
        true_r = c["interpolation_cache"][0, :, 0].double() - ms["Z"][0].double() - grid_ops.stencil_spmv(model._grid, A64, ms["U"][0:1].double())[0]
        scale = float(c["interpolation_cache"].abs().max())
        err = float((ms["R"][0].double() - true_r).abs().max())
        print(f"{dtype}: |R - (b - Z - A U)| = {err:.3e}, allowed {tol * scale * 50:.3e}")
        assert err < tol * scale * 50
        warm = model.prediction_cache["cg_iters"][0]
        model._mean_state = None
        model._dump_caches()
        cold = model.prediction_cache["cg_iters"][0]
        print(f"{dtype}: refresh after the decay {warm} iterations, cold solve {cold}")
        assert 0 < warm <= cold


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_sample_paths_match_the_oracle_at_the_decayed_weights(dtype):
    """8 probes, three batches, gamma = 0.8: path by path against Matheron's rule in data space with weights wa_i gamma^age.  Rule of
    tests/test_sample_paths_gpu.py: 3 x the deviation of the model's own posterior mean from the oracle."""
    from online_gp_amd import settings

    S, seed, gamma, batches, q = 8, 21, 0.8, 3, 60
    c = CASES["d2"]
    X, y, noise, _ = _data("d2", batches, q)
    with settings.dense_small_grids(False), settings.spectral_factor(False), settings.cg_tolerance(1e-10 if dtype == torch.float64 else None), torch.no_grad():
        model = _stream("d2", dtype, gamma, batches=batches, q=q, probes=S, seed=seed)
        m = model._grid.m
        z = torch.randn((S, m), generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(dtype)
        paths = model.sample_paths(S, base_samples=z.to(DEV))
        U = model.prediction_cache["pred_mean"][0, :, 0].double().cpu().numpy()
    assert paths.last_converged
    # the oracle sees the points in the model's precision (they were rounded on their way in)
    r = lambda a: torch.as_tensor(a, dtype=dtype).double().numpy()
    Xn, yn, nz = r(X), r(y), r(noise)
    wa = gamma ** ((batches - 1) - np.arange(batches * q) // q) / nz
    gbl = [[-1.1, 1.1]] * c["d"]
    O = dataspace.DataSpaceGP(gbl, c["g"], "matern52", c["ell"], c["osc"], S2).fit(Xn, yn, 1.0 / wa)
    g0, h, gg = spec.make_grid(gbl, c["g"])
    W = ref.dense_w(g0, h, gg, Xn)
    Kuu = ref.kuu_dense(O.cols)
    u_mean = Kuu @ (W.T @ O.alpha)
    dev_mean = np.abs(U - u_mean).max() / np.abs(u_mean).max()
    eta = (ref.sym_sqrt(Kuu) @ z.double().numpy().T).T
    uo = ref.path_dataspace(Kuu, W, wa, yn, S2, eta, ref.normals(seed, np.arange(batches * q), S))
    dev_path = np.abs(paths.values.double().cpu().numpy() - uo).max() / np.abs(uo).max()
    print(f"{dtype}: path deviation {dev_path:.3e}, mean deviation {dev_mean:.3e}, ratio {dev_path / dev_mean:.2f}")
    assert dev_path <= 3.0 * dev_mean


# ------------------------------------------------------------------------------------------------------------ bookkeeping
def _buffers(model):
    c = model._kernel_cache
    out = {"stencil": c["WtW"].stencil, "b": c["interpolation_cache"], "cnt": c["_cnt"], "stats": c["_stats"]}
    if "path_probes" in c:
        out["probes"] = c["path_probes"]
    return out


def test_functional_update_decays_the_clone_and_fantasies_do_not_decay():
    from online_gp_amd import settings
    from online_gp_amd.distributed import ShardedStatsUpdater

    gamma, q = 0.8, 40
    X, y, noise, _ = _data("d2", 6, 40)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=DEV)
    Xn, yn, nn = t(X[:q]) * 0.9, t(y[:q])[:, None], t(noise[:q])[:, None]
    with settings.dense_small_grids(False), settings.spectral_factor(False), torch.no_grad():
        model = _stream("d2", torch.float64, gamma, batches=2, probes=8)
        keep = {k: v.clone() for k, v in _buffers(model).items()}
        wsum = list(model._wsum)
        child = model.condition_on_observations(Xn, yn, nn, inplace=False)
        for k, v in _buffers(model).items():
            assert torch.equal(v, keep[k]), k                          # the parent: bit for bit
        assert model._wsum == wsum and model.num_data == 80 and child.num_data == 120 and child.forgetting_factor == gamma
        # the clone decayed before it absorbed: the same as decaying a copy in place and absorbing there
        twin = _stream("d2", torch.float64, gamma, batches=2, probes=8)
        twin.condition_on_observations(Xn, yn, nn, inplace=True)
        for k, v in _buffers(child).items():
            w = _buffers(twin)[k]
            assert float((v - w).abs().max()) <= 1e-12 * float(w.abs().max()), k
        assert abs(child._wsum[0] - twin._wsum[0]) <= 1e-12 * twin._wsum[0]
        cnt_decayed = gamma * float(keep["cnt"].sum()) + float((1.0 / nn).sum())
        assert abs(float(_buffers(child)["cnt"].sum()) - cnt_decayed) <= 1e-10 * cnt_decayed
        # a fantasy is a what-if on the current state: no decay (plain and batched form), parent untouched
        fant = model.get_fantasy_model(Xn, yn[:, 0], nn)
        cnt_plain = float(keep["cnt"].sum()) + float((1.0 / nn).sum())
        assert abs(float(_buffers(fant)["cnt"].sum()) - cnt_plain) <= 1e-10 * cnt_plain
        ld_plain = float(keep["stats"][0, 1]) + float(nn.log().sum())
        assert abs(float(_buffers(fant)["stats"][0, 1]) - ld_plain) <= 1e-10 * abs(ld_plain)
        model.get_fantasy_model(Xn[None, :4], yn[None, :4, 0])
        for k, v in _buffers(model).items():
            assert torch.equal(v, keep[k]), k
        with pytest.raises(NotImplementedError):
            ShardedStatsUpdater(_stream("d2", torch.float64, gamma, batches=1))
    with pytest.raises(ValueError):
        _stream("d2", torch.float64, 1.5, batches=1)
    with pytest.raises(ValueError):
        model.forget_(0.0)


def _kernels_of(fn):
    """Names of the kernels the device ran for fn() (torch profiler)."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]


def test_one_more_launch_per_stream_step_and_none_without_forgetting():
    """The one-call streaming step of a forgetting model runs the kernels of a plain one plus exactly one, the decay -- once per step --
    and stays on that path; with forgetting_factor=None no decay kernel is ever launched."""
    from online_gp_amd import settings
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    d, g, q, n0 = 2, 24, 64, 1024
    gen = torch.Generator().manual_seed(0)
    X = (torch.rand((n0 + 10 * q, d), generator=gen) * 2 - 1).to(DEV)
    y = torch.sin(2 * X.sum(1, keepdim=True))
    batch = lambda s: (X[n0 + s * q:n0 + (s + 1) * q], y[n0 + s * q:n0 + (s + 1) * q])
    names = {}
    with settings.dense_small_grids(False), settings.spectral_factor(False), settings.deferred_refresh(False), torch.no_grad():
        for gamma in (None, 0.9):
            model = FixedNoiseOnlineSKIGP(X[:n0], y[:n0], None, grid_bounds=torch.tensor([[-1.1, 1.1]] * d), grid_size=g, learn_additional_noise=True,
                                          forgetting_factor=gamma).eval()
            for s in range(4):                                           # (the data volume does not double over the 10 steps: no profile look)
                model.stream_step(*batch(s))
            # like with like: the steps that ran on the one-call path (a plain stream leaves it for a step now and then, when its
            # growing data volume makes it look at the preconditioner again)
            runs = []
            for s in range(4, 10):
                fast = model._stream_fast_state(*batch(s)) is not None
                ks = _kernels_of(lambda s=s: model.stream_step(*batch(s)))
                if fast:
                    runs.append(ks)
            assert len(runs) >= 3, (gamma, len(runs))
            if gamma is not None:
                assert len(runs) == 6                                    # a decay never takes the step off the one-call path
            names[gamma] = runs
            want = float(n0)
            for s in range(10):
                want = (gamma or 1.0) * want + q
            cnt = float(model._kernel_cache["_cnt"].sum())
            assert abs(cnt - want) <= 1e-4 * want and abs(model._wsum[0] - want) <= 1e-9 * want and model.num_data == n0 + 10 * q
    plain = set().union(*names[None])
    forgetting = set().union(*names[0.9])
    print("plain:", sorted(plain), "\nextra with forgetting:", sorted(forgetting - plain))
    assert not [n for n in plain if "decay" in n]
    assert plain <= forgetting and len(forgetting - plain) == 1 and "decay_stats" in next(iter(forgetting - plain))
    assert all(sum("decay_stats" in n for n in run) == 1 for run in names[0.9])


def test_wrappers_pass_the_factor_and_update_decays():
    from online_gp_amd.models import OnlineSKIBotorchModel, OnlineSKIRegression
    from online_gp_amd.models.stems import Identity

    gen = torch.Generator().manual_seed(1)
    X = (torch.rand((60, 2), generator=gen) * 2 - 1).to(DEV)
    y = torch.sin(2 * X.sum(1, keepdim=True))
    r = OnlineSKIRegression(Identity(2), X[:40], y[:40], 1e-2, 10, 1.0, forgetting_factor=0.5)
    assert r.gp.forgetting_factor == 0.5
    r.update(X[40:], y[40:], update_gp=False)
    assert abs(float(r.gp._kernel_cache["_cnt"].sum()) - (0.5 * 40 + 20)) < 1e-3 and r.gp.num_data == 60
    assert abs(r.gp._wsum[0] - 40.0) < 1e-9
    b = OnlineSKIBotorchModel(X[:40].double(), y[:40].double(), torch.ones(40, 1, dtype=torch.float64, device=DEV),
                              grid_bounds=torch.tensor([[-1.1, 1.1]] * 2), grid_size=10, forgetting_factor=0.5)
    assert b.forgetting_factor == 0.5 and OnlineSKIBotorchModel(X[:40].double(), y[:40].double(), torch.ones(40, 1, dtype=torch.float64, device=DEV),
                                                                 grid_bounds=torch.tensor([[-1.1, 1.1]] * 2), grid_size=10).forgetting_factor is None


# ------------------------------------------------------------------------------------------------------------ behaviour
def test_forgetting_follows_a_sign_flip():
    """d = 1, g = 32: 200 points of sin(x), then 200 of -sin(x), in batches of 20.  The forgetting model (gamma = 0.7) ends closer to
    -sin than the model that weighs the first point like the last.  A relative statement between two runs; no fixed number."""
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    gen = torch.Generator().manual_seed(7)
    X = ((torch.rand((400, 1), generator=gen, dtype=torch.float64) * 2 - 1) * 3.0).to(DEV)
    sign = torch.cat([torch.ones(200), -torch.ones(200)]).to(DEV, torch.float64)[:, None]
    y = sign * torch.sin(X) + 0.05 * torch.randn((400, 1), generator=gen, dtype=torch.float64).to(DEV)
    Xs = torch.linspace(-3, 3, 64, dtype=torch.float64, device=DEV)[:, None]
    rmse = {}
    with torch.no_grad():
        for gamma in (None, 0.7):
            model = FixedNoiseOnlineSKIGP(X[:20], y[:20], None, grid_bounds=torch.tensor([[-3.3, 3.3]]), grid_size=32, learn_additional_noise=True,
                                          forgetting_factor=gamma).eval()
            for lo in range(20, 400, 20):
                model.condition_on_observations(X[lo:lo + 20], y[lo:lo + 20], None, inplace=True)
            rmse[gamma] = float((model(Xs).mean + torch.sin(Xs[:, 0])).pow(2).mean().sqrt())
    print(f"rmse against -sin: forgetting {rmse[0.7]:.4f}, plain {rmse[None]:.4f}")
    assert rmse[0.7] < rmse[None]
