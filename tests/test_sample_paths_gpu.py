"""GPU: posterior sample paths.  The probe kernel (wiski_scatter_probes) against the host reference of
tests/sample_paths_reference.py; the probes' bookkeeping through every way a point enters the statistics; the paths against
Matheron's rule in data space, path by path; GridSamplePaths evaluation and gradients; the at-size smoke run; the harness's
pathwise acquisitions.

Measured on an MI355X (each test prints its figures before it asserts; run with -s to see them):
  probe kernel, worst |P - P_ref| / (4 c eps sum|terms|) over d = 1..4:   0.038 (fp64), 0.027 (fp32)
  paths vs data-space oracle / mean vs oracle (PCG route):                6.4e-8 / 6.1e-8 (d2 fp64), 3.2e-6 / 2.5e-6 (d2 fp32),
                                                                          3.7e-8 / 8.5e-8 (d3 fp64), 2.8e-6 / 5.4e-6 (d3 fp32)
  50^3, 2 000 + 20 000 streamed points, S = 16: within 5 standard errors at 64 / 64 points, 5 CG iterations,
                                                                          20 of 20 steps on the one-call streaming path
"""
from collections import Counter

import numpy as np
import pytest
import torch

import sample_paths_reference as ref
from oracle import dataspace, spec

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = {torch.float32: 2.0 ** -23, torch.float64: 2.0 ** -52}
GRIDS = {1: [12], 2: [8, 9], 3: [6, 7, 5], 4: [5, 6, 5, 4]}


def _grid(d, g, lo=-1.1, hi=1.1):
    from online_gp_amd import grid_ops

    return grid_ops.GridSpec(torch.tensor([[lo, hi]] * d), g)


def _points(rng, grid, n, boundary=0.15):
    """n points inside the grid; about `boundary` of them per dim in the one-hot boundary cells (first / last cell)."""
    d = grid.d
    x = rng.uniform(-1.05, 1.05, (n, d))
    for k in range(d):
        hi = grid.g0[k] + grid.h[k] * (grid.g[k] - 1)
        pick = rng.uniform(size=n) < boundary
        lo_side = rng.uniform(size=n) < 0.5
        xb = np.where(lo_side, grid.g0[k] + rng.uniform(0.02, 0.98, n) * grid.h[k], hi - rng.uniform(0.02, 0.98, n) * grid.h[k])
        x[:, k] = np.where(pick, xb, x[:, k])
    return x


def _kernel(kind, d, gb, g, ell, osc):
    from online_gp_amd.kernels import GridInterpolationKernel, MaternKernel, RBFKernel, ScaleKernel

    base = RBFKernel(ard_num_dims=d) if kind == "rbf" else MaternKernel(nu=2.5, ard_num_dims=d)
    k = GridInterpolationKernel(ScaleKernel(base), grid_size=g, num_dims=d, grid_bounds=gb)
    k.base_kernel.outputscale = osc
    k.base_kernel.base_kernel.lengthscale = torch.as_tensor(np.broadcast_to(ell, (d,)).copy())
    return k


def _probe_tolerance(cnt, asum, dtype):
    """4 c eps sum|terms| per node (c contributions, eps of the working precision), all from the reference: every increment is
    rounded once (eps / 2 of its size), every one of the c atomic adds rounds a partial sum that is at most sum|terms| (eps / 2
    each), and the reference's own fp64 evaluation differs from the kernel's by a few ulps per term."""
    return 4.0 * cnt[:, None] * EPS[dtype] * asum


# ------------------------------------------------------------------------------------------------------- the probe kernel
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_probe_kernel_matches_host_reference(d, dtype):
    from online_gp_amd import grid_ops

    rng = np.random.default_rng(10 + d)
    grid = _grid(d, GRIDS[d])
    S, seed = 6, 0x1234_5678_9ABC_DEF1
    err = grid_ops.new_err_flag(DEV)
    P = torch.zeros((grid.m, S), dtype=dtype, device=DEV)
    Pr, cnt, asum = np.zeros((grid.m, S)), np.zeros(grid.m), np.zeros((grid.m, S))
    first = (1 << 32) - 100                                  # the batches straddle the low counter word
    rep = _points(rng, grid, 5)
    batches = [(_points(rng, grid, 200), None),              # unit weights (NULL)
               (_points(rng, grid, 200), rng.uniform(0.2, 5.0, 200)),
               (np.repeat(rep, 10, axis=0), rng.uniform(0.2, 5.0, 50))]      # repeated points: colliding atomics
    for x, wa in batches:
        xt = torch.as_tensor(x, dtype=dtype, device=DEV)
        wt = None if wa is None else torch.as_tensor(wa, dtype=dtype, device=DEV)
        grid_ops.scatter_probes(grid, xt, wt, first, seed, P, err)
        x64 = xt.double().cpu().numpy()                      # the reference sees the points and weights the kernel saw
        w64 = None if wt is None else wt.double().cpu().numpy()
        p, c, a = ref.probes(grid.g0, grid.h, grid.g, x64, w64, first, seed, S, with_bounds=True)
        Pr, cnt, asum, first = Pr + p, cnt + c, asum + a, first + x.shape[0]
    assert int(err.item()) == 0
    got = P.double().cpu().numpy()
    tol = _probe_tolerance(cnt, asum, dtype)
    dev = np.abs(got - Pr)
    print(f"probes d={d} {dtype}: max |P - ref| = {dev.max():.3e}, worst dev / tol = {(dev / np.maximum(tol, 1e-300)).max():.3f}, "
          f"nodes touched {int((cnt > 0).sum())} / {grid.m}, min contributions {int(cnt[cnt > 0].min())}")
    assert (got[cnt == 0] == 0).all()
    assert (dev <= tol).all()
    # outside the grid: flagged, contributes nothing
    P2 = P.clone()
    xo = torch.full((3, d), 5.0, dtype=dtype, device=DEV)
    grid_ops.scatter_probes(grid, xo, None, first, seed, P2, err)
    assert int(err.item()) & 1 and torch.equal(P, P2)


# ------------------------------------------------------------------------------------------------------------ bookkeeping
def _kernels_of(fn):
    """Names of the kernels the device ran for fn(), in order (torch profiler)."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]


def test_probes_follow_every_way_a_point_enters_the_statistics():
    from online_gp_amd import settings
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    rng = np.random.default_rng(5)
    d, g, S, n = 2, [12, 14], 8, 600
    gb = torch.tensor([[-1.1, 1.1]] * d)
    grid = _grid(d, g)
    X = torch.as_tensor(_points(rng, grid, n), device=DEV)
    y = torch.sin(3 * X.sum(1, keepdim=True))
    mk = lambda x0, y0, **kw: FixedNoiseOnlineSKIGP(x0, y0, None, grid_bounds=gb, grid_size=g, learn_additional_noise=True, **kw)
    Pr, cnt, asum = ref.probes(grid.g0, grid.h, grid.g, X.cpu().numpy(), None, 0, 77, S, with_bounds=True)
    tol = _probe_tolerance(cnt, asum, torch.float64)

    def check(model, what):
        P = model._kernel_cache["path_probes"]
        assert P.shape == (grid.m, S) and model._kernel_cache["path_count"] == n == model.num_data
        dev = np.abs(P.cpu().numpy() - Pr)
        print(f"{what}: worst dev / tol = {(dev / np.maximum(tol, 1e-300)).max():.3f}")
        assert (dev <= tol).all(), what

    # constructor + in-place updates of mixed batch sizes
    a = mk(X[:100], y[:100], num_path_probes=S - 1, path_seed=77)          # odd S rounds up
    for lo, hi in ((100, 150), (150, 151), (151, 300), (300, 600)):
        a.condition_on_observations(X[lo:hi], y[lo:hi], None, inplace=True)
    check(a, "init + updates")
    # set_train_data in one go (restarts the index at 0)
    b = mk(X[:10], y[:10], num_path_probes=S, path_seed=77)
    b.set_train_data(X, y, torch.ones_like(y))
    check(b, "set_train_data")
    # functional chain; a parent's buffer is never touched by its child
    c0 = mk(X[:100], y[:100], num_path_probes=S, path_seed=77)
    keep = c0._kernel_cache["path_probes"].clone()
    c1 = c0.condition_on_observations(X[100:350], y[100:350], torch.ones_like(y[100:350]), inplace=False)
    assert torch.equal(c0._kernel_cache["path_probes"], keep) and c0._kernel_cache["path_count"] == 100
    keep1 = c1._kernel_cache["path_probes"].clone()
    c2 = c1.condition_on_observations(X[350:], y[350:], inplace=False)
    assert torch.equal(c1._kernel_cache["path_probes"], keep1) and c1._kernel_cache["path_probes"].data_ptr() != c2._kernel_cache["path_probes"].data_ptr()
    check(c2, "functional chain")
    # kernel_cache hand-over (the BO loop's re-initialisation)
    h = FixedNoiseOnlineSKIGP(covar_module=c2.covar_module, kernel_cache=c2._kernel_cache, learn_additional_noise=True, likelihood=c2.likelihood,
                              num_data=c2.num_data)
    check(h, "kernel_cache hand-over")
    with pytest.raises(ValueError, match="carries no path probes"):
        plain = mk(X[:100], y[:100])
        FixedNoiseOnlineSKIGP(covar_module=plain.covar_module, kernel_cache=plain._kernel_cache, num_data=100, num_path_probes=4)
    with pytest.raises(ValueError, match="carries 8 probes"):
        FixedNoiseOnlineSKIGP(covar_module=c2.covar_module, kernel_cache=c2._kernel_cache, likelihood=c2.likelihood, num_data=n, num_path_probes=4)
    # the one-call streaming step (beyond the dense regime), probes on and off
    with settings.dense_small_grids(False), settings.spectral_factor(False), torch.no_grad():
        s1 = mk(X[:100], y[:100], num_path_probes=S, path_seed=77).eval()
        s0 = mk(X[:100], y[:100]).eval()
        for m_ in (s1, s0):
            m_.prediction_cache
        # every kernel the device runs, by name (torch profiler): the two models are in the same state and see the same batches, so
        # with probes on a step runs exactly the launches of the step with probes off, plus ONE k_scatter_probes
        fast = 0
        for lo in range(100, 600, 100):
            k0 = _kernels_of(lambda: s0.stream_step(X[lo:lo + 100], y[lo:lo + 100]))
            k1 = _kernels_of(lambda: s1.stream_step(X[lo:lo + 100], y[lo:lo + 100]))
            fast += s1.__dict__.get("_stream_step_cache") is not None and s0.__dict__.get("_stream_step_cache") is not None
            probes = [k for k in k1 if "k_scatter_probes" in k]
            print(f"stream_step at {lo}: {len(k0)} launches with probes off, {len(k1)} with probes on")
            assert len(k0) > 0 and not any("k_scatter_probes" in k for k in k0)
            assert len(probes) == 1 and Counter(k1) - Counter(probes) == Counter(k0)
        assert fast >= 4, "the one-call streaming path was not taken"
        check(s1, "stream_step")
        k0 = _kernels_of(lambda: (s0.condition_on_observations(X[:5], y[:5], None, inplace=True), s0.prediction_cache))
        assert len(k0) > 0 and not any("k_scatter_probes" in k for k in k0)
        assert "path_probes" not in s0._kernel_cache and "path_seed" not in s0._kernel_cache and "path_count" not in s0._kernel_cache
        with pytest.raises(ValueError, match="num_path_probes"):
            s1.sample_paths(S + 2)
        with pytest.raises(RuntimeError, match="num_path_probes"):
            s0.sample_paths(2)
    with pytest.raises(NotImplementedError):
        FixedNoiseOnlineSKIGP(X[:50], torch.cat([y[:50], y[:50]], 1), None, grid_bounds=gb, grid_size=g, num_path_probes=4)
    from online_gp_amd.distributed import ShardedStatsUpdater

    with pytest.raises(NotImplementedError):
        ShardedStatsUpdater(a)


# ------------------------------------------------------------------------------- paths against the data-space oracle
def _oracle_setup(d, g, kind, ell, osc, s2, X, y, noise):
    gb = [[-1.1, 1.1]] * d
    O = dataspace.DataSpaceGP(gb, g, kind, ell, osc, s2).fit(X, y, noise)
    g0, h, gg = spec.make_grid(gb, g)
    W = ref.dense_w(g0, h, gg, X)
    Kuu = ref.kuu_dense(O.cols)
    u_mean = Kuu @ (W.T @ O.alpha)
    return Kuu, W, u_mean


CASES = {
    "d2": dict(d=2, g=[12, 14], n=300, batch=60, hetero=True, ell=[0.35, 0.5], osc=1.2),
    "d3": dict(d=3, g=[8, 8, 8], n=400, batch=100, hetero=False, ell=[0.6, 0.5, 0.7], osc=1.1),
}


def _build(case, dtype, dense, S=8, seed=21):
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    c = CASES[case]
    d, g, n = c["d"], c["g"], c["n"]
    rng = np.random.default_rng(100 + d)
    grid = _grid(d, g)
    X = torch.as_tensor(_points(rng, grid, n, boundary=0.05), dtype=dtype, device=DEV)
    Xn = X.double().cpu().numpy()
    yn = np.sin(2.5 * Xn.sum(1)) + 0.3 * rng.standard_normal(n)
    y = torch.as_tensor(yn, dtype=dtype, device=DEV)[:, None]
    noise = torch.as_tensor(rng.uniform(0.3, 2.5, n) if c["hetero"] else np.ones(n), dtype=dtype, device=DEV)[:, None]
    gb = torch.tensor([[-1.1, 1.1]] * d)
    nz = (lambda lo, hi: noise[lo:hi]) if c["hetero"] else (lambda lo, hi: None)
    b = c["batch"]
    model = FixedNoiseOnlineSKIGP(X[:b], y[:b], nz(0, b), covar_module=_kernel("matern52", d, gb, g, c["ell"], c["osc"]),
                                  learn_additional_noise=True, num_path_probes=0 if dense else S, path_seed=seed)
    model.likelihood.second_noise = 0.3
    model.eval()
    for lo in range(b, n, b):
        model.condition_on_observations(X[lo:lo + b], y[lo:lo + b], nz(lo, lo + b), inplace=True)
    return model, Xn, y.double().cpu().numpy()[:, 0], noise.double().cpu().numpy()[:, 0]


def _hypers(model):
    ell = model.covar_module.base_kernel.base_kernel.lengthscale.detach().double().cpu().numpy().reshape(-1)
    return ell, float(model.covar_module.base_kernel.outputscale), float(model._sigma2(0))


def _compare_with_oracle(model, case, Xn, yn, noise, S, seed, dense, what):
    c = CASES[case]
    m = model._grid.m
    z = torch.randn((S, m), generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(model._dtype)
    paths = model.sample_paths(S, base_samples=z.to(DEV))
    assert paths.last_converged and paths.values.shape == (S, m) and bool(torch.isfinite(paths.values).all())
    ell, osc, s2 = _hypers(model)
    Kuu, W, u_mean = _oracle_setup(c["d"], c["g"], "matern52", ell, osc, s2, Xn, yn, noise)
    zn = z.double().numpy()
    U = model.prediction_cache["pred_mean"][0, :, 0].double().cpu().numpy()
    dev_mean = np.abs(U - u_mean).max() / np.abs(u_mean).max()
    if dense:
        # u = M b + sigma chol(M + jitter) z with the factor recomputed by torch in fp64 from the model's M; the mean from the oracle
        M = model.prediction_cache["pred_cov"].dense.double().cpu()
        M = 0.5 * (M + M.t())
        L = torch.linalg.cholesky(M + paths.jitter * torch.eye(m, dtype=torch.float64)).numpy()
        uo = u_mean[None] + np.sqrt(s2) * zn @ L.T
    else:
        eps = ref.normals(seed, np.arange(Xn.shape[0]), S)
        eta = (ref.sym_sqrt(Kuu) @ zn.T).T
        uo = ref.path_dataspace(Kuu, W, 1.0 / noise, yn, s2, eta, eps)
    dev_path = np.abs(paths.values.double().cpu().numpy() - uo).max() / np.abs(uo).max()
    print(f"{what}: path deviation {dev_path:.3e}, mean deviation {dev_mean:.3e}, ratio {dev_path / dev_mean:.2f}")
    assert dev_path <= 3.0 * dev_mean, (what, dev_path, dev_mean)
    return paths


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", ["d2", "d3"])
def test_paths_match_the_data_space_oracle_pcg(case, dtype):
    """Path by path against Matheron's rule in data space; allowed deviation: 3 x what the model's own posterior mean shows
    against oracle/dataspace.py on the same problem at the same tolerance (both on the PCG route)."""
    from online_gp_amd import settings

    S, seed = 8, 21
    tol = 1e-10 if dtype == torch.float64 else None
    with settings.dense_small_grids(False), settings.spectral_factor(False), settings.cg_tolerance(tol), torch.no_grad():
        model, Xn, yn, noise = _build(case, dtype, dense=False, S=S, seed=seed)
        _compare_with_oracle(model, case, Xn, yn, noise, S, seed, False, f"pcg {case} {dtype}")


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", ["d2", "d3"])
def test_paths_match_the_oracle_dense_regime(case, dtype):
    with torch.no_grad():
        model, Xn, yn, noise = _build(case, dtype, dense=True)
        assert hasattr(model.prediction_cache["pred_cov"], "dense") and "path_probes" not in model._kernel_cache
        p = _compare_with_oracle(model, case, Xn, yn, noise, 11, 0, True, f"dense {case} {dtype}")     # any number of paths, no probes
        assert p.jitter > 0


def test_probes_do_not_depend_on_the_hyperparameters():
    from online_gp_amd import settings

    S, seed = 8, 21
    with settings.dense_small_grids(False), settings.spectral_factor(False), settings.cg_tolerance(1e-10), torch.no_grad():
        model, Xn, yn, noise = _build("d2", torch.float64, dense=False, S=S, seed=seed)
        first = model.sample_paths(S, seed=1).values.clone()
        keep = model._kernel_cache["path_probes"].clone()
        model.likelihood.second_noise = 0.55
        model.covar_module.base_kernel.base_kernel.lengthscale = torch.tensor([0.5, 0.3], dtype=torch.float64)
        model.hyperparameters_changed()
        _compare_with_oracle(model, "d2", Xn, yn, noise, S, seed, False, "pcg d2 after a hyper-parameter step")
        assert torch.equal(model._kernel_cache["path_probes"], keep)
        assert not torch.allclose(model.sample_paths(S, seed=1).values, first)


# ------------------------------------------------------------------------------------------------- evaluating the paths
def test_grid_sample_paths_call_gradient_and_determinism():
    from online_gp_amd import settings

    rng = np.random.default_rng(8)
    with settings.dense_small_grids(False), settings.spectral_factor(False), settings.cg_tolerance(1e-10):
        with torch.no_grad():
            model, Xn, yn, noise = _build("d2", torch.float64, dense=False)
            p8 = model.sample_paths(8, seed=4)
            p3 = model.sample_paths(3, seed=4)
            # same arguments, same state: the same paths, computed again (nothing is cached).  Two solves of the same systems, each
            # stopped at a relative residual of 1e-10: agreement to 1e-6 leaves four orders for the conditioning of the system
            again = model.sample_paths(8, seed=4)
            assert again is not p8 and torch.allclose(again.values, p8.values, rtol=0, atol=1e-6 * float(p8.values.abs().max()))
            assert not torch.allclose(model.sample_paths(8, seed=5).values, p8.values, rtol=0, atol=1e-3)
            # fresh base samples give fresh paths, whatever address the allocator hands the new tensor
            m_ = model._grid.m
            gen = torch.Generator(device=DEV).manual_seed(1)
            draws = [model.sample_paths(4, base_samples=torch.randn((4, m_), generator=gen, device=DEV, dtype=torch.float64)).values for _ in range(6)]
            for i in range(6):
                for j in range(i):
                    assert float((draws[i] - draws[j]).abs().max()) > 1e-2
            # path s is a function of (z_s, probe s) alone: the first three of eight equal three drawn on their own (same bound)
            z = torch.randn((8, model._grid.m), generator=torch.Generator().manual_seed(6), dtype=torch.float64).to(DEV)
            pa, pb = model.sample_paths(8, base_samples=z), model.sample_paths(3, base_samples=z[:3].contiguous())
            assert torch.allclose(pb.values, pa.values[:3], rtol=0, atol=1e-6 * float(pa.values.abs().max()))
        g = model._grid
        Xq = torch.as_tensor(rng.uniform(-0.8, 0.8, (5, 7, 2)), device=DEV)
        Wq = ref.dense_w(g.g0, g.h, g.g, Xq.reshape(-1, 2).cpu().numpy())
        for p in (p8, p3):                                                  # both gather forms
            F = p(Xq)
            assert F.shape == (p.num_paths, 5, 7)
            want = (Wq @ p.values.cpu().numpy().T).T.reshape(p.num_paths, 5, 7)
            assert np.abs(F.cpu().numpy() - want).max() <= 1e-12 * np.abs(want).max()
            assert torch.equal(p(Xq), F)
            assert torch.equal(p.max_values(Xq), F.reshape(p.num_paths, -1).max(-1).values)
            # X-gradient against central differences (interior points: the paths are C^1 there)
            Xg = Xq[0].clone().requires_grad_(True)
            cw = torch.as_tensor(rng.standard_normal((p.num_paths, 7)), device=DEV)
            (p(Xg) * cw).sum().backward()
            hstep = 1e-6
            for k in range(2):
                e = torch.zeros(2, dtype=torch.float64, device=DEV)
                e[k] = hstep
                with torch.no_grad():
                    fd = ((p(Xq[0] + e) - p(Xq[0] - e)) * cw).sum(0) / (2 * hstep)
                assert torch.allclose(Xg.grad[:, k], fd, rtol=1e-6, atol=1e-7 * float(p.values.abs().max()))
        with pytest.raises(RuntimeError, match="out of bounds"):
            p8(torch.full((2, 2), 3.0, dtype=torch.float64, device=DEV))
        assert p8(Xq).shape == (8, 5, 7)                                    # the flag was cleared


# ----------------------------------------------------------------------------------------------------------- at size
def test_sample_paths_at_size_50_cubed():
    from online_gp_amd import settings
    from online_gp_amd.models import FixedNoiseOnlineSKIGP

    rng = np.random.default_rng(0)
    n0, S, dtype = 2000, 16, torch.float32                 # n0 points build the model, then 20 000 stream in
    n = n0 + 20000
    centres = rng.uniform(-0.7, 0.7, (6, 3))
    Xn = np.clip(centres[rng.integers(0, 6, n)] + 0.12 * rng.standard_normal((n, 3)), -1.0, 1.0)
    yn = np.sin(2 * Xn.sum(1)) + 0.1 * rng.standard_normal(n)
    X = torch.as_tensor(Xn, dtype=dtype, device=DEV)
    y = torch.as_tensor(yn, dtype=dtype, device=DEV)[:, None]
    with torch.no_grad():
        model = FixedNoiseOnlineSKIGP(X[:n0], y[:n0], None, grid_bounds=torch.tensor([[-1.1, 1.1]] * 3), grid_size=50, learn_additional_noise=True,
                                      num_path_probes=S, path_seed=9).eval()
        model.prediction_cache
        fast = 0
        for lo in range(n0, n, 1000):
            model.stream_step(X[lo:lo + 1000], y[lo:lo + 1000])
            fast += model.__dict__.get("_stream_step_cache") is not None
        # the one-call path may hand a step to the generic one when the data volume has doubled since the preconditioner's density
        # profile was looked at (models: _stream_fast_state): 2 000 -> 22 000 doubles fewer than 4 times
        print(f"50^3: {fast} of 20 steps on the one-call streaming path")
        assert fast >= 16, "the one-call streaming path was not taken"
        assert model._kernel_cache["path_count"] == n == model.num_data
        paths = model.sample_paths(S, seed=2)
        assert paths.last_converged and bool(torch.isfinite(paths.values).all())
        Xt = torch.as_tensor(np.clip(centres[rng.integers(0, 6, 64)] + 0.15 * rng.standard_normal((64, 3)), -1.0, 1.0), dtype=dtype, device=DEV)
        with settings.spectral_factor(False):
            post = model(Xt)
            mu, sd = post.mean.double(), post.variance.double().clamp_min(0).sqrt()
        F = paths(Xt).double()
        inside = ((F.mean(0) - mu).abs() <= 5.0 * sd / np.sqrt(S))
        spread = F.std(0) / sd
        print(f"50^3: solve iterations {paths.iters}, points within 5 standard errors {int(inside.sum())} / 64, "
              f"sample std / posterior std: median {float(spread.median()):.2f}")
        assert int(inside.sum()) >= 60


# ----------------------------------------------------------------------------------------------------------- harness
def _bo_model(d, g, n, dtype=torch.float64, probes=0, seed=0):
    from online_gp_amd.models import OnlineSKIBotorchModel

    rng = np.random.default_rng(seed)
    X = torch.as_tensor(rng.uniform(0.02, 0.98, (n, d)), dtype=dtype, device=DEV)
    y = torch.sin(4 * X.sum(1, keepdim=True)) + 0.05 * torch.as_tensor(rng.standard_normal((n, 1)), dtype=dtype, device=DEV)
    gb = torch.tensor([[-0.1, 1.1]] * d)
    return OnlineSKIBotorchModel(X, y, None, covar_module=_kernel("matern52", d, gb, g, 0.3, 1.0), learn_additional_noise=True,
                                 num_path_probes=probes, path_seed=5).eval(), X, y


@pytest.mark.parametrize("dense", [True, False], ids=["dense", "pcg"])
def test_optimize_acqf_thompson_and_nei(dense):
    from online_gp_amd import harness, settings

    d, q = 2, 3
    with settings.dense_small_grids(dense), settings.spectral_factor(False):
        model, X, y = _bo_model(d, 12, 80, probes=0 if dense else 8)
        unit = torch.stack([torch.zeros(d, dtype=torch.float64), torch.ones(d, dtype=torch.float64)])
        Xb, v = harness.optimize_acqf(model, "ts", unit, q, num_restarts=4, raw_samples=64, maxiter=30, seed=3)
        assert Xb.shape == (q, d) and bool(((Xb >= 0) & (Xb <= 1)).all())
        paths = model.sample_paths(q, seed=3)                               # the draw of that call
        g = torch.Generator(device="cpu").manual_seed(3)
        raw = torch.rand((64, q, d), generator=g, dtype=torch.float64).to(DEV)
        with torch.no_grad():
            best_raw = harness.ts_values(paths, raw).max()
            assert torch.allclose(harness.ts_values(paths, Xb[None])[0], v)
        print(f"ts ({'dense' if dense else 'pcg'}): optimised value {float(v):.4f}, best raw sample {float(best_raw):.4f}")
        assert float(v) >= float(best_raw)
        # nei: candidates that are baseline points cannot improve on the baseline -> exactly 0; elsewhere it is >= 0
        with torch.no_grad():
            v0 = harness.acqf_values(model, X[:6].reshape(2, 3, d), "nei", X_baseline=X, num_mc_samples=8, seed=1)
            assert torch.equal(v0, torch.zeros_like(v0))
            v1 = harness.acqf_values(model, raw[:16], "nei", X_baseline=X[:3], num_mc_samples=8, seed=1)
            assert bool((v1 >= 0).all()) and float(v1.max()) > 0
        Xn, vn = harness.optimize_acqf(model, "nei", unit, q, num_restarts=2, raw_samples=32, maxiter=10, seed=4, num_mc_samples=8, X_baseline=X)
        assert Xn.shape == (q, d) and float(vn) >= 0
        with pytest.raises(ValueError, match="nei needs X_baseline"):
            harness.optimize_acqf(model, "nei", unit, q, raw_samples=4, num_restarts=1, maxiter=2)


def test_thompson_sample_picks_each_paths_argmax():
    from online_gp_amd import harness

    model, X, y = _bo_model(3, 10, 120)                                     # 10^3: dense regime
    assert hasattr(model.prediction_cache["pred_cov"], "dense")
    rng = np.random.default_rng(2)
    cand = torch.as_tensor(rng.uniform(0, 1, (500, 3)), device=DEV)
    q = 5
    picks = harness.thompson_sample(model, cand, q, seed=7)
    paths = model.sample_paths(q, seed=7)
    g = model._grid
    Wc = ref.dense_w(g.g0, g.h, g.g, cand.cpu().numpy())
    F = Wc @ paths.values.cpu().numpy().T                                   # [500, q] from dense oracle weights
    assert picks.shape == (q, 3)
    assert torch.equal(picks, cand[torch.as_tensor(F.argmax(0), device=DEV)])
    assert np.allclose(paths.max_values(cand).cpu().numpy(), F.max(0), rtol=1e-12, atol=0)


def test_bayesopt_thompson_carries_the_probes():
    from online_gp_amd import harness
    from online_gp_amd.models import OnlineSKIBotorchModel

    d, q, S = 2, 2, 4
    bounds = torch.tensor([[0.0, 1.0]] * d, dtype=torch.float64)
    fn = lambda Z: -((Z - 0.6) ** 2).sum(-1)
    gen = torch.Generator().manual_seed(0)
    init_x = torch.rand(12, d, generator=gen, dtype=torch.float64).to(DEV)
    init_y = fn(init_x).reshape(-1, 1)
    gb = torch.tensor([[-0.1, 1.1]] * d)

    def make_model(train_x, train_y, old):
        if old is None:
            return OnlineSKIBotorchModel(train_x, train_y, None, covar_module=_kernel("matern52", d, gb, 12, 0.3, 1.0), learn_additional_noise=True,
                                         num_path_probes=S, path_seed=13)
        return OnlineSKIBotorchModel(covar_module=old.covar_module, kernel_cache=old._kernel_cache, learn_additional_noise=True,
                                     likelihood=old.likelihood, num_data=old.num_data)

    rows, tx, ty, model = harness.bayesopt(fn, bounds, make_model, init_x, init_y, num_steps=3, batch_size=q, fit_iters=2, num_candidates=32,
                                           acqf_optimizer="gradient", acqf="ts", num_restarts=2, maxiter=10)
    assert len(rows) == 3 and tx.shape[0] == 12 + 3 * q == model.num_data == model._kernel_cache["path_count"]
    g = model._grid
    Pr, cnt, asum = ref.probes(g.g0, g.h, g.g, tx.cpu().numpy(), None, 0, 13, S, with_bounds=True)
    dev = np.abs(model._kernel_cache["path_probes"].cpu().numpy() - Pr)
    assert (dev <= _probe_tolerance(cnt, asum, torch.float64)).all()
