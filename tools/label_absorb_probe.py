"""Cost of a labelled batch against a plain multi-output absorb of the same points; run from the repository root.

Per grid, class count and precision: 4 096 uniform points with the carry (u, res), 30 back-to-back calls through grid_ops between two
HIP events after 5 warm-up calls -- grid_ops.scatter_stats_multi (values for every output), grid_ops.scatter_stats_label (labels),
grid_ops.label_sites and grid_ops.label_proba -- in microseconds per call.  The statistics are not zeroed between calls: the sums grow,
the work per call does not depend on them.  Then the model: a 12 x 12 grid, three classes, batches of 50, an update and a small
prediction behind it, with values and with labels, median of ten in milliseconds."""
import sys, time
import numpy as np, torch
sys.path.insert(0, ".")
from online_gp_amd import grid_ops
from online_gp_amd.models import FixedNoiseOnlineSKIGP

dev = "cuda"
def timeit(fn, reps=30):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3

for g, C, n, dt in (([64, 64], 3, 4096, torch.float32), ([64, 64], 16, 4096, torch.float32), ([50, 50, 50], 3, 4096, torch.float32), ([50, 50, 50], 3, 4096, torch.float64)):
    d = len(g)
    grid = grid_ops.GridSpec([[-1.0, 1.0]] * d, g)
    gen = torch.Generator(device=dev).manual_seed(0)
    X = (torch.rand((n, d), device=dev, dtype=dt, generator=gen) * 1.8 - 0.9)
    H = (grid.R + 1) // 2
    z = lambda *s: torch.zeros(s, device=dev, dtype=dt)
    b, A, cnt, res, stats, err = z(C, grid.m), z(C, H, grid.m), z(C, grid.m), z(C, grid.m), torch.zeros((C, 2), device=dev, dtype=torch.float64), grid_ops.new_err_flag(dev)
    U = torch.randn((C, grid.m), device=dev, dtype=dt, generator=gen) * 0.5
    Y = torch.randn((C, n), device=dev, dtype=dt, generator=gen)
    one = torch.ones(n, device=dev, dtype=dt)
    pvar = torch.rand((C, n), device=dev, dtype=dt, generator=gen)
    lab = torch.randint(0, C, (n,), device=dev, generator=gen).to(dt)
    t_multi = timeit(lambda: grid_ops.scatter_stats_multi(grid, X, Y, one, one, one, b, A, cnt, stats, err, u=U, res=res))
    t_label = timeit(lambda: grid_ops.scatter_stats_label(grid, X, lab, pvar, [0.7] * C, one, one, one, b, A, cnt, stats, err, U, res=res))
    mu = torch.randn((C, n), device=dev, dtype=dt, generator=gen)
    t_sites = timeit(lambda: grid_ops.label_sites(mu, pvar, pvar + 0.5, lab))
    t_proba = timeit(lambda: grid_ops.label_proba(mu, pvar, pvar + 0.5))
    print(f"grid {g} C {C} n {n} {dt}: multi absorb {t_multi:.1f} us  label absorb {t_label:.1f} us  label_sites {t_sites:.1f} us  label_proba {t_proba:.1f} us", flush=True)

# the model's update: 12 x 12 grid, three classes, batches of 50
rng = np.random.default_rng(0)
for dt in (torch.float32,):
    X0 = torch.as_tensor(rng.uniform(-0.9, 0.9, (20, 2)), device=dev, dtype=dt)
    mk = lambda: FixedNoiseOnlineSKIGP(X0, torch.zeros((20, 3), device=dev, dtype=dt), torch.ones((20, 3), device=dev, dtype=dt), grid_bounds=torch.tensor([[-1.0, 1.0]] * 2), grid_size=[12, 12]).eval()
    for what in ("values", "labels"):
        m = mk()
        ts = []
        for k in range(14):
            Xb = torch.as_tensor(rng.uniform(-0.9, 0.9, (50, 2)), device=dev, dtype=dt)
            yb = torch.randn((50, 3), device=dev, dtype=dt)
            lb = torch.randint(0, 3, (50,), device=dev).to(dt)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            if what == "values": m.condition_on_observations(Xb, yb, inplace=True)
            else: m.condition_on_observations(Xb, None, labels=lb, inplace=True)
            m(Xb[:4]).mean.sum().item()
            ts.append(time.perf_counter() - t0)
        print(f"model update + a prediction, 12 x 12, C = 3, q = 50, {dt}, {what}: median {np.median(ts[4:]) * 1e3:.2f} ms", flush=True)
